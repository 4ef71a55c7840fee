"""The attention family -- csrc/attention.hip (the streaming, one-shot resident, persistent and decode kernels, the VALU temporal
kernels), attention_pair.inc (paired-block causal), attention_duo.inc (the ViT backward as two items per CU) and
attention_temporal_long.inc (matrix-core temporal attention) -- against the fp64 references of tests/ref_attention.py, element by
element, at the smallest shapes that reach each of the 53 instances of the variant table and each branch (tests/attention_cases.py
says which and why, and derives the gates).  The backward kernels are given bf16(o_ref) and fp32(lse_ref), not a forward kernel's
output, so that an instance is judged on its own.  Every tensor is a view into a guarded buffer; everything called identical or
untouched is compared on the raw bits.  pytest -s prints every comparison's worst residual in units of the element's scale;
profiles/attention_kernel_errors.md holds the table.  Run on the MI355X box: pytest -m gpu tests/test_attention_kernels_gpu.py"""
import os
import subprocess
import sys

import pytest

import attention_cases as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("MPV_ATTN_PERSIST", "MPV_ATTN_PAIR", "MPV_ATTN_DUO", "MPV_TEMPORAL_ROWS")


def _pairs(cases):
    return [(c, k) for c in cases for k in c["classes"]]


def _ids(pairs):
    return [f"{c['name']}-{k}" for c, k in pairs]


def _run(dev, c, klass):
    from youku_mplug_amd import _lib, ops
    A.run_attention(ops, _lib, dev, c, klass)


@pytest.mark.parametrize("c,klass", _pairs(A.STREAMING), ids=_ids(_pairs(A.STREAMING)))
def test_streaming_vs_fp64(dev, c, klass):
    """attn_fwd_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel <64>, <80>, <96>: more keys than a resident kernel holds, causal with
    sk > sq, an odd sk under dropout with head_dim 72 in the <80> instance, a single row one key over the decode kernel's limit."""
    _run(dev, c, klass)


@pytest.mark.parametrize("c,klass", _pairs(A.ONE_SHOT), ids=_ids(_pairs(A.ONE_SHOT)))
def test_one_shot_vs_fp64(dev, c, klass):
    """The resident kernels: the small head_dim-64 instances (head_dim 8 and 40, causal with sk > sq), res<64> above the paired range,
    res<80> and res<96> under dropout and at RES_MAX_ROWS, the 7-tile instances that the duo backward does not take."""
    _run(dev, c, klass)


@pytest.mark.parametrize("c,klass", _pairs(A.PAIRED), ids=_ids(_pairs(A.PAIRED)))
def test_paired_vs_fp64(dev, c, klass):
    """attention_pair.inc under dropout: the 7-block instances at 208 (as shipped) and 161 rows (six blocks), the 5-block forward and dQ
    with the one-shot dK/dV, a single row, odd offsets, a batch of 17."""
    _run(dev, c, klass)


@pytest.mark.parametrize("c,klass", _pairs(A.PERSISTENT), ids=_ids(_pairs(A.PERSISTENT)))
def test_persistent_and_duo_vs_fp64(dev, c, klass):
    """The persistent forward (LEAN at 197 keys, the plain instance at 201) over more items than CUs, the duo dQ and dK/dV, at the
    shortest and the longest 7-tile sequence."""
    _run(dev, c, klass)


@pytest.mark.parametrize("c,klass", _pairs(A.DECODE), ids=_ids(_pairs(A.DECODE)))
def test_decode_vs_fp64(dev, c, klass):
    """attn_decode_kernel<8> / <16>, forward only: one key, DEC_MAX_SK keys, head_dim 8 / 80 / 96, plain and pre-scaled q."""
    _run(dev, c, klass)


@pytest.mark.parametrize("c", A.ALL_TEMPORAL, ids=lambda c: c["name"])
def test_temporal_vs_fp64(dev, c):
    """The bf16-row instances, the run-time fp32-row kernel (T = 1, head_dim 4, and 70000 problems on 16384 workgroups: the stride
    loop) and the matrix-core instances with a ragged last workgroup, in the layout and with the canaries of
    test_temporal_long_gpu.run_kernel_case."""
    from youku_mplug_amd import _lib, ops
    A.run_temporal(ops, _lib, dev, c)


def knob_arm_main(which):
    """The body of a knob arm's child process: the cases that arm changes, with the planned names and the gates of the default arm."""
    import torch
    from youku_mplug_amd import _lib, ops
    dev = torch.device("cuda:0")
    _lib.check(_lib.lib().mpv_check_device(), "mpv_check_device")
    if which == "pair":
        for c in A.PAIR_KNOB_CASES:
            for klass in c["classes"]:
                A.run_attention(ops, _lib, dev, c, klass)
    else:
        for c in A.TEMPORAL_F32_KNOB:
            A.run_temporal(ops, _lib, dev, c)
    print(f"knob arm {which}: ok")


def test_knob_arms_vs_fp64(dev):
    """attn_bwd_dkv_pair64_kernel<192, 3> (MPV_ATTN_PAIR=2) and the six temporal_attn_kernel<., T, 96> (MPV_TEMPORAL_ROWS=fp32) are
    reached under a measurement knob only, and knobs are read once per process: one fresh child process per arm, one after the other; a
    child that fails or dies fails the test and nothing further is started."""
    for arm in sorted(A.KNOB_ARMS):
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        name, value = arm.split("=")
        env[name] = value
        env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests"), ROOT] + env.get("PYTHONPATH", "").split(os.pathsep))
        code = f"import test_attention_kernels_gpu as t; t.knob_arm_main({A.KNOB_ARMS[arm]!r})"
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        print(r.stdout[-20000:])
        assert r.returncode == 0, (arm, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
        assert f"knob arm {A.KNOB_ARMS[arm]}: ok" in r.stdout, (arm, r.stdout[-1500:])
