"""The attention dispatch, checked without a GPU: mpv_attn_plan_describe / mpv_temporal_attn_plan_describe (csrc/attention.hip:
attn_plan, temporal_plan and the variant table) must reproduce the recorded dispatch of the parent commit (tests/attn_plan_cases.py)
exactly -- instance, grid, block and dynamic LDS -- in the default arm and under every measurement knob, and every planned LDS
request must fit its instance's opt-in limit and a CU's 160 KiB."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import pytest

import attn_plan_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("MPV_ATTN_PERSIST", "MPV_ATTN_PAIR", "MPV_ATTN_DUO", "MPV_TEMPORAL_ROWS")


_lib = None


def _binding():
    """youku-mplug_amd/_lib.py on its own (ctypes only): the child processes of the knob arms need nothing else of the package."""
    global _lib
    if _lib is None:
        spec = importlib.util.spec_from_file_location("mpv_lib_binding", os.path.join(ROOT, "youku-mplug_amd", "_lib.py"))
        _lib = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_lib)
    return _lib


def attn_desc(case):
    """The recorder's descriptor: dummy aligned pointers, [batch][row][head][head_dim] strides."""
    _lib = _binding()
    B, H, Sq, Sk, hd, causal, p = case
    d = _lib.AttnDesc()
    d.q = d.k = d.v = d.o = d.lse = 0x100000
    d.q_bs = d.o_bs = Sq * H * hd
    d.k_bs = d.v_bs = Sk * H * hd
    d.q_hs = d.k_hs = d.v_hs = d.o_hs = hd
    d.q_rs = d.k_rs = d.v_rs = d.o_rs = H * hd
    d.batch, d.heads, d.sq, d.sk, d.head_dim, d.causal = B, H, Sq, Sk, hd, causal
    d.scale, d.dropout_p = 0.125, p
    return d


def describe(case):
    """[(name, grid_x, grid_y, block, lds_bytes, lds_limit)] for the launches of a case: three roles (attention) or one (temporal)."""
    _lib = _binding()
    lib, info, out = _lib.lib(), _lib.AttnPlanInfo(), []
    if len(case) == 7:
        d = attn_desc(case)
        for role in (0, 1, 2):
            _lib.check(lib.mpv_attn_plan_describe(C.byref(d), role, C.byref(info)), "mpv_attn_plan_describe")
            out.append((info.variant.decode(), info.grid_x, info.grid_y, info.block, info.lds_bytes, info.lds_limit))
    else:
        bwd, n_outer, n_inner, T, heads, hd = case
        _lib.check(lib.mpv_temporal_attn_plan_describe(n_outer, n_inner, T, heads, hd, bwd, C.byref(info)), "mpv_temporal_attn_plan_describe")
        out.append((info.variant.decode(), info.grid_x, info.grid_y, info.block, info.lds_bytes, info.lds_limit))
    return out


def expected(case, arm=None):
    rows = cases.KNOB_ARMS[arm].get(case) if arm else None
    if rows is None:
        rows = cases.ATTN[case] if len(case) == 7 else cases.TEMPORAL[case]
    return [tuple(r) for r in (rows if len(case) == 7 else (rows,))]


ALL_CASES = list(cases.ATTN) + list(cases.TEMPORAL)


@pytest.fixture(scope="module")
def default_plans():
    assert not any(k in os.environ for k in KNOBS), "a dispatch knob is set in the environment: this process cannot observe the default arm"
    return {case: describe(case) for case in ALL_CASES}


def test_plan_reproduces_the_parent_dispatch(default_plans):
    bad = [(case, [g[:5] for g in got], expected(case)) for case, got in default_plans.items() if [g[:5] for g in got] != expected(case)]
    assert not bad, (len(bad), bad[:5])
    reached = {g[0] for got in default_plans.values() for g in got}
    assert len(reached) >= 37, sorted(reached)      # the 37 instances the parent's default arm reaches over these cases


def test_planned_lds_fits_the_variant_limit_and_a_cu(default_plans):
    for case, got in default_plans.items():
        for name, gx, gy, block, lds, limit in got:
            assert 0 <= lds <= limit <= 160 * 1024, (case, name, lds, limit)
            assert gx >= 1 and gy >= 1 and block % 64 == 0 and 64 <= block <= 512, (case, name, gx, gy, block)
            # above the 64 KiB default the launch needs the opt-in, which walks exactly the rows whose limit is above it
            assert lds <= 64 * 1024 or limit > 64 * 1024, (case, name, lds, limit)


def test_duo_limit_covers_the_longest_seven_tile_sequence(default_plans):
    """S = 224, head_dim 96: 46 + 42 KiB (dQ) and 2 + 84 KiB (dK/dV) -- the limits are derived from the layout at that shape."""
    dq, dkv = default_plans[(2, 2, 224, 224, 96, 0, 0.0)][1:]
    assert dq[0] == "attn_bwd_dq_duo96_kernel<256>" and dq[4] == dq[5] == 88 * 1024, dq
    assert dkv[0] == "attn_bwd_dkv_duo96_kernel<256>" and dkv[4] == dkv[5] == 86 * 1024, dkv


@pytest.mark.parametrize("arm", sorted(cases.KNOB_ARMS))
def test_knob_arm_reproduces_the_parent_dispatch(arm):
    """Knobs are read once per process: each setting is planned in a fresh child process (host code only, no GPU is touched)."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    name, value = arm.split("=")
    env[name] = value
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests"), ROOT] + env.get("PYTHONPATH", "").split(os.pathsep))
    code = "import json, test_attn_plan_cpu as t; print(json.dumps([[list(c), t.describe(c)] for c in t.ALL_CASES]))"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {tuple(c): [tuple(g[:5]) for g in rows] for c, rows in json.loads(r.stdout.strip().splitlines()[-1])}
    assert set(got) == set(ALL_CASES)
    bad = [(case, rows, expected(case, arm)) for case, rows in got.items() if rows != expected(case, arm)]
    assert not bad, (len(bad), bad[:5])
    assert any(got[c] != expected(c) for c in cases.KNOB_ARMS[arm]), "the arm must leave the default somewhere"


def test_describe_refuses_what_the_entry_points_refuse():
    _lib = _binding()
    lib, info = _lib.lib(), _lib.AttnPlanInfo()
    d = attn_desc((2, 2, 160, 160, 64, 1, 0.0))
    assert lib.mpv_attn_plan_describe(None, 0, C.byref(info)) != 0
    assert lib.mpv_attn_plan_describe(C.byref(d), 0, None) != 0
    assert lib.mpv_attn_plan_describe(C.byref(d), 3, C.byref(info)) != 0
    for field, bad in (("head_dim", 100), ("head_dim", 12), ("q", 0), ("q", 0x100008), ("q_rs", 130), ("dropout_p", 1.0), ("scale", 0.0), ("sk", 0),
                       ("sq", 161)):      # causal needs sk >= sq
        d = attn_desc((2, 2, 160, 160, 64, 1, 0.0))
        setattr(d, field, bad)
        assert lib.mpv_attn_plan_describe(C.byref(d), 0, C.byref(info)) != 0, (field, bad)
        assert b"mpv_attn_plan_describe" in lib.mpv_last_error()
    assert lib.mpv_temporal_attn_plan_describe(2, 6, 17, 2, 96, 0, C.byref(info)) != 0
    assert lib.mpv_temporal_attn_plan_describe(2, 6, 8, 2, 96, 0, None) != 0
