"""The references, gates and case tables of the attention suite, checked without a GPU: tests/ref_attention.py against fp64 autograd
of the textbook form and a masked-einsum formulation, the dropout mask against a scalar restatement of the hash, the needle inputs, the
rounding model against every gate of tests/attention_cases.py, the planned instance of every case by name (mpv_attn_plan_describe,
as tests/test_attn_plan_cpu.py), the coverage of the variant table, and four planted faults that the comparison of the GPU test must
name.  pytest -s prints the model's residual per case: the `model` column of profiles/attention_kernel_errors.md."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_cases as A
import ref_attention as R
import ref_norm
import test_attn_plan_cpu as plan_cpu

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
MODEL_CASES = [(c, k) for c in A.ALL_ATTN for k in c["classes"]]


def _ids(pairs):
    return [f"{c['name']}-{k}" for c, k in pairs]


# ------------------------------------------------------------------------------------------------------------------ references
def _textbook(q, k, v, do, vis, scale, sqb, keep, ds):
    """fp64 autograd of softmax(mask(q'' k^T)) keep ds V; the leaf is q (sqb = 0) or q' (then dq = scale x its gradient).  q'' and the
    scale the C ABI passes are formed here, not taken from the module under test."""
    sc = float(np.float32(scale))
    if sqb == 1:
        qq = (q.float() * torch.tensor(scale, dtype=torch.float32)).to(torch.bfloat16).to(F64)
    else:
        qq = q.to(F64) * (1.0 if sqb == 2 else sc)
    qq = qq.clone().requires_grad_(True)
    kk, vv = k.to(F64).clone().requires_grad_(True), v.to(F64).clone().requires_grad_(True)
    s = torch.einsum("bhid,bhjd->bhij", qq, kk).masked_fill(~vis, float("-inf"))
    P = s.softmax(-1)
    o = torch.einsum("bhij,bhjd->bhid", P * (keep.to(F64) * ds if keep is not None else 1.0), vv)
    (o * do.to(F64)).sum().backward()
    dq = qq.grad * sc          # sqb = 0: d/dq of (sc q) k = sc x d/d(sc q); sqb = 1 / 2: the documented convention
    return o.detach(), torch.logsumexp(s.detach(), -1), dq, kk.grad, vv.grad


@pytest.mark.parametrize("sq,sk,hd,causal,p,sqb", [(5, 7, 8, 0, 0.0, 0), (9, 20, 16, 1, 0.0, 0), (9, 21, 16, 1, 0.25, 1), (33, 33, 24, 1, 0.1, 2),
                                                   (1, 6, 8, 1, 0.0, 0), (12, 12, 8, 0, 0.5, 1)])
def test_references_vs_fp64_autograd(sq, sk, hd, causal, p, sqb):
    B, H, scale = 2, 3, hd ** -0.5
    q, k, v, do = (A.rn((B, H, s, hd), 7 + i, CPU) for i, s in enumerate((sq, sk, sk, sq)))
    keep = R.attn_keep_mask(11, 5, B, H, sq, sk, p) if p else None
    ds = R.drop_scale(p) if p else 1.0
    # the causal rule written out, not taken from the module under test
    vis = torch.tensor([[(not causal) or j <= i + (sk - sq) for j in range(sk)] for i in range(sq)])
    o, lse, dq, dk, dv = _textbook(q, k, v, do, vis, scale, sqb, keep, ds)
    fwd = R.attn_fwd_ref(q, k, v, causal, scale, sqb, keep, ds)
    bwd = R.attn_bwd_ref(q, k, v, o, lse, do, causal, scale, sqb, keep, ds)
    for name, got, want in (("o", fwd["o"], o), ("lse", fwd["lse"], lse), ("dq", bwd["dq"], dq), ("dk", bwd["dk"], dk), ("dv", bwd["dv"], dv)):
        R.close_elementwise(got, want, 1e-12, 1e-13, f"reference {name}")
    assert (fwd["P"].sum(-1) - 1).abs().max() < 1e-13
    if causal:      # the hidden part of every row carries exactly nothing
        assert float(fwd["P"].masked_select(~vis.expand_as(fwd["P"])).abs().max() if (~vis).any() else 0.0) == 0.0


def test_scales_bound_the_terms():
    """|o| <= scale_o and so on: a scale is a sum of absolute terms, so it bounds its element (a wrong scale would loosen or tighten a gate)"""
    c = A.ONE_SHOT[0]
    r = A.references(c, "randn", CPU, items=2)
    assert bool((r["fwd"]["o"].abs() <= r["fwd"]["scale_o"] * (1 + 1e-12)).all())
    for n in ("dq", "dk", "dv"):
        assert bool((r["bwd"][n].abs() <= r["bwd"]["scale_" + n] * (1 + 1e-9) + 1e-300).all()), n


def test_temporal_ref_vs_fp64_autograd():
    B, N, T, heads, hd = 2, 3, 5, 2, 8
    D, N1, scale = heads * hd, N + 1, hd ** -0.5
    qkv, dout = A.rn((B * T * N1, 3 * D), 1, CPU), A.rn((B * T * N1, D), 2, CPU)
    q, k, v = R.temporal_split(qkv, B, N, T, heads, hd)
    qq = (q.float() * torch.tensor(scale, dtype=torch.float32)).to(torch.bfloat16).to(F64).clone().requires_grad_(True)
    kk, vv = k.to(F64).clone().requires_grad_(True), v.to(F64).clone().requires_grad_(True)
    out = (qq @ kk.transpose(-1, -2)).softmax(-1) @ vv
    (out * R.temporal_rows(dout, B, N, T, heads, hd).to(F64)).sum().backward()
    ref = R.temporal_ref(qkv, dout, B, N, T, heads, hd, scale)
    for name, want in (("out", out.detach()), ("dq", qq.grad * float(np.float32(scale))), ("dk", kk.grad), ("dv", vv.grad)):
        R.close_elementwise(ref[name], want, 1e-12, 1e-13, f"temporal reference {name}")
        assert bool((ref[name].abs() <= ref["scale_" + name] * (1 + 1e-9)).all()), name


# ------------------------------------------------------------------------------------------------------------------ dropout mask
def test_keep_mask_is_attentions_key_pair_convention():
    seed, p = 0x123456789ABCDEF, 0.3
    for (B, H, sq, sk, offset) in ((2, 3, 5, 7, 0), (1, 2, 4, 6, 9), (1, 1, 3, 5, (3 << 36) + 1), (2, 1, 2, 8, 4)):
        m = R.attn_keep_mask(seed, offset, B, H, sq, sk, p)
        for b in range(B):
            for h in range(H):
                for r in range(sq):
                    for key in range(sk):
                        assert bool(m[b, h, r, key]) == R.attn_keep_scalar(seed, offset, b, h, r, key, H, sq, sk, p), (b, h, r, key)
        g = ref_norm.keep_mask(seed, offset, B * H * sq, sk, p).view(B, H, sq, sk)          # pairs on the global element index
        base = offset + torch.arange(B * H * sq).view(B, H, sq) * sk
        even = (base % 2) == 0
        assert torch.equal(m[even], g[even])
        if bool((~even).any()):
            assert not torch.equal(m[~even], g[~even]), "an odd row base must change the pairing"
    rate = R.attn_keep_mask(seed, 1, 4, 4, 64, 65, 0.1).float().mean().item()
    assert abs(rate - 0.9) < 0.01, rate
    cell = {0x7000: seed}
    assert torch.equal(R.attn_keep_mask(R.SEED_INDIRECT_BIT | 0x7000, 3, 1, 2, 4, 6, p, deref=cell.__getitem__), R.attn_keep_mask(seed, 3, 1, 2, 4, 6, p))


# ------------------------------------------------------------------------------------------------------------------ needles
@pytest.mark.parametrize("c", [c for c in A.ALL_ATTN if "needle" in c["classes"]], ids=lambda c: c["name"])
def test_needles_dominate_their_rows(c):
    _, _, sq, sk, hd, causal, _ = c["shape"]
    pairs = R.needle_pairs(sq, sk, causal)
    assert len({r for r, _ in pairs}) == len(pairs) == len({k for _, k in pairs})
    keys = {k for _, k in pairs}
    assert sk - 1 in keys
    if sq >= 4:          # (a single query row holds one needle: the last key)
        assert 0 in keys and (32 * ((sk - 1) // 32) in keys)
    if causal:
        assert (0, sk - sq) in pairs and (sq - 1, sk - 1) in pairs
    P = A.references(c, "needle", CPU, items=2)["fwd"]["P"]
    for r, k in pairs:
        assert float(P[:, :, r, k].min()) > 0.9, (c["name"], r, k, float(P[:, :, r, k].min()))


# ------------------------------------------------------------------------------------------------------------------ rounding model
@pytest.mark.parametrize("c,klass", MODEL_CASES, ids=_ids(MODEL_CASES))
def test_rounding_model_is_inside_every_gate(c, klass):
    """The references with P (o, dV), dS (dQ, dK) and the outputs rounded to bf16 stay inside the gates through the comparison the GPU
    test uses, and inside their bf16 part alone: what the model cannot know (fp32 accumulation and its order, v_exp_f32) is the EPS
    part of a coefficient, itself twice the worst fp32 accumulation error of the longest case (attention_cases, GATES).  Batch and
    heads are capped at 2: items are independent."""
    r = A.references(c, klass, CPU, items=2, model=True)
    got = dict(o=r["fwd_model"]["o"], lse=r["fwd"]["lse"].to(torch.float32))
    names = ["o", "lse"]
    if c["plan"][1] is not None:
        got.update({n: r["bwd_model"][n] for n in ("dq", "dk", "dv")})
        names += ["dq", "dk", "dv"]
    A.compare(got, r, f"model {c['name']}[{klass}]")
    for n in names:
        src = r["fwd"] if n in ("o", "lse") else r["bwd"]
        rtol, coef, eps = A.GATES[n]
        res = R.residual(got[n], src[n], src["scale_" + n], rtol)
        print(f"[model] {c['name']}[{klass}] {n}: residual {res:.3e} of gate {coef:.3e}")
        assert res <= coef - eps, (n, res, coef)          # the model knows no fp32 effect: the EPS part stays unused


@pytest.mark.parametrize("c", A.TEMPORAL_B16 + A.TEMPORAL_RUNTIME[:4] + A.TEMPORAL_MFMA, ids=lambda c: c["name"])
def test_temporal_rounding_model_is_inside_every_gate(c):
    B, N, T, heads, hd = c["shape"]
    qkv, dout, Rr = A.temporal_inputs(c, CPU)
    ref = R.temporal_ref(qkv, dout[:Rr], B, N, T, heads, hd, hd ** -0.5)
    mod = R.temporal_ref(qkv, dout[:Rr], B, N, T, heads, hd, hd ** -0.5, model=True)
    for n in ("out", "dq", "dk", "dv"):
        rtol, coef, eps = A.TEMPORAL_GATES[n]
        R.close_gated(mod[n], ref[n], ref["scale_" + n], (rtol, coef), f"model {c['name']} {n}")
        res = R.residual(mod[n], ref[n], ref["scale_" + n], rtol)
        print(f"[model] {c['name']} {n}: residual {res:.3e} of gate {coef:.3e}")
        assert res <= coef - eps, (n, res)


# ------------------------------------------------------------------------------------------------------------------ plans
def plan_names(which):
    """[(case name, [instance names])] of the default tables or of a knob arm's cases, through the describe entries (host code only)"""
    b = plan_cpu._binding()
    if which == "default":
        attn, temporal = A.ALL_ATTN, A.ALL_TEMPORAL
    else:
        attn, temporal = (A.PAIR_KNOB_CASES, []) if which == "pair" else ([], A.TEMPORAL_F32_KNOB)
    out = [(c["name"], [g[0] for g in plan_cpu.describe(c["shape"])]) for c in attn]
    return out + [(c["name"], [g[0] for g in A.temporal_describe(b, c)]) for c in temporal]


def _want(cases):
    return [(c["name"], c["plan"]) for c in cases]


def test_every_case_is_planned_onto_the_instances_it_names():
    assert not any(k in os.environ for k in plan_cpu.KNOBS)
    got = dict(plan_names("default"))
    for c in A.ALL_ATTN + A.ALL_TEMPORAL:
        want = [n for n in c["plan"] if n]
        assert got[c["name"]][:len(want)] == want, (c["name"], got[c["name"]], want)
    big = next(c for c in A.TEMPORAL_RUNTIME if c["shape"][1] == 70000)
    grids = A.temporal_describe(plan_cpu._binding(), big)
    assert grids[0][1] == grids[1][1] == 16384, grids          # the grid cap: the kernels' stride loop runs


@pytest.mark.parametrize("arm", sorted(A.KNOB_ARMS))
def test_knob_arm_cases_are_planned_onto_the_instances_they_name(arm):
    env = {k: v for k, v in os.environ.items() if k not in plan_cpu.KNOBS}
    name, value = arm.split("=")
    env[name] = value
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests"), ROOT] + env.get("PYTHONPATH", "").split(os.pathsep))
    code = f"import json, test_attention_refs_cpu as t; print(json.dumps(t.plan_names({A.KNOB_ARMS[arm]!r})))"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {n: tuple(v) for n, v in json.loads(r.stdout.strip().splitlines()[-1])}
    cases = A.PAIR_KNOB_CASES if A.KNOB_ARMS[arm] == "pair" else A.TEMPORAL_F32_KNOB
    assert cases and all(got[c["name"]] == tuple(c["plan"]) for c in cases), (got, _want(cases))


def test_the_tables_name_the_whole_variant_table():
    src = open(os.path.join(ROOT, "youku-mplug_amd", "csrc", "attention.hip")).read()
    body = src[src.index("#define ATTN_VARIANTS(X)"):src.index("enum AttnVariantId")]
    table = set(re.findall(r"((?:attn|temporal)_\w+_kernel<[^()]*>)\)\s*\\?\n", body))
    assert len(table) == 53, len(table)
    named = A.instances_named()
    assert named == table, (sorted(table - named), sorted(named - table))


# ------------------------------------------------------------------------------------------------------------------ planted faults
FAULT_CASE = next(c for c in A.ONE_SHOT if c["name"] == "small64-causal-33x70-drop")


@pytest.fixture(scope="module")
def fault_ref():
    return A.references(FAULT_CASE, "randn", CPU, model=True)


def _model_outputs(r):
    return dict(o=r["fwd_model"]["o"].clone(), lse=r["fwd"]["lse"].to(torch.float32), **{n: r["bwd_model"][n].clone() for n in ("dq", "dk", "dv")})


def test_planted_fault_last_term_dropped_from_dv(fault_ref):
    r = fault_ref
    B, H, sq, sk, hd, causal, p = FAULT_CASE["shape"]
    b, h = next((b, h) for b in range(B) for h in range(H) if bool(r["keep"][b, h, sq - 1, sk - 1]))
    got = _model_outputs(r)
    A.compare(got, r, "unperturbed")
    pt = r["fwd"]["P"][b, h, sq - 1, sk - 1] * r["ds"]
    got["dv"][b, h, sk - 1] = R.rbf(got["dv"][b, h, sk - 1] - pt * r["do"][b, h, sq - 1].to(F64))
    with pytest.raises(AssertionError, match=rf"dv: element \({b}, {h}, {sk - 1}, \d+\)"):
        A.compare(got, r, "dropped term")


def test_planted_fault_causal_bound_without_the_shift(fault_ref):
    r = fault_ref
    B, H, sq, sk, hd, causal, p = FAULT_CASE["shape"]
    wrong = R.visible_mask(sq, sq, True).new_zeros(sq, sk)
    wrong[:, :sq] = R.visible_mask(sq, sq, True)          # j <= i
    bad = R.attn_fwd_ref(r["q"], r["k"], r["v"], causal, r["scale"], 0, r["keep"], r["ds"], visible=wrong, model=True)
    with pytest.raises(AssertionError, match=r"j <= i o: element \(\d+, \d+, \d+, \d+\)"):
        A.compare(dict(o=bad["o"], lse=bad["lse"].to(torch.float32)), r, "j <= i")


def test_planted_fault_mask_paired_on_the_global_index(fault_ref):
    r = fault_ref
    B, H, sq, sk, hd, causal, p = FAULT_CASE["shape"]
    assert FAULT_CASE["offset"] % 2 == 1
    keep = ref_norm.keep_mask(FAULT_CASE["seed"], FAULT_CASE["offset"], B * H * sq, sk, p).view(B, H, sq, sk)
    assert not torch.equal(keep, r["keep"])
    bad = R.attn_fwd_ref(r["q"], r["k"], r["v"], causal, r["scale"], 0, keep, r["ds"], model=True)
    with pytest.raises(AssertionError, match=r"o: element \(\d+, \d+, \d+, \d+\)"):
        A.compare(dict(o=bad["o"]), r, "global pairing")
    badb = R.attn_bwd_ref(r["q"], r["k"], r["v"], r["o_given"], r["lse_given"], r["do"], causal, r["scale"], 0, keep, r["ds"], model=True)
    with pytest.raises(AssertionError, match=r"dv: element"):
        A.compare(dict(dv=badb["dv"]), r, "global pairing")


@pytest.mark.parametrize("kind,parts", [("padded", 1), ("packed", 3)])
def test_planted_fault_one_store_into_a_guard_column(kind, parts):
    B, S, H, hd = 2, 5, 2, 8
    arena, views, (bs, hs, rs) = A.cut(kind, B, S, H, hd, parts, A.GUARD_BITS, CPU, pad_items=6)
    for v in views:
        v.copy_(A.rn((B, H, S, hd), 3, CPU))
    arena.check("untouched", arena.row)
    front = A.SLACK_ROWS * rs
    if kind == "padded":
        spot = front + 1 * bs + 2 * rs + H * hd + 3          # a gap column of batch 1, row 2
    else:
        spot = front + B * bs + 4                            # the first row behind the last batch: a padding item's row
    arena.buf[spot] = 1.0
    with pytest.raises(AssertionError, match=rf"guard element {spot} \(row {spot // rs}, column {spot % rs}"):
        arena.check("planted", arena.row)
    a32, lse = A.stat(2, 2, 5, CPU)
    lse.fill_(1.0)
    a32.check("lse")
    a32.buf[A.SLACK_ROWS + 2 * 2 * 5] = 0.5
    with pytest.raises(AssertionError, match="guard element"):
        a32.check("lse")
