"""The fp64 reference of tests/ref_gemm.py is right, a correct implementation fits inside the gates, and the defects the gates exist for
do not (no GPU).
First half: gemm_ref against an independent formulation on tiny shapes -- the product as an einsum over operands gathered element by
element from the flat buffers, the epilogue as a scalar Python loop (math.erf / math.tanh, torch's own bf16 cast, a scalar restatement of
the dropout hash) -- and the bracket of rule 2 (ref_gemm's module text) around a rounding boundary.
Second half: the torch stand-in (tests/standin_ops.py gemm / gemm_batched) over the cases of tests/test_gemm_kernels_gpu.py, through the
same runners and the SAME gates (measured on the kernels), omitting only the two multi-band shapes; then the stand-in with one named
defect at a time, which must FAIL those gates."""
import math

import pytest
import torch

import gemm_cases as G
import ref_gemm as R
import ref_norm
import standin_ops

BF = torch.bfloat16
F64 = torch.float64
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------------------------ references
def _bf(x):
    return float(torch.tensor(x, dtype=F64).to(BF).item())


def test_rbf_rounds_once_to_nearest_even():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(4096, generator=gen, dtype=F64) * torch.tensor(2.0, dtype=F64) ** torch.randint(-20, 20, (4096,), generator=gen)
    assert torch.equal(R.rbf(x), x.to(torch.float32).to(BF).to(F64))          # random values: nowhere near a double-rounding boundary
    u = 2.0 ** -8
    ties = torch.tensor([1 + u, 1 + 3 * u, -(1 + u), 2 + 2 * u, 1 + u + 2.0 ** -40, 1 + u - 2.0 ** -40, 0.0, 255.5, 256.0], dtype=F64)
    want = torch.tensor([1.0, 1 + 4 * u, -1.0, 2.0, 1 + 2 * u, 1.0, 0.0, 256.0, 256.0], dtype=F64)
    assert torch.equal(R.rbf(ties), want)


def _flat_gather(buf, rows, ld, cols):
    f = buf.reshape(-1)
    return torch.stack([torch.stack([f[int(r) * ld + c] for c in range(cols)]) for r in rows]).to(F64)


def _mapped(m, n):
    g, s, o = m
    return [r if g == 0 else (r // g) * s + (r % g) + o for r in range(n)]


@pytest.mark.parametrize("form", ["nt", "nn", "tn"])
def test_product_and_scale_match_an_einsum_over_flat_gathers(form):
    """every operand form with padded leading dimensions and every row map: z, its scale and colsum to 1e-12 of the scale"""
    M, N, K = 8, 16, 11 if form == "tn" else 24
    ta, tb = form == "tn", form != "nt"
    amap, kmap = (2, 3, 1), (3, 4, 1)
    gen = torch.Generator().manual_seed(K)
    A, B = G.operands(gen, M, N, K)
    lda, ldb = (M if ta else K) + 8, (N if tb else K) + 16
    abuf = G.lay(A.t().contiguous(), kmap, lda, G.NAN) if ta else G.lay(A, amap, lda, G.NAN)
    bbuf = G.lay(B, kmap, ldb, G.NAN) if tb else G.lay(B.t().contiguous(), G.IDENT, ldb, G.NAN)
    bias = torch.randn(N, generator=gen).to(BF)
    ref = R.gemm_ref(abuf, bbuf, M, N, K, trans_a=ta, trans_b=tb, lda=lda, ldb=ldb, amap=amap, kmap=kmap, bias=bias, alpha=-0.5,
                     alpha_dev=torch.tensor([0.25]), want_colsum=ta)
    a = _flat_gather(abuf, _mapped(kmap, K), lda, M).t() if ta else _flat_gather(abuf, _mapped(amap, M), lda, K)
    b = _flat_gather(bbuf, _mapped(kmap, K), ldb, N) if tb else _flat_gather(bbuf, range(N), ldb, K).t()
    z = torch.einsum("mk,kn->mn", a, b) * -0.125 + bias.to(F64)
    s = torch.einsum("mk,kn->mn", a.abs(), b.abs()) * 0.125 + bias.to(F64).abs()
    assert ((ref["z"].lo - z).abs() <= 1e-12 * s).all() and ((ref["z"].scale - s).abs() <= 1e-12 * s).all()
    assert (z.abs() <= s * (1 + 1e-12)).all() and ref["c"] is ref["z"]
    if ta:
        assert ((ref["colsum"].lo - a.sum(1)).abs() <= 1e-12 * a.abs().sum(1)).all()
        assert torch.equal(ref["colsum"].scale, a.abs().sum(1))


def _act_scalar(z, kind):
    if kind == 1:
        return 0.5 * z * (1.0 + math.erf(z / math.sqrt(2.0)))
    if kind == 2:
        return 0.5 * z * (1.0 + math.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))
    return max(z, 0.0)


def _act_grad_numeric(z, kind, h=1e-6):
    return (_act_scalar(z + h, kind) - _act_scalar(z - h, kind)) / (2 * h)


def _keep_scalar(seed, idx, thr):
    M32 = 0xffffffff

    def mix(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & M32
        x ^= x >> 15
        x = (x * 0x846ca68b) & M32
        return x ^ (x >> 16)
    ka, kb = mix(seed & M32), mix(((seed >> 32) & M32) ^ 0x85ebca6b)
    ctr = idx - (idx & 1)
    w = mix((((ctr & M32) + ka) & M32) ^ (((ctr >> 32) + kb) & M32))
    return ((w >> 16) if idx & 1 else (w & 0xffff)) >= thr


EPILOGUES = [
    dict(), dict(act=1), dict(act=2), dict(act=3), dict(act=1, preact_deriv=True), dict(act=2, preact_deriv=True),
    dict(act_bwd=1), dict(act_bwd=2), dict(act_bwd=4), dict(act_bwd=3), dict(drop=True), dict(drop=True, residual=True), dict(residual=True),
    dict(accumulate=True), dict(act=3, residual=True, accumulate=True), dict(colscale=(8, 0.125)), dict(out_f32=True), dict(out_f32=True, accumulate=True),
    dict(act=1, act_bwd=4, drop=True, residual=True, accumulate=True),
]


@pytest.mark.parametrize("e", EPILOGUES, ids=[",".join(e) or "plain" for e in EPILOGUES])
def test_epilogue_matches_a_scalar_restatement(e):
    """the documented order of the epilogue, element by element in Python floats: zb = bf16(acc * alpha + bias) (colscale: rounded again),
    act, act' (or the parked derivative), dropout on the row NUMBER's index, residual and C_old through the cmap; zdelta = 0"""
    M, N, K = 6, 16, 8
    cmap = (2, 3, 1)
    gen = torch.Generator().manual_seed(11)
    A, B = G.operands(gen, M, N, K)
    bias = torch.randn(N, generator=gen).to(BF)
    f32 = bool(e.get("out_f32"))
    res = G.lay(torch.randn(M, N, generator=gen).to(BF), cmap, N + 8, G.NAN)
    old = G.lay(torch.randn(M, N, generator=gen).to(torch.float32 if f32 else BF), cmap, N, G.NAN)
    zz = G.lay(torch.randn(M, N, generator=gen).to(BF), G.IDENT, N + 8, G.NAN)
    p = 0.25
    ref = R.gemm_ref(A, B.t().contiguous(), M, N, K, lda=K, ldb=K, cmap=cmap, bias=None if f32 else bias, act=e.get("act", 0),
                     preact_deriv=e.get("preact_deriv", False), residual=res if e.get("residual") else None,
                     act_bwd_z=zz if e.get("act_bwd") else None, act_bwd=e.get("act_bwd", 0), drop=(p, G.DROP_SEED, G.DROP_OFFSET) if e.get("drop") else None,
                     alpha=0.5, out_f32=f32, c_old=old if e.get("accumulate") else None, colscale=e.get("colscale"))
    rows = _mapped(cmap, M)
    for m in range(M):
        for n in range(N):
            acc = sum(float(A[m, k]) * float(B[k, n]) for k in range(K))
            z = acc * 0.5 + (0.0 if f32 else float(bias[n]))
            o = float(old[rows[m], n]) if e.get("accumulate") else 0.0
            if f32:
                assert abs(float(ref["c"].lo[m, n]) - (z + o)) <= 1e-12 and ref["c"].lo[m, n] == ref["c"].hi[m, n]
                continue
            assert abs(float(ref["z"].lo[m, n]) - z) <= 1e-12
            zb = _bf(z) if e else z          # (a plain C is compared with z itself: its one rounding is the gate's rtol)
            if e.get("colscale") and n < e["colscale"][0]:
                zb = _bf(zb * e["colscale"][1])
            v = _act_scalar(zb, e["act"]) if e.get("act") else zb
            if e.get("preact_deriv"):
                a = R.DERIV_APPROX[e["act"]]          # the bracket is the derivative -+ the polynomial's documented error
                assert abs(float(ref["deriv"].lo[m, n]) + a - _act_grad_numeric(zb, e["act"])) <= 1e-8
                assert abs(float(ref["deriv"].hi[m, n]) - a - _act_grad_numeric(zb, e["act"])) <= 1e-8
            if e.get("act_bwd"):
                t = float(zz[m, n])
                v *= t if e["act_bwd"] == 4 else (float(t > 0) if e["act_bwd"] == 3 else _act_grad_numeric(t, e["act_bwd"]))
            if e.get("drop"):
                keep = _keep_scalar(G.DROP_SEED, G.DROP_OFFSET + m * N + n, ref_norm.drop_threshold(p))
                v = v * ref_norm.drop_scale(p) if keep else 0.0
            if e.get("residual"):
                v += float(res[rows[m], n])
            v += o
            a = R.BWD_APPROX * abs(zb) * (ref_norm.drop_scale(p) if e.get("drop") and keep else 1.0) if e.get("act_bwd") in (1, 2) else 0.0
            assert abs(float(ref["c"].lo[m, n]) + a - v) <= 1e-8 * max(1.0, abs(v)) and abs(float(ref["c"].hi[m, n]) - a - v) <= 1e-8 * max(1.0, abs(v)), (m, n)
            assert float(ref["c"].scale[m, n]) * (1 + 2.0 ** -7) >= abs(v)          # (a sum of absolute terms, of the UNROUNDED z)


def test_rule_2_brackets_both_neighbours_across_a_rounding_boundary():
    """z = 1 + 2^-8 exactly (a tie between 1 and 1 + 2^-7): with zdelta > 0 the reference of relu(zb) + residual spans both neighbours, a
    kernel that landed on either passes and one a further step away does not; with z well inside a rounding cell the bracket is one value."""
    a = torch.tensor([[1.0, 2.0 ** -8] + [0.0] * 6, [1.0, 0.25] + [0.0] * 6], dtype=BF)
    b = torch.ones(8, 8, dtype=BF)
    res = torch.ones(2, 8, dtype=BF)
    ref = R.gemm_ref(a, b, 2, 8, 8, lda=8, ldb=8, act=3, residual=res, zdelta=1e-6)["c"]
    assert ref.lo[0, 0] == 2.0 and ref.hi[0, 0] == 2.0 + 2.0 ** -7 and ref.lo[1, 0] == ref.hi[1, 0] == 2.25
    gate = (G.RTOL_BF16, 0.0)
    for v in (2.0, 2.0 + 2.0 ** -7):
        R.close_ref(torch.tensor([[v] * 8, [2.25] * 8], dtype=BF), ref, gate, "either neighbour")
    with pytest.raises(AssertionError):
        R.close_ref(torch.tensor([[2.0 + 2.0 ** -5] * 8, [2.25] * 8], dtype=BF), ref, gate, "two steps up")
    with pytest.raises(AssertionError):
        R.close_ref(torch.tensor([[float("nan")] * 8, [2.25] * 8], dtype=BF), ref, gate, "NaN")


# ------------------------------------------------------------------------------------------------------------------ stand-ins
def _ids(cases):
    return [c[0] for c in cases]


ALL_CASES = G.SMALL_M_CASES + G.K128_CASES + G.K256_CASES


@pytest.fixture(autouse=True)
def _strict_standin(monkeypatch):
    """the stand-in to the letter of the header (standin_ops.GEMM_STRICT): the correctly rounded fp32 sum -- the host BLAS's summation order
    is not under test -- and the small-M kernel's residual exception"""
    monkeypatch.setattr(standin_ops, "GEMM_STRICT", True)


@pytest.mark.parametrize("name,c", ALL_CASES, ids=_ids(ALL_CASES))
def test_standin_gemm_fits_the_gates(name, c):
    G.run_gemm(standin_ops, CPU, c)


@pytest.mark.parametrize("form,batch,M,N,K", G.BATCHED)
def test_standin_gemm_batched_fits_the_gates(form, batch, M, N, K):
    G.run_batched(standin_ops, CPU, form, batch, M, N, K)


def test_dispatch_restatements():
    """tail_parts / splitk128 (the tables' path names depend on them) at the shapes whose part counts the tables state"""
    assert [G.tail_parts(*s) for s in ((128, 128, 2048), (128, 128, 2112), (128, 128, 8192), (384, 256, 2048), (136, 136, 72))] == [2, 2, 8, 2, 1]
    assert [G.splitk128(128, 128, k) for k in (71, 200, 3077)] == [1, 1, 10]


def test_band_plans_of_the_table():
    """the two multi-band shapes: mpv_gemm_plan_bands (host-only) names two and three bands on 256 CUs, and one row fewer of tiles does not
    make them smaller cases of the same plan"""
    import ctypes as C

    from youku_mplug_amd import _lib
    f = _lib.lib().mpv_gemm_plan_bands
    for (name, c), want, preact, ext in G.BANDS:
        out6 = (C.c_int * 6)()
        nb = f(c["M"], c["N"], c["K"], 256, preact, ext, out6)
        assert tuple(out6[2 * i] for i in range(nb)) == want, name
        assert sum(out6[2 * i] * out6[2 * i + 1] for i in range(nb)) >= c["M"]


# ------------------------------------------------------------------------------------------------------------------ mutations
# (defect, a case of the tables that must reject it): the gates are tighter than the errors the old `max|a - b| / max|b| <= 1e-2` let through
MUTATIONS = [
    ("bf16_partials", "k128-tail-128x128x2048-plain"),            # the running sum rounded to bf16 between K-tiles
    ("act_unrounded", "k128-nt-136x136x72-erf"),                   # act(acc + bias) instead of act(bf16(acc + bias))
    ("act_unrounded", "k256-r256-nt-264x328x192-EP_TANH_PRE-deriv"),
    ("drop_last_k", "k128-tn-128x128x3077"),                        # the last reduction row dropped
    ("drop_last_k", "small_m-gen-5x16x200"),
    ("alpha_after_bias", "k128-nt-136x136x72-alpha-bias"),          # (acc + bias) * alpha
]


@pytest.mark.parametrize("mutation,name", MUTATIONS)
def test_gates_reject_the_named_defects(monkeypatch, mutation, name):
    c = dict(ALL_CASES)[name]
    G.run_gemm(standin_ops, CPU, c)
    monkeypatch.setattr(standin_ops, "GEMM_MUTATION", mutation)
    with pytest.raises(AssertionError, match="element"):
        G.run_gemm(standin_ops, CPU, c)


def test_gates_respect_the_cap():
    """no coefficient above 2^-12 of the scale (a sixteenth of a bf16 ulp of the element's sum of absolute terms)"""
    for key, (rtol, coef) in G.GATES.items():
        assert 0.0 <= coef <= G.COEF_CAP and rtol in (G.RTOL_BF16, G.RTOL_F32), key
    assert math.isclose(G.COEF_CAP, 2.0 ** -12)
