"""The fp64 references of tests/ref_norm.py are right, and a correct implementation fits inside the gates (no GPU).
First half: ln_fwd_ref / ln_bwd_ref against F.layer_norm + autograd in fp64, keep_mask against a scalar pure-Python restatement of
mpv_rand_pair / mpv_keep / mpv_drop_threshold (csrc/mpv_common.h), stream_ref's rounding points.
Second half: the torch stand-ins of the same entry points (tests/standin_ops.py) run over the cases of
tests/test_norm_kernels_gpu.py, through the same runners and the SAME gates (measured on the kernels)."""
import math

import pytest
import torch
import torch.nn.functional as F

import norm_cases as K
import ref_norm as R
import standin_ops

BF = torch.bfloat16
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("rows,cols,eps", [(7, 12, 1e-5), (5, 260, 1e-6), (3, 1032, 1e-5)])
def test_ln_refs_match_torch_layer_norm_and_autograd(rows, cols, eps):
    """Forward, statistics, dx (with a residual gradient), dgamma and dbeta (with a starting value) to 1e-12 of the values' scale."""
    gen = torch.Generator().manual_seed(rows * 1000 + cols)
    x = (torch.randn(rows, cols, generator=gen, dtype=torch.float64) * 3 + 2).requires_grad_(True)
    gamma = (1 + 0.1 * torch.randn(cols, generator=gen, dtype=torch.float64)).requires_grad_(True)
    beta = (0.1 * torch.randn(cols, generator=gen, dtype=torch.float64)).requires_grad_(True)
    dy, dres, dg0, db0 = (torch.randn(s, generator=gen, dtype=torch.float64) for s in ((rows, cols), (rows, cols), (cols,), (cols,)))
    y = F.layer_norm(x, (cols,), gamma, beta, eps)
    (y * dy).sum().backward()
    ry, mean, rstd = R.ln_fwd_ref(x.detach(), gamma.detach(), beta.detach(), eps)
    assert (ry - y.detach()).abs().max().item() <= 1e-12
    assert (mean - x.detach().mean(1)).abs().max().item() <= 1e-12
    assert (rstd - 1 / torch.sqrt(x.detach().var(1, unbiased=False) + eps)).abs().max().item() <= 1e-10
    dx, dg, db = R.ln_bwd_ref(dy, x.detach(), gamma.detach(), mean, rstd, dres, dg0, db0)
    assert (dx - (x.grad + dres)).abs().max().item() <= 1e-11
    assert (dg - (gamma.grad + dg0)).abs().max().item() <= 1e-11
    assert (db - (beta.grad + db0)).abs().max().item() <= 1e-11
    dx2, dg2, db2 = R.ln_bwd_ref(dy, x.detach(), gamma.detach(), mean, rstd)
    assert (dx2 - x.grad).abs().max().item() <= 1e-11 and (dg2 - gamma.grad).abs().max().item() <= 1e-11


def test_ln_scales_bound_the_outputs():
    """a scale is a sum of absolute terms: never below the magnitude of the element it belongs to"""
    gen = torch.Generator().manual_seed(3)
    x, _ = K.ln_input(9, 36, K.KINDS_F32, gen)
    gamma, beta = K.ln_params(36, gen)
    dy, dres = torch.randn(9, 36, generator=gen), torch.randn(9, 36, generator=gen)
    y, mean, rstd = R.ln_fwd_ref(x, gamma, beta, 1e-5)
    sy, smean, _ = R.ln_fwd_scales(x, gamma, beta, mean, rstd)
    dx, dg, db = R.ln_bwd_ref(dy, x, gamma, mean, rstd, dres)
    sdx, sdg, sdb = R.ln_bwd_scales(dy, x, gamma, mean, rstd, dres)
    assert (y.abs().max(1).values <= sy * (1 + 1e-12)).all() and (mean.abs() <= smean * (1 + 1e-12)).all()
    assert (dx.abs().max(1).values <= sdx * (1 + 1e-12)).all() and (dg.abs() <= sdg * (1 + 1e-12)).all() and (db.abs() <= sdb * (1 + 1e-12)).all()


def _mix32_scalar(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def _keep_scalar(seed, idx, p):
    """mpv_keep(seed, ctr, half, mpv_drop_threshold(p)) for the element with index idx, in Python integers"""
    thr = int(torch.tensor(p, dtype=torch.float32).mul(65536.0).add(0.5).item())      # fp32 arithmetic, truncated
    ctr, half = idx & ~1, idx & 1
    ka, kb = _mix32_scalar(seed & 0xffffffff), _mix32_scalar(((seed >> 32) & 0xffffffff) ^ 0x85ebca6b)
    r = _mix32_scalar((((ctr & 0xffffffff) + ka) & 0xffffffff) ^ (((ctr >> 32) + kb) & 0xffffffff))
    return ((r >> 16) if half else (r & 0xffff)) >= thr


@pytest.mark.parametrize("p", [0.1, 0.5, 0.25])
@pytest.mark.parametrize("offset", [0, K.DROP_OFFSET, (1 << 32) - 40, (5 << 32) + 1000])
def test_keep_mask_matches_scalar_restatement(p, offset):
    """7 x 52 = 364 indices per case; the offsets cross 2^32 inside the case and lie above it (the counter's high word reaches the
    hash); the seed's high half is non-zero."""
    rows, cols = 7, 52
    got = R.keep_mask(K.DROP_SEED, offset, rows, cols, p)
    want = torch.tensor([[_keep_scalar(K.DROP_SEED, offset + r * cols + c, p) for c in range(cols)] for r in range(rows)])
    assert torch.equal(got, want)
    assert not torch.equal(got, R.keep_mask(K.DROP_SEED ^ (1 << 40), offset, rows, cols, p)), "the seed's high half does nothing"
    assert R.drop_threshold(0.1) == 6554 and R.drop_threshold(0.5) == 32768


def test_keep_mask_fraction_and_stream_ref_rounding():
    keep = R.keep_mask(K.DROP_SEED, K.DROP_OFFSET, 64, 1024, 0.1)
    K.check_drop_fraction(keep, 0.1, "keep_mask")
    # the addend is rounded to bf16 BEFORE it is added, in one fp32 addition: 1 + bf16(3 * 1.1111112) = 1 + 3.328125
    add = torch.tensor([[3.0, 3.0]], dtype=BF)
    h = torch.tensor([[1.0, 1.0]])
    out = R.stream_ref(h, add, torch.tensor([[True, False]]), R.drop_scale(0.1))
    assert out.dtype == torch.float32 and out.tolist() == [[4.328125, 1.0]]
    assert R.stream_ref(h, add).tolist() == [[4.0, 4.0]]


# ------------------------------------------------------------------------------------------------------------------ stand-ins
def _ids(runs):
    return [r[0] for r in runs]


@pytest.mark.parametrize("name,args,kw", K.LN_FWD_RUNS, ids=_ids(K.LN_FWD_RUNS))
def test_standin_layernorm_fwd_fits_the_gates(name, args, kw):
    K.run_ln_fwd(standin_ops, CPU, *args, **kw)


@pytest.mark.parametrize("name,args,kw", K.LN_BWD_RUNS, ids=_ids(K.LN_BWD_RUNS))
def test_standin_layernorm_bwd_fits_the_gates(name, args, kw):
    K.run_ln_bwd(standin_ops, CPU, *args, **kw)


@pytest.mark.parametrize("name,args,kw", K.STREAM_FWD_RUNS, ids=_ids(K.STREAM_FWD_RUNS))
def test_standin_ln_stream_fwd_fits_the_gates(name, args, kw):
    K.run_stream_fwd(standin_ops, CPU, *args, **kw)


@pytest.mark.parametrize("name,args,kw", K.STREAM_BWD_RUNS, ids=_ids(K.STREAM_BWD_RUNS))
def test_standin_ln_stream_bwd_fits_the_gates(name, args, kw):
    K.run_ln_bwd(standin_ops, CPU, *args, **kw)


@pytest.mark.parametrize("rows,cols,p,inbf,amap", K.STREAM_DROP_EQ)
def test_standin_stream_drop_equals_predropped_addend(rows, cols, p, inbf, amap):
    K.run_stream_drop_equals_prebuilt(standin_ops, CPU, rows, cols, 1e-5, p, inbf=inbf, amap=amap)


def test_gates_respect_the_cap():
    """no coefficient above 2^-12 of the scale (a sixteenth of a bf16 ulp of the row's largest term)"""
    for key, (rtol, coef) in K.GATES.items():
        assert 0.0 <= coef <= K.COEF_CAP and rtol in (K.RTOL_BF16, K.RTOL_F32), key
    assert math.isclose(K.COEF_CAP, 2.0 ** -12)
