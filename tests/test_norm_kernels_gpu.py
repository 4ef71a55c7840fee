"""The LayerNorm family of csrc/norm.hip -- mpv_layernorm_fwd / _bwd (16-byte and 4-wide kernels, every instance), the deferred and
immediate parameter-gradient reductions, mpv_ln_stream_fwd(_drop) (wave-per-row and workgroup-per-row) and mpv_ln_stream_bwd --
against the fp64 references of tests/ref_norm.py, element by element, at the smallest shapes that reach each instance and edge (the
tables of tests/norm_cases.py say which).  Tolerances: norm_cases.GATES (rtol from the number format, coefficient = 2 x the residual
measured on an MI355X, per unit of the row's scale; pytest -s prints every comparison's worst residual; profiles/norm_kernel_errors.md
holds the table).  Everything called bit for bit, exact or untouched is compared on the raw bits.
Run on the MI355X box: pytest -m gpu tests/test_norm_kernels_gpu.py"""
import pytest
import torch

import norm_cases as K
import ref_norm as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _ids(runs):
    return [r[0] for r in runs]


@pytest.mark.parametrize("name,args,kw", K.LN_FWD_RUNS, ids=_ids(K.LN_FWD_RUNS))
def test_layernorm_fwd_vs_fp64(dev, name, args, kw):
    """y, mean and rstd of mpv_layernorm_fwd (see norm_cases.run_ln_fwd for what else is asserted: constant rows, padding, rows
    outside the maps, want_stats=False)."""
    from youku_mplug_amd import ops
    K.run_ln_fwd(ops, dev, *args, **kw)


@pytest.mark.parametrize("name,args,kw", K.LN_BWD_RUNS, ids=_ids(K.LN_BWD_RUNS))
def test_layernorm_bwd_vs_fp64(dev, name, args, kw):
    """dx, dgamma, dbeta and dx_drop of mpv_layernorm_bwd in every parameter-gradient mode (norm_cases.run_ln_bwd)."""
    from youku_mplug_amd import ops
    K.run_ln_bwd(ops, dev, *args, **kw)


@pytest.mark.parametrize("name,args,kw", K.STREAM_FWD_RUNS, ids=_ids(K.STREAM_FWD_RUNS))
def test_ln_stream_fwd_vs_fp64(dev, name, args, kw):
    """h_out bit for bit, y, mean and rstd of mpv_ln_stream_fwd(_drop) (norm_cases.run_stream_fwd)."""
    from youku_mplug_amd import ops
    K.run_stream_fwd(ops, dev, *args, **kw)


@pytest.mark.parametrize("name,args,kw", K.STREAM_BWD_RUNS, ids=_ids(K.STREAM_BWD_RUNS))
def test_ln_stream_bwd_vs_fp64(dev, name, args, kw):
    """dx and dx_drop of mpv_ln_stream_bwd: x read from the fp32 stream (norm_cases.run_ln_bwd, stream=True)."""
    from youku_mplug_amd import ops
    K.run_ln_bwd(ops, dev, *args, **kw)


def test_ln_stream_fwd_grid_wraps(dev):
    """65536 + 3 rows of 1024 columns: the workgroup-per-row kernel's grid is capped at 65536 and its row loop runs again."""
    from youku_mplug_amd import ops
    K.run_stream_wrap(ops, dev)


@pytest.mark.parametrize("rows,cols,p,inbf,amap", K.STREAM_DROP_EQ)
def test_ln_stream_fwd_drop_equals_predropped_addend(dev, rows, cols, p, inbf, amap):
    """mpv_ln_stream_fwd_drop == mpv_ln_stream_fwd on the addend dropped on the host with keep_mask, bit for bit in h_out, y, mean, rstd."""
    from youku_mplug_amd import ops
    K.run_stream_drop_equals_prebuilt(ops, dev, rows, cols, 1e-5, p, inbf=inbf, amap=amap)


@pytest.mark.parametrize("cols", [520, 1024])
@pytest.mark.parametrize("p", K.DROP_PS)
def test_ln_stream_fwd_drop_equals_dropping_in_the_gemm(dev, cols, p):
    """include/mpv.h: dropping `add` in the LayerNorm is bit-identical to dropping it in the epilogue of the GEMM that produced it
    (same seed, offset, shape): h_out, y, mean and rstd."""
    from youku_mplug_amd import ops
    M, Kd = 64, 64
    gen = torch.Generator().manual_seed(cols)
    a = torch.randn(M, Kd, generator=gen).to(BF).to(dev)
    w = (torch.randn(cols, Kd, generator=gen) * 0.2).to(BF).to(dev)
    h, _, gamma, beta, _ = K.stream_case(M, cols, False)
    h, gamma, beta = h.to(dev), gamma.to(dev), beta.to(dev)
    plain = ops.gemm(a, w, M, cols, Kd)
    dropped = ops.gemm(a, w, M, cols, Kd, dropout_p=p, seed=K.DROP_SEED, offset=K.DROP_OFFSET)
    assert not torch.equal(plain, dropped)
    here = ops.ln_stream_fwd(h, plain, gamma, beta, 1e-5, M, cols, add_dropout_p=p, seed=K.DROP_SEED, offset=K.DROP_OFFSET)
    there = ops.ln_stream_fwd(h, dropped, gamma, beta, 1e-5, M, cols)
    for name, u, v in zip(("y", "h_out", "mean", "rstd"), here, there):
        assert K.same_bits(u, v), f"{name} differs between dropping in the LayerNorm and in the GEMM ({M}x{cols}, p {p})"
    keep = R.keep_mask(K.DROP_SEED, K.DROP_OFFSET, M, cols, p, device=dev)
    assert K.same_bits(dropped, R.dropped_addend(plain, keep, R.drop_scale(p)).to(BF)), "the GEMM's mask is not keep_mask's"
