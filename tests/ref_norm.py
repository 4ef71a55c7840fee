"""Plain fp64 references of the LayerNorm family (csrc/norm.hip: mpv_layernorm_fwd / _bwd, mpv_ln_stream_fwd(_drop) / _bwd) and a
host replica of the counter-hash dropout mask, TEST INFRASTRUCTURE ONLY.  Each function is the textbook form of the operation in
float64 torch, on whatever device its inputs live on; none of them looks at tests/standin_ops.py or at the kernels' source.
tests/test_norm_refs_cpu.py checks them against F.layer_norm + autograd in fp64 and against a scalar restatement of the hash;
tests/test_norm_kernels_gpu.py compares the HIP kernels with them element by element.

Every reference also returns the SCALE of each output: the sum of the absolute values of the terms that form an element, and of that the
largest of the row (of the column for dgamma / dbeta).  The gates of tests/norm_cases.py are rtol |ref| + coefficient x scale."""
import numpy as np
import torch

from ref_loss_optim import F64, close_elementwise, f32, worst  # noqa: F401  (re-exported: the one comparison of both suites)

BF = torch.bfloat16
TINY = 1e-300


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd_ref(x, gamma, beta, eps):
    """x [rows, cols]: the bf16 or fp32 values actually given to the kernel -> (y, mean, rstd) in fp64, biased variance."""
    xv, g, b = x.to(F64), gamma.to(F64).reshape(1, -1), beta.to(F64).reshape(1, -1)
    mean = xv.mean(dim=1)
    var = ((xv - mean[:, None]) ** 2).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + float(eps))
    return (xv - mean[:, None]) * rstd[:, None] * g + b, mean, rstd


def ln_fwd_scales(x, gamma, beta, mean, rstd):
    """-> per-row scales of (y, mean, rstd).  y = x rstd gamma - mean rstd gamma + beta: three terms; mean = sum x / n: n terms;
    rstd: itself (a relative bound)."""
    xv, g, b = x.to(F64), gamma.to(F64).reshape(1, -1).abs(), beta.to(F64).reshape(1, -1).abs()
    sy = ((xv.abs() + mean.abs()[:, None]) * rstd[:, None] * g + b).max(dim=1).values
    return sy, xv.abs().mean(dim=1), rstd


def ln_bwd_ref(dy, x, gamma, mean, rstd, dres=None, dgamma0=None, dbeta0=None):
    """-> (dx, dgamma, dbeta) in fp64 from the statistics GIVEN (the fp64 ones of ln_fwd_ref, not a kernel's):
    x^ = (x - mean) rstd, g = dy gamma, dx = rstd (g - mean_row(g) - x^ mean_row(g x^)) + dres,
    dgamma = dgamma0 + sum_rows dy x^, dbeta = dbeta0 + sum_rows dy."""
    d, xv, gm = dy.to(F64), x.to(F64), gamma.to(F64).reshape(1, -1)
    xh = (xv - mean.to(F64)[:, None]) * rstd.to(F64)[:, None]
    g = d * gm
    c1, c2 = g.mean(dim=1, keepdim=True), (g * xh).mean(dim=1, keepdim=True)
    dx = rstd.to(F64)[:, None] * (g - c1 - xh * c2)
    if dres is not None:
        dx = dx + dres.to(F64)
    dg, db = (d * xh).sum(dim=0), d.sum(dim=0)
    if dgamma0 is not None:
        dg, db = dg + dgamma0.to(F64).reshape(-1), db + dbeta0.to(F64).reshape(-1)
    return dx, dg, db


def ln_bwd_scales(dy, x, gamma, mean, rstd, dres=None, dgamma0=None, dbeta0=None):
    """-> (per-row scale of dx, per-column scales of dgamma and dbeta): the terms of ln_bwd_ref with every sum taken over absolute
    values (|rstd g| + |rstd| mean|g| + |rstd x^| mean|g x^| + |dres|, the row's largest; sum |dy x^| + |dgamma0|; sum |dy| + |dbeta0|)."""
    d, xv, gm = dy.to(F64), x.to(F64), gamma.to(F64).reshape(1, -1)
    rs = rstd.to(F64)[:, None]
    xh = (xv - mean.to(F64)[:, None]) * rs
    g = (d * gm).abs()
    s = rs * (g + g.mean(dim=1, keepdim=True) + xh.abs() * (g * xh.abs()).mean(dim=1, keepdim=True))
    if dres is not None:
        s = s + dres.to(F64).abs()
    sg, sb = (d * xh).abs().sum(dim=0), d.abs().sum(dim=0)
    if dgamma0 is not None:
        sg, sb = sg + dgamma0.to(F64).reshape(-1).abs(), sb + dbeta0.to(F64).reshape(-1).abs()
    return s.max(dim=1).values, sg, sb


def close_scaled(got, ref, scale, gate, what, dim=0):
    """|got - ref| <= rtol |ref| + coef * scale for every element, scale per row (dim 0) or per column (dim 1) of a 2-D output, or
    per element of a 1-D one: both sides are divided by the scale and go through close_elementwise, whose printed residual is then
    the measured coefficient."""
    rtol, coef = gate
    s = scale.to(F64).clamp_min(TINY)
    if got.dim() == 2:
        s = s[:, None] if dim == 0 else s[None, :]
    close_elementwise(got.detach().to(F64) / s, ref.to(F64) / s, rtol, coef, what)


# ------------------------------------------------------------------------------------------------------------------ dropout
def _mul32(x, c):
    """(x * c) mod 2^32 on int64 tensors holding 32-bit values, without leaving 63 bits"""
    return (x * (c & 0xffff) + (((x * (c >> 16)) & 0xffff) << 16)) & 0xffffffff


def _mix32(x):
    """csrc/mpv_common.h mpv_mix32 on an int64 tensor (or a Python int) of 32-bit values"""
    if isinstance(x, int):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xffffffff
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xffffffff
        return x ^ (x >> 16)
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7feb352d)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846ca68b)
    return x ^ (x >> 16)


def drop_threshold(p):
    """mpv_drop_threshold: (uint32)(p * 65536.0f + 0.5f) in float arithmetic"""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def drop_scale(p):
    """1.0f / (1.0f - p) as the launchers form it, a Python float holding the fp32 value"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(seed, offset, rows, cols, p, device="cpu"):
    """bool [rows, cols], True where the element is kept: mpv_rand_pair / mpv_keep / mpv_drop_threshold of csrc/mpv_common.h with
    integer tensors.  Element index = offset + row * cols + col; the pair's counter is the even index at or below it; an even index
    takes the low 16 bits of the pair's word, an odd one the high 16 bits; kept iff that field >= thr."""
    M = 0xffffffff
    ka, kb = _mix32(seed & M), _mix32(((seed >> 32) & M) ^ 0x85ebca6b)
    idx = (offset + torch.arange(rows, dtype=torch.int64, device=device)[:, None] * cols
           + torch.arange(cols, dtype=torch.int64, device=device)[None, :])
    ctr = idx - (idx & 1)
    word = _mix32((((ctr & M) + ka) & M) ^ (((ctr >> 32) + kb) & M))
    field = torch.where((idx & 1) == 1, word >> 16, word & 0xffff)
    return field >= drop_threshold(p)


def dropped_addend(add, keep, scale):
    """the addend the stream kernel forms from `add` (bf16): bf16(add * scale) where kept, +0 elsewhere, as fp32 values"""
    v = (add.float() * torch.tensor(scale, dtype=torch.float32, device=add.device)).to(BF).float()
    return torch.where(keep, v, torch.zeros_like(v))


def stream_ref(h_in, add, keep=None, scale=1.0):
    """h_out = h_in + addend in ONE fp32 addition (both steps of the kernel are exactly reproducible: bit for bit); keep None: no dropout."""
    a = add.float() if keep is None else dropped_addend(add, keep, scale)
    return h_in.float() + a
