"""Plain fp64 reference of the bf16 GEMM family (csrc/gemm.hip, csrc/gemm256.hip: mpv_gemm_bf16 / mpv_gemm_bf16_batched) as
include/mpv.h documents it, TEST INFRASTRUCTURE ONLY.  One function, gemm_ref, restates every operand form, leading dimension, row map
and epilogue option in float64 torch on whatever device its inputs live on; it looks neither at tests/standin_ops.py nor at the kernels'
source.  tests/test_gemm_refs_cpu.py checks it against an independent einsum / gather formulation; tests/test_gemm_kernels_gpu.py
compares the HIP kernels with it element by element.

Every output comes with its SCALE per element: the sum of the absolute terms that enter it,
    z, c, deriv:  |alpha| sum_k |a||b| + |bias|  (x |act'(z)| or the dropout scale where the epilogue multiplies) + |residual| + |C_old|
    colsum:       sum_k |a|
The gates of tests/gemm_cases.py are rtol |ref| + coefficient x scale.

THE DOCUMENTED EPILOGUE.  acc is the fp32 sum.  z = acc * alpha + bias; zb = bf16(z) (columns below colscale_cols: bf16(zb * colscale));
row_tap_out <- zb; preact_out <- zb, or bf16(act'(zb)) with preact_deriv; v = act(zb); v *= act'(act_bwd_z) (or act_bwd_z itself:
ACT_DERIV); v = dropout(v); v += residual; v += C_old; C <- bf16(v).  An fp32 output is acc * alpha (+ C_old) with no rounding.
The one documented exception (include/mpv.h, residual): the small-M forward kernel without an activation forms bf16(z + residual) from
the unrounded z (residual_on_fp32).

ROUNDING TIES.  zb is an intermediate ROUNDING: the kernel rounds its fp32 z, the reference would round the fp64 z, and where the two sit
on either side of a rounding boundary the two zb are neighbours -- a whole bf16 step that no accumulation allowance covers.  Each output
states how it is compared:
    z (a plain bf16 C, row_tap_out, preact_out without preact_deriv)  against the fp64 z directly: ONE rounding, the gate's rtol.
    c behind an intermediate, WHERE the kernel also emitted zb (preact_out without preact_deriv): rule 1 -- z is gated as above, and c is
      compared with the fp64 epilogue of THE KERNEL'S OWN zb bits (z_from).
    c behind an intermediate that the kernel did not emit, deriv, the colscale columns: rule 2 -- the kernel's fp32 z lies within
      d = zdelta x scale of the fp64 z (gemm_cases.ZDELTA: the worst case of the fp32 accumulation), rounding is monotone,
      so the kernel's zb lies in [bf16(z - d), bf16(z + d)]: almost always one value, across a boundary the two neighbours.  The output
      is accepted if it is within its gate of the fp64 epilogue of any zb in that interval: Ref.lo / Ref.hi bracket those references,
      and close_ref measures the distance to the bracket.

THE GELU' POLYNOMIALS.  csrc/mpv_common.h evaluates GELU' as 1/2 + x Q(x^2) on x clamped to [-4, 4] and documents its absolute error: 1.1e-4
inside the clamp, 5e-4 beyond it (the frozen tail value).  Exactly: left of -4 the true GELU' runs from GELU'(-4) = -5.03e-4 (erf; -3.3e-4
tanh) up to 0 while the kernel stays at its value for -4, which is GELU'(-4) -+ the inside error: at most 5.03e-4 + 7.4e-5 = 5.8e-4.  That is
an approximation the project chose, not an accumulation error, and no multiple of the product's scale describes it: the brackets of deriv
and of a C behind an EVALUATED derivative (act_bwd erf / tanh) are widened by it -- BWD_APPROX = 5.8e-4 per unit of the value it multiplies.
The tanh flavour of preact_deriv comes from the OTHER form there (mpv_gelu_tanh_both_t: 1/2 + s + x / 2 (1 - 4 s^2) u'(x) on the forward polynomial s, documented error ds = 2.8e-5), for which the file
states no bound; derived here: |d deriv| <= ds + |x| u'(x) 4 |s| ds <= 2.8e-5 (1 + 4 x 2.51 x 2) = 5.9e-4 inside the clamp, plus the
frozen tail |GELU'_tanh(-4)| = 3.3e-4 beyond it: 9.2e-4."""
from dataclasses import dataclass

import torch

from ref_loss_optim import F64, close_elementwise
from ref_norm import drop_scale, keep_mask

BF = torch.bfloat16
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_RELU, ACT_DERIV = 0, 1, 2, 3, 4
TINY = 1e-300
BWD_APPROX = 5.8e-4                                       # module text: the error of the GELU' polynomial, tail included
DERIV_APPROX = {ACT_GELU_ERF: 5.8e-4, ACT_GELU_TANH: 9.2e-4}


@dataclass
class Ref:
    lo: torch.Tensor        # fp64; lo == hi wherever the reference is a single value
    hi: torch.Tensor
    scale: torch.Tensor


def map_rows(m, n, device="cpu"):
    g, s, o = m
    r = torch.arange(n, dtype=torch.int64, device=device)
    return r if g == 0 else (r // g) * s + (r % g) + o


def rbf(x):
    """fp64 -> the nearest bf16 value (ties to even), as fp64, in ONE rounding (a cast through fp32 would round twice).  Normal range only."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0), e - 8)


def act64(z, kind):
    if kind == ACT_GELU_ERF:
        return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))
    if kind == ACT_GELU_TANH:
        return 0.5 * z * (1.0 + torch.tanh(0.7978845608028654 * (z + 0.044715 * z ** 3)))
    assert kind == ACT_RELU
    return z.clamp_min(0.0)


def act_grad64(z, kind):
    if kind == ACT_GELU_ERF:
        return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327
    if kind == ACT_GELU_TANH:
        u = 0.7978845608028654 * (z + 0.044715 * z ** 3)
        t = torch.tanh(u)
        return 0.5 * (1.0 + t) + 0.5 * z * (1.0 - t * t) * 0.7978845608028654 * (1.0 + 3.0 * 0.044715 * z * z)
    assert kind == ACT_RELU
    return (z > 0).to(F64)


def gemm_ref(a, b, M, N, K, *, trans_a=False, trans_b=False, lda, ldb, amap=(0, 0, 0), cmap=(0, 0, 0), kmap=(0, 0, 0), bias=None, act=0,
             preact_deriv=False, residual=None, act_bwd_z=None, act_bwd=0, drop=None, alpha=1.0, alpha_dev=None, out_f32=False, c_old=None,
             colscale=None, want_colsum=False, zdelta=0.0, z_from=None, residual_on_fp32=False):
    """a, b: the 2-D [rows, ld] buffers the kernel is given (lda / ldb == their row pitch); residual / c_old: [*, ld] buffers laid out
    through cmap; act_bwd_z: [>= M, ldz], rows NOT mapped; bias: [>= N]; drop = (p, seed, offset), element index offset + m * N + n with m
    the row NUMBER; c_old: the prior contents of C (accumulate); z_from: the kernel's own zb [M, N] (rule 1 of the module text).
    -> dict of Ref over [M, N] (colsum: [M]): "z" always (the value before the activation: what row_tap_out / a non-derivative preact_out
    hold), "c", "deriv" with preact_deriv, "colsum" with want_colsum."""
    dev = a.device
    assert a.shape[1] == lda and b.shape[1] == ldb and not (trans_a and not trans_b)
    kr, cr = map_rows(kmap, K, dev), map_rows(cmap, M, dev)
    A = a[kr, :M].to(F64).t() if trans_a else a[map_rows(amap, M, dev), :K].to(F64)          # [M, K]
    B = b[kr, :N].to(F64) if trans_b else b[:N, :K].to(F64).t()                            # [K, N]
    al = float(alpha) * (float(alpha_dev.to(F64).item()) if alpha_dev is not None else 1.0)
    z = (A @ B) * al
    sz = (A.abs() @ B.abs()) * abs(al)
    if bias is not None:
        z, sz = z + bias[:N].to(F64)[None, :], sz + bias[:N].to(F64).abs()[None, :]
    out = {}
    if want_colsum:
        out["colsum"] = Ref(A.sum(1), A.sum(1), A.abs().sum(1))
    old = c_old[cr, :N].to(F64) if c_old is not None else None
    if out_f32:
        c, sc = (z + old, sz + old.abs()) if old is not None else (z, sz)
        out["z"] = out["c"] = Ref(c, c, sc)
        return out
    out["z"] = Ref(z, z, sz)
    only_z = not (act or act_bwd or drop or residual is not None or old is not None or colscale)
    if only_z:
        out["c"] = out["z"]
        return out
    if residual_on_fp32 and residual is not None and not (act or act_bwd or drop or old is not None or colscale):
        r = residual[cr, :N].to(F64)          # mpv.h, residual: the small-M kernel's exception -- ONE rounding of z + residual
        out["c"] = Ref(z + r, z + r, sz + r.abs())
        return out
    if z_from is not None:
        zs = [z_from.to(F64)]
    else:
        d = zdelta * sz
        zs = [rbf(z - d), rbf(z + d)]
    if colscale:
        nc, s = colscale
        s = float(torch.tensor(s, dtype=torch.float32).item())
        zs = [torch.cat([rbf(t[:, :nc] * s), t[:, nc:]], 1) for t in zs]
        sz = torch.cat([sz[:, :nc] * abs(s), sz[:, nc:]], 1)
    # the bracket's ends are the only bf16 values in it when they are the same or adjacent; where heavy cancellation makes d exceed a bf16
    # step of z there are values between them, and GELU / GELU' are not monotone: every one of them is then within L x width / 2 of the
    # ends' references (L: the Lipschitz constant, 1.13 for GELU and 1 for GELU'), carried as `slack` through the multiplications below
    w = zs[-1] - zs[0]
    wide = torch.where(w > torch.ldexp(torch.ones_like(w), torch.frexp(torch.maximum(zs[0].abs(), zs[-1].abs()))[1] - 8), 0.5 * w, torch.zeros_like(w))
    slack = torch.zeros_like(z)
    if preact_deriv:
        ds = [act_grad64(t, act) for t in zs]
        e = wide + DERIV_APPROX[act]
        out["deriv"] = Ref(torch.minimum(ds[0], ds[-1]) - e, torch.maximum(ds[0], ds[-1]) + e, sz)
    vs, sc = zs, sz
    if act:
        vs = [act64(t, act) for t in vs]
        slack = wide * (0.0 if act == ACT_RELU else 1.13)
    if act_bwd:
        zz = act_bwd_z[:M, :N].to(F64)
        mul = zz if act_bwd == ACT_DERIV else act_grad64(zz, act_bwd)
        slack = slack * mul.abs()
        if act_bwd in (ACT_GELU_ERF, ACT_GELU_TANH):          # the epilogue EVALUATES GELU': its documented approximation, per unit of v
            slack = slack + torch.maximum(vs[0].abs(), vs[-1].abs()) * BWD_APPROX
            sc = sc * (1.0 + BWD_APPROX / mul.abs().clamp_min(TINY))          # (the allowance is a term of the element like any other)
        vs, sc = [t * mul for t in vs], sc * mul.abs()
    if drop:
        p, seed, offset = drop
        keep, ds = keep_mask(seed, offset, M, N, p, device=dev), drop_scale(p)
        vs, sc = [torch.where(keep, t * ds, torch.zeros_like(t)) for t in vs], torch.where(keep, sc * ds, torch.zeros_like(sc))
        slack = torch.where(keep, slack * ds, torch.zeros_like(slack))
    if residual is not None:
        r = residual[cr, :N].to(F64)
        vs, sc = [t + r for t in vs], sc + r.abs()
    if old is not None:
        vs, sc = [t + old for t in vs], sc + old.abs()
    out["c"] = Ref(torch.minimum(vs[0], vs[-1]) - slack, torch.maximum(vs[0], vs[-1]) + slack, sc)
    return out


def close_ref(got, ref, gate, what):
    """|got - r| <= rtol |r| + coef * scale for every element, r the point of [ref.lo, ref.hi] nearest to got (the reference itself where
    lo == hi).  Both sides are divided by the scale and go through close_elementwise, whose printed residual is then the measured
    coefficient."""
    rtol, coef = gate
    g = got.detach().to(F64)
    assert tuple(g.shape) == tuple(ref.lo.shape), f"{what}: shape {tuple(g.shape)} vs reference {tuple(ref.lo.shape)}"
    r = torch.where(torch.isfinite(g), torch.minimum(torch.maximum(g, ref.lo), ref.hi), ref.lo)
    s = ref.scale.clamp_min(TINY)
    close_elementwise(g / s, r / s, rtol, coef, what)
