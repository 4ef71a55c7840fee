"""fp64 reference of mpv_logits_guide (include/mpv.h), written from the contract alone: per row the two maxima,
the centred rows, g = c + (scale - 1) * (c - u) and the plausibility ban c < log(alpha), all in double precision -- no fp32 step,
no rounding to bf16.  It returns the quantities the CPU test's bound is made of; the stand-in (tests/standin_guidance.py) is the fp32
restatement that the kernel must equal bit for bit."""
import math

import torch


def guide(cond, uncond, *, scale, alpha=0.0, vocab=None):
    """cond [rows, ld_c], uncond [rows, ld_u] (bf16 or any float) -> a dict of fp64 [rows, vocab] tensors: g (the guided logits before
    rounding), c, u (the centred rows), banned (bool: c < log(alpha); all False with alpha 0) and plaus_log (a float)"""
    V = int(vocab) if vocab is not None else min(cond.shape[1], uncond.shape[1])
    x, y = cond[:, :V].to(torch.float64), uncond[:, :V].to(torch.float64)
    c = x - x.max(dim=1, keepdim=True).values
    u = y - y.max(dim=1, keepdim=True).values
    g = c + (float(scale) - 1.0) * (c - u)
    plaus_log = math.log(alpha) if alpha > 0.0 else float("-inf")
    return dict(g=g, c=c, u=u, banned=c < plaus_log, plaus_log=plaus_log)


def ulp_bf16(x):
    """the spacing of bf16 (8 significant bits) at the fp64 values x; below the smallest normal it is the subnormal spacing"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def fp32_slack(ref, scale):
    """what the three fp32 roundings on the way to g (each subtract, the multiply, the add) may move it by, per element:
    4 * 2^-24 * (|c| + |u| + |scale - 1| * |c - u|) -- each rounding is relative 2^-24 of a quantity no larger than that sum; the factor
    4 leaves room for their propagation.  It also bounds the error of c, the one quantity the plausibility ban compares."""
    c, u = ref["c"], ref["u"]
    return 4 * 2.0 ** -24 * (c.abs() + u.abs() + abs(float(scale) - 1.0) * (c - u).abs())


def bound(ref, scale):
    """what an fp32 evaluation of the contract followed by the rounding to bf16 may differ from the reference by, per element: half a
    bf16 ulp of the reference, and fp32_slack"""
    return ulp_bf16(ref["g"]) / 2 + fp32_slack(ref, scale)
