"""Torch stand-ins for the contrastive head's device entry points (include/mpv.h: mpv_maxsim_fwd, mpv_maxsim_route,
mpv_smoothed_ce), TEST INFRASTRUCTURE ONLY, in the manner of tests/standin_ops.py: each restates its C contract (bf16 operands,
fp32 arithmetic, the argmax's lowest-q tie rule) with plain torch on host tensors.  `install(monkeypatch)` installs
standin_ops first and these on top."""
import torch

import standin_ops

BF = torch.bfloat16


def maxsim_fwd(a, t, R, Q, C, E, *, alpha_dev=None, trans=False):
    A = a.float().reshape(R, Q, E)
    s = torch.einsum("rqe,ce->rcq", A, t.float().reshape(C, E))
    m = s.max(dim=-1).values
    q = torch.arange(Q, dtype=torch.int64)
    arg = torch.where(s == m[..., None], q, Q).min(dim=-1).values.to(torch.int32)       # ties: the lowest q
    sim = m * (alpha_dev.float().reshape(()) if alpha_dev is not None else 1.0)
    if trans:
        sim, arg = sim.t(), arg.t()
    return sim.contiguous(), arg.contiguous()


def maxsim_route(dsim, arg, R, Q, C, *, trans=False):
    d, a = (dsim.t(), arg.t()) if trans else (dsim, arg)
    d, a = d.reshape(R, C), a.reshape(R, C).long()
    g = torch.zeros(R, Q, C, dtype=BF)
    g.scatter_(1, a[:, None, :], d.to(BF)[:, None, :])
    return g.reshape(R * Q, C)


def smoothed_ce(sim, target, eps, scale, rows, cols, want_grad=True):
    s = sim.float().view(rows, cols)
    t = torch.full((rows, cols), eps / cols)
    t[torch.arange(rows), target.view(-1)[:rows]] += 1.0 - eps
    losses = -(torch.log_softmax(s, dim=1) * t).sum(1)
    if not want_grad:
        return losses, None, None
    g = (torch.softmax(s, dim=1) - t) * scale
    return losses, g.to(BF), (g * s).sum(1)


NAMES = ["maxsim_fwd", "maxsim_route", "smoothed_ce"]


def install(monkeypatch):
    standin_ops.install(monkeypatch)
    from youku_mplug_amd import ops
    g = globals()
    for n in NAMES:
        monkeypatch.setattr(ops, n, g[n])
