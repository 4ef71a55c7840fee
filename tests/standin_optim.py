"""Torch arithmetic of the two optimizer kernels (ops.grad_sumsq / ops.adamw_step_grouped; optim/adamw.py:66-115), TEST INFRASTRUCTURE
ONLY: tests/test_engine_cpu.py puts them in place of the kernel calls to run the real engine on CPU, and
tests/test_loss_optim_refs_cpu.py runs them against the fp64 references.  Nothing in the product imports this file."""
import math

TILE = 256


def grad_sumsq(g, out):
    out.add_(g.float().pow(2).sum())


def adamw_step_grouped(p16, master, m, v, g16, tile_group, lrs, wds, beta1, beta2, eps, step, grad_scale=1.0, sumsq=None, max_norm=0.0):
    g = g16.float() * grad_scale
    if max_norm > 0:
        norm = math.sqrt(float(sumsq)) * grad_scale
        g = g * min(1.0, max_norm / (norm + 1e-6))
    tg = tile_group.long().repeat_interleave(TILE)
    for gi, (lr, wd) in enumerate(zip(lrs, wds)):
        sel = tg == gi
        if not sel.any():
            continue
        master[sel] *= 1.0 - lr * wd
        m[sel] = beta1 * m[sel] + (1 - beta1) * g[sel]
        v[sel] = beta2 * v[sel] + (1 - beta2) * g[sel] ** 2
        denom = (v[sel].sqrt() / math.sqrt(1 - beta2 ** step)) + eps
        master[sel] -= (lr / (1 - beta1 ** step)) * m[sel] / denom
    p16.copy_(master.to(p16.dtype))
