"""Plain fp64 references of the kernels that end a training step (loss, retrieval head, optimizer), TEST INFRASTRUCTURE ONLY.
Each function is the textbook form of the operation in float64 torch, on whatever device its inputs live on; none of them looks
at tests/standin_ops.py or at the kernels' source, so an error shared by those two does not hide here.
tests/test_loss_optim_refs_cpu.py checks these references against torch's own implementations (torch.optim.AdamW,
F.cross_entropy, explicit loops); tests/test_loss_optim_kernels_gpu.py compares the HIP kernels with them element by element.
"""
import math

import torch

F64 = torch.float64


def f32(x):
    """x as the C ABI hands it to a kernel: rounded to float.  The references take the hyper-parameters the kernels were given, so that
    what is measured is the kernels' arithmetic and not the quantisation of the arguments (float(0.999) makes 1 - beta2 differ from
    0.001 by 4.7e-5 of itself: a property of the float ABI, noted in profiles/loss_optim_kernel_errors.md)."""
    if isinstance(x, (list, tuple)):
        return type(x)(f32(v) for v in x)
    return float(torch.tensor(float(x), dtype=torch.float32).item())


def worst(got, ref, rtol):
    """-> (flat index, |got - ref|, residual |got - ref| - rtol |ref|) of the element with the largest residual; a non-finite
    difference (NaN / inf on one side only) counts as an infinite residual."""
    got, ref = got.detach().to(F64).reshape(-1), ref.detach().to(F64).reshape(-1)
    assert got.shape == ref.shape, f"shape mismatch: {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    same_inf = torch.isinf(got) & torch.isinf(ref) & (got == ref)
    err = torch.where(same_inf, torch.zeros_like(err), err)
    res = err - rtol * torch.where(same_inf, torch.zeros_like(ref), ref.abs())
    res = torch.where(torch.isfinite(res), res, torch.full_like(res, math.inf))
    i = int(res.argmax().item())
    return i, float(err[i].item()), float(res[i].item())


def close_elementwise(got, ref, rtol, atol, what):
    """Every element must satisfy |got - ref| <= rtol * |ref| + atol.  Prints the worst residual (so a run with -s is also a
    measurement) and, on failure, names the worst element: its index, both values, its error and its allowance."""
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs reference {tuple(ref.shape)}"
    if got.numel() == 0:
        return
    i, err, res = worst(got, ref, rtol)
    g, r = float(got.detach().reshape(-1)[i].item()), float(ref.detach().reshape(-1)[i].item())
    print(f"[elementwise] {what}: worst residual |got - ref| - {rtol:.3e} |ref| = {res:.3e} (atol {atol:.3e}) at got {g!r} ref {r!r}")
    if not res <= atol:
        idx = tuple(int(k) for k in torch.unravel_index(torch.tensor(i), tuple(got.shape))) if got.dim() else ()
        raise AssertionError(f"{what}: element {idx} got {g!r} reference {r!r}: |diff| {err:.3e} > {rtol:.3e} * |ref| + {atol:.3e} "
                             f"= {rtol * abs(r) + atol:.3e}")


# ------------------------------------------------------------------------------------------------------------------ AdamW
def adamw_ref(master, m, v, g, group, lrs, wds, betas, eps, step, grad_scale=1.0, sumsq=None, max_norm=0.0):
    """One decoupled-weight-decay Adam step in fp64 -> (master, m, v), inputs untouched.
    group: integer id per ELEMENT; element i uses lrs[group[i]] / wds[group[i]], an id >= 8 leaves the element as it is (whatever
    its gradient holds).  The gradient is g * grad_scale, times the clip coefficient max_norm / (sqrt(sumsq) * grad_scale + 1e-6)
    when max_norm > 0, sumsq is given and that coefficient is below 1."""
    b1, b2 = betas
    p0, m0, v0 = master.to(F64), m.to(F64), v.to(F64)
    group = group.to(torch.int64)
    live = group < 8
    gid = torch.where(live, group, torch.zeros_like(group))
    lr = torch.tensor([float(x) for x in lrs], dtype=F64, device=p0.device)[gid]
    wd = torch.tensor([float(x) for x in wds], dtype=F64, device=p0.device)[gid]
    gs = float(grad_scale)
    if sumsq is not None and max_norm > 0:
        coef = float(max_norm) / (math.sqrt(float(sumsq)) * float(grad_scale) + 1e-6)
        if coef < 1.0:
            gs *= coef
    gg = torch.where(live, g.to(F64), torch.zeros_like(p0)) * gs          # (a dead element's gradient may be NaN: never read)
    p1 = p0 * (1.0 - lr * wd)
    m1 = b1 * m0 + (1.0 - b1) * gg
    v1 = b2 * v0 + (1.0 - b2) * gg * gg
    denom = v1.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    p1 = p1 - lr / (1.0 - b1 ** step) * m1 / denom
    return torch.where(live, p1, p0), torch.where(live, m1, m0), torch.where(live, v1, v0)


# ------------------------------------------------------------------------------------------------------------------ cross-entropy
def ce_ref(logits, labels, weight=None):
    """logits [rows, V] (any float type), labels int64 [rows], weight [rows] or None (= ones)
    -> (losses [rows], dlogits [rows, V] = (softmax - onehot) * weight, loss_sum = sum losses * weight), all fp64.
    A label outside [0, V) gives a zero loss and a zero gradient row."""
    x = logits.to(F64)
    rows, V = x.shape
    ok = (labels >= 0) & (labels < V)
    w = torch.ones(rows, dtype=F64, device=x.device) if weight is None else weight.to(F64)
    mx = x.max(dim=1, keepdim=True).values
    ex = (x - mx).exp()
    se = ex.sum(dim=1, keepdim=True)
    lse = (mx + se.log()).squeeze(1)
    safe = torch.where(ok, labels, torch.zeros_like(labels))
    losses = torch.where(ok, lse - x.gather(1, safe[:, None]).squeeze(1), torch.zeros_like(lse))
    onehot = torch.zeros_like(x)
    onehot.scatter_(1, safe[:, None], 1.0)
    d = (ex / se - onehot) * (w * ok.to(F64))[:, None]
    return losses, d, (losses * w).sum()


# ------------------------------------------------------------------------------------------------------------------ retrieval head
def soft_target_ce_ref(sim, row_ids, col_ids, scale):
    """targets[i][j] = [row_ids[i] == col_ids[j]] / count_i; losses[i] = -sum_j log_softmax(sim_i)[j] targets[i][j];
    dsim = d(scale * sum_i losses[i]) / d sim, by autograd; dts[i] = sum_j dsim[i][j] sim[i][j].  All fp64."""
    s = sim.detach().to(F64).clone().requires_grad_(True)
    t = (row_ids.reshape(-1, 1) == col_ids.reshape(1, -1)).to(F64)
    t = t / t.sum(dim=1, keepdim=True)
    losses = -(torch.log_softmax(s, dim=1) * t).sum(dim=1)
    (dsim,) = torch.autograd.grad(losses.sum() * float(scale), s)
    return losses.detach(), dsim, (dsim * s.detach()).sum(dim=1)


def l2norm_ref(x, dy=None, eps=1e-12):
    """F.normalize(x, dim=-1, eps) in fp64 -> (y, norm = max(||x||, eps), dx); dx (None without dy) is the autograd gradient of
    sum(y * dy) with respect to x."""
    xv = x.detach().to(F64).clone().requires_grad_(True)
    y = torch.nn.functional.normalize(xv, p=2.0, dim=-1, eps=eps)
    norm = xv.detach().norm(dim=-1).clamp_min(eps)
    dx = None
    if dy is not None:
        (dx,) = torch.autograd.grad((y * dy.to(F64)).sum(), xv)
    return y.detach(), norm, dx
