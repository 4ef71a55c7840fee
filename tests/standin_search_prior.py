"""Torch stand-ins for the searches with per-row priors and the bank pass (include/mpv.h, "Searches with per-row priors":
mpv_sim_*_prior, mpv_sim_*_prior_q8, mpv_sim_bank_lse*), TEST INFRASTRUCTURE ONLY, in the manner of tests/standin_search.py.  They
restate the contract in plain torch on host tensors:
  score      fl(fl(scale * s) + prior[g]) with s the fp32 product of the bf16 rows -- a multiplication, then an addition;
  eligible   a row whose score is NaN or -inf is never returned, beats nothing, and as a target is no target;
  order      higher score first, equal scores by the lower index; fewer than k eligible rows -> the (-inf, -1) tail;
  rank       under the same scores, `scale` applied;
  lse        log sum_b exp(beta * s(b, g)), here torch.logsumexp in fp32 (stable for any finite beta).
`install(monkeypatch)` installs standin_search_q8 (and with it the plain search stand-ins and standin_ops) and these on top."""
import torch

import standin_search
import standin_search_q8

NEG_INF = float("-inf")


def _prior(what, g, prior):
    from youku_mplug_amd._lib import MpvError
    if not torch.is_tensor(prior) or prior.dtype != torch.float32 or tuple(prior.shape) != (g.shape[0],) or not prior.is_contiguous():
        raise MpvError(f"{what}: prior must be a contiguous float32 tensor of shape ({g.shape[0]},)")
    return prior


def scores(q, g, prior, scale=None):
    """fp32 [Nq, Ng]: the two separately rounded operations of the contract"""
    s = (q.float() @ g.float().t()) * torch.tensor(1.0 if scale is None else float(scale), dtype=torch.float32)
    return s + prior[None, :]


def eligible_order(s):
    """-> (order [Nq, Ng], count [Nq]): per query the rows by (-score, index) with the rows that are not eligible (NaN, -inf) moved
    behind all others, and the number of eligible rows"""
    ok = s > NEG_INF                                   # False for NaN and for -inf
    key = torch.where(ok, -s, torch.full_like(s, float("inf")))
    return torch.sort(key, dim=1, stable=True).indices, ok.sum(dim=1)


def topk_from_scores(s, k):
    order, count = eligible_order(s)
    nq, ng = s.shape
    idx = order[:, :k]
    vals = torch.gather(s, 1, idx)
    if ng < k:
        vals = torch.cat([vals, torch.full((nq, k - ng), NEG_INF, dtype=s.dtype, device=s.device)], dim=1)
        idx = torch.cat([idx, torch.full((nq, k - ng), -1, dtype=torch.long, device=s.device)], dim=1)
    tail = torch.arange(k, device=s.device)[None, :] >= count[:, None]
    return torch.where(tail, torch.full_like(vals, NEG_INF), vals), torch.where(tail, torch.full_like(idx, -1), idx)


def rank_from_scores(s, target):
    nq, ng = s.shape
    target = target.reshape(nq, -1)
    order, _ = eligible_order(s)
    pos = torch.empty_like(order)
    pos.scatter_(1, order, torch.arange(ng, device=s.device).expand_as(order))
    inside = (target >= 0) & (target < ng)
    t = target.clamp(0, ng - 1)
    ok = inside & (torch.gather(s, 1, t) > NEG_INF)
    r = torch.where(ok, torch.gather(pos, 1, t), torch.full_like(t, ng))
    return r.min(dim=1).values.to(torch.int32)


def sim_topk_prior(q, g, prior, k, scale=None, slices=0):
    from youku_mplug_amd._lib import MpvError
    standin_search._check(q, g)
    if not 1 <= k <= 32:
        raise MpvError(f"mpv_sim_topk_prior: k ({k}) must be in [1, 32]")
    return topk_from_scores(scores(q, g, _prior("sim_topk_prior", g, prior), scale), k)


def sim_rank_prior(q, g, prior, target, scale=None, slices=0):
    from youku_mplug_amd._lib import MpvError
    standin_search._check(q, g)
    if target.dtype != torch.int64:
        raise MpvError(f"sim_rank_prior: target must be int64 (got {target.dtype})")
    target = target.reshape(target.shape[0], -1)
    if target.shape[0] != q.shape[0] or not 1 <= target.shape[1] <= 32:
        raise MpvError("sim_rank_prior: bad target shape")
    return rank_from_scores(scores(q, g, _prior("sim_rank_prior", g, prior), scale), target)


def sim_topk_prior_q8(q, codes, g_scale, prior, k, scale=None, slices=0):
    return sim_topk_prior(q, standin_search_q8._gallery("sim_topk_prior_q8", codes, g_scale, (2,)), prior, k, scale=scale)


def sim_rank_prior_q8(q, codes, g_scale, prior, target, scale=None, slices=0):
    return sim_rank_prior(q, standin_search_q8._gallery("sim_rank_prior_q8", codes, g_scale, (2,)), prior, target, scale=scale)


def sim_bank_lse(bank, g, beta):
    from youku_mplug_amd._lib import MpvError
    standin_search._check(bank, g)
    if not torch.isfinite(torch.tensor(float(beta))):
        raise MpvError("mpv_sim_bank_lse: beta must be finite")
    # one matrix-vector product per gallery row: the same arithmetic whatever else is in the gallery, as the contract demands
    # (lse[g] is a function of the bank, beta and row g alone, bit for bit) -- a blocked matrix product does not promise that
    bf = bank.float()
    x = torch.stack([torch.mv(bf, row) for row in g.float()], dim=1) * torch.tensor(float(beta), dtype=torch.float32)
    return torch.stack([torch.logsumexp(x[:, j], dim=0) for j in range(x.shape[1])])


def sim_bank_lse_q8(bank, codes, g_scale, beta):
    return sim_bank_lse(bank, standin_search_q8._gallery("sim_bank_lse_q8", codes, g_scale, (2,)), beta)


NAMES = ["sim_topk_prior", "sim_rank_prior", "sim_topk_prior_q8", "sim_rank_prior_q8", "sim_bank_lse", "sim_bank_lse_q8"]


def install(monkeypatch):
    standin_search_q8.install(monkeypatch)
    from youku_mplug_amd import ops
    g = globals()
    for n in NAMES:
        monkeypatch.setattr(ops, n, g[n])
