"""Torch stand-ins for the query-max search ops (include/mpv.h: mpv_maxsim_topk, mpv_maxsim_rank), TEST INFRASTRUCTURE ONLY, in the
manner of tests/standin_search.py: they restate the C contract -- the score of two items is the max over their rows' products, the
max taken before the scale, NaN products never win, order rule "higher score first, equal scores by the lower item index, NaN items
never" -- with plain torch on host tensors, and refuse what the ops refuse.  `install(monkeypatch)` installs standin_search first
and these on top."""
import torch

import standin_search


def _side(name, t):
    from youku_mplug_amd._lib import MpvError
    if not torch.is_tensor(t) or t.dtype != torch.bfloat16:
        raise MpvError(f"maxsim search: {name} must be bfloat16 (got {getattr(t, 'dtype', type(t))})")
    if t.dim() not in (2, 3) or t.shape[0] == 0 or t.shape[-2] == 0 or t.stride(-1) != 1:
        raise MpvError(f"maxsim search: {name} must be a non-empty [items, dim] or [items, group, dim] tensor with contiguous rows")
    return t if t.dim() == 3 else t[:, None, :]


def item_scores(q, g, dtype=torch.float32):
    """[nq, ng] item scores in `dtype`: max over both groups' rows of the row products; NaN only where every product is NaN"""
    from youku_mplug_amd._lib import MpvError
    q3, g3 = _side("queries", q), _side("gallery", g)
    if q3.shape[2] != g3.shape[2]:
        raise MpvError("maxsim search: feature widths differ")
    D = q3.shape[2]
    if D % 32 != 0 or not 32 <= D <= 1024:
        raise MpvError(f"mpv_maxsim: dim ({D}) must be a multiple of 32 in [32, 1024]")
    if q3.shape[1] > 1 and g3.shape[1] > 1:
        raise MpvError("mpv_maxsim: only one of q_group and g_group may exceed 1")
    if max(q3.shape[1], g3.shape[1]) > 1024:
        raise MpvError("mpv_maxsim: groups must be in [1, 1024]")
    p = q3.reshape(-1, D).to(dtype) @ g3.reshape(-1, D).to(dtype).t()
    p = p.view(q3.shape[0], q3.shape[1], g3.shape[0], g3.shape[1]).permute(0, 2, 1, 3).reshape(q3.shape[0], g3.shape[0], -1)
    nan = torch.isnan(p)
    s = torch.where(nan, torch.full_like(p, float("-inf")), p).max(dim=2).values
    return torch.where(nan.all(dim=2), torch.full_like(s, float("nan")), s)


def topk_of(s, k):
    """(vals, idx) of the k first items per row of the score matrix s by the order rule; NaN scores and the tail are (-inf, -1)"""
    idx = standin_search.order(s)[:, :k]                   # a stable sort of -s: NaN last
    vals = torch.gather(s, 1, idx)
    bad = torch.isnan(vals)
    vals = torch.where(bad, torch.full_like(vals, float("-inf")), vals)
    idx = torch.where(bad, torch.full_like(idx, -1), idx)
    if s.shape[1] < k:
        pad = k - s.shape[1]
        vals = torch.cat([vals, torch.full((s.shape[0], pad), float("-inf"), dtype=s.dtype)], dim=1)
        idx = torch.cat([idx, torch.full((s.shape[0], pad), -1, dtype=torch.long)], dim=1)
    return vals, idx


def rank_of(s, target):
    """int32 [nq]: min over valid, non-NaN targets of the number of items that come before the target; ng when there is none"""
    Ng = s.shape[1]
    o = standin_search.order(s)
    pos = torch.empty_like(o)
    pos.scatter_(1, o, torch.arange(Ng).expand_as(o))
    ok = (target >= 0) & (target < Ng)
    tc = target.clamp(0, Ng - 1)
    ok &= ~torch.isnan(torch.gather(s, 1, tc))
    r = torch.where(ok, torch.gather(pos, 1, tc), torch.full_like(target, Ng))
    return r.min(dim=1).values.to(torch.int32)


def maxsim_topk(q, g, k, scale=None, slices=0):
    from youku_mplug_amd._lib import MpvError
    s = item_scores(q, g)
    if not 1 <= k <= 32:
        raise MpvError(f"mpv_maxsim_topk: k ({k}) must be in [1, 32]")
    if not 0 <= slices <= 4096:
        raise MpvError(f"mpv_maxsim_topk: slices ({slices}) must be in [0, 4096]")
    return topk_of(s * (1.0 if scale is None else scale), k)


def maxsim_rank(q, g, target, slices=0):
    from youku_mplug_amd._lib import MpvError
    s = item_scores(q, g)
    if target.dtype != torch.int64:
        raise MpvError(f"maxsim_rank: target must be int64 (got {target.dtype})")
    target = target.reshape(target.shape[0], -1)
    if target.shape[0] != s.shape[0] or not 1 <= target.shape[1] <= 32:
        raise MpvError("maxsim_rank: bad target shape")
    return rank_of(s, target)


NAMES = ["maxsim_topk", "maxsim_rank"]


def install(monkeypatch):
    standin_search.install(monkeypatch)
    from youku_mplug_amd import ops
    g = globals()
    for n in NAMES:
        monkeypatch.setattr(ops, n, g[n])
