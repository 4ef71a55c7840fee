"""mpv_sim_topk / mpv_sim_rank (csrc/retrieval_search.hip) against the fp32 torch formulation: exact cases on small-integer features
(ties included), real-valued features within the summation-order bound, and the consistency of the two calls."""
import pytest
import torch

from standin_search import order as _order       # gallery indices per row by (-score, index)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SLICES = (0, 1, 3, 17)


def _ints(n, d, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-2, 3, (n, d), generator=g).to(BF).to(dev)


@pytest.mark.parametrize("D", [64, 256, 1024])
def test_topk_exact_with_ties(dev, D):
    """Entries in {-2..2} are exact in bf16 and every partial sum (|s| <= 4 D) is exact in fp32: values must match the fp32
    reference bit for bit and indices exactly, ties (many) broken by the lower index, for every slice count."""
    from youku_mplug_amd import ops
    shapes = [(1, 1), (1, 5), (7, 5), (7, 127), (65, 127), (1, 4097), (65, 4097), (7, 100003), (1, 100003)]
    if D == 1024:
        shapes = shapes[:7] + [(7, 20011)]
    for Nq, Ng in shapes:
        q, g = _ints(Nq, D, dev, 10 + Nq), _ints(Ng, D, dev, 20 + Ng % 97)
        s = q.float() @ g.float().t()
        order = _order(s)
        for k in (1, 10, 32):
            kk = min(k, Ng)
            for scale in (None, 0.25):
                ri = order[:, :kk]
                rv = torch.gather(s, 1, ri) * (1.0 if scale is None else scale)
                got = [ops.sim_topk(q, g, k, scale=scale, slices=sl) for sl in (SLICES if scale is None else (0, 5))]
                for v, i in got:
                    assert torch.equal(i[:, :kk], ri), (D, Nq, Ng, k)
                    assert torch.equal(v[:, :kk], rv), (D, Nq, Ng, k)
                    assert (i[:, kk:] == -1).all() and (v[:, kk:] == float("-inf")).all()      # Ng < k: filler
                    assert torch.equal(v, got[0][0]) and torch.equal(i, got[0][1])             # identical across slice counts
        assert Ng < 127 or (s == s[:, :1]).sum() > Nq                                          # the larger cases do contain ties


@pytest.mark.parametrize("D", [64, 256, 1024])
def test_rank_exact(dev, D):
    """sim_rank against the position read off the stable sort: one target, several targets, -1 padding, a target that ties with
    other rows (integer scores: nearly every target does; one row is forced to), and no target at all."""
    from youku_mplug_amd import ops
    for Nq, Ng in ((1, 1), (7, 5), (65, 127), (7, 4097), (65, 20011), (1, 100003)):
        q, g = _ints(Nq, D, dev, 30 + Nq), _ints(Ng, D, dev, 40 + Ng % 97)
        if Ng > 4:
            g[3] = g[1]
            g[Ng - 1] = g[1]                                          # rows 1, 3 and the last tie for every query
        s = q.float() @ g.float().t()
        order = _order(s)
        pos = torch.empty_like(order)
        pos.scatter_(1, order, torch.arange(Ng, device=dev).expand(Nq, Ng))
        gen = torch.Generator().manual_seed(Nq * 1000 + Ng)
        single = torch.randint(0, Ng, (Nq,), generator=gen).to(dev)
        multi = torch.randint(0, Ng, (Nq, 4), generator=gen).to(dev)
        multi[:, 2] = -1
        multi[0, :] = torch.tensor([Ng - 1, -1, -1, -1])              # the tied row: ranked after rows 1 and 3
        if Nq > 1:
            multi[1, :] = -1                                          # no target: Ng
        for tgt in (single, multi):
            t2 = tgt.reshape(Nq, -1)
            want = torch.where(t2 >= 0, torch.gather(pos, 1, t2.clamp(min=0)), torch.full_like(t2, Ng)).min(dim=1).values.int()
            for sl in SLICES:
                assert torch.equal(ops.sim_rank(q, g, tgt, slices=sl), want), (D, Nq, Ng, sl)
        if Ng > 4:
            assert (pos[0, Ng - 1] >= pos[0, 3]).item() and (pos[0, 3] > pos[0, 1]).item()


def _real(n, d, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1).to(BF).to(dev)


def excluded_positions(s, b, k):
    """-> (order [Nq, k + 1], compare [Nq, k] bool): position j of a query is compared only if the reference's scores at positions
    j - 1, j, j + 1 (position k = the best row left out) are more than 2 b apart, b the larger bound of the two rows involved"""
    order = _order(s)[:, :k + 1]
    sv, bv = torch.gather(s, 1, order), torch.gather(b, 1, order)
    sure = (sv[:, :-1] - sv[:, 1:]) > 2 * torch.maximum(bv[:, :-1], bv[:, 1:])           # gap j -> j + 1, j = 0 .. k - 1
    compare = sure.clone()
    compare[:, 1:] &= sure[:, :-1]
    return order, compare


@pytest.mark.parametrize("D,Ng", [(256, 100000), (64, 100000)])
def test_topk_real_features_and_rank_consistency(dev, D, Ng):
    """L2-normalised gaussian rows rounded to bf16, Nq = 512, k = 10, seeds 0 (queries) and 1 (gallery).  Every returned value is
    within b = D * 2^-24 * sum_i |q_i g_i| of the fp32 reference score of the returned row (no exclusion).  Indices are compared
    per entry where the reference order is certain (excluded_positions); the excluded share must stay under 3 %.  Measured
    from the fp32 reference alone for these seeds and sizes (host fp32 matmul): 1.23 % at D = 256, 0.20 % at D = 64.
    Then, for every query, sim_rank of the row sim_topk returned at position j is j."""
    from youku_mplug_amd import ops
    Nq, k = 512, 10
    q, g = _real(Nq, D, dev, 0), _real(Ng, D, dev, 1)
    s = q.float() @ g.float().t()
    b = D * 2.0 ** -24 * (q.float().abs() @ g.float().abs().t())
    order, compare = excluded_positions(s, b, k)
    share = 1.0 - compare.float().mean().item()
    print(f"D={D} Ng={Ng}: excluded share {100 * share:.2f} %, mean b {b.mean().item():.3e}")
    assert share <= 0.03
    vals, idx = ops.sim_topk(q, g, k)
    assert ((idx >= 0) & (idx < Ng)).all()
    err = (vals - torch.gather(s, 1, idx)).abs()
    bound = torch.gather(b, 1, idx)
    print(f"  worst value error / bound: {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    assert (vals[:, :-1] >= vals[:, 1:]).all()
    assert torch.equal(idx[compare], order[:, :k][compare])
    for sl in (1, 7):
        v2, i2 = ops.sim_topk(q, g, k, slices=sl)
        assert torch.equal(v2, vals) and torch.equal(i2, idx)
    for j in range(k):
        r = ops.sim_rank(q, g, idx[:, j].contiguous())
        assert (r == j).all(), (j, (r != j).sum().item())
