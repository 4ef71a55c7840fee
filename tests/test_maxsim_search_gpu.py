"""mpv_maxsim_topk / mpv_maxsim_rank (csrc/maxsim_search.hip) against the definition: exact-arithmetic cases that must equal the fp64
reference bit for bit (ties included), group == 1 against mpv_sim_topk / mpv_sim_rank, slice independence, built ties, NaN rows,
rank with several / unused / no targets, and random unit rows within the summation-order bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maxsim_cases as mc                      # noqa: E402
import standin_maxsim_search as sm             # noqa: E402

pytestmark = pytest.mark.gpu


def _ref_topk(q, g, k, scale=1.0):
    return sm.topk_of(sm.item_scores(q, g, torch.float64) * scale, k)


def _ref_rank(q, g, target):
    return sm.rank_of(sm.item_scores(q, g, torch.float64), target.reshape(target.shape[0], -1))


def _targets(nq, ng, seed):
    """[nq, 3]: a real target, a second one or an unused slot, an unused slot; query 0 has no valid target at all"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, ng, (nq, 3), generator=g)
    t[:, 1] = torch.where(torch.rand(nq, generator=g) < 0.5, t[:, 1], torch.full((nq,), -1))
    t[:, 2] = -1
    if nq > 1:
        t[0] = torch.tensor([-1, ng, -7])
    return t


# (side, dim, group, nq, ng, k, row stride pad, scale): the axes of the issue paired, not crossed.  ng * group is no multiple of
# 128 except where group = 256 forces it; k = 32 with ng = 5 is ng < k; group = 1 on either side is the ungrouped call.
EXACT = [
    ("g", 32, 1, 1, 37, 5, 0, 1.0),
    ("g", 160, 3, 33, 37, 32, 8, 0.5),
    ("g", 256, 32, 70, 5, 32, 0, 1.0),
    ("g", 32, 40, 33, 37, 1, 16, 4.0),
    ("g", 160, 256, 70, 5, 5, 0, 1.0),
    ("g", 256, 256, 1, 1, 1, 8, 2.0),
    ("q", 32, 3, 70, 37, 5, 8, 1.0),
    ("q", 160, 32, 33, 5, 32, 0, 0.25),
    ("q", 256, 40, 1, 37, 1, 16, 1.0),
    ("q", 160, 256, 33, 37, 32, 0, 2.0),
    ("q", 256, 1, 70, 1, 5, 8, 1.0),
]


@pytest.mark.parametrize("side,dim,group,nq,ng,k,pad,scale", EXACT)
def test_exact_cases_equal_the_fp64_definition(dev, side, dim, group, nq, ng, k, pad, scale):
    from youku_mplug_amd import ops
    qd = mc.exact_features(nq, group if side == "q" else None, dim, 7, row_stride=dim + pad, device=dev)
    gd = mc.exact_features(ng, group if side == "g" else None, dim, 8, row_stride=dim + pad, device=dev)
    assert qd.stride(-2) == dim + pad and gd.stride(-2) == dim + pad
    q, g = qd.cpu(), gd.cpu()
    rv, ri = _ref_topk(q, g, k, scale)
    vals, idx = ops.maxsim_topk(qd, gd, k, scale=scale)
    n_ties = int((rv[:, 1:] == rv[:, :-1]).sum())
    print(f"{side} dim {dim} group {group} nq {nq} ng {ng} k {k}: {n_ties} tied neighbours in the reference lists")
    assert torch.equal(idx.cpu(), ri)
    assert torch.equal(vals.cpu().double(), rv)
    t = _targets(nq, ng, 3)
    rank = ops.maxsim_rank(qd, gd, t.to(dev))
    assert rank.dtype == torch.int32 and torch.equal(rank.cpu(), _ref_rank(q, g, t))


def test_group_one_is_sim_topk_and_sim_rank_bit_for_bit(dev):
    from youku_mplug_amd import ops
    q, g = mc.unit_rows(70, None, 256, 1).to(dev), mc.unit_rows(1000, None, 256, 2).to(dev)
    t = torch.randint(0, 1000, (70, 2), generator=torch.Generator().manual_seed(3)).to(dev)
    for k, scale in ((10, None), (32, 14.285)):
        v0, i0 = ops.sim_topk(q, g, k, scale=scale)
        for qq, gg in ((q, g), (q[:, None, :], g), (q, g[:, None, :])):
            v1, i1 = ops.maxsim_topk(qq, gg, k, scale=scale)
            assert torch.equal(i0, i1) and torch.equal(v0.view(torch.int32), v1.view(torch.int32))
    assert torch.equal(ops.sim_rank(q, g, t), ops.maxsim_rank(q, g, t))


@pytest.mark.parametrize("side", ["g", "q"])
def test_slices_give_bit_identical_outputs(dev, side):
    from youku_mplug_amd import ops
    q = mc.unit_rows(33, 40 if side == "q" else None, 64, 5).to(dev)
    g = mc.unit_rows(301, 40 if side == "g" else None, 64, 6).to(dev)
    t = torch.randint(0, 301, (33, 2), generator=torch.Generator().manual_seed(4)).to(dev)
    outs = []
    for s in (0, 1, 3, 7):
        v, i = ops.maxsim_topk(q, g, 10, scale=3.0, slices=s)
        outs.append((v.view(torch.int32), i, ops.maxsim_rank(q, g, t, slices=s)))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o))


def _e(i, v, dim=32):
    r = torch.zeros(dim)
    r[i] = v
    return r


def test_ties_go_to_the_lower_item_and_a_last_row_maximum_is_found(dev):
    from youku_mplug_amd import ops
    z = torch.zeros(32)
    # gallery grouped: item 0 has its maximum at the LAST row of its group, item 1 at the first, both 0.5; item 2 scores 0.25
    g = torch.stack([torch.stack([_e(0, .25), z, _e(0, .5)]), torch.stack([_e(0, .5), _e(0, .25), z]),
                     torch.stack([_e(0, .25), z, z])]).to(torch.bfloat16)
    q = _e(0, 1.0)[None].to(torch.bfloat16)
    v, i = ops.maxsim_topk(q.to(dev), g.to(dev), 3)
    assert i.tolist() == [[0, 1, 2]] and v.tolist() == [[0.5, 0.5, 0.25]]
    assert ops.maxsim_rank(q.to(dev), g.to(dev), torch.tensor([[1]], device=dev)).tolist() == [1]
    assert ops.maxsim_rank(q.to(dev), g.flip(0).contiguous().to(dev), torch.tensor([[2]], device=dev)).tolist() == [1]
    # queries grouped: the clip's rows are e0, e1, e2; title 0 meets the LAST row, title 1 the first, both 0.5
    clip = torch.stack([_e(0, 1.0), _e(1, 1.0), _e(2, 1.0)])[None].to(torch.bfloat16)
    titles = torch.stack([_e(2, .5), _e(0, .5), _e(1, .25)]).to(torch.bfloat16)
    v, i = ops.maxsim_topk(clip.to(dev), titles.to(dev), 2)
    assert i.tolist() == [[0, 1]] and v.tolist() == [[0.5, 0.5]]
    assert ops.maxsim_rank(clip.to(dev), titles.to(dev), torch.tensor([[1, 2]], device=dev)).tolist() == [1]


@pytest.mark.parametrize("side", ["g", "q"])
def test_nan_rows(dev, side):
    """item 0 has one NaN row among finite ones: scored by the finite rows.  Item 1 is all NaN: never returned, ranked after all."""
    from youku_mplug_amd import ops
    nan = float("nan")
    grouped = mc.exact_features(4, 3, 32, 11).clone()
    single = mc.exact_features(5, None, 32, 12).clone()
    if side == "g":                                   # NaN rows in the grouped gallery
        grouped[0, 1] = nan
        grouped[1] = nan
        q, g = single, grouped
    else:                                             # a NaN row in query item 0; title 1 is NaN; query item 1 is all NaN
        grouped[0, 1] = nan
        grouped[1] = nan
        single[1] = nan
        q, g = grouped, single
    ng = g.shape[0]
    rv, ri = _ref_topk(q, g, ng)
    v, i = ops.maxsim_topk(q.to(dev), g.to(dev), ng)
    assert torch.equal(i.cpu(), ri) and torch.equal(v.cpu().double(), rv)
    assert not (i.cpu() == 1).any() and (i.cpu()[:, -1] == -1).all()            # the NaN item is never returned
    fin = torch.nan_to_num(grouped.float(), nan=-9.0)                           # item 0's score is that of its finite rows
    if side == "g":
        want0 = (single.float() @ fin[0, [0, 2]].t()).max(dim=1).values
        got0 = torch.stack([v.cpu()[r][i.cpu()[r] == 0] for r in range(v.shape[0])]).flatten()
        assert torch.equal(got0, want0)
    else:
        assert torch.isinf(v.cpu()[1]).all()                                    # the all-NaN query item finds nothing
        assert torch.equal(v.cpu()[0, 0], (fin[0, [0, 2]] @ single[[0, 2, 3, 4]].float().t()).max())
    t = torch.tensor([[1, -1], [0, 1], [2, -1], [1, 1], [3, 0]])[:q.shape[0]]
    rank = ops.maxsim_rank(q.to(dev), g.to(dev), t.to(dev)).cpu()
    assert torch.equal(rank, _ref_rank(q, g, t))
    assert rank[0] == ng                                                        # the NaN target counts as no target


def test_random_unit_rows_within_the_summation_bound(dev):
    from youku_mplug_amd import ops
    seed = mc.pick_seed()
    print("unit-row seed", seed)
    assert seed is not None, "no seed without near-ties among the 32"
    D = mc.UNIT_SHAPE["dim"]
    bound = D * 2.0 ** -24 * 1.01
    for q, g in mc.unit_case(seed):
        rv, ri = _ref_topk(q, g, 5)
        v, i = ops.maxsim_topk(q.to(dev), g.to(dev), 5)
        err = (v.cpu().double() - rv).abs().max().item()
        print(f"max |fp32 - fp64| {err:.3e} (bound {bound:.3e})")
        assert torch.equal(i.cpu(), ri)
        assert err <= bound
        t = _targets(q.shape[0], g.shape[0], 9)
        assert torch.equal(ops.maxsim_rank(q.to(dev), g.to(dev), t.to(dev)).cpu(), _ref_rank(q, g, t))
