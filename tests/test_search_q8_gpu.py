"""mpv_sim_*_q8 / mpv_maxsim_*_q8 (include/mpv.h, "Searches over an FP8 gallery") on the GPU.  The whole gate is equality with an
existing, tested kernel: every comparison is torch.equal of (values, indices) or of ranks between the _q8 op on (codes, scales) and
the bf16 op on the dequantised gallery deq(code) * scale -- no tolerance anywhere.  The inputs are built so that a kernel that
ignores or misplaces a scale cannot pass: the rows are multiplied by per-row factors 2^-6 .. 2^3 before they are quantised (the
neighbouring rows of one tile carry different exponents), and the queries are not unit rows.  The quantiser of the inputs is the
torch restatement of the contract (tests/standin_w8.py); ops.quantize_rows_e4m3 itself is what the index tests go through."""
import ctypes

import pytest
import torch

import maxsim_cases as mc
import standin_search_q8 as sq
import standin_w8

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FACTORS = 2.0 ** torch.arange(-6, 4).float()          # 2^-6 .. 2^3


def _rows(n, dim, seed):
    """bf16 [n, dim]: random unit rows times a per-row power of two that changes from row to row"""
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=1)
    f = FACTORS[(torch.arange(n) * 7 + seed) % len(FACTORS)]
    return (x * f[:, None]).to(BF)


def _queries(n, dim, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, dim, generator=g) * 3).to(BF).to(dev)


def _pitched(codes, pitch, dev):
    """the codes [.., dim] as a view of device storage whose rows are `pitch` codes apart (the gap holds 0x7F, a NaN code)"""
    dim = codes.shape[-1]
    store = torch.full((codes.numel() // dim, pitch), 0x7F, dtype=torch.uint8)
    store[:, :dim] = codes.reshape(-1, dim)
    store = store.to(dev)
    return store[:, :dim] if codes.dim() == 2 else store.view(codes.shape[0], codes.shape[1], pitch)[:, :, :dim]


def _gallery(rows, dev, pitch=None):
    """bf16 rows [.., dim] -> (codes on the device at row pitch dim + 16, scales [..], the dequantised bf16 gallery)"""
    dim = rows.shape[-1]
    codes, scale = standin_w8.quantize_rows_e4m3(rows.reshape(-1, dim).contiguous())
    codes, scale = codes.view(rows.shape), scale.view(rows.shape[:-1])
    return _pitched(codes, pitch or dim + 16, dev), scale.to(dev), sq.dequantize(codes, scale).to(dev)


def _same(got, want, what):
    assert torch.equal(got[1], want[1]), what
    assert torch.equal(got[0], want[0]), what


# ------------------------------------------------------------------------------------------------ sim
@pytest.mark.parametrize("dim", [32, 160, 256, 1024])
def test_sim_q8_equals_bf16_on_the_dequantised_gallery(dev, dim):
    """dim: a partial chunk / chunk + partial chunk / two chunks / the maximum; ng: tile and 128-row super-tile edges; ng < k: the
    tail (-inf, -1); every slice count; row pitch dim + 16"""
    from youku_mplug_amd import ops
    for ng in (1, 31, 33, 133):
        codes, scale, deq = _gallery(_rows(ng, dim, 100 + ng), dev)
        assert codes.stride(0) == dim + 16 and len(set(scale.tolist())) > min(ng, 3) - 1
        for nq in (1, 33):
            q = _queries(nq, dim, 200 + nq, dev)
            gen = torch.Generator().manual_seed(ng * 100 + nq)
            target = torch.randint(0, ng, (nq, 3), generator=gen).to(dev)
            target[:, 1] = -1
            target[0, 0] = ng - 1
            for slices in (0, 1, 3):
                for k in (1, 10, 32):
                    got = ops.sim_topk_q8(q, codes, scale, k, scale=0.5 if k == 10 else None, slices=slices)
                    want = ops.sim_topk(q, deq, k, scale=0.5 if k == 10 else None, slices=slices)
                    _same(got, want, (dim, ng, nq, k, slices))
                    if ng < k:
                        assert (got[1][:, ng:] == -1).all() and (got[0][:, ng:] == float("-inf")).all()
                    assert (got[1][:, :min(k, ng)] >= 0).all()
                assert torch.equal(ops.sim_rank_q8(q, codes, scale, target, slices=slices), ops.sim_rank(q, deq, target, slices=slices)), \
                    (dim, ng, nq, slices)


def test_sim_q8_scales_matter_on_this_data(dev):
    """the inputs do tell a kernel that drops the scales apart: the search of the bare codes gives other indices"""
    from youku_mplug_amd import ops
    codes, scale, deq = _gallery(_rows(133, 256, 1), dev)
    q = _queries(33, 256, 2, dev)
    bare = ops.sim_topk(q, codes.contiguous().view(torch.float8_e4m3fn).float().to(BF), 10)
    assert not torch.equal(bare[1], ops.sim_topk_q8(q, codes, scale, 10)[1])


def test_sim_q8_special_galleries(dev):
    from youku_mplug_amd import ops
    dim, ng = 256, 133
    q = _queries(33, dim, 7, dev)
    rows = _rows(ng, dim, 8)
    rows[5] = 0                                              # zero rows: scale 2^0, every code 0
    rows[40:43] = 0
    rows[77] = rows[3]                                       # duplicated rows: the tie goes to the lower index
    rows[130] = rows[3]
    rows[50] = (torch.randint(-8, 9, (dim,), generator=torch.Generator().manual_seed(1)).float() / 8).to(BF)    # exact in e4m3
    rows[50, 0] = 1.0
    rows[51] = (rows[50].view(torch.int16) + (rows[50] != 0).to(torch.int16)).view(BF)     # one bf16 ulp away: other rows in bf16 ...
    rows[51, 0] = 1.0
    codes, scale, deq = _gallery(rows, dev)
    assert not torch.equal(rows[50], rows[51]) and torch.equal(codes[50], codes[51]) and scale[50] == scale[51]    # ... one row in e4m3
    assert (codes[5] == 0).all() and scale[5] == 1.0
    target = torch.tensor([[77, -1], [130, 3], [51, -1], [5, 41]] + [[50, 51]] * 29).to(dev)
    for slices in (0, 1, 3):
        got = ops.sim_topk_q8(q, codes, scale, 32, slices=slices)
        _same(got, ops.sim_topk(q, deq, 32, slices=slices), slices)
        assert torch.equal(ops.sim_rank_q8(q, codes, scale, target, slices=slices), ops.sim_rank(q, deq, target, slices=slices))
    # the duplicates and the collided pair appear in index order wherever they appear
    for a, b in ((3, 77), (77, 130), (50, 51)):
        pa, pb = (got[1] == a).float().argmax(dim=1), (got[1] == b).float().argmax(dim=1)
        both = (got[1] == a).any(dim=1) & (got[1] == b).any(dim=1)
        assert (pa[both] < pb[both]).all()
    r3, r77, r130 = (ops.sim_rank_q8(q, codes, scale, torch.full((33,), t, dtype=torch.int64, device=dev)) for t in (3, 77, 130))
    assert torch.equal(r77, r3 + 1) and torch.equal(r130, r3 + 2)


def test_sim_q8_nan_codes(dev):
    """hand-made codes holding 0x7F / 0xFF: a NaN score is never returned, beats nothing, and as a target behaves as in mpv_sim_rank"""
    from youku_mplug_amd import ops
    dim, ng = 160, 70
    rows = _rows(ng, dim, 11)
    codes, scale = standin_w8.quantize_rows_e4m3(rows)
    codes[4, 17] = 0x7F
    codes[33, 159] = 0xFF
    codes[34] = 0x7F
    codes[69, 0] = 0x7F
    deq = sq.dequantize(codes, scale)
    assert torch.isnan(deq[4, 17]) and torch.isnan(deq[33, 159]) and torch.isnan(deq[34]).all() and torch.isnan(deq).sum() == dim + 3
    codes, scale, deq = _pitched(codes, dim + 16, dev), scale.to(dev), deq.to(dev)
    q = _queries(5, dim, 12, dev)
    target = torch.tensor([[4, -1], [0, 34], [69, 33], [1, 2], [34, 34]]).to(dev)
    for slices in (0, 1, 3):
        got = ops.sim_topk_q8(q, codes, scale, 32, slices=slices)
        _same(got, ops.sim_topk(q, deq, 32, slices=slices), slices)
        assert not torch.isnan(got[0]).any() and not sum((got[1] == r).any() for r in (4, 33, 34, 69))
        assert torch.equal(ops.sim_rank_q8(q, codes, scale, target, slices=slices), ops.sim_rank(q, deq, target, slices=slices))
    all_k = ops.sim_topk_q8(q, codes, scale, 32, slices=2)
    more = ops.sim_topk_q8(q, codes[:20], scale[:20], 32)                      # 19 valid rows: the tail after them is (-inf, -1)
    assert (more[1][:, 19:] == -1).all() and (more[1][:, :19] >= 0).all() and torch.equal(all_k[0], got[0])


def test_sim_q8_rank_of_the_jth_result_is_j(dev):
    from youku_mplug_amd import ops
    codes, scale, deq = _gallery(_rows(133, 256, 21), dev)
    q = _queries(33, 256, 22, dev)
    vals, idx = ops.sim_topk_q8(q, codes, scale, 10)
    for j in range(10):
        assert (ops.sim_rank_q8(q, codes, scale, idx[:, j].contiguous()) == j).all(), j


def test_sim_q8_exact_features_equal_the_search_of_the_original_gallery(dev):
    """entries from {-2 .. 2} / 16 are e4m3 numbers: quantisation loses nothing and the _q8 search IS the bf16 search"""
    from youku_mplug_amd import ops
    g = mc.exact_features(133, None, 256, 3)
    codes, scale, deq = _gallery(g, dev)
    assert torch.equal(deq.cpu(), g)
    q = mc.exact_features(33, None, 256, 4, device=dev)
    t = (torch.arange(33) * 4 % 133).to(dev)
    for slices in (0, 1, 3):
        _same(ops.sim_topk_q8(q, codes, scale, 32, slices=slices), ops.sim_topk(q, g.to(dev), 32, slices=slices), slices)
        assert torch.equal(ops.sim_rank_q8(q, codes, scale, t, slices=slices), ops.sim_rank(q, g.to(dev), t, slices=slices))


# ------------------------------------------------------------------------------------------------ maxsim (q_group = 1)
@pytest.mark.parametrize("dim", [32, 256])
@pytest.mark.parametrize("group", [1, 5, 33, 40])
def test_maxsim_q8_equals_bf16_on_the_dequantised_gallery(dev, dim, group):
    """g_group 1 (also bit-identical to sim_*_q8), 5, 33 and 40 (groups straddle the 32-row tiles); rank with several targets and
    -1 slots; one item whose rows are all NaN codes and one with a single NaN row"""
    from youku_mplug_amd import ops
    ng, nq = 9, 33
    rows = _rows(ng * group, dim, 300 + group).view(ng, group, dim)
    codes, scale = standin_w8.quantize_rows_e4m3(rows.reshape(-1, dim))
    codes, scale = codes.view(ng, group, dim), scale.view(ng, group)
    codes[2] = 0x7F                                          # item 2: every product NaN -- never returned, no target
    codes[6, group // 2, 3] = 0xFF                           # item 6: one NaN row, which never wins the max (all of it when group == 1)
    deq = sq.dequantize(codes, scale).to(dev)
    codes, scale = _pitched(codes, dim + 16, dev), scale.to(dev)
    q = _queries(nq, dim, 400 + group, dev)
    target = torch.tensor([[i % ng, -1, (i * 5 + 1) % ng] for i in range(nq)]).to(dev)
    target[1] = torch.tensor([2, -1, -1])                   # only the NaN item: no target
    target[3] = -1
    for slices in (0, 1, 2):
        for k in (1, 10):
            got = ops.maxsim_topk_q8(q, codes, scale, k, scale=2.0 if k == 10 else None, slices=slices)
            _same(got, ops.maxsim_topk(q, deq, k, scale=2.0 if k == 10 else None, slices=slices), (dim, group, k, slices))
            assert not (got[1] == 2).any() and (group > 1 or not (got[1] == 6).any())
        r = ops.maxsim_rank_q8(q, codes, scale, target, slices=slices)
        assert torch.equal(r, ops.maxsim_rank(q, deq, target, slices=slices)), (dim, group, slices)
        assert r[1] == ng and r[3] == ng
    assert (got[1][:, 9 - 1 - (group == 1):] == -1).all()    # k = 10 > the valid items
    if group == 1:
        flat = codes[:, 0]
        _same(ops.maxsim_topk_q8(q, codes, scale, 10), ops.sim_topk_q8(q, flat, scale[:, 0].contiguous(), 10), "sim")
        _same(ops.maxsim_topk_q8(q, flat, scale[:, 0].contiguous(), 10), ops.sim_topk_q8(q, flat, scale[:, 0].contiguous(), 10), "2-D")
        t1 = target[:, :1].contiguous()
        ok = (t1[:, 0] != 2) & (t1[:, 0] != 6) & (t1[:, 0] >= 0)                # a NaN target is no target here, a target for mpv_sim_rank
        assert torch.equal(ops.maxsim_rank_q8(q, codes, scale, t1)[ok], ops.sim_rank_q8(q, flat, scale[:, 0].contiguous(), t1)[ok])


def test_maxsim_q8_group_1024(dev):
    from youku_mplug_amd import ops
    ng, group, dim = 3, 1024, 32
    codes, scale, deq = _gallery(_rows(ng * group, dim, 500).view(ng, group, dim), dev)
    q = _queries(5, dim, 501, dev)
    t = torch.tensor([[0, 2], [1, -1], [2, 2], [-1, -1], [0, 1]]).to(dev)
    for slices in (0, 1, 2):
        _same(ops.maxsim_topk_q8(q, codes, scale, 4, slices=slices), ops.maxsim_topk(q, deq, 4, slices=slices), slices)
        assert torch.equal(ops.maxsim_rank_q8(q, codes, scale, t, slices=slices), ops.maxsim_rank(q, deq, t, slices=slices))


def test_maxsim_q8_rank_of_the_jth_result_is_j_and_exact_features(dev):
    from youku_mplug_amd import ops
    codes, scale, deq = _gallery(_rows(9 * 40, 256, 600).view(9, 40, 256), dev)
    q = _queries(33, 256, 601, dev)
    vals, idx = ops.maxsim_topk_q8(q, codes, scale, 9)
    for j in range(9):
        assert (ops.maxsim_rank_q8(q, codes, scale, idx[:, j].contiguous()) == j).all(), j
    g = mc.exact_features(9, 40, 256, 5)
    codes, scale, deq = _gallery(g, dev)
    assert torch.equal(deq.cpu(), g)
    qe = mc.exact_features(33, None, 256, 6, device=dev)
    _same(ops.maxsim_topk_q8(qe, codes, scale, 9), ops.maxsim_topk(qe, g.to(dev), 9), "exact")
    t = (torch.arange(33) % 9).to(dev)
    assert torch.equal(ops.maxsim_rank_q8(qe, codes, scale, t), ops.maxsim_rank(qe, g.to(dev), t))


# ------------------------------------------------------------------------------------------------ index classes
def test_fp8_indexes_equal_bf16_indexes_of_their_dequantised_rows(dev):
    """two adds across a capacity growth, quantised on the device by ops.quantize_rows_e4m3"""
    from youku_mplug_amd._lib import MpvError
    from youku_mplug_amd.retrieval import MaxSimIndex, RetrievalIndex
    rows = _rows(133, 256, 700).to(dev)
    index = RetrievalIndex(256, device=dev, capacity=40, storage="fp8")
    assert index.add(rows[:33]) == 0 and index.capacity == 40 and index.add(rows[33:]) == 33 and index.capacity >= 133
    codes, scale = standin_w8.quantize_rows_e4m3(rows.cpu())
    assert torch.equal(index.codes.cpu(), codes) and torch.equal(index.scales.cpu(), scale)
    assert index.nbytes == 133 * 256 + 133 * 4
    with pytest.raises(MpvError, match=r"dequantized\(\)"):
        index.features
    twin = RetrievalIndex(256, device=dev)
    twin.add(index.dequantized())
    assert twin.nbytes == 133 * 512
    q = _queries(33, 256, 701, dev)
    t = torch.tensor([[i * 4 % 133, -1] for i in range(33)]).to(dev)
    _same(index.search(q, 10, scale=0.5), twin.search(q, 10, scale=0.5), "RetrievalIndex.search")
    assert torch.equal(index.rank(q, t), twin.rank(q, t))

    clips = _rows(9 * 40, 256, 702).view(9, 40, 256).to(dev)
    vi = MaxSimIndex(256, 40, device=dev, capacity=4, storage="fp8")
    assert vi.add(clips[:3]) == 0 and vi.capacity == 4 and vi.add(clips[3:]) == 3 and vi.capacity >= 9
    vt = MaxSimIndex(256, 40, device=dev)
    vt.add(vi.dequantized())
    _same(vi.search(q, 9), vt.search(q, 9), "MaxSimIndex.search")
    t9 = (torch.arange(33) % 9).to(dev)
    assert torch.equal(vi.rank(q, t9), vt.rank(q, t9))
    with pytest.raises(MpvError, match="bf16"):             # grouped queries against an fp8 index of single rows
        ti = MaxSimIndex(256, device=dev, storage="fp8")
        ti.add(rows[:8])
        ti.search(clips, 3)


# ------------------------------------------------------------------------------------------------ refusals
def test_q8_refusals_reach_no_launch(dev):
    """every refusal: a negative code and the outputs untouched"""
    from youku_mplug_amd import _lib, ops
    lib = _lib.lib()
    dim, ng, nq, k = 64, 40, 3, 4
    codes, scale, deq = _gallery(_rows(ng, dim, 800), dev, pitch=dim + 16)
    loose = _gallery(_rows(ng, dim, 800), dev, pitch=dim + 8)[0]            # a pitch the bf16 entries would take
    store = torch.zeros(ng * dim + 16, dtype=torch.uint8, device=dev)
    q = _queries(nq, dim, 801, dev)
    q3 = _queries(nq * 2, dim, 802, dev).view(nq, 2, dim)
    vals = torch.full((nq, k), 7.0, device=dev)
    idx = torch.full((nq, k), 7, dtype=torch.int64, device=dev)
    rank = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    target = torch.zeros((nq, 1), dtype=torch.int64, device=dev)

    def sim(gallery, g_rs):
        d = _lib.SimSearchDesc()
        d.queries, d.gallery, d.q_rs, d.g_rs, d.nq, d.ng, d.dim, d.k, d.scale = q.data_ptr(), gallery, dim, g_rs, nq, ng, dim, k, 1.0
        return d

    def maxsim(gallery, g_rs, queries=q.data_ptr(), q_group=1):
        d = _lib.MaxSimSearchDesc()
        d.queries, d.gallery, d.q_rs, d.g_rs, d.nq, d.ng, d.dim, d.k, d.scale = queries, gallery, dim, g_rs, nq, ng // 4, dim, k, 1.0
        d.q_group, d.g_group = q_group, 4 if q_group == 1 else 1
        return d

    cases = [(sim(codes.data_ptr(), dim + 16), None), (sim(store.data_ptr() + 8, dim), scale), (sim(loose.data_ptr(), dim + 8), scale)]
    for d, gs in cases:
        p = None if gs is None else gs.data_ptr()
        assert lib.mpv_sim_topk_q8(ctypes.byref(d), p, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), None) < 0
        assert lib.mpv_sim_rank_q8(ctypes.byref(d), p, target.data_ptr(), 1, rank.data_ptr(), ws.data_ptr(), ws.numel(), None) < 0
        assert lib.mpv_sim_topk_q8_workspace_size(ctypes.byref(d), p) == 0 and lib.mpv_sim_rank_q8_workspace_size(ctypes.byref(d), p, 1) == 0
    cases = [(maxsim(codes.data_ptr(), dim + 16), None), (maxsim(store.data_ptr() + 8, dim), scale), (maxsim(loose.data_ptr(), dim + 8), scale),
             (maxsim(codes.data_ptr(), dim + 16, q3.data_ptr(), 2), scale)]
    for d, gs in cases:
        p = None if gs is None else gs.data_ptr()
        assert lib.mpv_maxsim_topk_q8(ctypes.byref(d), p, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), None) < 0
        assert lib.mpv_maxsim_rank_q8(ctypes.byref(d), p, target.data_ptr(), 1, rank.data_ptr(), ws.data_ptr(), ws.numel(), None) < 0
        assert lib.mpv_maxsim_topk_q8_workspace_size(ctypes.byref(d), p) == 0
        assert lib.mpv_maxsim_rank_q8_workspace_size(ctypes.byref(d), p, 1) == 0
    torch.cuda.synchronize()
    assert (vals == 7.0).all() and (idx == 7).all() and (rank == 7).all() and (ws == 0).all()
    # and through the ops: an error that names the cause, raised before anything is written
    for call, word in ((lambda: ops.sim_topk_q8(q, loose, scale, k), "multiple of 16"),
                       (lambda: ops.maxsim_topk_q8(q3, codes, scale, k), "q_group"),
                       (lambda: ops.sim_topk_q8(q, codes, scale[:5], k), "g_scale"),
                       (lambda: ops.sim_topk_q8(q, deq, scale, k), "uint8")):
        with pytest.raises(_lib.MpvError, match=word):
            call()
    good = sim(codes.data_ptr(), dim + 16)                                   # the descriptor itself is fine
    assert lib.mpv_sim_topk_q8(ctypes.byref(good), scale.data_ptr(), vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), None) == 0
    torch.cuda.synchronize()
    _same((vals, idx), ops.sim_topk(q, deq, k), "good")
