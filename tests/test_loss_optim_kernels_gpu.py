"""The kernels that end a training step -- grouped / flat AdamW, the gradient norm, cross-entropy, the retrieval head's soft-target CE,
L2 normalisation, row gather / scatter, the embedding dropout -- against the fp64 references of tests/ref_loss_optim.py, element by
element, at the smallest shapes that reach each code path (see the case tables there).  Tolerances: loss_optim_cases.GATES (rtol from
the number format, atol = 2 x the residual measured on an MI355X; pytest -s prints every comparison's worst residual; the table is in
profiles/loss_optim_kernel_errors.md);
everything called bit-identical, unchanged or exact below is compared with torch.equal on the raw bits.
Run on the MI355X box: pytest -m gpu tests/test_loss_optim_kernels_gpu.py"""
import math

import pytest
import torch

import loss_optim_cases as K
import ref_loss_optim as R
from loss_optim_cases import GATES
from ref_loss_optim import close_elementwise

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def bits(t):
    """the raw bits of t (so that NaN == NaN and -0.0 != 0.0)"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------ grouped AdamW
_adamw_cases = {}


def _adamw_dev_case(ntiles, dev):
    """the case on the device + its fp32 sum of squares from ops.grad_sumsq (taken from the gradient with zeros on the skipped tiles,
    as the engine's padding holds them; the NaN copy is what the step kernels read)"""
    from youku_mplug_amd import ops
    if ntiles not in _adamw_cases:
        c = {k: t.to(dev) for k, t in K.adamw_case(ntiles).items()}
        sumsq = torch.zeros((), device=dev)
        ops.grad_sumsq(c["g_clean"], sumsq)
        c["sumsq"] = sumsq
        _adamw_cases[ntiles] = c
    return _adamw_cases[ntiles]


def _max_norm(c, clip, gs):
    norm = math.sqrt(c["sumsq"].item()) * gs
    return {"off": 0.0, "active": 0.37 * norm, "above": 2.5 * norm}[clip]


def _grouped_step(entry, c, step, gs, max_norm, lo=0, hi=None):
    """one step on fresh copies of the case's state, through either entry point, on tiles [lo, hi) -> (p16, master, m, v)"""
    from youku_mplug_amd import ops
    hi = c["tile_group"].numel() if hi is None else hi
    sl = slice(lo * K.TILE, hi * K.TILE)
    p16, master, m, v = (c[k][sl].clone() for k in ("p16", "master", "m", "v"))
    g, tg = c["g"][sl], c["tile_group"][lo:hi]
    if entry == "grouped":
        ops.adamw_step_grouped(p16, master, m, v, g, tg, K.ADAMW_LRS, K.ADAMW_WDS, *K.ADAMW_BETAS, K.ADAMW_EPS, step, gs, c["sumsq"], max_norm)
    else:
        hyper = torch.zeros(18, dtype=torch.float32, device=p16.device)
        ops.adamw_hyper_upload(K.ADAMW_LRS, K.ADAMW_WDS, *K.ADAMW_BETAS, step, hyper)
        ops.adamw_step_grouped_dev(p16, master, m, v, g, tg, hyper, *K.ADAMW_BETAS, K.ADAMW_EPS, gs, c["sumsq"], max_norm)
    return p16, master, m, v


def _adamw_combos(ntiles):
    if ntiles < 100:
        return [(s, gs, clip) for s in K.ADAMW_STEPS for gs in (1.0, 0.5) for clip in ("off", "active", "above")]
    # 8.4 M elements: five combinations in which every step, both grad_scales and every clip setting occur (the fp64 reference, not the
    # kernel, is what takes the time)
    return [(1000, 0.5, "active"), (1, 1.0, "above"), (2, 0.5, "off"), (3, 1.0, "active"), (1000, 1.0, "off")]


@pytest.mark.parametrize("ntiles", K.ADAMW_TILES)
@pytest.mark.parametrize("entry", ["grouped", "grouped_dev"])
def test_adamw_grouped_vs_fp64(dev, entry, ntiles):
    """mpv_adamw_step_grouped / _dev: master, m, v element-wise against adamw_ref (steps 1, 2, 3, 1000; grad_scale 1 and 0.5; clip
    off / active / max_norm above the norm, which must also equal the unclipped update bit for bit); p16 == bf16(master); skipped
    tiles (id 255: first tile, last tile, both tiles of a pair) keep their sentinel bits although their gradients are NaN.
    Measured on MI355X (residual over rtol 2^-22 -> atol = 2 x): master 3.1e-9 -> 6.2e-9, m 6.2e-8 -> 1.3e-7, v 2.9e-11 -> 5.8e-11
    (all three at 32771 tiles)."""
    c = _adamw_dev_case(ntiles, dev)
    dead = c["dead"]
    for step, gs, clip in _adamw_combos(ntiles):
        mn = _max_norm(c, clip, gs)
        p16, master, m, v = _grouped_step(entry, c, step, gs, mn)
        rp, rm, rv = R.adamw_ref(c["master"], c["m"], c["v"], c["g"], c["group"], R.f32(K.ADAMW_LRS), R.f32(K.ADAMW_WDS), R.f32(K.ADAMW_BETAS),
                                 R.f32(K.ADAMW_EPS), step, R.f32(gs), c["sumsq"].item(), R.f32(mn))
        tag = f"{entry} {ntiles} tiles step {step} grad_scale {gs} clip {clip}"
        close_elementwise(master, rp, *GATES["adamw.master"], f"{tag}: master")
        close_elementwise(m, rm, *GATES["adamw.m"], f"{tag}: m")
        close_elementwise(v, rv, *GATES["adamw.v"], f"{tag}: v")
        assert same_bits(p16[~dead], master[~dead].bfloat16()), f"{tag}: p16 != bf16(master)"
        for name, got in (("master", master), ("m", m), ("v", v), ("p16", p16)):
            assert same_bits(got[dead], c[name][dead]), f"{tag}: a skipped tile's {name} was written"
        assert not torch.equal(master[~dead], c["master"][~dead])
        if clip == "above":
            for a, b in zip((p16, master, m, v), _grouped_step(entry, c, step, gs, 0.0)):
                assert same_bits(a, b), f"{tag}: max_norm above the norm changed the update"
        if clip == "active":
            assert not torch.equal(m, _grouped_step(entry, c, step, gs, 0.0)[2]), f"{tag}: the clip did nothing"


@pytest.mark.parametrize("ntiles", [9, 32768 + 3])
def test_adamw_grouped_entry_points_bit_identical(dev, ntiles):
    """include/mpv.h: hyper_dev as written by mpv_adamw_hyper_pack makes mpv_adamw_step_grouped_dev update bit-identically."""
    c = _adamw_dev_case(ntiles, dev)
    for step, gs, clip in [(1, 1.0, "off"), (3, 0.5, "active"), (1000, 1.0, "active")]:
        mn = _max_norm(c, clip, gs)
        for a, b in zip(_grouped_step("grouped", c, step, gs, mn), _grouped_step("grouped_dev", c, step, gs, mn)):
            assert same_bits(a, b), (ntiles, step, gs, clip)


@pytest.mark.parametrize("entry", ["grouped", "grouped_dev"])
@pytest.mark.parametrize("ntiles,lo,hi", [(9, 3, 8), (9, 4, 9), (32768 + 3, 1001, 32768 + 2), (32768 + 3, 32766, 32768 + 3)])
def test_adamw_grouped_subslice_equals_whole(dev, entry, ntiles, lo, hi):
    """ZeRO-1 calls the kernel on tiles [lo, hi) of the buffers with the whole gradient's norm: the same bits as those tiles of the
    whole-buffer call (odd and even tile counts, starts on either tile of a pair)."""
    c = _adamw_dev_case(ntiles, dev)
    mn = _max_norm(c, "active", 0.5)
    whole = _grouped_step(entry, c, 3, 0.5, mn)
    part = _grouped_step(entry, c, 3, 0.5, mn, lo, hi)
    for a, b in zip(whole, part):
        assert same_bits(a[lo * K.TILE:hi * K.TILE], b)


def test_adamw_engine_step_uses_each_parameters_own_group(dev):
    """One real step of the engine on CONFIG_TINY: the updated fp32 master against adamw_ref with the per-element group derived from
    each parameter's NAME (1-D / bias / LayerNorm.weight / the model's no_weight_decay list: no decay; visual_encoder.* except the
    temporal tensors: lr x 0.1 -- the rule of the reference's optimizer factory), never from flat.tile_group.  A bias that gets
    decayed or a visual-encoder tensor at the full lr fails here."""
    import types
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict
    from youku_mplug_amd import engine as eng
    from youku_mplug_amd.pretrain import synthetic_model
    cfg, lr0, wd0, clip = CONFIG_TINY, 1e-4, 0.05, 3.0
    model = synthetic_model(cfg, device=dev)
    model.load_state_dict({k: v.to(BF) for k, v in make_state_dict(cfg, 0).items()})
    video, ids, mask = make_inputs(cfg, 2, 8, seed=1234, ragged=True)
    model.train()
    skip = model.no_weight_decay()
    groups = eng.get_parameter_groups(model, wd0, skip, visual_backbone_scale=True)
    e, _, _, _ = eng.initialize(model=model, model_parameters=groups, config=dict(lr=lr0, clip_grad=clip))
    loss, _ = e(video.to(dev).to(BF), types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev)))
    e.backward(loss)
    flat, opt = e.flat, e.optimizer
    g0, p0, m0, v0 = flat.grads.clone(), opt.master.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    e.step()
    # the (lr, wd) of every element, from names
    pairs, group = [], torch.full((flat.numel,), 255, dtype=torch.int64)
    where = {id(p): (o, n) for p, o, n in flat.slots}
    unused = {id(p) for p in model.unused_parameters()} if hasattr(model, "unused_parameters") else set()
    seen = 0
    for name, p in model.named_parameters():
        if not p.requires_grad or id(p) in unused:
            continue
        no_decay = p.dim() == 1 or "bias" in name or "LayerNorm.weight" in name or name in skip
        vis = "visual_encoder." in name and "temporal" not in name
        pair = (lr0 * (0.1 if vis else 1.0), 0.0 if no_decay else wd0)
        if pair not in pairs:
            pairs.append(pair)
        o, n = where[id(p)]
        group[o:o + n] = pairs.index(pair)
        seen += 1
    assert seen == len(where) - len(unused & set(where)) and len(pairs) >= 3, (seen, len(where), pairs)
    sumsq = opt.sumsq.item()
    assert sumsq > 0 and math.isfinite(sumsq)
    rp, rm, rv = R.adamw_ref(p0, m0, v0, g0, group.to(dev), R.f32([a for a, _ in pairs]), R.f32([b for _, b in pairs]), R.f32((0.9, 0.999)), R.f32(1e-6),
                             1, 1.0, sumsq, clip)
    close_elementwise(opt.master, rp, *GATES["adamw.master"], "engine step: master")
    close_elementwise(opt.exp_avg, rm, *GATES["adamw.m"], "engine step: exp_avg")
    close_elementwise(opt.exp_avg_sq, rv, *GATES["adamw.v"], "engine step: exp_avg_sq")
    live = (group < 8).to(dev)
    assert same_bits(flat.params[live], opt.master[live].bfloat16())
    assert not torch.equal(opt.master[live], p0[live])


# ------------------------------------------------------------------------------------------------------------------ flat AdamW, norm
@pytest.mark.parametrize("n", [4, 1028, 4 * (4096 * 256) + 8])      # one thread; two workgroups, ragged; past 4096 x 256 threads x 4
def test_adamw_flat_vs_fp64(dev, n):
    """mpv_adamw_step at step 1000, unclipped (max_norm above the norm, and max_norm = 0), grad_scale 0.5: master / m / v against
    adamw_ref, p16 == bf16(master).
    Measured on MI355X (residual over rtol 2^-22 -> atol = 2 x): master 3.1e-9 -> 6.2e-9, m 6.2e-8 -> 1.3e-7, v 2.9e-11 -> 5.8e-11
    (all three at 32771 tiles)."""
    from youku_mplug_amd import ops
    gen = torch.Generator().manual_seed(70 + n % 1000)
    master0, m0 = torch.randn(n, generator=gen).to(dev), (torch.randn(n, generator=gen) * 0.5).to(dev)
    v0, g = (torch.rand(n, generator=gen) * 2).to(dev), (torch.randn(n, generator=gen) * 3).to(BF).to(dev)
    sumsq = torch.zeros((), device=dev)
    ops.grad_sumsq(g, sumsq)
    lr, wd, gs = 3e-4, 0.01, 0.5
    outs = []
    for mn in (0.0, 2.5 * math.sqrt(sumsq.item()) * gs):
        p16, master, m, v = torch.zeros(n, dtype=BF, device=dev), master0.clone(), m0.clone(), v0.clone()
        ops.adamw_step(p16, master, m, v, g, lr, *K.ADAMW_BETAS, K.ADAMW_EPS, wd, 1000, gs, sumsq, mn)
        rp, rm, rv = R.adamw_ref(master0, m0, v0, g, torch.zeros(n, dtype=torch.int64, device=dev), R.f32([lr]), R.f32([wd]), R.f32(K.ADAMW_BETAS),
                                 R.f32(K.ADAMW_EPS), 1000, R.f32(gs), sumsq.item(), R.f32(mn))
        close_elementwise(master, rp, *GATES["adamw.master"], f"flat n={n} max_norm={mn:.3g}: master")
        close_elementwise(m, rm, *GATES["adamw.m"], f"flat n={n} max_norm={mn:.3g}: m")
        close_elementwise(v, rv, *GATES["adamw.v"], f"flat n={n} max_norm={mn:.3g}: v")
        assert same_bits(p16, master.bfloat16())
        outs.append((p16, master, m, v))
    for a, b in zip(*outs):
        assert same_bits(a, b)


@pytest.mark.parametrize("n", [1, 7, 8, 13, 2048 + 5, 8 * 256 * 3 + 3])
def test_grad_sumsq_exact_on_integers(dev, n):
    """Gradients are integers in [-8, 8]: every partial sum is an integer below 2^24, exact in fp32 in any order, so the result must
    EQUAL the integer sum; a second call adds to the scalar (`+=` in include/mpv.h)."""
    from youku_mplug_amd import ops
    gi = torch.randint(-8, 9, (n,), generator=torch.Generator().manual_seed(n))
    want = int((gi * gi).sum())
    g = gi.to(BF).to(dev)
    sumsq = torch.zeros((), device=dev)
    ops.grad_sumsq(g, sumsq)
    assert sumsq.item() == float(want), (sumsq.item(), want)
    ops.grad_sumsq(g, sumsq)
    assert sumsq.item() == float(2 * want), (sumsq.item(), 2 * want)
    s3 = torch.full((), 5.0, device=dev)
    ops.grad_sumsq(g, s3)
    assert s3.item() == float(want + 5)


# ------------------------------------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("rows,V,ld,kind0,lab0", K.CE_CASES)
def test_cross_entropy_vs_fp64(dev, rows, V, ld, kind0, lab0):
    """mpv_cross_entropy: losses, dlogits and loss_sum element-wise against ce_ref, with per-row weights and with weight = None.
    Labels outside [0, V) and rows of weight 0 give exactly-zero gradient rows (and a zero loss for the former); with ld > V the
    NaN in the padding columns of logits is never read and the sentinel in dlogits' padding columns keeps its bits; loss_sum is
    bit-identical over 10 calls.
    Measured on MI355X: losses 6.6e-7 over 2^-22 -> atol 1.4e-6; loss_sum never leaves 2^-22 -> 0; dlogits 1.5e-39 over
    2^-8 (a bf16 subnormal flushed to zero) -> 3.1e-39."""
    from youku_mplug_amd import ops
    logits, labels, weight = (t.to(dev) for t in K.ce_case(rows, V, ld, kind0, lab0))
    outside = (labels < 0) | (labels >= V)
    for w in (weight, None):
        dl = torch.full((rows, ld), K.CE_PAD_SENTINEL, dtype=BF, device=dev)
        losses, total = ops.cross_entropy(logits, labels, w, rows, V, ld=ld, dlogits=dl)
        rl, rd, rt = R.ce_ref(logits[:, :V], labels, w)
        tag = f"CE ({rows}, {V}, {ld}) weight={'yes' if w is not None else 'None'}"
        close_elementwise(losses, rl, *GATES["ce.losses"], f"{tag}: losses")
        close_elementwise(dl[:, :V], rd, *GATES["ce.dlogits"], f"{tag}: dlogits")
        close_elementwise(total, rt, *GATES["ce.loss_sum"], f"{tag}: loss_sum")
        assert same_bits(dl[:, V:], torch.full((rows, ld - V), K.CE_PAD_SENTINEL, dtype=BF, device=dev)), f"{tag}: padding columns written"
        assert (losses[outside] == 0).all() and (dl[:, :V][outside] == 0).all(), f"{tag}: a label outside the vocabulary contributed"
        if w is not None:
            assert (dl[:, :V][w == 0] == 0).all(), f"{tag}: a row of weight 0 has a gradient"
        for _ in range(10):
            l2, t2 = ops.cross_entropy(logits, labels, w, rows, V, ld=ld, dlogits=None)
            assert same_bits(t2, total) and same_bits(l2, losses), f"{tag}: not reproducible"


@pytest.mark.parametrize("rows,V,kind0,lab0", [(5, 51200, 0, 0), (3, 16384, 0, 5), (4, 1024, 1, 3)])
def test_cross_entropy_in_place_equals_out_of_place(dev, rows, V, kind0, lab0):
    """dlogits aliasing logits (how the LM head calls it): every wave must have finished reading the row's statistics and the
    target logit before any wave overwrites it -- 16 waves per row at V = 51200.  Same bits as the out-of-place call."""
    from youku_mplug_amd import ops
    logits, labels, weight = (t.to(dev) for t in K.ce_case(rows, V, V, kind0, lab0))
    dl = torch.empty_like(logits)
    losses, total = ops.cross_entropy(logits, labels, weight, rows, V, dlogits=dl)
    for _ in range(3):
        buf = logits.clone()
        l2, t2 = ops.cross_entropy(buf, labels, weight, rows, V, dlogits=buf)
        assert same_bits(l2, losses) and same_bits(t2, total) and same_bits(buf, dl)


# ------------------------------------------------------------------------------------------------------------------ soft-target CE
@pytest.mark.parametrize("rows,cols", K.SOFT_CE_CASES)
def test_soft_target_ce_vs_fp64(dev, rows, cols):
    """mpv_soft_target_ce: losses, dsim (bf16) and dts against soft_target_ce_ref (fp64 autograd); want_grad=False returns the same
    losses bit for bit.
    Measured on MI355X: losses and dsim never leave 2^-22 / 2^-8 -> atol 0; dts 4.5e-6 over 2^-22 at (1, 8) -> 9.0e-6."""
    from youku_mplug_amd import ops
    sim, rid, cid, scale = K.soft_ce_case(rows, cols)
    sim, rid, cid = sim.to(dev), rid.to(dev), cid.to(dev)
    losses, dsim, dts = ops.soft_target_ce(sim, rid, cid, scale, rows, cols)
    rl, rd, rt = R.soft_target_ce_ref(sim, rid, cid, scale)
    close_elementwise(losses, rl, *GATES["soft_ce.losses"], f"soft CE ({rows}, {cols}): losses")
    close_elementwise(dsim, rd, *GATES["soft_ce.dsim"], f"soft CE ({rows}, {cols}): dsim")
    close_elementwise(dts, rt, *GATES["soft_ce.dts"], f"soft CE ({rows}, {cols}): dts")
    l2, d2, t2 = ops.soft_target_ce(sim, rid, cid, scale, rows, cols, want_grad=False)
    assert d2 is None and t2 is None and same_bits(l2, losses)


def test_soft_target_ce_row_without_a_matching_column_is_finite(dev):
    """retrieval.py builds col_ids as the all-gather of the ranks' row_ids, its own among them, so every row matches at least one
    column and count_i >= 1: a row without a match cannot occur in the product.  The division by count_i = 0 such a row implies
    must still not poison the outputs: only finiteness is asserted for it; the matching rows are checked as usual."""
    from youku_mplug_amd import ops
    gen = torch.Generator().manual_seed(12)
    sim = (torch.randn(3, 70, generator=gen) * 10).to(dev)
    rid = torch.tensor([4, 99, 6], device=dev)
    cid = (torch.arange(70) % 9).to(dev)                         # 0..8: no 99
    losses, dsim, dts = ops.soft_target_ce(sim, rid, cid, 0.1, 3, 70)
    assert torch.isfinite(losses).all() and torch.isfinite(dsim.float()).all() and torch.isfinite(dts).all()
    rl, rd, rt = R.soft_target_ce_ref(sim[[0, 2]], rid[[0, 2]], cid, 0.1)
    close_elementwise(losses[[0, 2]], rl, *GATES["soft_ce.losses"], "soft CE beside an unmatched row: losses")
    close_elementwise(dsim[[0, 2]], rd, *GATES["soft_ce.dsim"], "soft CE beside an unmatched row: dsim")
    close_elementwise(dts[[0, 2]], rt, *GATES["soft_ce.dts"], "soft CE beside an unmatched row: dts")


# ------------------------------------------------------------------------------------------------------------------ L2 normalisation
@pytest.mark.parametrize("cols", K.L2NORM_COLS)
def test_l2norm_fwd_bwd_vs_fp64(dev, cols):
    """mpv_l2norm_fwd / _bwd at rows 1, 5, 7, 64 (a workgroup holds four rows): y, norm and dx against F.normalize + autograd in fp64,
    an all-zero row (norm = eps, y = 0, dx = dy / eps) and a row of 1e-20-sized values among them.
    Measured on MI355X: y, norm and dx never leave 2^-8 / 2^-22 / 2^-8 -> atol 0."""
    from youku_mplug_amd import ops
    for rows in K.L2NORM_ROWS:
        x, dy = (t.to(dev) for t in K.l2norm_case(rows, cols))
        y, nrm = ops.l2norm_fwd(x, rows, cols)
        dx = ops.l2norm_bwd(dy, x, nrm, rows, cols)
        ry, rn, rdx = R.l2norm_ref(x, dy)
        close_elementwise(y, ry, *GATES["l2norm.y"], f"l2norm ({rows}, {cols}): y")
        close_elementwise(nrm, rn, *GATES["l2norm.norm"], f"l2norm ({rows}, {cols}): norm")
        close_elementwise(dx, rdx, *GATES["l2norm.dx"], f"l2norm ({rows}, {cols}): dx")


# ------------------------------------------------------------------------------------------------------------------ gather / scatter
@pytest.mark.parametrize("rows,cols,ld,nsrc", K.ROWS_CASES)
def test_gather_scatter_rows_exact(dev, rows, cols, ld, nsrc):
    """mpv_gather_rows with repeated indices and a source pitch ld >= cols; mpv_scatter_rows with distinct indices into a
    sentinel-filled destination: rows not named and columns [cols, ld) keep their bits; scatter(gather(x)) gives x back."""
    from youku_mplug_amd import ops
    src, gidx, sidx = (t.to(dev) for t in K.rows_case(rows, cols, ld, nsrc))
    got = ops.gather_rows(src, gidx, rows, cols, ld=ld)
    assert same_bits(got, src[gidx][:, :cols].contiguous())
    dst = torch.full((nsrc, ld), -77.0, dtype=BF, device=dev)
    ops.scatter_rows(got, sidx, dst, rows, cols, ld=ld)
    want = torch.full((nsrc, ld), -77.0, dtype=BF, device=dev)
    want[sidx, :cols] = got
    assert same_bits(dst, want)
    back = ops.gather_rows(dst, sidx, rows, cols, ld=ld)          # gather(scatter(a)) == a ...
    assert same_bits(back, got)
    rt = src.clone()                                              # ... and scatter(gather(x)) == x on the rows it names
    ops.scatter_rows(ops.gather_rows(src, sidx, rows, cols, ld=ld), sidx, rt, rows, cols, ld=ld)
    assert same_bits(rt, src)


# ------------------------------------------------------------------------------------------------------------------ embedding dropout
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,Q,L,H", [(3, 8, 6, 256), (2, 128, 32, 2048)])
def test_gpt_embed_dropout_masks_identical(dev, B, Q, L, H, p):
    """wte = query = dh = 1, wpe = 0: every output of mpv_gpt_embed_fwd / _bwd / _bwd_full is exactly 0 or bf16(1 / (1 - p)), so
    the keep masks can be read off exactly.  The three masks are IDENTICAL (_bwd on the query rows, _bwd_full on all rows), and
    the keep rate lies within 4 sigma of 1 - p, sigma = sqrt(p (1 - p) / N) over N = B (Q + L) H elements: N = 10752 for
    (3, 8, 6, 256) and N = 655360 for (2, 128, 32, 2048)."""
    from youku_mplug_amd import ops
    S, V = Q + L, 32
    one = lambda *shape: torch.ones(*shape, dtype=BF, device=dev)
    ids = torch.randint(0, V, (B, L), device=dev)
    seed, offset = 12345, 64
    h = ops.gpt_embed_fwd(one(B * Q, H), ids, one(V, H), torch.zeros(S, H, dtype=BF, device=dev), B, Q, L, H, dropout_p=p, seed=seed, offset=offset)
    dq = ops.gpt_embed_bwd(one(B * S, H), B, Q, L, H, dropout_p=p, seed=seed, offset=offset)
    df = ops.gpt_embed_bwd_full(one(B * S, H), B * S, H, dropout_p=p, seed=seed, offset=offset)
    kept_value = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32).to(BF).item()
    for name, t in (("fwd", h), ("bwd", dq), ("bwd_full", df)):
        assert ((t == 0) | (t == kept_value)).all(), f"{name}: a value other than 0 and bf16(1 / (1 - p))"
    keep = h != 0
    assert torch.equal(df != 0, keep), "bwd_full's mask differs from the forward's"
    assert torch.equal(dq.view(B, Q, H) != 0, keep.view(B, S, H)[:, :Q]), "bwd's mask differs from the forward's on the query rows"
    N = B * S * H
    rate, sigma = keep.float().mean().item(), math.sqrt(p * (1 - p) / N)
    assert abs(rate - (1 - p)) <= 4 * sigma, f"keep rate {rate:.5f} vs {1 - p} over N = {N} elements (4 sigma = {4 * sigma:.5f})"
    h2 = ops.gpt_embed_fwd(one(B * Q, H), ids, one(V, H), torch.zeros(S, H, dtype=BF, device=dev), B, Q, L, H, dropout_p=p, seed=seed + 1, offset=offset)
    assert not torch.equal(h2 != 0, keep), "the mask does not depend on the seed"


def test_gpt_embed_bwd_full_without_dropout_is_the_identity(dev):
    from youku_mplug_amd import ops
    B, Q, L, H = 3, 8, 6, 256
    dh = torch.randn(B * (Q + L), H, generator=torch.Generator().manual_seed(5)).to(BF).to(dev)
    assert same_bits(ops.gpt_embed_bwd_full(dh, B * (Q + L), H), dh)
    assert same_bits(ops.gpt_embed_bwd(dh, B, Q, L, H), dh.view(B, Q + L, H)[:, :Q].reshape(B * Q, H))
