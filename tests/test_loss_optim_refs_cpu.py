"""The fp64 references of tests/ref_loss_optim.py are right, and a correct implementation fits inside the gates (no GPU).
First half: each reference against an implementation it shares nothing with -- torch.optim.AdamW + clip_grad_norm_,
F.cross_entropy, the formula of include/mpv.h written as loops, the definition of F.normalize at a zero row.
Second half: the torch stand-ins of the same entry points (tests/standin_ops.py, tests/standin_optim.py) run over the inputs of tests/test_loss_optim_kernels_gpu.py and through the SAME gates (measured on the kernels); the three places
where a stand-in's own arithmetic differs from the kernels' carry their own tolerance, each documented where it is applied."""
import math

import pytest
import torch
import torch.nn.functional as F

import loss_optim_cases as K
import ref_loss_optim as R
import standin_ops
import standin_optim
from loss_optim_cases import GATES
from ref_loss_optim import close_elementwise

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("max_norm", [0.0, 0.7, 1e6], ids=["unclipped", "clipped", "clip-above-norm"])
def test_adamw_ref_matches_torch_adamw(max_norm):
    """Three groups with their own lr / weight decay, five steps, fp64 parameters: agreement to 1e-12 (relative to 1, the scale of
    the parameters).  The clipped run's norm (about 17) is far above max_norm = 0.7; 1e6 is far above the norm."""
    gen = torch.Generator().manual_seed(7)
    sizes, lrs, wds = [37, 5, 64], [1e-2, 3e-3, 1e-3], [0.05, 0.0, 0.3]
    params = [torch.randn(s, generator=gen, dtype=torch.float64).requires_grad_(True) for s in sizes]
    opt = torch.optim.AdamW([{"params": [p], "lr": lr, "weight_decay": wd} for p, lr, wd in zip(params, lrs, wds)],
                            betas=(0.9, 0.999), eps=1e-6)
    master = torch.cat([p.detach() for p in params]).clone()
    m, v = torch.zeros_like(master), torch.zeros_like(master)
    group = torch.cat([torch.full((s,), i) for i, s in enumerate(sizes)])
    for step in range(1, 6):
        g = torch.randn(sum(sizes), generator=gen, dtype=torch.float64) * 2.0
        for p, gp in zip(params, g.split(sizes)):
            p.grad = gp.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        master, m, v = R.adamw_ref(master, m, v, g, group, lrs, wds, (0.9, 0.999), 1e-6, step, 1.0, float((g * g).sum()), max_norm)
        assert (torch.cat([p.detach() for p in params]) - master).abs().max().item() <= 1e-12, step
    st = [opt.state[p] for p in params]
    assert (torch.cat([s["exp_avg"] for s in st]) - m).abs().max().item() <= 1e-12
    assert (torch.cat([s["exp_avg_sq"] for s in st]) - v).abs().max().item() <= 1e-12


def test_adamw_ref_grad_scale_and_skipped_elements():
    """grad_scale multiplies the gradient before everything else (a step on g with scale s = a step on s g with scale 1, s a power
    of two so that the product is exact), and an element with id >= 8 keeps master / m / v whatever its gradient holds."""
    gen = torch.Generator().manual_seed(8)
    n = 40
    p, m, v = (torch.randn(n, generator=gen, dtype=torch.float64) for _ in range(3))
    v = v.abs()
    g = torch.randn(n, generator=gen, dtype=torch.float64)
    group = torch.randint(0, 2, (n,), generator=gen)
    group[::7] = 255
    gn = g.clone()
    gn[::7] = float("nan")
    ss = float((g[group < 8] ** 2).sum())
    a = R.adamw_ref(p, m, v, gn, group, [1e-3, 2e-3], [0.1, 0.0], (0.9, 0.999), 1e-6, 3, 0.5, ss, 0.25)
    b = R.adamw_ref(p, m, v, g * 0.5, group, [1e-3, 2e-3], [0.1, 0.0], (0.9, 0.999), 1e-6, 3, 1.0, ss * 0.25, 0.25)
    for x, y, x0 in zip(a, b, (p, m, v)):
        assert torch.equal(x, y)
        assert torch.equal(x[::7], x0[::7]) and not torch.equal(x[group < 8], x0[group < 8])


def test_ce_ref_matches_torch_cross_entropy():
    gen = torch.Generator().manual_seed(9)
    rows, V = 11, 40
    x = (torch.randn(rows, V, generator=gen, dtype=torch.float64) * 5).requires_grad_(True)
    labels = torch.randint(0, V, (rows,), generator=gen)
    labels[3] = -100                                             # F.cross_entropy's ignore_index
    w = torch.rand(rows, generator=gen, dtype=torch.float64)
    w[5] = 0.0
    ref_l = F.cross_entropy(x, labels, reduction="none", ignore_index=-100)
    (ref_l * w).sum().backward()
    losses, d, total = R.ce_ref(x.detach(), labels, w)
    assert (losses - ref_l.detach()).abs().max().item() <= 1e-12 and losses[3].item() == 0.0
    assert (d - x.grad).abs().max().item() <= 1e-12
    assert abs(total.item() - (ref_l * w).sum().item()) <= 1e-12
    assert (d[3] == 0).all() and (d[5] == 0).all()
    labels[4] = V                                                # one past the end: also outside
    losses, d, _ = R.ce_ref(x.detach(), labels, None)
    assert losses[4].item() == 0.0 and (d[4] == 0).all()
    assert (losses[:3] - ref_l.detach()[:3]).abs().max().item() <= 1e-12          # weight=None = ones
    assert abs(R.ce_ref(torch.full((1, 64), 1.5), torch.tensor([9]))[0].item() - math.log(64)) <= 1e-12


def test_soft_target_ce_ref_matches_the_header_formula_in_loops():
    """include/mpv.h: targets[i][j] = [row_ids[i] == col_ids[j]] / count_i; losses[i] = -sum_j log_softmax(sim_i)[j] targets[i][j];
    dsim = (softmax - targets) * scale; dts[i] = sum_j dsim[i][j] sim[i][j] -- with plain Python floats on a 3 x 5 case."""
    sim = [[0.3, -1.2, 2.5, 0.0, 1.1], [4.0, 3.5, -2.0, 0.7, 0.7], [-0.4, -0.4, -0.4, 6.0, 1.0]]
    rid, cid, scale = [7, 2, 7], [2, 7, 9, 7, 2], 0.125
    losses, dsim, dts = R.soft_target_ce_ref(torch.tensor(sim, dtype=torch.float64), torch.tensor(rid), torch.tensor(cid), scale)
    for i in range(3):
        cnt = sum(1 for c in cid if c == rid[i])
        z = sum(math.exp(s) for s in sim[i])
        loss, dt = 0.0, 0.0
        for j in range(5):
            t = (1.0 / cnt) if cid[j] == rid[i] else 0.0
            loss -= (sim[i][j] - math.log(z)) * t
            gij = (math.exp(sim[i][j]) / z - t) * scale
            dt += gij * sim[i][j]
            assert abs(dsim[i, j].item() - gij) <= 1e-12
        assert abs(losses[i].item() - loss) <= 1e-12 and abs(dts[i].item() - dt) <= 1e-12


def test_l2norm_ref_zero_row_and_plain_row():
    """Zero row: ||x|| = 0 < eps, so y = x / eps = 0, norm = eps and dx = dy / eps.  Plain row: dx = (dy - y <y, dy>) / ||x||."""
    x = torch.tensor([[0.0, 0.0, 0.0, 0.0], [3.0, 0.0, -4.0, 0.0]])
    dy = torch.tensor([[1.0, -2.0, 0.5, 0.0], [1.0, 2.0, 3.0, 4.0]])
    y, n, dx = R.l2norm_ref(x, dy, eps=1e-12)
    assert n.tolist() == [1e-12, 5.0] and (y[0] == 0).all()
    assert (y[1] - torch.tensor([0.6, 0.0, -0.8, 0.0], dtype=torch.float64)).abs().max().item() <= 1e-15
    assert torch.equal(dx[0], dy[0].double() / 1e-12)
    yy = y[1]
    want = (dy[1].double() - yy * (yy * dy[1].double()).sum()) / 5.0
    assert (dx[1] - want).abs().max().item() <= 1e-15


def test_close_elementwise_names_the_worst_element():
    ref = torch.tensor([[1.0, 100.0], [0.0, -2.0]])
    got = ref.clone()
    close_elementwise(got, ref, 0.0, 0.0, "exact")
    got[1, 0] = 1e-3                                             # small in max-abs / max-ref terms (1e-5), wrong element-wise
    with pytest.raises(AssertionError, match=r"element \(1, 0\) got 0\.001.* reference 0\.0"):
        close_elementwise(got, ref, 2.0 ** -8, 1e-6, "one bad element")
    close_elementwise(got, ref, 2.0 ** -8, 2e-3, "inside atol")
    got[0, 1] = float("nan")
    with pytest.raises(AssertionError, match=r"element \(0, 1\)"):
        close_elementwise(got, ref, 2.0 ** -8, 1.0, "NaN is never close")


# ------------------------------------------------------------------------------------------------------------------ stand-ins, same gates
@pytest.mark.parametrize("ntiles", K.ADAMW_TILES)
def test_adamw_stub_fits_the_gates(ntiles):
    c = K.adamw_case(ntiles)
    sumsq = torch.zeros(())
    standin_optim.grad_sumsq(c["g_clean"], sumsq)
    norm = math.sqrt(sumsq.item())
    for step, gs, max_norm in [(1, 1.0, 0.0), (1000, 0.5, 0.37 * norm * 0.5), (3, 0.5, 2.5 * norm * 0.5)]:
        p16, master, m, v = (c[k].clone() for k in ("p16", "master", "m", "v"))
        standin_optim.adamw_step_grouped(p16, master, m, v, c["g"], c["tile_group"], K.ADAMW_LRS, K.ADAMW_WDS, *K.ADAMW_BETAS, K.ADAMW_EPS, step, gs,
                                sumsq, max_norm)
        rp, rm, rv = R.adamw_ref(c["master"], c["m"], c["v"], c["g"], c["group"], K.ADAMW_LRS, K.ADAMW_WDS, K.ADAMW_BETAS, K.ADAMW_EPS,
                                 step, gs, sumsq.item(), max_norm)
        tag = f"stub {ntiles} tiles step {step} gs {gs} max_norm {max_norm:.3g}"
        close_elementwise(master, rp, *GATES["adamw.master"], f"{tag} master")
        # STUB ONLY: torch rounds the Python scalars beta1 and 1 - beta1 to fp32 one by one (the kernel computes 1.0f - beta1 from the
        # rounded beta1, which the GPU test's reference is given): 2^-25 (0.9 |m0| + 0.1 |g|) <= 3e-8 * 4.2 on top of the kernel's gate
        close_elementwise(m, rm, GATES["adamw.m"][0], GATES["adamw.m"][1] + 1.3e-7, f"{tag} m")
        close_elementwise(v, rv, *GATES["adamw.v"], f"{tag} v")
        d = c["dead"]
        assert torch.equal(master[d], c["master"][d]) and torch.equal(m[d], c["m"][d]) and torch.equal(v[d], c["v"][d])


@pytest.mark.parametrize("rows,V,ld,kind0,lab0", K.CE_CASES)
def test_cross_entropy_standin_fits_the_gates(rows, V, ld, kind0, lab0):
    logits, labels, weight = K.ce_case(rows, V, ld, kind0, lab0)
    for w in (weight, None):
        dl = torch.full((rows, ld), K.CE_PAD_SENTINEL, dtype=BF)
        losses, total = standin_ops.cross_entropy(logits, labels, w, rows, V, ld=ld, dlogits=dl)
        rl, rd, rt = R.ce_ref(logits[:, :V], labels, w)
        tag = f"stand-in CE ({rows}, {V}, {ld}) weight={'yes' if w is not None else 'None'}"
        close_elementwise(losses, rl, *GATES["ce.losses"], f"{tag} losses")
        close_elementwise(dl[:, :V], rd, *GATES["ce.dlogits"], f"{tag} dlogits")
        close_elementwise(total, rt, *GATES["ce.loss_sum"], f"{tag} loss_sum")
        assert (dl[:, V:] == K.CE_PAD_SENTINEL).all()
        out = (labels < 0) | (labels >= V)
        assert (losses[out] == 0).all() and (dl[:, :V][out] == 0).all()


@pytest.mark.parametrize("rows,cols", K.SOFT_CE_CASES)
def test_soft_target_ce_standin_fits_the_gates(rows, cols):
    sim, rid, cid, scale = K.soft_ce_case(rows, cols)
    losses, dsim, dts = standin_ops.soft_target_ce(sim, rid, cid, scale, rows, cols)
    rl, rd, rt = R.soft_target_ce_ref(sim, rid, cid, scale)
    close_elementwise(losses, rl, *GATES["soft_ce.losses"], f"stand-in soft CE ({rows}, {cols}) losses")
    close_elementwise(dsim, rd, *GATES["soft_ce.dsim"], f"stand-in soft CE ({rows}, {cols}) dsim")
    # STAND-IN ONLY: it sums dts over the bf16-ROUNDED dsim, the kernel (and include/mpv.h's formula) over the fp32 gradient.  The
    # rounding of each of the `cols` terms enters the sum: sum_j 2^-8 |dsim sim|.  The kernel's gate is checked on the GPU.
    own = K.RTOL_BF16 * (rd.abs() * sim.double().abs()).sum(1)
    assert ((dts.double() - rt).abs() <= own + GATES["soft_ce.dts"][0] * rt.abs() + GATES["soft_ce.dts"][1]).all()


@pytest.mark.parametrize("cols", K.L2NORM_COLS)
def test_l2norm_standin_fits_the_gates(cols):
    for rows in K.L2NORM_ROWS:
        x, dy = K.l2norm_case(rows, cols)
        y, nrm = standin_ops.l2norm_fwd(x, rows, cols)
        dx = standin_ops.l2norm_bwd(dy, x, nrm, rows, cols)
        ry, rn, rdx = R.l2norm_ref(x, dy)
        close_elementwise(y, ry, *GATES["l2norm.y"], f"stand-in l2norm ({rows}, {cols}) y")
        # STAND-IN ONLY: torch's CPU norm adds up to 2052 squares in long serial chains, the kernel at most 9 per lane and a 6-level
        # tree, and meets 2^-22 with no atol; the stand-in gets 2^-20 (16 half-ulps)
        close_elementwise(nrm, rn, 2.0 ** -20, GATES["l2norm.norm"][1], f"stand-in l2norm ({rows}, {cols}) norm")
        close_elementwise(dx, rdx, *GATES["l2norm.dx"], f"stand-in l2norm ({rows}, {cols}) dx")


@pytest.mark.parametrize("rows,cols,ld,nsrc", K.ROWS_CASES)
def test_gather_scatter_standins_are_exact(rows, cols, ld, nsrc):
    src, gidx, sidx = K.rows_case(rows, cols, ld, nsrc)
    got = standin_ops.gather_rows(src, gidx, rows, cols, ld=ld)
    assert torch.equal(got, src[gidx][:, :cols])
    dst = torch.full((nsrc, ld), -77.0, dtype=BF)
    standin_ops.scatter_rows(got, sidx, dst, rows, cols, ld=ld)
    want = torch.full((nsrc, ld), -77.0, dtype=BF)
    want[sidx, :cols] = got
    assert torch.equal(dst, want)


def test_gpt_embed_standins_without_dropout():
    B, Q, L, H = 3, 8, 6, 256
    dh = torch.randn(B * (Q + L), H).to(BF)
    assert torch.equal(standin_ops.gpt_embed_bwd_full(dh, B * (Q + L), H), dh)
    assert torch.equal(standin_ops.gpt_embed_bwd(dh, B, Q, L, H), dh.view(B, Q + L, H)[:, :Q].reshape(B * Q, H))
