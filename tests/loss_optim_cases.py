"""Inputs and gates shared by tests/test_loss_optim_kernels_gpu.py (the HIP kernels) and tests/test_loss_optim_refs_cpu.py (the torch
stand-ins over the same inputs), TEST INFRASTRUCTURE ONLY.  The inputs are built on the host from fixed seeds; the tables say which
code path each shape reaches.

GATES: every tolerance of those two files, one place so that the CPU stand-in check and the GPU kernel check cannot drift apart.
The form is |got - ref| <= rtol * |ref| + atol for EVERY element (ref_loss_optim.close_elementwise):
  * bf16 outputs: rtol = 2^-8, one round-to-nearest of a correct fp32 value (half an ulp of an 8-bit significand); atol covers what
    lies under that rounding (the fp32 chain, the fast exp / log).
  * fp32 outputs: rtol = 2^-22, i.e. four half-ulp roundings of fp32 -- the length of the shortest chains here (exp_avg: two
    products and a sum); atol carries the longer chains, cancellation, and row reductions.
"""
import torch

RTOL_BF16 = 2.0 ** -8
RTOL_F32 = 2.0 ** -22

# (rtol, atol) per kernel output; atol = 2 x the largest residual |got - ref| - rtol |ref| over every comparison of the GPU file,
# measured against the fp64 references on an MI355X (the case that gave it beside each; 0.0: no element ever left the rtol band).
# profiles/loss_optim_kernel_errors.md holds the table.
GATES = {
    "adamw.master": (RTOL_F32, 6.2e-09),      # measured 3.083e-09: grouped 32771 tiles step 1 grad_scale 1.0 clip above
    "adamw.m": (RTOL_F32, 1.3e-07),      # measured 6.211e-08: grouped 32771 tiles step 3 grad_scale 1.0 clip active
    "adamw.v": (RTOL_F32, 5.8e-11),      # measured 2.866e-11: grouped 32771 tiles step 3 grad_scale 1.0 clip active
    "ce.losses": (RTOL_F32, 1.4e-06),      # measured 6.617e-07: CE (300, 1024, 1024) weight=yes
    "ce.loss_sum": (RTOL_F32, 0.0),      # measured 0.000e+00: CE (3, 16384, 16384) weight=yes
    "ce.dlogits": (RTOL_BF16, 3.1e-39),      # measured 1.541e-39: CE (300, 1024, 1024) weight=None
    "soft_ce.losses": (RTOL_F32, 0.0),      # measured -1.524e-06: soft CE (5, 7)
    "soft_ce.dsim": (RTOL_BF16, 0.0),      # measured -3.549e-34: soft CE (33, 66)
    "soft_ce.dts": (RTOL_F32, 9e-06),      # measured 4.463e-06: soft CE (1, 8)
    "l2norm.norm": (RTOL_F32, 0.0),      # measured -2.344e-19: l2norm (5, 4)
    "l2norm.y": (RTOL_BF16, 0.0),      # measured 0.000e+00: l2norm (5, 4)
    "l2norm.dx": (RTOL_BF16, 0.0),      # measured -1.466e-11: l2norm (64, 2048)
}


# ------------------------------------------------------------------------------------------------------------------ shared cases
# Inputs of the GPU kernel tests, built once on the host from fixed seeds; the CPU file runs the torch stand-ins over the same
# inputs and through the same GATES, which shows that a correct implementation fits inside them.
TILE = 256
ADAMW_LRS = [1e-3, 1e-3, 1e-4, 3e-4]          # group 2: an lr_scale = 0.1 group; group 1: the no-decay group
ADAMW_WDS = [0.05, 0.0, 0.05, 0.01]
ADAMW_BETAS, ADAMW_EPS = (0.9, 0.999), 1e-6
# 1 / 2 / 7 / 9 tiles: some waves of the only workgroup return at once, odd counts end on a tile without a partner;
# 32768 + 3: past 4096 workgroups x 8 tiles, so the stride loop runs again and THAT pass ends on an unpaired tile
ADAMW_TILES = [1, 2, 7, 9, 32768 + 3]
ADAMW_STEPS = [1, 2, 3, 1000]
SENTINEL = {"master": 1234.5, "m": -7.25, "v": 3.5, "p16": -99.0}


def adamw_tile_groups(ntiles, seed=0):
    """uint8 [ntiles]: runs of varying length over groups 0..3, 255 (skip) on the first tile, on both tiles (4, 5) of one wave's
    pair, on the last tile of the 7-tile and the large map (9 tiles: the unpaired last tile is live), and on 0.5 % of a large map."""
    g = torch.Generator().manual_seed(1000 + seed + ntiles)
    if ntiles == 1:
        return torch.tensor([2], dtype=torch.uint8)
    if ntiles == 2:
        return torch.tensor([255, 1], dtype=torch.uint8)
    runs = torch.randint(1, max(2, min(200, ntiles // 3)), (ntiles,), generator=g)
    ids = torch.randint(0, 4, (ntiles,), generator=g).repeat_interleave(runs)[:ntiles].clone()
    ids[1], ids[2], ids[3], ids[6] = 1, 2, 3, 0          # every group is present in the smallest maps too
    ids[0] = ids[4] = ids[5] = 255
    if ntiles != 9:
        ids[ntiles - 1] = 255
    if ntiles > 1000:
        ids[torch.rand(ntiles, generator=g) < 0.005] = 255
        ids[32768], ids[32769] = 3, 1                      # the second pass of the stride loop starts on a live pair
    return ids.to(torch.uint8)


def adamw_case(ntiles, seed=0):
    """master / m / v fp32, p16 bf16, g bf16 and the tile map of one grouped step.  Skipped tiles hold SENTINEL values; `g` carries
    NaN there (nothing of a skipped tile may reach a store), `g_clean` zeros (what the engine's padding holds: the norm is taken
    from it)."""
    n = ntiles * TILE
    gen = torch.Generator().manual_seed(2000 + seed + ntiles)
    tg = adamw_tile_groups(ntiles, seed)
    dead = (tg >= 8).repeat_interleave(TILE)
    master = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.5
    v = torch.rand(n, generator=gen) * 2.0
    g = (torch.randn(n, generator=gen) * 3.0).to(torch.bfloat16)
    master[dead], m[dead], v[dead] = SENTINEL["master"], SENTINEL["m"], SENTINEL["v"]
    p16 = master.to(torch.bfloat16)
    p16[dead] = SENTINEL["p16"]
    g_clean = g.clone()
    g_clean[dead] = 0.0
    g = g.clone()
    g[dead] = float("nan")
    return {"master": master, "m": m, "v": v, "p16": p16, "g": g, "g_clean": g_clean, "tile_group": tg,
            "group": tg.to(torch.int64).repeat_interleave(TILE), "dead": dead}


# (rows, V, ld, first row kind, first label kind): V >= 16384 runs cross_entropy_kernel<1024>, below it <256>; ld > V leaves padding
# columns; 300 rows make weighted_sum_kernel's 256 threads wrap
CE_CASES = [(5, 51200, 51200, 0, 0), (3, 16384, 16384, 0, 5), (3, 16376, 16384, 2, 2), (4, 1024, 1032, 1, 3), (300, 1024, 1024, 0, 0)]
CE_PAD_SENTINEL = -123.0


def ce_case(rows, V, ld, kind0=0, lab0=0, seed=0):
    """-> logits bf16 [rows, ld] (NaN in the padding columns), labels int64 [rows], weight fp32 [rows].
    Row kinds, cycled from kind0: randn x 3 | all logits equal (loss = log V) | one logit of +60 over ~0, that logit the target |
    the same with another target | a row spanning about +-80.  Label kinds, cycled from lab0: 0, 7, 8, V - 1, V - 8 (chunk
    boundaries of the 8-wide loads), -100 and V (outside: zero loss, zero gradient), then random.  Every fourth row has weight 0."""
    gen = torch.Generator().manual_seed(3000 + seed + rows + V)
    lab_kinds = [0, 7, 8, V - 1, V - 8, -100, V]
    labels = torch.empty(rows, dtype=torch.int64)
    x = torch.empty(rows, V)
    for r in range(rows):
        k = lab0 + r
        labels[r] = lab_kinds[k % 9] if k % 9 < 7 else int(torch.randint(0, V, (1,), generator=gen))
        lab = int(labels[r]) if 0 <= int(labels[r]) < V else 5
        kind = (kind0 + r) % 5
        if kind == 0:
            x[r] = torch.randn(V, generator=gen) * 3.0
        elif kind == 1:
            x[r] = 1.5
        elif kind in (2, 3):
            x[r] = torch.randn(V, generator=gen) * 0.05
            x[r, lab if kind == 2 else (lab + 13) % V] = 60.0
        else:
            x[r] = torch.linspace(-80.0, 80.0, V)[torch.randperm(V, generator=gen)]
    logits = torch.full((rows, ld), float("nan"), dtype=torch.bfloat16)
    logits[:, :V] = x.to(torch.bfloat16)
    weight = (torch.rand(rows, generator=gen) + 0.5) / rows
    weight[2::4] = 0.0
    return logits, labels, weight


# (rows, cols); 64 columns are exactly one sweep of a wave, 65 / 66 / 200 leave a ragged last sweep, 7 and 8 less than one.
# (33, 66) models world = 2: col_ids = cat(row_ids, row_ids)
SOFT_CE_CASES = [(1, 8), (5, 7), (16, 64), (6, 65), (7, 200), (33, 66)]


def soft_ce_case(rows, cols, seed=0):
    """-> sim fp32 [rows, cols] (randn x 10), row_ids [rows], col_ids [cols] with duplicates; every row id occurs among the
    columns (the head gathers its own ids: retrieval.py), other columns carry ids no row has."""
    gen = torch.Generator().manual_seed(4000 + seed + rows * 1000 + cols)
    row_ids = torch.randint(0, rows // 2 + 1, (rows,), generator=gen) * 3 + 1
    if (rows, cols) == (33, 66):
        col_ids = torch.cat([row_ids, row_ids])
    else:
        extra = torch.randint(0, rows + 2, (cols - rows,), generator=gen) * 3 // 2          # a mix of present and absent ids
        col_ids = torch.cat([row_ids, extra])[torch.randperm(cols, generator=gen)]
    sim = torch.randn(rows, cols, generator=gen) * 10.0
    return sim, row_ids, col_ids, 0.5 / rows


L2NORM_ROWS = [1, 5, 7, 64]
L2NORM_COLS = [4, 256, 260, 768, 2048, 2052]          # a lane takes 4 columns, a wave 256 per sweep: less than one, one, ragged, ...


def l2norm_case(rows, cols, seed=0):
    """-> x, dy bf16 [rows, cols]: randn x 3; with 5 rows or more, row 1 is all zero (the eps clamp is active) and row 2 is of the
    order 1e-20 (its squares are fp32 subnormals)."""
    gen = torch.Generator().manual_seed(5000 + seed + rows * 10000 + cols)
    x = torch.randn(rows, cols, generator=gen) * 3.0
    if rows >= 5:
        x[1] = 0.0
        x[2] = torch.randn(cols, generator=gen) * 1e-20
    dy = torch.randn(rows, cols, generator=gen)
    return x.to(torch.bfloat16), dy.to(torch.bfloat16)


# (rows, cols, ld, source rows); the last one is past 16384 workgroups x 256 items of 4 columns: the grid-stride loop wraps
ROWS_CASES = [(5, 64, 64, 9), (7, 256, 320, 12), (8200, 2048, 2048, 8300)]


def rows_case(rows, cols, ld, nsrc, seed=0):
    """-> src bf16 [nsrc, ld], gather index [rows] WITH repeats, scatter index [rows]: distinct rows of [0, nsrc) in random order."""
    gen = torch.Generator().manual_seed(6000 + seed + rows)
    src = torch.randn(nsrc, ld, generator=gen).to(torch.bfloat16)
    gidx = torch.randint(0, nsrc, (rows,), generator=gen)
    gidx[rows // 2] = gidx[0]
    sidx = torch.randperm(nsrc, generator=gen)[:rows].contiguous()
    return src, gidx, sidx
