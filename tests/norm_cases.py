"""Shapes, inputs, gates and the case runners shared by tests/test_norm_kernels_gpu.py (the HIP kernels of csrc/norm.hip) and
tests/test_norm_refs_cpu.py (the torch stand-ins over the same cases), TEST INFRASTRUCTURE ONLY.  A runner takes the module that
provides the entry points (youku_mplug_amd.ops or tests/standin_ops.py) and a device, builds the case on the host from a fixed
seed, calls the entry point and compares every output with the fp64 references of tests/ref_norm.py through GATES -- one code path,
so the CPU stand-in check and the GPU kernel check cannot drift apart.

GATES: |got - ref| <= rtol |ref| + coef x scale for EVERY element.  rtol is the number format's (2^-8: one round-to-nearest to bf16;
2^-22 for the fp32 statistics); scale is the largest sum of absolute terms of the row (ref_norm.ln_fwd_scales / ln_bwd_scales; per
column for dgamma / dbeta); coef = 2 x the largest residual (|got - ref| - rtol |ref|) / scale measured against the fp64 references on
an MI355X (profiles/norm_kernel_errors.md), and never above COEF_CAP = 2^-12: a sixteenth of a bf16 ulp of the row's largest term."""
import math

import torch

import ref_norm as R
from loss_optim_cases import RTOL_BF16, RTOL_F32

BF = torch.bfloat16
IDENT = (0, 0, 0)
COEF_CAP = 2.0 ** -12

# (rtol, coef) per kernel output; beside each the measured residual / scale and the case that gave it (0.0: no element ever left the
# rtol band)
GATES = {
    "ln_fwd.y": (RTOL_BF16, 6.4e-08),          # measured 3.189e-08: ln_fwd 13x2568 eps 1e-06
    "ln_fwd.mean": (RTOL_F32, 3.1e-09),        # measured 1.571e-09: ln_fwd 13x2564 eps 1e-05
    "ln_fwd.rstd": (RTOL_F32, 1.8e-07),        # measured 9.126e-08: ln_fwd 13x4096 eps 1e-05
    "ln_bwd.dx": (RTOL_BF16, 3.5e-09),         # measured 1.771e-09: ln_bwd 13x4096 eps 1e-05 dparam None
    "ln_bwd.dgamma": (RTOL_BF16, 5.2e-06),     # measured 2.610e-06: ln_bwd 13x2560 eps 1e-05 dparam overwrite
    "ln_bwd.dbeta": (RTOL_BF16, 0.0),          # measured 0.000e+00: ln_bwd 13x2056 eps 1e-05 dparam overwrite (first of the cases at 0)
    "stream_fwd.y": (RTOL_BF16, 8.3e-08),      # measured 4.165e-08: stream_fwd 13x2560 h_in bf16 add True eps 1e-06
    "stream_fwd.mean": (RTOL_F32, 2e-07),      # measured 1.018e-07: stream_fwd 13x1016 h_in fp32 add True eps 1e-05
    "stream_fwd.rstd": (RTOL_F32, 0.0),        # measured -6.707e-08: stream_fwd 13x8 h_in fp32 add False eps 1e-05
    "stream_bwd.dx": (RTOL_BF16, 7.6e-06),     # measured 3.816e-06: stream_bwd 4099x64 eps 1e-05
}

# ------------------------------------------------------------------------------------------------------------------ case tables
ROWS = 13          # a dozen or so: every input kind three times, and the last workgroup keeps one live wave
EPSS = (1e-5, 1e-6)

# mpv_layernorm_fwd / _bwd, 16-byte family (cols % 8 == 0 and ldx % 8 == 0 and ldy % 8 == 0): n8 = ceil(cols / 512) picks
# ln_fwd8_kernel / ln_bwd8_kernel / ln_bwd8_plain_kernel <2> (n8 <= 2), <3>, <4>, <5>, <8> (n8 >= 6)
LN16_COLS = [
    8,           # <2>: a single 16-byte chunk, 63 idle lanes
    512,         # <2>: exactly one sweep of the wave
    520,         # <2>: the second sweep holds one live lane
    1024, 1032,  # <2> | <3>: the third sweep holds one live lane
    1536, 1544,  # <3> | <4>
    2048, 2056,  # <4> | <5>
    2560, 2568,  # <5> | <8>: sweep 6 holds one live lane, sweeps 7 and 8 are idle
    4096,        # <8>: the widest row, every sweep full
]
# 4-wide family (cols % 8 != 0, or a leading dimension that is a multiple of 4 only): nc = ceil(cols / 256) picks
# ln_fwd_kernel / ln_bwd_kernel <3> (nc <= 3), <6>, <8>, <10>, <16>
LN4_COLS = [
    4, 12,       # <3>: one and three 8-byte chunks
    252, 260,    # <3>: one sweep less a lane | one sweep and one lane
    764, 772,    # <3> | <6>: nc = 3 | 4
    1540,        # <8>: nc = 7
    2052,        # <10>: nc = 9
    2564,        # <16>: nc = 11
    4092,        # <16>: nc = 16, the last lane of the last sweep idle
]
# (cols, ld): 768 columns pushed onto the 4-wide kernels by ld = 772 | the 16-byte family with 8 padding columns.  The padding holds NaN
# on inputs and a sentinel on outputs
LN_PADDED = [(768, 772), (768, 776)]
# rows at 64 columns: a workgroup of four waves (a wave per row) whose waves partly return
LN_FEW_ROWS = [1, 3, 4, 5]
# rows at 8 columns on the forward: 4096 workgroups x 4 rows | the stride loop runs again for three rows
LN_FWD_MANY_ROWS = [16384, 16387]
# rows at 64 columns WITH parameter gradients: 64 | 65 partial rows (ln_dparam_reduce one-level | two-level, whose second level-1 group
# folds a single row); 768 workgroups x 4 rows | the prefetching kernel's stride loop runs and its last pass prefetches past `rows`
LN_BWD_DPARAM_ROWS = [256, 257, 3072, 3075]
# rows at 64 columns WITHOUT parameter gradients: the 1024-workgroup cap | past it
LN_BWD_PLAIN_ROWS = [4096, 4099]
# row maps: widths of the 16-byte and of the 4-wide family
LN_MAP_COLS = [200, 260]
# dropout (dx_drop of both backwards): one width per family below and above the one-sweep instances
LN_DROP_COLS = [520, 2568, 260, 2564]
DROP_PS = [0.1, 0.5]
DROP_SEED = (0x1234 << 32) | 0x9abcdef1          # above 2^32: both halves of the seed reach the hash
DROP_OFFSET = 123456                               # non-zero, even

# mpv_ln_stream_fwd(_drop): cols < 1024 runs the wave-per-row ln_stream_fwd_kernel<2>, cols >= 1024 ln_stream_fwd_wg_kernel
STREAM_FWD_COLS = [
    8, 512, 520, 1016,   # wave per row: one chunk | one sweep | one lane of the second sweep | the last lane of the second sweep idle
    1024,                # workgroup per row, two full waves
    1032,                # the third wave holds a single live lane
    2560,                # five waves
    4088,                # eight waves, the last lane idle
    4096,                # eight full waves
]
# mpv_ln_stream_bwd: ln_bwd8_plain_kernel<2 | 4 | 5 | 8, XF32> by n8 = ceil(cols / 512) (there is no <3> on this entry)
STREAM_BWD_COLS = [8, 1024, 1032, 2048, 2056, 2560, 2568, 4096]      # <2>, <2> | <4>, <4> | <5>, <5> | <8>, <8>
# the workgroup-per-row kernel's grid (65536) wraps: bf16 h_in, no add
STREAM_WRAP = (65536 + 3, 1024)

SENT_BF, SENT_F32 = -99.0, 1234.5
KINDS_BF16 = ("randn3", "const", "mean64", "small")
KINDS_F32 = KINDS_BF16 + ("mean1e3", "outlier")
CONST = 1.5


# ------------------------------------------------------------------------------------------------------------------ inputs
def ln_input(rows, cols, kinds, gen, kind0=0):
    """fp32 [rows, cols], the kinds cycled over the rows from kind0: randn x 3 | a constant row (rstd = eps^-1/2, y = beta) | mean 64,
    unit spread | values of order 1e-3 | (fp32 stream) mean 1e3, unit spread | one 1e4 outlier channel among unit ones.
    -> (x, names of the rows' kinds)"""
    x = torch.empty(rows, cols)
    names = []
    for r in range(rows):
        k = kinds[(kind0 + r) % len(kinds)]
        names.append(k)
        v = torch.randn(cols, generator=gen)
        if k == "randn3":
            v = v * 3.0
        elif k == "const":
            v = torch.full((cols,), CONST)
        elif k == "mean64":
            v = v + 64.0
        elif k == "small":
            v = v * 1e-3
        elif k == "mean1e3":
            v = v + 1e3
        else:
            v[int(torch.randint(0, cols, (1,), generator=gen))] = 1e4
        x[r] = v
    return x, names


def ln_params(cols, gen):
    """gamma = 1 + 0.1 randn with two exact zeros (first and last column) and one negative entry, beta = 0.1 randn; bf16"""
    gamma = 1.0 + 0.1 * torch.randn(cols, generator=gen)
    gamma[0] = gamma[cols - 1] = 0.0
    gamma[cols // 2] = -gamma[cols // 2].abs()
    return gamma.to(BF), (0.1 * torch.randn(cols, generator=gen)).to(BF)


def map_rows(m, n):
    g, s, o = m
    r = torch.arange(n, dtype=torch.int64)
    return r if g == 0 else (r // g) * s + (r % g) + o


def place(t, m, ld, fill):
    """t [n, cols] laid out behind a row map with row pitch ld: every element outside the mapped rows' first cols columns is `fill`
    (NaN for an input: nothing of it may reach a result; a sentinel for an output).  An unmapped buffer gets no extra row."""
    n, cols = t.shape
    idx = map_rows(m, n)
    buf = torch.full((int(idx.max()) + 1 + (1 if m[0] else 0), ld), fill, dtype=t.dtype)
    buf[idx, :cols] = t
    return buf


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def take(buf, m, n, cols):
    return buf[map_rows(m, n).to(buf.device), :cols]


def assert_untouched(buf, m, n, cols, sentinel, what):
    """every element outside the mapped rows' first cols columns still holds the sentinel's bits"""
    mask = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    mask[map_rows(m, n).to(buf.device), :cols] = True
    rest = buf[~mask]
    assert same_bits(rest, torch.full_like(rest, sentinel)), f"{what}: written outside the mapped rows / columns"


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * p for k, p in zip(key, (1, 10007, 1000003, 7919))) % (2 ** 31))


def _ulps(a, b):
    return (bits(a).to(torch.int64) - bits(b).to(torch.int64)).abs().max().item()


def check_const_rstd(rstd, names, eps, what):
    """a constant row: the variance is exactly 0, so rstd = rsqrt(eps): the same bits on every such row, and within one fp32 ulp of
    the correctly rounded eps^-1/2 (the accuracy of the hardware's reciprocal square root)"""
    c = [i for i, k in enumerate(names) if k == "const"]
    if not c:
        return
    got = rstd[c].float().cpu()
    want = torch.full_like(got, 1.0 / math.sqrt(R.f32(eps)))
    assert same_bits(got, got[:1].expand_as(got).contiguous()), f"{what}: rstd differs among constant rows"
    assert _ulps(got, want) <= 1, f"{what}: rstd of a constant row {got[0].item()!r} is not eps^-1/2 = {want[0].item()!r}"


# ------------------------------------------------------------------------------------------------------------------ runners
def run_ln_fwd(ops, dev, rows, cols, eps, *, ldx=None, ldy=None, xmap=IDENT, ymap=IDENT, kind0=0):
    """ops.layernorm_fwd on one case: y, mean, rstd against ln_fwd_ref; y of a constant row == beta bit for bit; nothing outside the
    mapped rows and the first cols columns is written; want_stats=False gives the same y bit for bit."""
    tag = f"ln_fwd {rows}x{cols} ld {ldx or cols}/{ldy or cols} eps {eps:g} xmap {xmap} ymap {ymap}"
    gen = _gen(rows, cols, ldx or 0, 1)
    x, names = ln_input(rows, cols, KINDS_BF16, gen, kind0)
    x = x.to(BF)
    gamma, beta = ln_params(cols, gen)
    xbuf = place(x, xmap, ldx or cols, float("nan")).to(dev)
    x, gamma, beta = x.to(dev), gamma.to(dev), beta.to(dev)
    outs = []
    for want_stats in (True, False):
        ybuf = place(torch.full((rows, cols), SENT_BF, dtype=BF), ymap, ldy or cols, SENT_BF).to(dev)
        _, mean, rstd = ops.layernorm_fwd(xbuf, gamma, beta, eps, rows, cols, out=ybuf, xmap=xmap, ymap=ymap, ldx=ldx, ldy=ldy,
                                          want_stats=want_stats)
        outs.append((ybuf, mean, rstd))
    (ybuf, mean, rstd), (ybuf2, mean2, rstd2) = outs
    assert mean2 is None and rstd2 is None
    assert same_bits(ybuf, ybuf2), f"{tag}: want_stats=False changed y"
    ry, rmean, rrstd = R.ln_fwd_ref(x, gamma, beta, R.f32(eps))
    sy, smean, srstd = R.ln_fwd_scales(x, gamma, beta, rmean, rrstd)
    y = take(ybuf, ymap, rows, cols)
    R.close_scaled(y, ry, sy, GATES["ln_fwd.y"], f"ln_fwd.y | {tag}")
    R.close_scaled(mean, rmean, smean, GATES["ln_fwd.mean"], f"ln_fwd.mean | {tag}")
    R.close_scaled(rstd, rrstd, srstd, GATES["ln_fwd.rstd"], f"ln_fwd.rstd | {tag}")
    assert_untouched(ybuf, ymap, rows, cols, SENT_BF, tag)
    c = [i for i, k in enumerate(names) if k == "const"]
    if c:
        assert same_bits(y[c], beta[None, :].expand(len(c), cols).contiguous()), f"{tag}: y of a constant row is not beta"
    check_const_rstd(rstd, names, eps, tag)


def run_ln_bwd(ops, dev, rows, cols, eps, *, stream=False, dparam=None, ldx=None, ldy=None, xmap=IDENT, ymap=IDENT, dres=True,
               drop_p=0.0, kind0=0):
    """ops.layernorm_bwd (stream: ops.ln_stream_bwd, x fp32) on one case.  The kernel is given the fp32 roundings of the fp64
    statistics; dx, dgamma, dbeta against ln_bwd_ref on the fp64 ones.  dparam: None (the frozen decoder) | "overwrite" | "accumulate"
    (dgamma / dbeta start from randn) | "defer" (through LnDparamBatch, three calls folded by one finish).  drop_p > 0: dx_drop ==
    bf16(float(dx) * fp32(1 / (1 - p))) where keep_mask keeps (index: the ROW NUMBER r, not the mapped row), +0 elsewhere, bit for bit,
    and the dropped fraction within 4 sigma of thr / 65536.  The first constant row has dy = 0: its dx is the residual gradient exactly."""
    key = "stream_bwd" if stream else "ln_bwd"
    lx, ly = ldx or cols, ldy or cols
    tag = f"{key} {rows}x{cols} ld {lx}/{ly} eps {eps:g} dparam {dparam} xmap {xmap} ymap {ymap} dres {dres} p {drop_p}"
    gen = _gen(rows, cols, lx, 2 + int(stream))
    x, names = ln_input(rows, cols, KINDS_F32 if stream else KINDS_BF16, gen, kind0)
    x = x if stream else x.to(BF)
    gamma, _ = ln_params(cols, gen)
    dy = torch.randn(rows, cols, generator=gen).to(BF)
    c0 = names.index("const") if "const" in names else None
    if c0 is not None:
        dy[c0] = 0.0
    dr = torch.randn(rows, cols, generator=gen).to(BF) if dres else None
    dg0 = torch.randn(cols, generator=gen).to(BF)
    db0 = torch.randn(cols, generator=gen).to(BF)
    nan = float("nan")
    xbuf, dybuf = place(x, xmap, lx, nan).to(dev), place(dy, ymap, ly, nan).to(dev)
    drbuf = place(dr, xmap, lx, nan).to(dev) if dres else None
    x, dy, gamma, dg0, db0 = x.to(dev), dy.to(dev), gamma.to(dev), dg0.to(dev), db0.to(dev)
    dr = dr.to(dev) if dres else None
    _, mean, rstd = R.ln_fwd_ref(x, gamma, gamma, R.f32(eps))
    mean32, rstd32 = mean.float(), rstd.float()
    blank = torch.full((rows, cols), SENT_BF, dtype=BF)
    dxbuf = place(blank, xmap, lx, SENT_BF).to(dev)
    ddbuf = place(blank, xmap, lx, SENT_BF).to(dev) if drop_p > 0 else None
    kw = dict(dres=drbuf, dx=dxbuf, dx_drop=ddbuf, dropout_p=drop_p, seed=DROP_SEED if drop_p > 0 else 0,
              offset=DROP_OFFSET if drop_p > 0 else 0, xmap=xmap, ymap=ymap)
    acc = dparam == "accumulate"
    dgamma = dbeta = None
    if stream:
        assert dparam is None and ldx is None and ldy is None
        ops.ln_stream_bwd(dybuf, xbuf, gamma, mean32, rstd32, rows, cols, **kw)
    elif dparam is None:
        ops.layernorm_bwd(dybuf, xbuf, gamma, mean32, rstd32, rows, cols, ldx=ldx, ldy=ldy, **kw)
    elif dparam in ("overwrite", "accumulate"):
        dgamma = dg0.clone() if acc else torch.full_like(dg0, SENT_BF)
        dbeta = db0.clone() if acc else torch.full_like(db0, SENT_BF)
        ops.layernorm_bwd(dybuf, xbuf, gamma, mean32, rstd32, rows, cols, ldx=ldx, ldy=ldy, dgamma=dgamma, dbeta=dbeta,
                          accumulate_dparams=acc, **kw)
    else:
        # three entries of one batch: this case overwriting, the same case accumulating, and its first rows only (another number
        # of partial rows) -- folded by ONE finish
        assert dparam == "defer"
        batch = ops.LnDparamBatch()
        few = max(1, rows // 3)
        pairs = [(torch.full_like(dg0, SENT_BF), torch.full_like(db0, SENT_BF), False, rows), (dg0.clone(), db0.clone(), True, rows),
                 (torch.full_like(dg0, SENT_BF), torch.full_like(db0, SENT_BF), False, few)]
        for dgm, dbt, a, n in pairs:
            if n != rows:
                kw["dx"] = dxbuf.clone()
            ops.layernorm_bwd(dybuf, xbuf, gamma, mean32, rstd32, n, cols, ldx=ldx, ldy=ldy, dgamma=dgm, dbeta=dbt, accumulate_dparams=a,
                              defer=batch, **kw)
        assert same_bits(pairs[0][0], torch.full_like(dg0, SENT_BF)), f"{tag}: a deferred call wrote dgamma before finish()"
        batch.finish()
        for dgm, dbt, a, n in pairs[1:]:
            args = (dy[:n], x[:n], gamma, mean[:n], rstd[:n], None, dg0 if a else None, db0 if a else None)
            _, rg, rb = R.ln_bwd_ref(*args)
            _, sg, sb = R.ln_bwd_scales(*args)
            R.close_scaled(dgm, rg, sg, GATES["ln_bwd.dgamma"], f"ln_bwd.dgamma | {tag} deferred entry accumulate {a} rows {n}")
            R.close_scaled(dbt, rb, sb, GATES["ln_bwd.dbeta"], f"ln_bwd.dbeta | {tag} deferred entry accumulate {a} rows {n}")
        dgamma, dbeta = pairs[0][0], pairs[0][1]
    args = (dy, x, gamma, mean, rstd, dr, dg0 if acc else None, db0 if acc else None)
    rdx, rdg, rdb = R.ln_bwd_ref(*args)
    sdx, sdg, sdb = R.ln_bwd_scales(*args)
    dx = take(dxbuf, xmap, rows, cols)
    R.close_scaled(dx, rdx, sdx, GATES[f"{key}.dx"], f"{key}.dx | {tag}")
    assert_untouched(dxbuf, xmap, rows, cols, SENT_BF, tag)
    if dgamma is not None:
        R.close_scaled(dgamma, rdg, sdg, GATES["ln_bwd.dgamma"], f"ln_bwd.dgamma | {tag}")
        R.close_scaled(dbeta, rdb, sdb, GATES["ln_bwd.dbeta"], f"ln_bwd.dbeta | {tag}")
    if c0 is not None:
        want = dr[c0] if dres else torch.zeros(cols, dtype=BF, device=dev)
        assert torch.equal(dx[c0], want), f"{tag}: dx of a constant row with dy = 0 is not the residual gradient"
    if drop_p > 0:
        keep = R.keep_mask(DROP_SEED, DROP_OFFSET, rows, cols, drop_p, device=dev)
        sc = torch.tensor(R.drop_scale(drop_p), dtype=torch.float32, device=dev)
        want = torch.where(keep, (dx.float() * sc).to(BF), torch.zeros_like(dx))
        assert same_bits(take(ddbuf, xmap, rows, cols), want), f"{tag}: dx_drop is not the masked, scaled dx"
        assert_untouched(ddbuf, xmap, rows, cols, SENT_BF, tag + " dx_drop")
        check_drop_fraction(keep, drop_p, tag)


def check_drop_fraction(keep, p, what):
    n, q = keep.numel(), R.drop_threshold(p) / 65536.0
    frac = 1.0 - keep.float().mean().item()
    assert abs(frac - q) <= 4.0 * math.sqrt(q * (1.0 - q) / n), f"{what}: dropped {frac:.5f} of {n}, expected {q:.5f}"


def stream_case(rows, cols, inbf, kind0=0, with_add=True):
    gen = _gen(rows, cols, int(inbf), 5)
    h, names = ln_input(rows, cols, KINDS_BF16 if inbf else KINDS_F32, gen, kind0)
    h = h.to(BF) if inbf else h
    gamma, beta = ln_params(cols, gen)
    add = (torch.randn(rows, cols, generator=gen) * 2.0).to(BF) if with_add else None
    return h, add, gamma, beta, names


def run_stream_fwd(ops, dev, rows, cols, eps, *, inbf=False, with_add=True, hmap=IDENT, amap=IDENT, ymap=IDENT, drop_p=0.0, kind0=0):
    """ops.ln_stream_fwd on one case: h_out == stream_ref bit for bit (with dropout: the addend built with keep_mask over the rows of
    `add`, i.e. the index uses the MAPPED row of add); y, mean, rstd against ln_fwd_ref of that exact sum; rows outside a map untouched."""
    tag = f"stream_fwd {rows}x{cols} h_in {'bf16' if inbf else 'fp32'} add {with_add} eps {eps:g} hmap {hmap} amap {amap} ymap {ymap} p {drop_p}"
    h, add, gamma, beta, names = stream_case(rows, cols, inbf, kind0, with_add)
    nan = float("nan")
    hbuf = place(h, hmap, cols, nan).to(dev)
    abuf = place(add, amap, cols, nan).to(dev) if with_add else None
    h, gamma, beta = h.to(dev), gamma.to(dev), beta.to(dev)
    ybuf = place(torch.full((rows, cols), SENT_BF, dtype=BF), ymap, cols, SENT_BF).to(dev)
    hobuf = torch.full(hbuf.shape, SENT_F32, dtype=torch.float32, device=dev) if with_add else None
    kw = dict(add_dropout_p=drop_p, seed=DROP_SEED, offset=DROP_OFFSET) if drop_p > 0 else {}
    _, ho, mean, rstd = ops.ln_stream_fwd(hbuf, abuf, gamma, beta, eps, rows, cols, h_out=hobuf, out=ybuf, hmap=hmap, amap=amap, ymap=ymap, **kw)
    if with_add:
        keep = None
        if drop_p > 0:
            keep = take(R.keep_mask(DROP_SEED, DROP_OFFSET, abuf.shape[0], cols, drop_p, device=dev), amap, rows, cols)
            check_drop_fraction(keep, drop_p, tag)
        v = R.stream_ref(h, add.to(dev), keep, R.drop_scale(drop_p))
        assert ho is hobuf
        assert same_bits(take(hobuf, hmap, rows, cols), v), f"{tag}: h_out is not the fp32 sum"
        assert_untouched(hobuf, hmap, rows, cols, SENT_F32, tag + " h_out")
    else:
        assert ho is None
        v = h
    ry, rmean, rrstd = R.ln_fwd_ref(v, gamma, beta, R.f32(eps))
    sy, smean, srstd = R.ln_fwd_scales(v, gamma, beta, rmean, rrstd)
    R.close_scaled(take(ybuf, ymap, rows, cols), ry, sy, GATES["stream_fwd.y"], f"stream_fwd.y | {tag}")
    R.close_scaled(mean, rmean, smean, GATES["stream_fwd.mean"], f"stream_fwd.mean | {tag}")
    R.close_scaled(rstd, rrstd, srstd, GATES["stream_fwd.rstd"], f"stream_fwd.rstd | {tag}")
    assert_untouched(ybuf, ymap, rows, cols, SENT_BF, tag)
    if not with_add:
        c = [i for i, k in enumerate(names) if k == "const"]
        assert same_bits(take(ybuf, ymap, rows, cols)[c], beta[None, :].expand(len(c), cols).contiguous()), f"{tag}: y of a constant row is not beta"
        check_const_rstd(rstd, names, eps, tag)


def run_stream_drop_equals_prebuilt(ops, dev, rows, cols, eps, p, *, inbf=False, amap=IDENT):
    """mpv_ln_stream_fwd_drop(h, add, p, seed, offset) == mpv_ln_stream_fwd(h, addend) bit for bit in h_out, y, mean and rstd, the
    addend built on the host with keep_mask: bf16(add * scale) where kept, +0 elsewhere."""
    h, add, gamma, beta, _ = stream_case(rows, cols, inbf)
    abuf = place(add, amap, cols, 0.0).to(dev)
    keep = R.keep_mask(DROP_SEED, DROP_OFFSET, abuf.shape[0], cols, p, device=dev)
    pre = R.dropped_addend(abuf, keep, R.drop_scale(p)).to(BF)
    h, gamma, beta = h.to(dev), gamma.to(dev), beta.to(dev)
    a = ops.ln_stream_fwd(h, abuf, gamma, beta, eps, rows, cols, amap=amap, add_dropout_p=p, seed=DROP_SEED, offset=DROP_OFFSET)
    b = ops.ln_stream_fwd(h, pre, gamma, beta, eps, rows, cols, amap=amap)
    for name, u, v in zip(("y", "h_out", "mean", "rstd"), a, b):
        assert same_bits(u, v), f"stream drop {rows}x{cols} p {p} amap {amap}: {name} differs from the pre-dropped addend's"
    c = ops.ln_stream_fwd(h, abuf, gamma, beta, eps, rows, cols, amap=amap)
    assert not torch.equal(a[1], c[1]), "the dropout did nothing"


def run_stream_wrap(ops, dev):
    """STREAM_WRAP: more rows than the workgroup-per-row kernel's grid.  Built and compared on the device, the fp64 reference formed
    in chunks of 8192 rows; kinds cycled as in ln_input (randn x 3 | constant | mean 64 | order 1e-3)."""
    rows, cols = STREAM_WRAP
    g = torch.Generator(device=dev).manual_seed(77)
    kind = torch.arange(rows, device=dev) % 4
    scale = torch.tensor([3.0, 0.0, 1.0, 1e-3], device=dev)[kind][:, None]
    shift = torch.tensor([0.0, CONST, 64.0, 0.0], device=dev)[kind][:, None]
    h = (torch.randn(rows, cols, device=dev, generator=g) * scale + shift).to(BF)
    gamma, beta = (t.to(dev) for t in ln_params(cols, _gen(rows, cols)))
    y, ho, mean, rstd = ops.ln_stream_fwd(h, None, gamma, beta, 1e-5, rows, cols)
    assert ho is None and y.shape == (rows, cols)
    tag = f"stream_fwd {rows}x{cols} h_in bf16 add False (grid wraps)"
    for lo in range(0, rows, 8192):
        s = slice(lo, min(rows, lo + 8192))
        ry, rmean, rrstd = R.ln_fwd_ref(h[s], gamma, beta, R.f32(1e-5))
        sy, smean, srstd = R.ln_fwd_scales(h[s], gamma, beta, rmean, rrstd)
        R.close_scaled(y[s], ry, sy, GATES["stream_fwd.y"], f"stream_fwd.y | {tag} rows {lo}+")
        R.close_scaled(mean[s], rmean, smean, GATES["stream_fwd.mean"], f"stream_fwd.mean | {tag} rows {lo}+")
        R.close_scaled(rstd[s], rrstd, srstd, GATES["stream_fwd.rstd"], f"stream_fwd.rstd | {tag} rows {lo}+")
    c = kind == 1
    assert same_bits(y[c], beta[None, :].expand(int(c.sum()), cols).contiguous()), f"{tag}: y of a constant row is not beta"


# ------------------------------------------------------------------------------------------------------------------ the runs
# (id, runner, args, kwargs): what both test files parametrise over.  XMAP skips every fifth row of its buffer; the backwards read dy
# through a DIFFERENT map; the forward's YMAP is one group of all rows behind a leading sentinel row
XMAP, YMAP_BWD, AMAP = (4, 5, 1), (3, 5, 2), (3, 4, 2)
YMAP_ALL = (ROWS, ROWS + 1, 1)


def _runs():
    fwd, bwd, sf, sb = [], [], [], []
    for i, c in enumerate(LN16_COLS + LN4_COLS):
        for eps in EPSS:
            fwd.append((f"{c}-eps{eps:g}", (ROWS, c, eps), dict(kind0=i)))
            for dp in (None, "overwrite"):
                bwd.append((f"{c}-eps{eps:g}-{dp}", (ROWS, c, eps), dict(dparam=dp, kind0=i)))
    for c in (8, 520, 1032, 2568, 4, 260, 2564):          # both families, the prefetching <2> and the one-row instances
        for dp in ("accumulate", "defer"):
            bwd.append((f"{c}-{dp}", (ROWS, c, 1e-5), dict(dparam=dp)))
    for c, ld in LN_PADDED:
        fwd.append((f"{c}-ld{ld}", (ROWS, c, 1e-5), dict(ldx=ld, ldy=ld)))
        for dp in (None, "overwrite", "defer"):
            bwd.append((f"{c}-ld{ld}-{dp}", (ROWS, c, 1e-5), dict(ldx=ld, ldy=ld, dparam=dp)))
        bwd.append((f"{c}-ld{ld}-drop", (ROWS, c, 1e-5), dict(ldx=ld, ldy=ld, dparam="overwrite", drop_p=0.1)))
    for r in LN_FEW_ROWS:
        fwd.append((f"rows{r}", (r, 64, 1e-6), dict(kind0=r)))
        for dp in (None, "overwrite", "defer"):
            bwd.append((f"rows{r}-{dp}", (r, 64, 1e-6), dict(dparam=dp, kind0=r)))
        for inbf in (False, True):
            sf.append((f"rows{r}-{'bf16' if inbf else 'fp32'}", (r, 64, 1e-6), dict(inbf=inbf, kind0=r)))
            sf.append((f"rows{r}x1032-{'bf16' if inbf else 'fp32'}", (r, 1032, 1e-6), dict(inbf=inbf, kind0=r)))
        sb.append((f"rows{r}", (r, 64, 1e-6), dict(stream=True, kind0=r)))
    for r in LN_FWD_MANY_ROWS:
        fwd.append((f"rows{r}x8", (r, 8, 1e-5), {}))
    for r in LN_BWD_DPARAM_ROWS:
        bwd.append((f"rows{r}-overwrite", (r, 64, 1e-5), dict(dparam="overwrite")))
    bwd.append(("rows257-accumulate", (257, 64, 1e-5), dict(dparam="accumulate")))
    bwd.append(("rows257-defer", (257, 64, 1e-5), dict(dparam="defer")))
    bwd.append(("rows3075-defer", (3075, 64, 1e-5), dict(dparam="defer")))
    for r in LN_BWD_PLAIN_ROWS:
        bwd.append((f"rows{r}-None", (r, 64, 1e-5), dict(dparam=None)))
        sb.append((f"rows{r}", (r, 64, 1e-5), dict(stream=True)))
    for c in LN_MAP_COLS:
        fwd.append((f"{c}-maps", (ROWS, c, 1e-6), dict(xmap=XMAP, ymap=YMAP_ALL)))
        for dp in (None, "overwrite"):
            bwd.append((f"{c}-maps-{dp}", (ROWS, c, 1e-6), dict(xmap=XMAP, ymap=YMAP_BWD, dparam=dp)))
            bwd.append((f"{c}-maps-{dp}-drop", (ROWS, c, 1e-6), dict(xmap=XMAP, ymap=YMAP_BWD, dparam=dp, drop_p=0.1)))
    for c in LN_DROP_COLS:
        for p in DROP_PS:
            for dp in (None, "overwrite"):
                bwd.append((f"{c}-p{p}-{dp}", (ROWS, c, 1e-5), dict(dparam=dp, drop_p=p)))
    for c in (520, 260):
        bwd.append((f"{c}-nodres", (ROWS, c, 1e-5), dict(dres=False)))
    for i, c in enumerate(STREAM_FWD_COLS):
        for inbf in (False, True):
            for eps in EPSS:
                sf.append((f"{c}-{'bf16' if inbf else 'fp32'}-eps{eps:g}", (ROWS, c, eps), dict(inbf=inbf, kind0=i)))
        if c in (8, 520, 1032, 4096):
            for inbf in (False, True):
                sf.append((f"{c}-{'bf16' if inbf else 'fp32'}-noadd", (ROWS, c, 1e-5), dict(inbf=inbf, with_add=False)))
    for c in (520, 1032):          # the wave-per-row and the workgroup-per-row kernel
        for p in (0.0, 0.1):
            sf.append((f"{c}-maps-p{p}", (ROWS, c, 1e-5), dict(hmap=XMAP, amap=AMAP, ymap=YMAP_ALL, drop_p=p)))
        sf.append((f"{c}-maps-bf16", (ROWS, c, 1e-5), dict(inbf=True, hmap=XMAP, amap=AMAP, ymap=YMAP_ALL)))
        sb.append((f"{c}-maps", (ROWS, c, 1e-5), dict(stream=True, xmap=XMAP, ymap=YMAP_BWD)))
        sb.append((f"{c}-maps-drop", (ROWS, c, 1e-5), dict(stream=True, xmap=XMAP, ymap=YMAP_BWD, drop_p=0.1)))
    for c in (520, 1032, 4096):
        for p in DROP_PS:
            sf.append((f"{c}-p{p}", (ROWS, c, 1e-5), dict(drop_p=p)))
    for i, c in enumerate(STREAM_BWD_COLS):
        for eps in EPSS:
            sb.append((f"{c}-eps{eps:g}", (ROWS, c, eps), dict(stream=True, kind0=i)))
    for c in (1024, 2568):
        for p in DROP_PS:
            sb.append((f"{c}-p{p}", (ROWS, c, 1e-5), dict(stream=True, drop_p=p)))
    sb.append(("1032-nodres", (ROWS, 1032, 1e-5), dict(stream=True, dres=False)))
    return fwd, bwd, sf, sb


LN_FWD_RUNS, LN_BWD_RUNS, STREAM_FWD_RUNS, STREAM_BWD_RUNS = _runs()
# (rows, cols, p, h_in bf16, amap): mpv_ln_stream_fwd_drop against the pre-dropped addend, both kernels, unmapped and through an amap
STREAM_DROP_EQ = [(ROWS, 520, 0.1, False, IDENT), (ROWS, 520, 0.5, True, AMAP), (ROWS, 1032, 0.5, False, IDENT), (ROWS, 1032, 0.1, False, AMAP),
                  (ROWS, 4096, 0.1, True, IDENT)]
