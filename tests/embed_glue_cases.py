"""Shapes, inputs, gates and the case runners shared by tests/test_embed_glue_kernels_gpu.py (the HIP kernels of csrc/elementwise.hip
and csrc/glue.hip that no other suite covers) and tests/test_embed_glue_refs_cpu.py (the torch stand-ins over the same cases), TEST
INFRASTRUCTURE ONLY.  A runner takes the module that provides the entry points (youku_mplug_amd.ops or tests/standin_ops.py) and a
device, builds the case from a fixed seed (on the host; the few cases past a grid cap on the device), calls the entry point and compares
every output with the fp64 references of tests/ref_embed_glue.py -- one code path for the kernels and the stand-ins.

GATES: |got - ref| <= rtol |ref| + atol for EVERY element; every number is derived, none is fitted to a kernel:
  moves            raw bits (im2col, row / segment copies, dpatch, token rows of the merge backward, saved, store_words, f32_to_bf16,
                   accum_f32, dropped positions, output padding and rows outside a map: "untouched" is compared on the bits too)
  "one_op"         one fp32 operation on bf16 inputs, then one rounding: rtol = 2^-8 + 2^-23 (half a bf16 ulp, plus the fp32 rounding
                   underneath that can move a tie), atol 0.  Where the operation documents two bf16 roundings the reference performs
                   the inner one itself; where the inner one rounds an fp32 SUM (the cls mean of the merge forward) either rounding
                   is accepted for an element whose fp64 mean lies within the fp32 sum's error bound of a bf16 tie (ref r16_both)
  "sum"            sums into bf16: rtol = 2^-8, atol = n 2^-24 sum|terms|, both per output element from the reference: the worst-case
                   bound of an fp32 sum of n terms in any order.  (close_scaled divides by that atol: the printed residual is the
                   fraction of it an element used; the coefficient is 1.)  A mean's n counts its T terms plus the rounding of 1 / T
                   and of the product
  "caption.weights" rtol = 2^-23: one fp32 division of exact integers;  labels exact
  "topk.values"    loss_optim_cases.GATES["ce.losses"] = (2^-22, 1.4e-6): the project's gate of the same __expf / __logf chain --
                   WIDENED per row by 2^-24 (|lse| + |lse - add|), lse the row's fp64 log-sum-exp (topk_atol; never above 10 x 1.4e-6:
                   asserted).  Why: every row but the +-80 ones fits the CE gate as it stands; those left it by up to 3.7e-6
                   (profiles/embed_glue_kernel_errors.md).  logprob_topk_merge_kernel forms lse = gmax + __logf(se) - add in fp32 and
                   then subtracts it from the logit: the two roundings happen at the magnitude of lse (half an fp32 ulp each: 3.8e-6
                   in the binade of 64), and the difference of two numbers of that size keeps them whole.  The cross-entropy kernel
                   has the same form; its cases hold logits of order 3
Dropout: seed above 2^32, offset even (mpv_common.h mpv_dropout_vec: the index of a vector's first element is even) and no multiple of 8."""
import torch

import ref_embed_glue as R
from loss_optim_cases import GATES as LO_GATES, RTOL_BF16
from norm_cases import DROP_SEED, IDENT, SENT_BF, _gen, assert_untouched, bits, map_rows, place, same_bits, take  # noqa: F401

BF = torch.bfloat16
F64 = torch.float64
NAN = float("nan")
GATES = {
    "one_op": (2.0 ** -8 + 2.0 ** -23, 0.0),
    "sum": (RTOL_BF16, 1.0),                      # x n 2^-24 sum|terms| (close_sum)
    "caption.weights": (2.0 ** -23, 0.0),
    "topk.values": LO_GATES["ce.losses"],
}
DROP_OFFSET = 123458          # even, 2 mod 8
EW_CAP = 16384 * 256          # ew_grid: work items of one sweep of the capped grid (elementwise.hip)
STREAM_CAP = 8192 * 256       # stream_grid (glue.hip), items of 8 elements
BAN = torch.finfo(BF).min     # generation.BAN_BEAM: the lowest finite bf16


# ------------------------------------------------------------------------------------------------------------------ helpers
def rnb(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


def big_randn(dev, seed, n):
    """n bf16 normal values made on the device (the cases past a grid cap: tens of MB)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, device=dev, generator=g).to(BF)


def close_one(got, ref, what):
    R.close_elementwise(got, ref, *GATES["one_op"], what)


def close_sum(got, ref, absum, n, what):
    R.close_scaled(got.reshape(-1), ref.reshape(-1), (absum * (n * 2.0 ** -24)).reshape(-1), GATES["sum"], what)


def sentinel_tail(buf, n, what, sent=SENT_BF):
    """everything of the flat buffer from element n on still holds the sentinel's bits"""
    rest = buf.reshape(-1)[n:]
    assert same_bits(rest, torch.full_like(rest, sent)), f"{what}: written behind the output"


# ------------------------------------------------------------------------------------------------------------------ im2col
def run_im2col(ops, dev, B, C, T, H, W, P, kpad, *, misalign=False, on_device=False):
    """cols == im2col_ref bit for bit (zero padding included).  misalign: the same values again through a view whose address is only
    2-byte aligned (the element-wise kernel): the same bits as the aligned call's."""
    tag = f"im2col {B}x{C}x{T}x{H}x{W} P {P} kpad {kpad}"
    n = B * C * T * H * W
    flat = big_randn(dev, n % 1000003, n) if on_device else rnb(_gen(B, T, H * W, P), n).to(dev)
    video = flat.view(B, C, T, H, W)
    assert video.data_ptr() % 16 == 0
    want = R.im2col_ref(video, B, C, T, H, W, P, kpad)
    got = ops.im2col_patches(video, B, C, T, H, W, P, kpad)
    assert same_bits(got, want), f"{tag}: differs from the index-built reference"
    if misalign:
        shifted = torch.empty(n + 8, dtype=BF, device=dev)
        shifted[1:n + 1] = flat
        v2 = shifted[1:n + 1].view(B, C, T, H, W)
        assert v2.data_ptr() % 16 == 2
        got2 = ops.im2col_patches(v2, B, C, T, H, W, P, kpad)
        assert same_bits(got2, want) and same_bits(got2, got), f"{tag}: the 2-byte aligned view gives other bits"


IM2COL_RUNS = [
    ("p16-kpadK-HneW", (2, 3, 2, 32, 48, 16, 768), {}),                     # im2col8_kernel, kpad = K, H != W
    ("p16-kpadK+8-B1-T3", (1, 3, 3, 32, 32, 16, 776), {}),                  # im2col8_kernel, one zero chunk per row; B = 1, odd T
    ("p14-kpad592-T1", (2, 3, 1, 28, 42, 14, 592), {}),                     # element-wise (P % 8 != 0), four zero columns; T = 1
    ("p16-kpad772", (1, 3, 1, 32, 32, 16, 772), {}),                        # element-wise through kpad % 8 != 0
    ("p16-both-paths", (2, 3, 3, 32, 16, 16, 768), dict(misalign=True)),    # im2col8 | element-wise through a 2-byte aligned view
    ("p16-wrap-8wide", (1, 3, 223, 224, 224, 16, 768), dict(on_device=True)),      # 43708 x 96 chunks = 4196k > 16384 x 256 = 4194k: the stride loop runs again
    ("p14-wrap-elementwise", (4, 3, 7, 224, 224, 14, 592), dict(on_device=True)),  # 7168 x 592 = 4243k elements > 4194k
]


# ------------------------------------------------------------------------------------------------------------------ ViT token assembly
def run_assemble_fwd(ops, dev, B, T, N, D, *, on_device=False):
    """x against assemble_fwd_ref (cls row without the temporal term, bf16(pos + temporal) formed by the reference); the temporal
    table has a NaN row behind the T used ones."""
    tag = f"assemble_fwd B {B} T {T} N {N} D {D}"
    if on_device:
        patch = big_randn(dev, 11, B * T * N * D).view(B * T * N, D)
        cls, pos, tem = big_randn(dev, 12, D), big_randn(dev, 13, (N + 1) * D).view(N + 1, D), big_randn(dev, 14, (T + 1) * D).view(T + 1, D)
    else:
        gen = _gen(B, T, N, D)
        patch, cls, pos, tem = (t.to(dev) for t in (rnb(gen, B * T * N, D), rnb(gen, D), rnb(gen, N + 1, D), rnb(gen, T + 1, D)))
    tem[T] = NAN
    x = ops.vit_embed_assemble_fwd(patch, cls, pos, tem, B, T, N, D)
    assert tuple(x.shape) == (B * T * (N + 1), D)
    close_one(x, R.assemble_fwd_ref(patch, cls, pos, tem[:T], B, T, N, D), f"assemble_fwd.x | {tag}")


ASSEMBLE_FWD_RUNS = [
    ("D4", (2, 2, 3, 4), {}),               # one 4-wide load per row
    ("D72", (2, 3, 5, 72), {}),             # a multiple of 8 that is none of 64
    ("N1", (3, 2, 1, 8), {}),               # one token behind the cls row
    ("T1", (2, 1, 3, 8), {}),
    ("B1", (1, 3, 4, 64), {}),
    ("wrap", (8, 8, 256, 1024), dict(on_device=True)),      # 64 x 257 x 256 = 4211k items > 4194k: the stride loop runs again
]


def run_assemble_bwd(ops, dev, B, T, N, D):
    """dpatch raw bits; dpos and dtemporal through the sum gate; dcls == dpos[0] bit for bit; a sentinel row / tail behind every output."""
    tag = f"assemble_bwd B {B} T {T} N {N} D {D}"
    dx = rnb(_gen(B, T, N, D), B * T * (N + 1), D).to(dev)
    dpatch = torch.full((B * T * N + 1, D), SENT_BF, dtype=BF, device=dev)
    dcls = torch.full((D + 8,), SENT_BF, dtype=BF, device=dev)
    dpos = torch.full((N + 2, D), SENT_BF, dtype=BF, device=dev)
    dtem = torch.full((T + 1, D), SENT_BF, dtype=BF, device=dev)
    ops.vit_embed_assemble_bwd(dx, dpatch[:B * T * N], dcls[:D], dpos[:N + 1], dtem, B, T, N, D)
    want_patch, (rpos, apos, npos), (rtem, atem, ntem) = R.assemble_bwd_ref(dx, B, T, N, D)
    assert same_bits(dpatch[:B * T * N], want_patch), f"{tag}: dpatch is not the token rows of dx"
    close_sum(dpos[:N + 1], rpos, apos, npos, f"assemble_bwd.dpos | {tag}")
    close_sum(dtem[:T], rtem, atem, ntem, f"assemble_bwd.dtemporal | {tag}")
    assert same_bits(dcls[:D], dpos[0]), f"{tag}: dcls is not dpos[0]"
    for buf, n, name in ((dpatch, B * T * N * D, "dpatch"), (dcls, D, "dcls"), (dpos, (N + 1) * D, "dpos"), (dtem, T * D, "dtemporal")):
        sentinel_tail(buf, n, f"{tag} {name}")


# B*T against the 16 row lanes of embed_bwd_pos_kernel, B*N against the 128 of embed_bwd_temporal_kernel, D against its 64-column stripes
ASSEMBLE_BWD_RUNS = [
    ("BT1-BN1-D8", (1, 1, 1, 8), {}),            # one row for one lane of each kernel; 2 column groups of 64: (N+1) D / 8 = 2
    ("BT15-BN127-D8", (1, 15, 127, 8), {}),      # one lane short of both; a stripe with one live 8-column group
    ("BT16-BN128-D72", (1, 16, 128, 72), {}),    # exactly the lanes; stripe 2 cut by c < D after one group; 1161 column groups (18 x 64 + 9)
    ("BT17-BN129-D64", (1, 17, 129, 64), {}),    # one lane takes a second row; one full stripe
    ("BT33-BN129-D136", (3, 11, 43, 136), {}),   # three trips of lane 0; stripe 3 holds one group; b = r / N crosses batches; 748 column groups
    ("BT15-BN3-D72", (3, 5, 1, 72), {}),         # N = 1 with three batches
]


# ------------------------------------------------------------------------------------------------------------------ cls merge
def run_cls_merge(ops, dev, B, T, N1, D):
    """mpv_vit_cls_merge_fwd / _bwd against the references (token rows of the forward: one_op; cls slots: xt + bf16(mean), either
    rounding of a mean at a tie; backward: token rows raw bits, cls slots the sum gate and the same bits for every t).  D % 8 == 0:
    mpv_vit_cls_fix_fwd on (y = xt + a, tap = the cls rows of a) and mpv_vit_cls_merge_bwd_inplace give the full-tensor kernels' bits,
    `saved` holds the cls rows of dy and restores it exactly."""
    tag = f"cls_merge B {B} T {T} N1 {N1} D {D}"
    gen = _gen(B, T, N1, D)
    xt, a, dy = (rnb(gen, B * T * N1, D).to(dev) for _ in range(3))
    y = ops.vit_cls_merge_fwd(xt, a, B, T, N1, D)
    ry, ry_alt = R.cls_merge_fwd_ref(xt, a, B, T, N1, D)
    yf = y.to(F64)
    close_one(y, torch.where((yf - ry).abs() <= (yf - ry_alt).abs(), ry, ry_alt), f"cls_merge_fwd.y | {tag}")
    da = ops.vit_cls_merge_bwd(dy, B, T, N1, D)
    dav, dyv = da.view(B, T, N1, D), dy.view(B, T, N1, D)
    assert same_bits(dav[:, :, 1:], dyv[:, :, 1:]), f"{tag}: token rows of da are not dy's"
    mean, amean, n = R.cls_merge_bwd_ref(dy, B, T, N1, D)
    close_sum(dav[:, 0, 0], mean, amean, n, f"cls_merge_bwd.da_cls | {tag}")
    assert same_bits(dav[:, :, 0], dav[:, :1, 0].expand(B, T, D)), f"{tag}: the cls slots of da differ over t"
    if D % 8:
        return
    y2 = ops.add(xt, a)
    ops.vit_cls_fix_fwd(xt, a.view(B * T, N1, D)[:, 0].contiguous(), y2, B, T, N1, D)
    assert same_bits(y2, y), f"{tag}: the cls fix-up differs from the full-tensor forward"
    dy2 = dy.clone()
    saved = ops.vit_cls_merge_bwd_inplace(dy2, B, T, N1, D)
    assert same_bits(dy2, da), f"{tag}: the in-place backward differs from the full-tensor one"
    assert same_bits(saved, dyv[:, :, 0].reshape(B * T, D)), f"{tag}: saved is not the cls rows of dy"
    ops.copy_rows(saved, dy2, B * T, D, dmap=(1, N1, 0))
    assert same_bits(dy2, dy), f"{tag}: saved does not restore dy"


CLS_MERGE_RUNS = [
    ("D4-T3", (2, 3, 2, 4), {}),          # the 4-wide pair only; N1 = 2
    ("D4-T16", (1, 16, 3, 4), {}),
    ("D8-T1", (2, 1, 2, 8), {}),          # a mean of one term: the cls slot is xt + a
    ("D72-T3", (3, 3, 2, 72), {}),        # 1 / 3 is no fp32 number
    ("D8-T16", (2, 16, 2, 8), {}),
    ("threads255", (255, 3, 2, 8), {}),   # B D / 8 threads of the 8-wide pair: one idle lane in the only workgroup
    ("threads256", (256, 1, 2, 8), {}),   # exactly one workgroup
    ("threads257", (257, 3, 2, 8), {}),   # a second workgroup with one live lane
    ("D72-N4", (2, 3, 4, 72), {}),
]


# ------------------------------------------------------------------------------------------------------------------ copy_rows / add
def run_copy_rows(ops, dev, rows, cols, *, smap=IDENT, dmap=IDENT, lds=None, ldd=None):
    """the mapped rows' first cols columns arrive bit for bit; NaN fills the source outside them, a sentinel the destination"""
    tag = f"copy_rows {rows}x{cols} lds {lds} ldd {ldd} smap {smap} dmap {dmap}"
    if rows == 0:
        src = torch.full((2, lds or cols), NAN, dtype=BF, device=dev)
        dst = torch.full((2, ldd or cols), SENT_BF, dtype=BF, device=dev)
        ops.copy_rows(src, dst, 0, cols, smap=smap, dmap=dmap, lds=lds, ldd=ldd)
        sentinel_tail(dst, 0, tag)
        return
    t = rnb(_gen(rows, cols, lds or 0, ldd or 0), rows, cols)
    src = place(t, smap, lds or cols, NAN).to(dev)
    dst = place(torch.full((rows, cols), SENT_BF, dtype=BF), dmap, ldd or cols, SENT_BF).to(dev)
    ops.copy_rows(src, dst, rows, cols, smap=smap, dmap=dmap, lds=lds, ldd=ldd)
    assert same_bits(take(dst, dmap, rows, cols), t.to(dev)), f"{tag}: rows differ"
    assert_untouched(dst, dmap, rows, cols, SENT_BF, tag)


COPY_ROWS_RUNS = [
    ("maps-offset-ld", (11, 12), dict(smap=(3, 5, 2), dmap=(4, 6, 1), lds=16, ldd=20)),      # both maps with an offset, both pitches padded
    ("dmap-only", (6, 4), dict(dmap=(1, 3, 2))),                                             # one 8-byte piece per row, scattered
    ("rows0", (0, 8), dict(smap=(2, 3, 1), lds=12)),
    ("wrap", (16400, 1024), dict(ldd=1028)),                                                 # 16400 x 256 = 4198k pieces > 4194k
]


def run_add(ops, dev, n, *, on_device=False):
    tag = f"add n {n}"
    if on_device:
        a, b = big_randn(dev, 21, n), big_randn(dev, 22, n)
    else:
        gen = _gen(n, 3)
        a, b = rnb(gen, n).to(dev), rnb(gen, n).to(dev)
    buf = torch.full((n + 8,), SENT_BF, dtype=BF, device=dev)
    ops.add(a, b, out=buf[:n])
    close_one(buf[:n], R.add_ref(a, b), f"add.out | {tag}")
    sentinel_tail(buf, n, tag)


ADD_RUNS = [
    ("n0", (0,), {}),                                             # nothing to do (an empty tensor's address is null)
    ("n4", (4,), {}),                                             # one lane
    ("n2060", (2060,), {}),                                       # three workgroups, the last one holding three lanes
    ("wrap", (4 * (EW_CAP + 3),), dict(on_device=True)),          # three pieces past the capped grid's first sweep
]


# ------------------------------------------------------------------------------------------------------------------ colsum
def run_colsum(ops, dev, rows, cols, *, ld=None, rmap=IDENT, accumulate=False):
    """out against colsum_ref through the sum gate.  Column 1 holds +x, -x pairs (an odd last row keeps its value): its exact sum is 0
    (or that last value) and its whole allowance is the atol; NaN outside the mapped rows / columns; a sentinel behind out."""
    tag = f"colsum {rows}x{cols} ld {ld} rmap {rmap} accumulate {accumulate}"
    gen = _gen(rows, cols, ld or 0, int(accumulate))
    x = rnb(gen, rows, cols)
    half = rows // 2
    x[1:2 * half:2, 1] = -x[0:2 * half:2, 1]
    buf = place(x, rmap, ld or cols, NAN).to(dev)
    out0 = rnb(gen, cols)
    out = torch.full((cols + 8,), SENT_BF, dtype=BF, device=dev)
    if accumulate:
        out[:cols] = out0.to(dev)
    ops.colsum(buf, rows, cols, out=out[:cols], ld=ld, rmap=rmap, accumulate=accumulate)
    ref, absum, n = R.colsum_ref(x.to(dev), out0.to(dev) if accumulate else None)
    close_sum(out[:cols], ref, absum, n, f"colsum.out | {tag}")
    sentinel_tail(out, cols, tag)


# rows: nsplit = min(ceil(rows / 4), 128) workgroups along the rows, each lane 4 loads in flight and a tail loop
COLSUM_RUNS = [
    ("rows1-cols4", (1, 4), {}),                   # nsplit 1, three idle row lanes, one column quad
    ("rows3-cols252", (3, 252), {}),               # nsplit 1; one quad short of a workgroup's 256 columns
    ("rows4-cols256", (4, 256), {}),               # nsplit 1, every row lane one row
    ("rows5-cols260", (5, 260), {}),               # nsplit 2; a second column workgroup with one live quad
    ("rows511-cols4", (511, 4), {}),               # nsplit 128 with one row missing from the last workgroup (tail loop only)
    ("rows512-cols260", (512, 260), {}),           # nsplit 128, one row per lane
    ("rows513-cols252", (513, 252), {}),           # nsplit capped: lane 0 of workgroup 0 takes a second row in the tail loop
    ("rows2049-cols256", (2049, 256), {}),         # the 4-deep unrolled loop runs once for every lane, the tail loop for one
    ("skip-cls", (12, 8), dict(rmap=(3, 4, 1))),   # the token rows of three frames of N1 = 4: the cls rows hold NaN
    ("ld", (5, 252), dict(ld=260)),
    ("accumulate", (513, 260), dict(accumulate=True)),
    ("accumulate-map-ld", (9, 4), dict(accumulate=True, rmap=(2, 3, 1), ld=8)),
]


# ------------------------------------------------------------------------------------------------------------------ GPT embedding front
def _check_dropped(got, ref, keep, what):
    """the dropped elements are +0 and no kept one is -- but for a kept element whose exact value is 0 (two bf16 numbers that cancel:
    about one sum in a thousand), which is +0 as well"""
    assert torch.equal(bits(got) == 0, ~keep | (ref == 0)), f"{what}: the +0 elements are not keep_mask's dropped ones"


def run_gpt_embed(ops, dev, B, Q, L, H, p, V=50):
    """mpv_gpt_embed_fwd, _bwd_full and (Q > 0) _bwd on one case: values through the one_op gate (with dropout the reference rounds the
    sum to bf16 before it scales), the +0 positions == ~keep_mask(seed, offset, B (Q + L), H, p) exactly in all three, _bwd == the
    query rows of _bwd_full bit for bit, p = 0: both backwards are raw copies.  ids hold 0 and V - 1; wpe has NaN rows behind Q + L."""
    tag = f"gpt_embed B {B} Q {Q} L {L} H {H} p {p}"
    S = Q + L
    gen = _gen(B, Q, L, H)
    query = rnb(gen, B * Q, H).to(dev) if Q else None
    ids = torch.randint(0, V, (B, max(L, 1)), generator=gen)
    ids[0, 0], ids[-1, -1] = 0, V - 1
    wte = rnb(gen, V, H).to(dev)
    wpe = torch.cat([rnb(gen, S, H), torch.full((2, H), NAN, dtype=BF)]).to(dev)
    dh = rnb(gen, B * S, H).to(dev)
    ids = ids.to(dev)
    kw = dict(dropout_p=p, seed=DROP_SEED, offset=DROP_OFFSET) if p > 0 else {}
    keep = R.keep_mask(DROP_SEED, DROP_OFFSET, B * S, H, p, device=dev) if p > 0 else None
    scale = R.drop_scale(p)
    h = ops.gpt_embed_fwd(query, ids, wte, wpe, B, Q, L, H, **kw)
    rh = R.gpt_embed_fwd_ref(query, ids, wte, wpe, B, Q, L, H, keep, scale)
    close_one(h, rh, f"gpt_embed_fwd.h | {tag}")
    df = ops.gpt_embed_bwd_full(dh, B * S, H, **kw)
    rdf = R.gpt_embed_bwd_full_ref(dh, keep, scale)
    close_one(df, rdf, f"gpt_embed_bwd_full.d | {tag}")
    if p > 0:
        _check_dropped(h, rh, keep, f"{tag} fwd")
        _check_dropped(df, rdf, keep, f"{tag} bwd_full")
    else:
        assert same_bits(df, dh), f"{tag}: bwd_full at p = 0 is not a copy"
    if Q:
        dq = ops.gpt_embed_bwd(dh, B, Q, L, H, **kw)
        assert same_bits(dq, df.view(B, S, H)[:, :Q].reshape(B * Q, H)), f"{tag}: bwd is not the query rows of bwd_full"


GPT_EMBED_RUNS = [
    ("Q0-H8", (2, 0, 5, 8, 0.0), {}),            # no query rows (a null query), one 16-byte piece per row
    ("Q0-p0.1", (2, 0, 5, 8, 0.1), {}),
    ("L0-p0.1", (2, 3, 0, 16, 0.1), {}),         # no token rows: ids is never read
    ("H72-p0.5", (2, 3, 4, 72, 0.5), {}),
    ("B1-p0.1", (1, 2, 3, 8, 0.1), {}),
    ("H264-p0", (3, 2, 5, 264, 0.0), {}),        # rows of 33 pieces: a workgroup's lanes straddle rows
    ("H64-p0.1", (2, 4, 3, 64, 0.1), {}),
    ("H64-p0.5", (2, 4, 3, 64, 0.5), {}),
]


def run_gpt_embed_bwd_full_wrap(ops, dev, rows=16400, H=2048, p=0.1):
    """16400 x 256 = 4198k pieces > 4194k: the stride loop runs again.  Compared in blocks of 1024 rows (the mask of a block is
    keep_mask with the offset moved to the block's first element)."""
    dh = big_randn(dev, 31, rows * H).view(rows, H)
    dh = torch.where(dh == 0, torch.ones_like(dh), dh)
    df = ops.gpt_embed_bwd_full(dh, rows, H, dropout_p=p, seed=DROP_SEED, offset=DROP_OFFSET)
    for lo in range(0, rows, 1024):
        n = min(1024, rows - lo)
        keep = R.keep_mask(DROP_SEED, DROP_OFFSET + lo * H, n, H, p, device=dev)
        ref = R.gpt_embed_bwd_full_ref(dh[lo:lo + n], keep, R.drop_scale(p))
        tag = f"gpt_embed_bwd_full {rows}x{H} p {p} (grid wraps) rows {lo}+"
        R.close_elementwise(df[lo:lo + n], ref, *GATES["one_op"], f"gpt_embed_bwd_full.d | {tag}")
        _check_dropped(df[lo:lo + n], ref, keep, tag)


def run_gpt_embed_rows(ops, dev, H, pos, MP=7, V=50):
    """mpv_gpt_embed_rows_fwd: the DEVICE positions `pos` (some below 0, some at or above max_positions = MP) clamp to wpe's ends -- the
    host list the wrapper checks holds the clamped ones; every row bit-identical to mpv_gpt_embed_fwd with Q = 0, L = 1 on the same
    token at the same (clamped) position."""
    rows = len(pos)
    tag = f"gpt_embed_rows rows {rows} H {H} pos {pos}"
    gen = _gen(rows, H, MP)
    ids = torch.randint(0, V, (rows,), generator=gen)
    ids[0], ids[-1] = V - 1, 0
    wte, wpe = rnb(gen, V, H).to(dev), rnb(gen, MP, H).to(dev)
    ids = ids.to(dev)
    clamped = [min(max(q, 0), MP - 1) for q in pos]
    out = ops.gpt_embed_rows_fwd(ids, torch.tensor(pos, dtype=torch.int32, device=dev), clamped, wte, wpe, rows, H)
    close_one(out, R.gpt_embed_rows_ref(ids, pos, wte, wpe), f"gpt_embed_rows_fwd.out | {tag}")
    for r in range(rows):
        one = ops.gpt_embed_fwd(None, ids[r:r + 1].view(1, 1), wte, wpe[clamped[r]:], 1, 0, 1, H)
        assert same_bits(out[r:r + 1], one), f"{tag}: row {r} differs from gpt_embed_fwd at position {clamped[r]}"


GPT_EMBED_ROWS_RUNS = [
    ("rows1", (8, [3]), {}),
    ("clamp-both-ends", (72, [-1, 0, 6, 7, -2 ** 31, 2 ** 31 - 1, 2]), {}),      # below 0 -> row 0; at / above max_positions = 7 -> row 6
]


# ------------------------------------------------------------------------------------------------------------------ log-prob top-k
TOPK_KINDS = ("equal", "tie-adjacent-slices", "tie-ends", "ban-slice", "ban-all-but", "range80", "randn3")
TOPK_ADDS = (0.0, -2.5, float("-inf"))      # per kind one row each: nothing | a live beam's score | a dead beam


def topk_rows(V, k, gen):
    """[len(TOPK_KINDS) * 3, V] bf16: every kind three times (the rows differ where the kind draws numbers).  per = ceil(V / 32) is the
    kernel's slice length: slice s covers columns [s per, (s + 1) per)."""
    per = -(-V // 32)
    out = []
    for kind in TOPK_KINDS:
        for _ in TOPK_ADDS:
            x = torch.randn(V, generator=gen).clamp(-6.0, 6.0)
            if kind == "equal":                    # (a) every index decided by the tie rule
                x = torch.full((V,), 1.5)
            elif kind == "tie-adjacent-slices":    # (b) the maximum twice: last column of slice s, first of slice s + 1
                s = 1 if 3 * per <= V else 0
                x[(s + 1) * per - 1] = x[(s + 1) * per] = 8.0
            elif kind == "tie-ends":               # (b) ... and at columns 0 and V - 1: the first and the last non-empty slice
                x[0] = x[V - 1] = 8.0
            elif kind == "ban-slice":              # (c) one whole slice banned
                lo = 2 * per if 2 * per < V else 0
                x[lo:min(V, lo + per)] = BAN
            elif kind == "ban-all-but":            # (c) everything banned but k - 1 entries (one entry for k = 1, see TOPK_RUNS)
                live = torch.randperm(V, generator=gen)[:max(k - 1, 1)]
                y = torch.full((V,), BAN)
                y[live] = x[live]
                x = y
            elif kind == "range80":                # (d)
                x = torch.rand(V, generator=gen) * 160.0 - 80.0
            else:
                x = x * 3.0
            out.append(x)
    return torch.stack(out).to(BF)


TOPK_ATOL_CAP = 1.4e-5      # ten times the CE gate's atol: the most the widening may reach


def topk_atol(lse, add):
    """per row: the CE gate's atol + half an fp32 ulp of lse (gmax + log(se)) + half an fp32 ulp of lse - add (a dead beam's -inf: 0)"""
    a = torch.zeros_like(lse) if add is None else add.to(F64)
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    atol = GATES["topk.values"][1] + 2.0 ** -24 * (lse.abs() + (lse - a).abs())
    assert float(atol.max()) <= TOPK_ATOL_CAP
    return atol


def run_logprob_topk(ops, dev, V, k, *, ld=None, with_add=True):
    """idx == the first k of the stable descending order of the bf16 logits, exactly, in every row (so no index repeats); values through
    the topk gate, -inf where add is -inf; NaN in the padding columns of ld > V."""
    tag = f"logprob_topk V {V} k {k} ld {ld} add {with_add}"
    x = topk_rows(V, k, _gen(V, k, ld or 0))
    rows = x.shape[0]
    buf = torch.full((rows, ld or V), NAN, dtype=BF)
    buf[:, :V] = x
    add = torch.tensor(TOPK_ADDS * len(TOPK_KINDS), dtype=torch.float32) if with_add else None
    val, idx = ops.logprob_topk(buf.to(dev), k, add=add.to(dev) if with_add else None, rows=rows, vocab=V, ld=ld)
    rval, ridx, lse = R.logprob_topk_ref(x, k, add)
    assert tuple(idx.shape) == (rows, k) and idx.dtype == torch.int64
    bad = (idx.cpu() != ridx).any(dim=1).nonzero().flatten().tolist()
    assert not bad, (f"{tag}: indices differ from the stable order of the logits in rows "
                     f"{[(r, TOPK_KINDS[r // 3], TOPK_ADDS[r % 3]) for r in bad]}; first: got {idx[bad[0]].tolist()} want {ridx[bad[0]].tolist()}")
    assert all(len(set(r)) == k for r in idx.cpu().tolist()), f"{tag}: an index repeats"
    # (divided by the row's atol: the printed residual is the fraction of it the worst element used)
    R.close_scaled(val.cpu(), rval, topk_atol(lse, add), (GATES["topk.values"][0], 1.0), f"logprob_topk.values | {tag}")


# V against the 32 slices: 8, 31: one column per slice and 24 / 1 empty slices; 32: every slice one column; 33: 17 slices of two
# (the last of one) and 15 empty ones; 1000: slices of 32, the last of 8 (shorter than k = 64, as every slice is); 51200: slices of 1600.
# k = V for V <= 64: every column is an answer, the last ones out of banned / tied entries.  ABSENT: a row whose EVERY entry is banned
# ("all but k - 1" for k = 1): its log-sum-exp BAN + log V is no fp32 number (BAN's ulp is 2e31), which the kernel's lse = gmax +
# log(sum) cannot hold -- generation never bans the stop token, so such a row does not reach the kernel; k = 1 keeps one entry
TOPK_RUNS = [(f"V{V}-k{k}" + ("-ld" if ld else "") + ("" if wa else "-noadd"), (V, k), dict(ld=ld, with_add=wa)) for V, k, ld, wa in [
    (8, 1, None, True), (8, 8, 11, True), (31, 1, 32, True), (31, 31, None, True), (32, 1, None, False), (32, 32, 35, True),
    (33, 1, None, True), (33, 33, 40, True), (33, 33, None, False), (1000, 1, 1003, True), (1000, 64, None, True), (1000, 64, 1008, False),
    (51200, 1, None, True), (51200, 64, 51203, True)]]


# ------------------------------------------------------------------------------------------------------------------ copy_segments
SEG_COUNTS = (1, 0, 7, 8, 9, 2049)      # one element | nothing | the tail loop only | one 16-byte piece | piece + tail | 256 pieces + tail


def run_copy_segments(ops, dev, nseg):
    """nseg segments, counts cycling SEG_COUNTS; every six segments the next of the four combinations of 16-byte / 2-byte aligned source
    and destination (24 segments: every count with every combination).  The whole destination buffer -- segments and the sentinel
    around every one -- bit for bit; NaN around every source."""
    tag = f"copy_segments n {nseg}"
    counts = [SEG_COUNTS[i % len(SEG_COUNTS)] for i in range(nseg)]
    start, pos = [], 8
    for c in counts:
        start.append(pos)
        pos += (c + 7) // 8 * 8 + 16
    gen = _gen(nseg, 9)
    src = torch.full((pos + 8,), NAN, dtype=BF)
    want = torch.full((pos + 8,), SENT_BF, dtype=BF)
    spans = []
    for i, (c, s0) in enumerate(zip(counts, start)):
        combo = (i // len(SEG_COUNTS)) % 4
        so, do = s0 + (combo & 1), s0 + (combo >> 1)
        v = rnb(gen, c)
        src[so:so + c] = v
        want[do:do + c] = v
        spans.append((so, do, c))
    src, dst = src.to(dev), torch.full((pos + 8,), SENT_BF, dtype=BF, device=dev)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    ops.copy_segments([(src[so:so + c], dst[do:do + c]) for so, do, c in spans])
    assert same_bits(dst, want.to(dev)), f"{tag}: a segment differs or its surroundings were written"


SEGMENT_RUNS = [
    ("n0", (0,), {}),        # no launch
    ("n1", (1,), {}),        # a single element
    ("n64", (64,), {}),      # one full pointer table; every count with every alignment pair; the empty segments' addresses are null
    ("n65", (65,), {}),      # a second launch of one segment
    ("n129", (129,), {}),    # three launches
]


# ------------------------------------------------------------------------------------------------------------------ fp32 window
def run_accum_f32(ops, dev, n, *, on_device=False):
    """first overwrites a NaN-filled accumulator; two more calls add: the bits of the same fp32 additions in the same order; sentinel behind"""
    tag = f"accum_f32 n {n}"
    if on_device:
        gs = [big_randn(dev, 41 + i, n) for i in range(3)]
    else:
        gen = _gen(n, 5)
        gs = [rnb(gen, n, scale=s).to(dev) for s in (1.0, 1e-2, 3.0)]
    buf = torch.full((n + 8,), 1234.5, dtype=torch.float32, device=dev)
    buf[:n] = NAN
    for i, g in enumerate(gs):
        ops.accum_f32(buf[:n], g, first=i == 0)
    assert same_bits(buf[:n], R.accum_f32_ref(gs)), f"{tag}: not the fp32 sum in call order"
    sentinel_tail(buf, n, tag, 1234.5)


F32_SPECIALS = [
    1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,              # ties: to the even 1.0 | to the even 1 + 2^-6
    -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -23,  # the negative tie | just above a tie: up
    float.fromhex("0x1.fffffep0"), float.fromhex("0x1.ffp0"),      # round up into the next binade (2.0) | the tie below 2.0 -> 2.0
    float.fromhex("0x1.fffffep127"),                   # the largest fp32: rounds to inf
    float("inf"), float("-inf"), 0.0, -0.0,
    1e-40, -1e-40, float.fromhex("0x1p-149"),          # fp32 subnormals (bf16 subnormals / zero)
    float.fromhex("0x1p-134"), float.fromhex("0x1.8p-133"),      # ties among bf16 subnormals (spacing 2^-133): to 0 | to 2 x 2^-133
    float.fromhex("0x1.fffffcp-127"),                  # the largest fp32 subnormal -> 2^-126, the smallest normal
]


def run_f32_to_bf16(ops, dev, n, *, on_device=False):
    tag = f"f32_to_bf16 n {n}"
    if on_device:
        g = torch.Generator(device=dev).manual_seed(51)
        src = torch.randn(n, device=dev, generator=g)
    else:
        src = torch.randn(n, generator=_gen(n, 6))
        if n:
            sp = torch.tensor(F32_SPECIALS, dtype=torch.float32)[:n]
            src[:len(sp)] = sp
        src = src.to(dev)
    buf = torch.full((n + 8,), SENT_BF, dtype=BF, device=dev)
    ops.f32_to_bf16(src, buf[:n])
    assert same_bits(buf[:n], R.f32_to_bf16_ref(src)), f"{tag}: not round-to-nearest-even"
    sentinel_tail(buf, n, tag)


WINDOW_RUNS = [
    ("n0", (0,), {}),                                              # nothing to do (null addresses)
    ("n8", (8,), {}),                                              # one lane
    ("n2056", (2056,), {}),                                        # two workgroups, the second with one lane
    ("wrap", (8 * (STREAM_CAP + 3),), dict(on_device=True)),       # three pieces past stream_grid's capped first sweep
]


def run_store_words(ops, dev, n):
    """n words arrive bit for bit (all-ones and NaN patterns among them); the word behind the last one keeps its sentinel"""
    gen = _gen(n, 7)
    words = ([0xFFFFFFFF, 0x7FC00000, 0xFFC00001, 0x7F800001, 0, 0x80000000] + torch.randint(0, 2 ** 32, (32,), generator=gen).tolist())[:n]
    if n == 1:
        words = [0xFFFFFFFF]
    dst = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ops.store_words(dst, words)
    want = words + [0x5A5A5A5A] * 2
    assert [v & 0xFFFFFFFF for v in dst.cpu().tolist()] == want, f"store_words n {n}"


STORE_WORDS_RUNS = [("n1", (1,), {}), ("n31", (31,), {}), ("n32", (32,), {})]      # one lane | one short of | the most words of a launch


# ------------------------------------------------------------------------------------------------------------------ composed projection
def run_compose(ops, dev, D, nb):
    """mpv_vit_compose_bwd_finish per block: dwf one_op, dbp the sum gate; the batched launch bit-identical to the per-block ones;
    mpv_vit_compose_bias_batched: bc the sum gate.  A sentinel behind every vector output."""
    tag = f"compose D {D} batch {nb}"
    gen = _gen(D, nb, 8)
    mk = lambda *s: [rnb(gen, *s).to(dev) for _ in range(nb)]
    P, wf, dbc, bp, bfv = mk(D, D), mk(D, D), mk(D), mk(D), mk(D)
    new_vec = lambda: torch.full((nb, D + 8), SENT_BF, dtype=BF, device=dev)
    dwf1, dbp1 = torch.full((nb, D, D), SENT_BF, dtype=BF, device=dev), new_vec()
    for i in range(nb):
        ops.vit_compose_bwd_finish(P[i], dbc[i], bp[i], wf[i], dwf1[i], dbp1[i, :D], D)
    for i in sorted({0, nb - 1}):
        rdwf, (rdbp, adbp, n) = R.compose_finish_ref(P[i], dbc[i], bp[i], wf[i], D)
        close_one(dwf1[i], rdwf, f"compose_finish.dwf | {tag} block {i}")
        close_sum(dbp1[i, :D], rdbp, adbp, n, f"compose_finish.dbp | {tag} block {i}")
    dwf2, dbp2, bc = torch.full((nb, D, D), SENT_BF, dtype=BF, device=dev), new_vec(), new_vec()
    ops.vit_compose_bwd_finish_batched(P, dbc, bp, wf, list(dwf2.unbind(0)), [dbp2[i, :D] for i in range(nb)], D)
    assert same_bits(dwf2, dwf1) and same_bits(dbp2, dbp1), f"{tag}: the batched finish differs from the per-block launches"
    ops.vit_compose_bias_batched(wf, bp, bfv, [bc[i, :D] for i in range(nb)], D)
    for i in range(nb):
        rbc, abc, n = R.compose_bias_ref(wf[i], bp[i], bfv[i], D)
        close_sum(bc[i, :D], rbc, abc, n, f"compose_bias.bc | {tag} block {i}")
    for buf, name in ((dbp1, "dbp"), (dbp2, "dbp batched"), (bc, "bc")):
        assert same_bits(buf[:, D:], torch.full_like(buf[:, D:], SENT_BF)), f"{tag}: written behind {name}"


# D: D D / 8 rank-1 threads against one 1024-thread workgroup; the column workgroup of 64 cut by j < D; 16 row lanes x 8 unrolled rows
COMPOSE_RUNS = [
    ("D8", (8, 1), {}),            # 8 rank-1 threads; 8 of 64 columns; tail loop only (rows 0..7 on lanes 0..7)
    ("D64-b16", (64, 16), {}),     # 512 threads; one full column workgroup; a full pointer table
    ("D72-b17", (72, 17), {}),     # a second column workgroup of 8; a second launch of one block
    ("D120", (120, 1), {}),        # 1800 threads: two rank-1 workgroups; tail loop only (120 < 128 rows)
    ("D128", (128, 1), {}),        # the unrolled loop once, no tail
    ("D136", (136, 1), {}),        # the unrolled loop once, a tail of 8 rows
    ("D520", (520, 1), {}),        # bias: lane 0 takes a second 512-column sweep; finish: four unrolled trips and a tail
]


# ------------------------------------------------------------------------------------------------------------------ caption targets
def run_caption_targets(ops, dev, B, L, plen):
    """labels exact, weights at rtol 2^-23 of caption_targets_ref, summing to 1.  Row b keeps its first 1 + (7 b + 3) % L mask entries;
    the LAST row's mask is all zero (B > 1).  plen: None | "zero" | "mixed": 0, L - 1, L, L + 5, 1, 0 ... down the rows."""
    tag = f"caption_targets B {B} L {L} plen {plen}"
    gen = _gen(B, L, 9)
    ids = torch.randint(0, 50000, (B, L), generator=gen)
    mask = torch.zeros((B, L), dtype=torch.int64)
    for b in range(B):
        mask[b, :L if b == 0 else 1 + (7 * b + 3) % L] = 1
    if B > 1:
        mask[B - 1] = 0
    pl = None
    if plen == "zero":
        pl = torch.zeros(B, dtype=torch.int64)
    elif plen == "mixed":
        pl = torch.tensor([(0, L - 1, L, L + 5, 1)[b % 5] for b in range(B)], dtype=torch.int64)
    labels, w = ops.caption_targets(ids.to(dev), mask.to(dev), None if pl is None else pl.to(dev))
    rl, rw = R.caption_targets_ref(ids, mask, pl)
    assert torch.equal(labels.cpu().view(-1), rl), f"{tag}: labels differ"
    R.close_elementwise(w.cpu().view(-1), rw, *GATES["caption.weights"], f"caption_targets.weights | {tag}")
    if L > 1:
        assert abs(w.cpu().double().sum().item() - 1.0) <= B * L * 2.0 ** -24, f"{tag}: the weights do not sum to 1"
    else:
        assert not w.cpu().any() and not labels.cpu().any()


# B x L against the single 256-thread workgroup's loop.  ABSENT: a batch whose every weight is excluded (0 / 0: outside the contract)
CAPTION_RUNS = [
    ("1x2", (1, 2, None), {}),              # one counted entry: weights (1, 0)
    ("3x85-mixed", (3, 85, "mixed"), {}),   # 255 entries: one idle lane
    ("1x256-zero", (1, 256, "zero"), {}),   # exactly one trip
    ("1x257", (1, 257, None), {}),          # lane 0 takes a second entry
    ("5x300-mixed", (5, 300, "mixed"), {}), # six trips; prompt lengths 0, L - 1, L, L + 5; the last row's mask all zero
    ("5x300-none", (5, 300, None), {}),
    ("4x1", (4, 1, None), {}),              # L = 1: labels 0, weights 0, nothing divided
    ("2x12-mixed", (2, 12, "mixed"), {}),
]


# ------------------------------------------------------------------------------------------------------------------ gather_rows_ld
def run_gather_rows_ld(ops, dev, rows, cols, lds, ldd, nsrc):
    """dst[r][:cols] = src[idx[r]][:cols] bit for bit (idx repeats rows and skips some); NaN in the source padding, sentinel elsewhere"""
    tag = f"gather_rows_ld {rows}x{cols} lds {lds} ldd {ldd}"
    gen = _gen(rows % 1000, cols, lds, ldd)
    t = rnb(gen, nsrc, cols)
    src = place(t, IDENT, lds, NAN).to(dev)
    idx = torch.randint(0, nsrc, (rows,), generator=gen)
    idx[0], idx[-1] = nsrc - 1, 0
    dst = torch.full((rows + 1, ldd), SENT_BF, dtype=BF, device=dev)
    ops.gather_rows_ld(src, idx.to(dev), dst, rows, cols, lds, ldd)
    assert same_bits(dst[:rows, :cols], t.to(dev)[idx.to(dev)]), f"{tag}: rows differ"
    assert_untouched(dst, IDENT, rows, cols, SENT_BF, tag)


GATHER_LD_RUNS = [
    ("pitches", (5, 8, 16, 24, 3), {}),              # one piece per row, both pitches padded
    ("cols264", (9, 264, 264, 272, 4), {}),          # 33 pieces per row
    ("wrap", (16400, 2048, 2048, 2048, 6), {}),      # 16400 x 256 = 4198k pieces > 4194k
]


# ------------------------------------------------------------------------------------------------------------------ all tables
# entry -> (runner, runs); both test files parametrise over every one
TABLES = {
    "im2col_patches": (run_im2col, IM2COL_RUNS),
    "vit_embed_assemble_fwd": (run_assemble_fwd, ASSEMBLE_FWD_RUNS),
    "vit_embed_assemble_bwd": (run_assemble_bwd, ASSEMBLE_BWD_RUNS),
    "vit_cls_merge": (run_cls_merge, CLS_MERGE_RUNS),
    "copy_rows": (run_copy_rows, COPY_ROWS_RUNS),
    "add": (run_add, ADD_RUNS),
    "colsum": (run_colsum, COLSUM_RUNS),
    "gpt_embed": (run_gpt_embed, GPT_EMBED_RUNS),
    "gpt_embed_bwd_full_wrap": (run_gpt_embed_bwd_full_wrap, [("wrap", (), {})]),
    "gpt_embed_rows_fwd": (run_gpt_embed_rows, GPT_EMBED_ROWS_RUNS),
    "logprob_topk": (run_logprob_topk, TOPK_RUNS),
    "copy_segments": (run_copy_segments, SEGMENT_RUNS),
    "accum_f32": (run_accum_f32, WINDOW_RUNS),
    "f32_to_bf16": (run_f32_to_bf16, WINDOW_RUNS),
    "store_words": (run_store_words, STORE_WORDS_RUNS),
    "vit_compose": (run_compose, COMPOSE_RUNS),
    "caption_targets": (run_caption_targets, CAPTION_RUNS),
    "gather_rows_ld": (run_gather_rows_ld, GATHER_LD_RUNS),
}
ALL_RUNS = [(f"{entry}-{rid}", entry, args, kw) for entry, (_, runs) in TABLES.items() for rid, args, kw in runs]
# the cases past a grid cap (every id holding "wrap"): 16 .. 34 M elements each, for the kernels' stride loops; the CPU file leaves them
# to the device file
WRAP_RUNS = [r for r in ALL_RUNS if "wrap" in r[0]]
HOST_RUNS = [r for r in ALL_RUNS if "wrap" not in r[0]]
