"""Case tables, inputs, gates and the case runners shared by tests/test_gemm_kernels_gpu.py (the HIP kernels of csrc/gemm.hip and
csrc/gemm256.hip) and tests/test_gemm_refs_cpu.py (the torch stand-in over the same cases), TEST INFRASTRUCTURE ONLY.  A runner takes the
module that provides gemm / gemm_batched (youku_mplug_amd.ops or tests/standin_ops.py) and a device, builds the case on the host from a
fixed seed, calls the entry point and compares EVERY element of every output with the fp64 reference of tests/ref_gemm.py through GATES
-- one code path, so the CPU stand-in check and the GPU kernel check cannot drift apart.

GATES[path.output] = (rtol, coef): |got - ref| <= rtol |ref| + coef x scale for every element.  rtol is the number format's (2^-8: one
round-to-nearest to bf16; 2^-22 for fp32 outputs); scale is the element's sum of absolute terms (ref_gemm); coef = 2 x the largest
residual (|got - ref| - rtol |ref|) / scale measured against the fp64 reference on an MI355X (profiles/gemm_kernel_errors.md), never above
COEF_CAP = 2^-12: a sixteenth of a bf16 ulp of the element's scale.  Outputs: z = the single rounding of acc * alpha + bias (a plain C,
row_tap_out, a pre-activation preact_out); c = a C behind an intermediate rounding (ref_gemm: rules 1 and 2); c32 = an fp32 C; deriv =
preact_out with preact_deriv; colsum.
ZDELTA (rule 2's bound on |fp32 z - fp64 z| / scale) = 2^-15: the matrix instructions add 16 or 32 products to the accumulator per step, a
step rounds once, by at most 2^-24 of the running sum (which never exceeds the scale), and the longest reduction of the tables has
8704 / 16 = 544 steps (the split paths add a handful more): 2^-15 in the worst case.  It is NOT the z gate's coefficient: one rounding
to bf16 uses half of rtol = 2^-8, so a z output can sit inside its gate with room to spare (coefficient 0) while z itself is off.

INPUTS.  A is unit Gaussian with rows 1, 8, 15, ... scaled by 2^-6 and rows 4, 11, 18, ... by 2^6 (small outputs beside large ones);
B is 0.5 x Gaussian + 0.1: the operands differ in spread and mean.  Every input buffer holds NaN in its padding columns, in the rows its
map skips and in one row behind the last; every output buffer holds a sentinel there, asserted untouched on the raw bits."""
import zlib

import torch

import ref_gemm as R
from loss_optim_cases import RTOL_BF16, RTOL_F32
from norm_cases import bits, same_bits

BF = torch.bfloat16
IDENT = (0, 0, 0)
COEF_CAP = 2.0 ** -12
ZDELTA = 2.0 ** -15
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_RELU, ACT_DERIV = 0, 1, 2, 3, 4
SENT_BF, SENT_F32 = -99.0, 1234.5
DROP_SEED = (0x1234 << 32) | 0x9abcdef1          # above 2^32: both halves of the seed reach the hash
DROP_OFFSET = 123456                               # non-zero, even
NAN = float("nan")

# kernel paths (the first word of a case's `path`): small_m = gemm_small_m_kernel; k128 = gemm_bf16_kernel, one part per tile; k128_tail =
# its tail split (fp32 partial tiles summed by the last arrival); k128_splitk = its weight-gradient split-K pass + splitk_reduce_kernel;
# k256 = gemm256_kernel unsplit; k256_splitk = its weight-gradient split + splitk_reduce_kernel; k256_fwdsplit = its forward split, bias
# and dropout in the reduce; batched = mpv_gemm_bf16_batched on gemm_bf16_kernel.
# (rtol, coef) per path and output; beside each the measured residual / scale and the case that gave it (0: no element ever left the
# rtol band).  A key that is absent was never measured: a case that needs it fails with a KeyError until it is
GATES = {
    "batched.z": (RTOL_BF16, 2.1e-08),      # measured 1.050e-08: batched tn x17 136x72x200 problem 5
    "k128.c": (RTOL_BF16, 2.9e-05),         # measured 1.440e-05: k128-nt-136x136x72-erf
    "k128.c32": (RTOL_F32, 1e-07),          # measured 4.818e-08: k128-tn-128x128x200-f32-accumulate
    "k128.colsum": (RTOL_BF16, 0),          # measured -3.757e-07: k128-tn-136x136x71-kmap-pads colsum_out
    "k128.deriv": (RTOL_BF16, 0),           # measured -5.399e-10: k128-nt-136x136x72-tanh-deriv preact_out
    "k128.z": (RTOL_BF16, 0),               # measured -1.132e-10: k128-nt-136x136x72-alpha-alpha_dev
    "k128_splitk.c": (RTOL_BF16, 0),        # measured 0.000e+00: k128-tn-128x128x3077-accumulate
    "k128_splitk.colsum": (RTOL_BF16, 0),   # measured -1.118e-07: k128-tn-136x136x3077-kmap-pads colsum_out
    "k128_splitk.z": (RTOL_BF16, 1.2e-09),  # measured 5.925e-10: k128-tn-128x128x3077-colsum
    "k128_tail.c": (RTOL_BF16, 4.3e-06),    # measured 2.142e-06: k128-tail-384x256x2048-erf-pre
    "k128_tail.z": (RTOL_BF16, 2.1e-08),    # measured 1.049e-08: k128-tail-384x256x2048-erf-pre preact_out
    "k256.c": (RTOL_BF16, 9.5e-06),         # measured 4.745e-06: k256-r160-nt-264x328x192-EP_ERF_PRE
    "k256.c32": (RTOL_F32, 6.3e-08),        # measured 3.139e-08: k256-r256-nt-264x328x192-f32
    "k256.colsum": (RTOL_BF16, 0),          # measured -3.339e-07: k256-tn-256x256x200 colsum_out
    "k256.deriv": (RTOL_BF16, 0),           # measured -3.355e-10: k256-r256-nt-264x328x192-EP_TANH_PRE-deriv preact_out
    "k256.z": (RTOL_BF16, 2.2e-08),         # measured 1.067e-08: k256-r160-nn-256x256x64
    "k256_fwdsplit.c": (RTOL_BF16, 0),      # measured 0.000e+00: k256-fwdsplit-nt-256x256x4096-bias-drop
    "k256_fwdsplit.z": (RTOL_BF16, 9.9e-09),# measured 4.717e-09: k256-fwdsplit-nt-256x256x4096-plain
    "k256_splitk.c": (RTOL_BF16, 0),        # measured 0.000e+00: k256-tn-264x328x340-split2-colsum-accumulate
    "k256_splitk.colsum": (RTOL_BF16, 0),   # measured -4.147e-08: k256-tn-264x328x340-split2-colsum-accumulate colsum_out
    "k256_splitk.z": (RTOL_BF16, 3.4e-09),  # measured 1.617e-09: k256-tn-264x328x340-split3
    "small_m.c": (RTOL_BF16, 3.1e-05),      # measured 1.466e-05: small_m-t4x16-5x6160x64-tanh
    "small_m.z": (RTOL_BF16, 7.8e-09),      # measured 3.899e-09: small_m-gen-5x6152x64
}
PATHS = ("small_m", "k128", "k128_tail", "k128_splitk", "k256", "k256_splitk", "k256_fwdsplit", "batched")


# ------------------------------------------------------------------------------------------------------------------ inputs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7fffffff)


def lay(t, m, ld, fill):
    """t [n, cols] laid out behind a row map with row pitch ld, one extra row behind the last: every element outside the mapped rows'
    first cols columns is `fill`"""
    n, cols = t.shape
    idx = R.map_rows(m, n)
    buf = torch.full((int(idx.max()) + 2, ld), fill, dtype=t.dtype)
    buf[idx, :cols] = t
    return buf


def untouched(buf, m, n, cols, sentinel, what):
    mask = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    mask[R.map_rows(m, n, buf.device), :cols] = True
    rest = buf[~mask]
    assert same_bits(rest, torch.full_like(rest, sentinel)), f"{what}: written outside the mapped rows / columns"


def operands(gen, M, N, K):
    """logical A [M, K] and B [K, N], bf16 (module text)"""
    A = torch.randn(M, K, generator=gen)
    r = torch.arange(M)
    A[r % 7 == 1] *= 2.0 ** -6
    A[r % 7 == 4] *= 2.0 ** 6
    return A.to(BF), (0.5 * torch.randn(K, N, generator=gen) + 0.1).to(BF)


def case(name, path, form, M, N, K, **kw):
    """one table entry.  form: "nt" forward (A [M][K], B [N][K]) | "nn" dgrad (B [K][N]) | "tn" weight gradient (A [K][M], B [K][N]).
    Options (all off by default): pad_a / pad_b / pad_c / pad_r / pad_z (extra columns of lda / ldb / ldc / ldr / ldz), amap / cmap / kmap,
    bias (True | "unaligned": 8 bytes past a 16-byte boundary), act, preact ("z" | "deriv"), residual, act_bwd, drop (p), alpha,
    alpha_dev, out_f32, accumulate, colscale (cols, s), tap (row_tap_group), colsum, keep_output, tile_hint, split_hint, repeat (extra launches that must
    give the same bits), ref_dev (fp64 reference on the device)."""
    return (name, dict(name=name, path=path, form=form, M=M, N=N, K=K, **kw))


def run_gemm(ops, dev, c, gates=None):
    """ops.gemm on one case of the tables: every output through its gate, sentinels untouched, dropped elements bit-exact, repeated
    launches identical.  -> the kernel's C (the mapped rows' first N columns)"""
    gates = gates or GATES
    g = lambda k, d=None: c.get(k, d)
    name, path, form, M, N, K = c["name"], c["path"], c["form"], c["M"], c["N"], c["K"]
    ta, tb = form == "tn", form != "nt"
    amap, cmap, kmap = g("amap", IDENT), g("cmap", IDENT), g("kmap", IDENT)
    gen = _gen(name)
    A, B = operands(gen, M, N, K)
    lda, ldb = (M if ta else K) + g("pad_a", 0), (N if tb else K) + g("pad_b", 0)
    ldc, ldr, ldz = N + g("pad_c", 0), N + g("pad_r", 0), N + g("pad_z", 0)
    abuf = lay(A.t().contiguous(), kmap, lda, NAN) if ta else lay(A, amap, lda, NAN)
    bbuf = lay(B, kmap, ldb, NAN) if tb else lay(B.t().contiguous(), IDENT, ldb, NAN)
    f32 = bool(g("out_f32"))
    cdt, sent = (torch.float32, SENT_F32) if f32 else (BF, SENT_BF)
    old = (torch.randn(M, N, generator=gen) * 4.0).to(cdt) if g("accumulate") else torch.full((M, N), sent, dtype=cdt)
    cbuf0 = lay(old, cmap, ldc, sent)
    kw, rkw = {}, {}
    if g("bias"):
        bb = torch.full((N + 16,), NAN, dtype=BF)
        o = 4 if g("bias") == "unaligned" else 0
        bb[o:o + N] = (torch.randn(N, generator=gen) * 0.5).to(BF)
        bb = bb.to(dev)
        assert bb.data_ptr() % 16 == 0
        kw["bias"] = bb[o:]
    if g("residual"):
        kw["residual"], kw["ldr"] = lay((torch.randn(M, N, generator=gen) * 2.0).to(BF), cmap, ldr, NAN).to(dev), ldr
    if g("act_bwd"):
        zz = torch.randn(M, N, generator=gen) * 2.0
        kw["act_bwd_z"], kw["ldz"], kw["act_bwd"] = lay(zz.to(BF), IDENT, ldz, NAN).to(dev), ldz, g("act_bwd")
    if g("alpha_dev") is not None:
        kw["alpha_dev"] = torch.tensor([g("alpha_dev")], dtype=torch.float32, device=dev)
    if g("drop"):
        kw.update(dropout_p=g("drop"), seed=DROP_SEED, offset=DROP_OFFSET)
        rkw["drop"] = (g("drop"), DROP_SEED, DROP_OFFSET)
    pre = lay(torch.full((M, N), SENT_BF, dtype=BF), cmap, ldc, SENT_BF).to(dev) if g("preact") else None
    ntap = (M + g("tap", 1) - 1) // g("tap", 1)
    tap = torch.full((ntap + 1, N), SENT_BF, dtype=BF, device=dev) if g("tap") else None
    csum = torch.full((M + 8,), SENT_BF, dtype=BF, device=dev) if g("colsum") else None
    if g("preact"):
        kw.update(preact_out=pre, preact_deriv=g("preact") == "deriv")
    if g("tap"):
        kw.update(row_tap_out=tap, row_tap_group=g("tap"))
    if g("colsum"):
        kw["colsum_out"] = csum
    abuf, bbuf = abuf.to(dev), bbuf.to(dev)
    cbuf = cbuf0.clone().to(dev)
    call = dict(trans_a=ta, trans_b=tb, lda=lda, ldb=ldb, ldc=ldc, act=g("act", 0), alpha=g("alpha", 0.0), amap=amap, cmap=cmap, kmap=kmap,
                accumulate=bool(g("accumulate")), out_f32=f32, tile_hint=g("tile_hint", 0), split_hint=g("split_hint", 0),
                colscale=g("colscale"), keep_output=bool(g("keep_output")), **kw)
    ops.gemm(abuf, bbuf, M, N, K, out=cbuf, **call)
    for i in range(g("repeat", 0)):
        again = cbuf0.clone().to(dev)
        ops.gemm(abuf, bbuf, M, N, K, out=again, **call)
        assert same_bits(again, cbuf), f"{name}: launch {i + 2} differs from the first"
    rows = R.map_rows(cmap, M, dev)
    got = cbuf[rows, :N]
    zk = pre[rows, :N] if g("preact") == "z" else None
    # ---- reference: on the host, or on the device for the two large cases
    rd = dev if g("ref_dev") else "cpu"
    t = lambda x: None if x is None else x.to(rd)
    ref = R.gemm_ref(t(abuf), t(bbuf), M, N, K, trans_a=ta, trans_b=tb, lda=lda, ldb=ldb, amap=amap, cmap=cmap, kmap=kmap, bias=t(kw.get("bias")),
                     act=g("act", 0), preact_deriv=g("preact") == "deriv", residual=t(kw.get("residual")), act_bwd_z=t(kw.get("act_bwd_z")),
                     act_bwd=g("act_bwd", 0), alpha=g("alpha", 0.0) or 1.0, alpha_dev=t(kw.get("alpha_dev")), out_f32=f32,
                     c_old=cbuf0.to(rd) if g("accumulate") else None, colscale=g("colscale"), want_colsum=bool(g("colsum")),
                     zdelta=ZDELTA, z_from=t(zk), residual_on_fp32=path == "small_m", **rkw)
    single = ref["c"] is ref["z"]
    key = "c32" if f32 else "z" if single else "c"
    R.close_ref(t(got), ref["c"], gates[f"{path}.{key}"], f"{path}.{key} | {name}")
    untouched(cbuf, cmap, M, N, sent, f"{name} C")
    if g("preact"):
        k2 = "z" if g("preact") == "z" else "deriv"
        R.close_ref(t(pre[rows, :N]), ref[k2], gates[f"{path}.{k2}"], f"{path}.{k2} | {name} preact_out")
        untouched(pre, cmap, M, N, SENT_BF, f"{name} preact_out")
    if g("tap"):
        sel = torch.arange(0, M, g("tap"), device=rd)
        zt = R.Ref(ref["z"].lo[sel], ref["z"].hi[sel], ref["z"].scale[sel])
        R.close_ref(t(tap[:ntap]), zt, gates[f"{path}.z"], f"{path}.z | {name} row_tap_out")
        assert same_bits(tap[ntap:], torch.full_like(tap[ntap:], SENT_BF)), f"{name}: written behind row_tap_out"
    if g("colsum"):
        R.close_ref(t(csum[:M]), ref["colsum"], gates[f"{path}.colsum"], f"{path}.colsum | {name} colsum_out")
        assert same_bits(csum[M:], torch.full_like(csum[M:], SENT_BF)), f"{name}: written behind colsum_out"
    if g("drop"):
        # a dropped element is the residual's bits, or +0: the mask is keep_mask's (a kept element that were dropped would miss its gate)
        keep = R.keep_mask(DROP_SEED, DROP_OFFSET, M, N, g("drop"), device=dev)
        want = kw["residual"][rows, :N] if g("residual") else torch.zeros(M, N, dtype=BF, device=dev)
        assert same_bits(got[~keep], want[~keep]), f"{name}: a dropped element is not {'the residual' if g('residual') else '+0'}"
        assert 0 < int((~keep).sum()) < M * N
    return got


def run_batched(ops, dev, form, batch, M, N, K):
    """ops.gemm_batched: `batch` products of one shape (contiguous operands, plain epilogue), each against the fp64 reference; a sentinel
    row behind every C"""
    ta, tb = form == "tn", form != "nt"
    name = f"batched {form} x{batch} {M}x{N}x{K}"
    gen = _gen(name)
    al, bl, cl = [], [], []
    for _ in range(batch):
        A, B = operands(gen, M, N, K)
        al.append(lay(A.t().contiguous() if ta else A, IDENT, M if ta else K, NAN).to(dev))
        bl.append(lay(B if tb else B.t().contiguous(), IDENT, N if tb else K, NAN).to(dev))
        cl.append(torch.full((M + 1, N), SENT_BF, dtype=BF, device=dev))
    ops.gemm_batched(al, bl, cl, M, N, K, trans_a=ta, trans_b=tb)
    for i, (a, b, c) in enumerate(zip(al, bl, cl)):
        ref = R.gemm_ref(a.cpu(), b.cpu(), M, N, K, trans_a=ta, trans_b=tb, lda=a.shape[1], ldb=b.shape[1])
        R.close_ref(c[:M].cpu(), ref["c"], GATES["batched.z"], f"batched.z | {name} problem {i}")
        assert same_bits(c[M:], torch.full_like(c[M:], SENT_BF)), f"{name}: problem {i} wrote behind its C"


# ------------------------------------------------------------------------------------------------------------------ case tables
CMAP5 = (2, 3, 1)          # rows 1, 2, 4, 5, 7, ...: every third row of C / the residual / preact_out is skipped, and row 0
KMAP = (3, 4, 1)           # reduction rows 1, 2, 3, 5, 6, 7, ...
AMAP = (4, 5, 1)


def tail_parts(M, N, K):
    """mpv_gemm_bf16's tail split of the 128x128 kernel (bf16 output, no colsum, unsplit): parts per tile of the last round"""
    nwg = -(-M // 128) * -(-N // 128)
    r, nk = nwg % 512, -(-K // 64)
    tg = min(8, 512 // r) if r else 1
    while tg > 1 and nk // tg < 16:
        tg -= 1
    return -(-nk // -(-nk // tg)) if tg > 1 else 1


def splitk128(M, N, K):
    """choose_splitk + the rounding of mpv_gemm_bf16: splits of a weight-gradient product on the 128x128 kernel (a workspace that is large enough)"""
    tiles = -(-M // 128) * -(-N // 128)
    best, best_eff = 1, 0.0
    for s in range(1, 33):
        if s > 1 and K // s < 256:
            break
        blocks = tiles * s
        eff = blocks / (-(-blocks // 512) * 512)
        if eff > best_eff + 0.02:
            best, best_eff = s, eff
    if best == 1:
        return 1
    kps = -(-(-(-K // best)) // 64) * 64
    return -(-K // kps)


def _small_m():
    """mpv_gemm_bf16's decode branch: forward form, M <= 16, bias / act / residual / cmap only.  Instances by its if-chain:
    <true,16,8>: N % 16 == 0, K % 64 == 0, K >= 4096, N <= 4096;  <true,4,8>: N % 16 == 0, K % 64 == 0, N <= 6144;
    <true,4,16>: N % 16 == 0, K % 64 == 0 (N > 6144);  <false>: anything else (N % 8 == 0, K % 8 == 0)."""
    out = []
    shapes = [
        ("t16x8", 16, 4096),       # <true,16,8>: 64 K-blocks on 16 waves = 4 each: exactly one unrolled batch (UN = 4) per wave
        ("t16x8", 16, 4160),       # 65 K-blocks, 5 per wave: 13 waves get blocks, the last of them none of the batch but one remainder step
        ("t16x8", 4096, 4096),     # the largest N of the instance (512 workgroups)
        ("t4x8", 16, 64),          # <true,4,8>: one K-block, waves 1-3 idle
        ("t4x8", 16, 576),         # 9 K-blocks, 3 per wave: the remainder loop only (UN = 8)
        ("t4x8", 16, 2112),        # 33 K-blocks, 9 per wave: one unrolled batch plus one
        ("t4x8", 6144, 64),        # the largest N of the instance
        ("t4x16", 6160, 64),       # <true,4,16>: the smallest N past 6144 that is a multiple of 16
        ("t4x16", 6160, 576),
        ("gen", 8, 64),            # <false>: half a column tile
        ("gen", 24, 64),           # a full and a half column tile
        ("gen", 6152, 64),         # N % 16 != 0 at the width of the widest instance
        ("gen", 16, 8),            # one half-chunk of one K-block: every other chunk masked
        ("gen", 16, 72),           # the second K-block holds one half-chunk
        ("gen", 16, 200),          # four K-blocks (one per wave), the last with 8 of 64 columns
    ]
    for inst, N, K in shapes:
        for M in (1, 5, 16):
            out.append(case(f"small_m-{inst}-{M}x{N}x{K}", "small_m", "nt", M, N, K, repeat=1 if M == 5 else 0))
    eps = [("bias", dict(bias=True)), ("erf", dict(bias=True, act=ACT_GELU_ERF)), ("tanh", dict(bias=True, act=ACT_GELU_TANH)),
           ("relu", dict(bias=True, act=ACT_RELU)), ("res-ldr", dict(residual=True, pad_r=8)), ("ldc", dict(pad_c=16, pad_a=8, pad_b=8)),
           ("cmap", dict(bias=True, residual=True, cmap=CMAP5)),          # the decoder's qkv row landing in the KV cache
           ("all", dict(bias=True, act=ACT_GELU_TANH, residual=True, pad_r=8, pad_c=16, cmap=CMAP5))]
    for inst, N, K in (("t16x8", 16, 4096), ("t4x8", 16, 576), ("t4x16", 6160, 64), ("gen", 24, 72)):
        for en, e in eps:
            out.append(case(f"small_m-{inst}-5x{N}x{K}-{en}", "small_m", "nt", 5, N, K, **e))
        # M = 17 leaves the decode branch: the SAME product on the 128x128 tile kernel, same reference, that path's gates
        out.append(case(f"small_m-{inst}-17x{N}x{K}-tile-kernel", "k128_tail" if tail_parts(17, N, K) > 1 else "k128", "nt", 17, N, K,
                        bias=True, act=ACT_GELU_TANH, residual=True))
    return out


def _k128():
    """gemm_bf16_kernel<TA, TB> pinned with tile_hint=128 (M < 256 or N < 256 reach it unpinned too)"""
    out = []
    h = dict(tile_hint=128)
    for form in ("nt", "nn", "tn"):
        for M, N, K in ((128, 128, 64),      # one full tile, one K step
                        (136, 136, 72),      # ragged on every edge: a second tile of 8 rows / columns, a second K step of 8 (tn: M % 8 == 0)
                        (8, 8, 8)):          # the smallest legal product (forward: pinned away from the decode branch by alpha below)
            # (8, 8, 8) in the forward form is the decode branch's (tile_hint does not pin it away): gemm_small_m_kernel<false>
            out.append(case(f"k128-{form}-{M}x{N}x{K}", "small_m" if (form == "nt" and M <= 16) else "k128", form, M, N, K, repeat=1, **h))
    for form in ("nt", "nn"):
        out.append(case(f"k128-{form}-129x136x72", "k128", form, 129, 136, 72, **h))          # M odd: one live row in the second tile
    # an option outside the decode branch's condition keeps the (8, 8, 8) forward product on the tile kernel
    out.append(case("k128-nt-8x8x8-f32", "k128", "nt", 8, 8, 8, out_f32=True, **h))
    # ---- weight gradients: transA puts no alignment condition on K
    for K in (71, 200, 3077):      # odd | ragged | choose_splitk: 1 tile, K / s >= 256 -> s = 12 -> 10 splits of 320 rows, the last of 197 (odd)
        p = "k128_splitk" if splitk128(128, 128, K) > 1 else "k128"
        out.append(case(f"k128-tn-128x128x{K}", p, "tn", 128, 128, K, repeat=1, **h))
        out.append(case(f"k128-tn-128x128x{K}-colsum", p, "tn", 128, 128, K, colsum=True, **h))
        out.append(case(f"k128-tn-136x136x{K}-kmap-pads", p, "tn", 136, 136, K, kmap=KMAP, pad_a=8, pad_b=16, colsum=True, **h))
    out.append(case("k128-tn-128x128x3077-accumulate", "k128_splitk", "tn", 128, 128, 3077, accumulate=True, **h))
    out.append(case("k128-tn-128x128x200-accumulate", "k128", "tn", 128, 128, 200, accumulate=True, **h))
    out.append(case("k128-tn-128x128x200-f32", "k128", "tn", 128, 128, 200, out_f32=True, **h))
    out.append(case("k128-tn-128x128x200-f32-accumulate", "k128", "tn", 128, 128, 200, out_f32=True, accumulate=True, alpha=0.5, **h))
    out.append(case("k128-nn-136x136x72-kmap", "k128", "nn", 136, 136, 72, kmap=KMAP, **h))
    out.append(case("k128-nt-136x136x72-amap-cmap", "k128", "nt", 136, 136, 72, amap=AMAP, cmap=CMAP5, pad_a=8, pad_c=8, **h))
    # ---- tail split: nwg % 512 tiles of the last round are cut along K while a part keeps >= 16 K steps
    for M, N, K, why in ((128, 128, 2048, "two parts of 16 steps"), (128, 128, 2112, "33 steps: parts of 17 and 16"),
                         (128, 128, 8192, "eight parts (the cap)"), (384, 256, 2048, "six tail tiles x two parts")):
        for en, e in (("bias-res", dict(bias=True, residual=True)), ("erf-pre", dict(bias=True, act=ACT_GELU_ERF, preact="z")),
                      ("plain", {})):
            out.append(case(f"k128-tail-{M}x{N}x{K}-{en}", "k128_tail", "nt", M, N, K, repeat=2 if en == "bias-res" else 0, **h, **e))
    out.append(case("k128-tail-nn-128x128x2048-drop-res", "k128_tail", "nn", 128, 128, 2048, drop=0.1, residual=True, **h))
    out.append(case("k128-tail-nt-128x128x2048-colscale", "k128_tail", "nt", 128, 128, 2048, bias=True, colscale=(64, 0.125), **h))
    # ---- every epilogue option singly at a ragged two-tile shape, then the model's combinations (model.py / generation.py call sites)
    S = (136, 136, 72)
    eps = [
        ("bias", dict(bias=True)), ("bias-unaligned", dict(bias="unaligned")),
        ("erf", dict(act=ACT_GELU_ERF)), ("tanh", dict(act=ACT_GELU_TANH)), ("relu", dict(act=ACT_RELU)),
        ("erf-pre", dict(bias=True, act=ACT_GELU_ERF, preact="z")), ("tanh-pre", dict(bias=True, act=ACT_GELU_TANH, preact="z")),
        ("erf-deriv", dict(bias=True, act=ACT_GELU_ERF, preact="deriv")), ("tanh-deriv", dict(bias=True, act=ACT_GELU_TANH, preact="deriv")),
        ("bwd-erf", dict(act_bwd=ACT_GELU_ERF, pad_z=8)), ("bwd-tanh", dict(act_bwd=ACT_GELU_TANH)), ("bwd-mul", dict(act_bwd=ACT_DERIV, pad_z=8)),
        ("drop", dict(bias=True, drop=0.1)), ("drop-res", dict(bias=True, drop=0.5, residual=True)),
        ("res", dict(residual=True)), ("res-pads", dict(bias=True, residual=True, pad_r=8, pad_c=16)),
        ("alpha", dict(alpha=0.125)), ("alpha-bias", dict(alpha=-0.03125, bias=True)), ("alpha_dev", dict(alpha_dev=0.37, bias=True)),
        ("alpha-alpha_dev", dict(alpha=0.5, alpha_dev=-1.5)),
        ("f32", dict(out_f32=True)), ("f32-accumulate", dict(out_f32=True, accumulate=True)), ("f32-alpha", dict(out_f32=True, alpha=0.25, pad_c=8)),
        ("accumulate", dict(accumulate=True)), ("accumulate-alpha_dev", dict(accumulate=True, alpha_dev=0.37)),
        ("colscale", dict(bias=True, colscale=(64, 0.125))), ("colscale-all", dict(bias=True, colscale=(136, 0.125))),
        ("tap-res", dict(bias=True, residual=True, tap=5)),          # the ViT block's per-frame cls rows beside the residual epilogue
        ("tap", dict(bias=True, tap=5)),
        ("pre-res-cmap", dict(bias=True, act=ACT_GELU_ERF, preact="z", residual=True, cmap=CMAP5, pad_c=8, pad_r=16)),
        ("relu-res-accumulate", dict(bias=True, act=ACT_RELU, residual=True, accumulate=True)),
    ]
    for en, e in eps:
        form = "nn" if "bwd" in en else "nt"
        out.append(case(f"k128-{form}-136x136x72-{en}", "k128", form, *S, **h, **e))
    return out


def _k256():
    """gemm256_kernel<TA, TB, KMAP, rows>: tile_hint 256 / 192 / 160, M >= 256 (any M for the short tiles), N >= 256, K % 64 == 0
    (a weight gradient without kmap: K >= 64)"""
    out = []
    for rows in (256, 192, 160):
        h = dict(tile_hint=rows)
        for form, extra, tag in (("nt", {}, "nt"), ("nn", {}, "nn"), ("nn", dict(kmap=KMAP), "nn-kmap"), ("tn", {}, "tn"), ("tn", dict(kmap=KMAP), "tn-kmap")):
            if rows != 256 and tag in ("nn-kmap", "tn", "tn-kmap"):
                continue          # the short tiles exist for the k-contiguous-A instances only (bandable in mpv_gemm256_try_launch)
            for M, N, K in ((256, 256, 64), (264, 328, 192)):          # one tile, one K-tile | ragged on M and N, three K-tiles
                out.append(case(f"k256-r{rows}-{tag}-{M}x{N}x{K}", "k256", form, M, N, K, repeat=1, **h, **extra))
        if rows != 256:
            for M in (160, 161, 192, 193, 333):      # one tile less / exactly / one row past a tile of either height; three short tiles
                out.append(case(f"k256-r{rows}-nt-{M}x256x64", "k256", "nt", M, 256, 64, bias=True, residual=True, **h))
    S = (264, 328, 192)
    eps = [
        ("EP_PLAIN-bias", "nt", dict(bias=True)), ("EP_PLAIN-keep_output", "nt", dict(bias=True, keep_output=True)), ("EP_PLAIN-colscale", "nt", dict(bias=True, colscale=(64, 0.125))),
        ("EP_ERF_PRE", "nt", dict(bias=True, act=ACT_GELU_ERF, preact="z")), ("EP_ERF_PRE-deriv", "nt", dict(bias=True, act=ACT_GELU_ERF, preact="deriv")),
        ("EP_TANH_PRE", "nt", dict(bias=True, act=ACT_GELU_TANH, preact="z")), ("EP_TANH_PRE-deriv", "nt", dict(bias=True, act=ACT_GELU_TANH, preact="deriv")),
        ("EP_BWD_ERF", "nn", dict(act_bwd=ACT_GELU_ERF, pad_z=8)), ("EP_BWD_TANH", "nn", dict(act_bwd=ACT_GELU_TANH)),
        ("EP_MUL", "nn", dict(act_bwd=ACT_DERIV, pad_z=8)),
        ("EP_RES", "nt", dict(bias=True, residual=True, pad_r=8, pad_c=16)), ("EP_RES-tap", "nt", dict(bias=True, residual=True, tap=5)),
        ("EP_RES-cmap", "nt", dict(bias=True, residual=True, cmap=CMAP5, amap=AMAP)),
        ("EP_DROP_RES", "nt", dict(bias=True, drop=0.1, residual=True)), ("EP_DROP", "nt", dict(bias=True, drop=0.5)),
        ("EP_GENERIC-relu-res-accumulate", "nt", dict(bias=True, act=ACT_RELU, residual=True, accumulate=True)),
        ("EP_GENERIC-tap", "nt", dict(bias=True, tap=5)), ("EP_GENERIC-alpha_dev-accumulate", "nt", dict(alpha_dev=0.37, accumulate=True)),
        ("f32", "nt", dict(out_f32=True)), ("f32-accumulate", "tn", dict(out_f32=True, accumulate=True)),
        ("alpha-bias", "nt", dict(alpha=-0.03125, bias=True)),
    ]
    for en, form, e in eps:
        for rows in ((256, 160) if en in ("EP_ERF_PRE", "EP_RES", "EP_DROP_RES", "EP_MUL") else (256,)):
            out.append(case(f"k256-r{rows}-{form}-264x328x192-{en}", "k256", form, *S, tile_hint=rows, **e))
    # a bias 8 bytes off a 16-byte boundary: mpv_gemm256_try_launch declines, the 128x128 kernel takes the product
    out.append(case("k256-nt-264x328x192-bias-unaligned-falls-to-128", "k128", "nt", *S, tile_hint=256, bias="unaligned", residual=True))
    # ---- weight gradients
    out.append(case("k256-tn-256x256x200", "k256", "tn", 256, 256, 200, tile_hint=256, split_hint=1, colsum=True))      # K % 64 != 0: a partial last K-tile
    out.append(case("k256-tn-256x256x71", "k256", "tn", 256, 256, 71, tile_hint=256, split_hint=1))                     # K odd
    for s in (2, 3):      # 328 rows = 6 K-tiles: 2 x 3 | 3 x 2; 340 rows: 3 + 3 K-tiles, the last of 20 rows | 2 + 2 + 2
        out.append(case(f"k256-tn-264x328x340-split{s}", "k256_splitk", "tn", 264, 328, 340, tile_hint=256, split_hint=s, repeat=1))
        out.append(case(f"k256-tn-264x328x340-split{s}-colsum-accumulate", "k256_splitk", "tn", 264, 328, 340, tile_hint=256, split_hint=s,
                        colsum=True, accumulate=True))
    out.append(case("k256-tn-256x256x320-split3-ragged", "k256_splitk", "tn", 256, 256, 320, tile_hint=256, split_hint=3))   # 5 K-tiles: 2 + 2 + 1
    out.append(case("k256-tn-kmap-256x256x384-split3", "k256_splitk", "tn", 256, 256, 384, tile_hint=256, split_hint=3, kmap=KMAP, colsum=True))
    # ---- forward split (t256 * 2 <= 256 tiles, K >= 4096): bias and dropout move into splitk_reduce_kernel
    for en, e in (("plain", {}), ("bias", dict(bias=True)), ("bias-drop", dict(bias=True, drop=0.1)), ("drop", dict(drop=0.5))):
        out.append(case(f"k256-fwdsplit-nt-256x256x4096-{en}", "k256_fwdsplit", "nt", 256, 256, 4096, tile_hint=256, repeat=1 if en == "bias-drop" else 0, **e))
    # choose_splitk256 asks for 17 splits of the 136 K-tiles (K / 17 = 512), mpv_gemm_bf16 clamps to 16 (the workspace's size): 16 x 9 K-tiles, the last of 1
    out.append(case("k256-fwdsplit-nt-256x256x8704-clamp16-bias-drop", "k256_fwdsplit", "nt", 256, 256, 8704, tile_hint=256, bias=True, drop=0.1))
    out.append(case("k256-fwdsplit-nn-264x328x4096-bias-drop", "k256_fwdsplit", "nn", 264, 328, 4096, tile_hint=256, bias=True, drop=0.1))
    # a residual keeps the same product out of the split: the tile epilogue (EP_DROP_RES) at K = 4096
    out.append(case("k256-nt-256x256x4096-drop-res-unsplit", "k256", "nt", 256, 256, 4096, tile_hint=256, bias=True, drop=0.1, residual=True))
    return out


SMALL_M_CASES, K128_CASES, K256_CASES = _small_m(), _k128(), _k256()
# (form, batch, M, N, K): mpv_gemm_bf16_batched -- one problem | GEMM_BATCH_MAX = 16 in one launch | 17: a second launch of one
BATCHED = [(f, b, M, N, K) for f in ("nt", "nn", "tn") for b in (1, 16, 17) for (M, N, K) in ((64, 64, 64), (136, 72, 200 if f == "tn" else 72))]
# multi-band launches (mpv_gemm256_try_launch with tile_hint = 0): the smallest shapes whose plan on 256 CUs has two / three bands.
# (name, case, the plan mpv_gemm_plan_bands must give, preact, ext_rows)
BANDS = [
    (case("bands2-nt-32648x768x768-res-cmap", "k256", "nt", 32648, 768, 768, bias=True, residual=True, cmap=CMAP5, ref_dev=True), (256, 160), 0, 1),
    (case("bands3-nn-16328x2304x2048-res-cmap", "k256", "nn", 16328, 2304, 2048, residual=True, cmap=CMAP5, ref_dev=True), (256, 192, 160), 0, 1),
]
