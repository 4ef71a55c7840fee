"""The case tables, gates, guarded buffers and runners of the attention suite (tests/test_attention_refs_cpu.py without a GPU,
tests/test_attention_kernels_gpu.py on the MI355X), TEST INFRASTRUCTURE ONLY.

A case is the smallest shape that reaches an instance of the variant table of csrc/attention.hip (ATTN_VARIANTS, 53 rows) or a branch
inside one: a ragged last tile, more rows than one block, causal with sk > sq, an odd sk / an odd dropout offset (where attention's
key-pair mask convention and the element-pair one differ), a batch that is no multiple of 8 (the grid pads it), head_dim below the
instantiated one.  Every case names the three instances (forward, dQ, dK/dV) the plan must give it on the 256 CUs of an MI355X; both
tests assert the names, so a dispatch change that leaves an instance without a case fails there and not in silence.

GATES.  |got - ref| <= rtol |ref| + coef x scale (ref_attention: the scale of an element is the sum of its absolute terms).
rtol = 2^-8 for a bf16 output, one rounding.  coef counts the bf16 intermediates on the path, plus EPS = 2^-12 per intermediate for
what fp32 does (accumulation and its order, v_exp_f32: n 2^-24 of the scale for n terms, 2^-13 at the 2049 keys of the longest case,
so EPS is twice the worst of it):
    o, dV    P                                   2^-8 + EPS
    dQ, dK   dS; the given o inside delta        2 x (2^-9 + EPS)
    lse      fp32: rtol 2^-20, coef 2^-20
    temporal out / dq / dk / dv                  2^-8 + EPS   (P or dS as the matrix-core instances round them; the VALU instances round less)
THE P ROUNDING COUNTS 2^-8, NOT 2^-9.  A rounding to bf16 (8 significant bits) moves a value by up to 2^-8 of itself -- the same figure as
rtol -- and 2^-9 only on the average over a binade.  An element of MANY terms stays near the average (the rounding model of
ref_attention measures 0.8e-3 .. 2.1e-3 of the scale on the rows of 100+ keys), but the case table is full of elements of ONE or TWO
terms, where a single rounding is the whole error: dV of a key that only the last causal rows see, o of the first causal rows, every
element at T <= 4, sq = 1.  There the rounding MODEL ITSELF reaches 3.6e-3 (dV, stream64-1x2049[needle]; 3.3e-3 for o, pair5-64-drop[needle];
2.9e-3 temporal out at T = 4), above 2^-9 + EPS = 2.2e-3: no kernel that rounds P to bf16 at all could meet that figure, so the
coefficient of the P rounding is its worst case.  dQ / dK keep 2 x (2^-9 + EPS) = 2^-8 + 2 EPS, which already is the worst case of the
one rounding of dS (the given o enters the reference and the kernel alike); the model stays below 1.5e-3 there.  The temporal dq / dk
have the one rounding of dS and no given o: 2^-8 + EPS, the same worst case (their model residual, many terms per element, is <= 5e-4).
WHAT THE CPU TEST HOLDS THE MODEL TO is `residual <= coef - EPS part`: the model, which knows no fp32 effect, must fit the bf16 part of a
gate alone.  It is NOT held to half the gate ("a factor 2 to spare"): on one-term elements the model legitimately uses 3.6e-3 of the
3.9e-3 a rounding allows.  The factor 2 is in EPS instead, against the worst fp32 accumulation error (above).
The gates come from these rounding points alone; profiles/attention_kernel_errors.md holds the rounding model's and the kernels'
measured residuals next to them.

GUARDS.  Every operand and output is a view into a larger buffer (Arena): at least 64 rows of slack in front of and behind each tensor,
gap columns and gap rows in the padded layout, the other tensors' columns in the packed one, and room for the 7 padding items of a
batch that is no multiple of 8 behind every output.  Operand slack holds the bf16 NaN pattern, output slack a fixed bit pattern; after
a run every output element is finite and every byte of slack is compared on the raw bits."""
import ctypes as C

import torch

import ref_attention as R

BF = torch.bfloat16

RTOL_BF16 = 2.0 ** -8
COEF_P = 2.0 ** -8 + R.EPS                                 # one rounding of P (or dS) to bf16, worst case (module text)
COEF_DS = 2 * (2.0 ** -9 + R.EPS)                          # dS and the given o inside delta
# name -> (rtol, coef, the EPS part of coef)
GATES = {"o": (RTOL_BF16, COEF_P, R.EPS), "dv": (RTOL_BF16, COEF_P, R.EPS), "dq": (RTOL_BF16, COEF_DS, 2 * R.EPS), "dk": (RTOL_BF16, COEF_DS, 2 * R.EPS),
         "lse": (2.0 ** -20, 2.0 ** -20, 0.0)}
TEMPORAL_GATES = {n: (RTOL_BF16, COEF_P, R.EPS) for n in ("out", "dq", "dk", "dv")}

NAN_BITS, GUARD_BITS, GUARD_BITS32 = 0x7FC0, 0x5A5A, 0x5A5A5A5A
SLACK_ROWS = 64
DROP_SEED = 0x9E3779B97F4A7C15 & ~(1 << 63)

# ------------------------------------------------------------------------------------------------------------------ instances
def _three(fwd, dq, dkv):
    return (fwd, dq, dkv)


STREAM = {hd: _three(f"attn_fwd_kernel<{hd}>", f"attn_bwd_dq_kernel<{hd}>", f"attn_bwd_dkv_kernel<{hd}>") for hd in (64, 80, 96)}
RES = {hd: _three(f"attn_fwd_res_kernel<{hd}>", f"attn_bwd_dq_res_kernel<{hd}>", f"attn_bwd_dkv_res_kernel<{hd}, 512>") for hd in (64, 80, 96)}
SMALL64 = _three("attn_fwd_res_kernel<64, 0, 5, 320, 3>", "attn_bwd_dq_res_kernel<64, 0, 320, 3>", "attn_bwd_dkv_res_kernel<64, 320, 3>")
VIT7 = _three("attn_fwd_res_kernel<96, 7>", "attn_bwd_dq_res_kernel<96, 7>", "attn_bwd_dkv_res_kernel<96, 512>")
PAIR7 = _three("attn_fwd_pair64_kernel<7, 256, 2>", "attn_bwd_dq_pair64_kernel<256, 3>", "attn_bwd_dkv_pair64_kernel<256, 3>")
PAIR5 = _three("attn_fwd_pair64_kernel<5, 192, 3>", "attn_bwd_dq_pair64_kernel<192, 3>", "attn_bwd_dkv_res_kernel<64, 320, 3>")
PAIR5_ALL = _three(PAIR5[0], PAIR5[1], "attn_bwd_dkv_pair64_kernel<192, 3>")          # MPV_ATTN_PAIR=2
DUO = ("attn_bwd_dq_duo96_kernel<256>", "attn_bwd_dkv_duo96_kernel<256>")
LEAN_DUO = _three("attn_fwd_pres_kernel<96, 7, 8, 512, 1, true>", *DUO)
PRES_DUO = _three("attn_fwd_pres_kernel<96, 7>", *DUO)
RES7_DUO = _three("attn_fwd_res_kernel<96, 7>", *DUO)
BOTH = ("randn", "needle")          # every case runs both input classes


def case(name, shape, plan, layout="bshd", classes=BOTH, sqb=0, offset=0, seed=DROP_SEED, seed_indirect=False):
    B, H, sq, sk, hd, causal, p = shape
    return dict(name=name, shape=shape, plan=plan, layout=layout, classes=classes, sqb=sqb, offset=offset, seed=seed, seed_indirect=seed_indirect)


# (B, H, Sq, Sk, hd, causal, p)
STREAMING = [
    case("stream64-40x300", (1, 2, 40, 300, 64, 0, 0.0), STREAM[64]),
    case("stream80-causal-40x300-drop", (1, 2, 40, 300, 80, 1, 0.1), STREAM[80], offset=7),                 # causal with sk > sq
    case("stream96-causal-290", (1, 1, 290, 290, 96, 1, 0.0), STREAM[96], layout="padded"),
    case("stream80-hd72-33x289-drop", (2, 2, 33, 289, 72, 0, 0.1), STREAM[80], layout="padded", offset=(3 << 36) + 1),      # odd sk
    case("stream64-1x2049", (2, 2, 1, 2049, 64, 0, 0.0), STREAM[64]),                        # one key over DEC_MAX_SK
]
ONE_SHOT = [
    case("small64-causal-33x70-drop", (3, 2, 33, 70, 64, 1, 0.1), SMALL64, offset=9),                       # causal with sk > sq
    case("small64-hd8-causal-33", (1, 2, 33, 33, 8, 1, 0.0), SMALL64, layout="packed"),
    case("small64-hd40-33x65", (1, 2, 33, 65, 40, 0, 0.0), SMALL64, layout="padded"),
    case("res64-161", (2, 2, 161, 161, 64, 0, 0.0), RES[64]),
    case("res64-causal-225-drop", (2, 2, 225, 225, 64, 1, 0.1), RES[64], layout="packed"),                  # one row over PAIR_MAX_ROWS
    case("res80-causal-160-drop", (2, 2, 160, 160, 80, 1, 0.1), RES[80], layout="packed", seed_indirect=True),
    case("res80-97x256", (2, 2, 97, 256, 80, 0, 0.0), RES[80], layout="padded"),
    case("res96-256-drop", (2, 2, 256, 256, 96, 0, 0.1), RES[96]),                                          # RES_MAX_ROWS
    case("res96-197-drop", (2, 2, 197, 197, 96, 0, 0.1), RES[96], sqb=1, offset=5),                         # ViT length, dropout, odd sk
    case("vit7-hd88-197", (2, 2, 197, 197, 88, 0, 0.0), VIT7, layout="packed", sqb=2),
    case("vit7-32x197", (2, 2, 32, 197, 96, 0, 0.0), VIT7, layout="padded"),
    case("res80-causal-160-drop-b17", (17, 2, 160, 160, 80, 1, 0.1), RES[80]),               # 7 padding items
]
PAIRED = [
    case("pair7-208-drop", (2, 2, 208, 208, 64, 1, 0.1), PAIR7, layout="packed", offset=1),
    case("pair7-161-drop", (3, 2, 161, 161, 64, 1, 0.1), PAIR7, layout="padded"),                           # six blocks: the fewest
    case("pair5-160-drop", (2, 2, 160, 160, 64, 1, 0.1), PAIR5, layout="packed"),
    case("pair5-64-drop", (2, 2, 64, 64, 64, 1, 0.1), PAIR5, offset=(1 << 33) + 3),
    case("pair5-1-drop", (2, 2, 1, 1, 64, 1, 0.1), PAIR5),
    case("pair7-161-drop-b17", (17, 2, 161, 161, 64, 1, 0.1), PAIR7),                        # 7 padding items
]
PERSISTENT = [
    case("lean-duo-33x8-197", (33, 8, 197, 197, 96, 0, 0.0), LEAN_DUO, sqb=1),
    case("pres-duo-9x32-201", (9, 32, 201, 201, 96, 0, 0.0), PRES_DUO),
    case("res7-duo-193-sqb", (2, 2, 193, 193, 96, 0, 0.0), RES7_DUO, sqb=1),                                # shortest 7-tile
    case("res7-duo-224", (2, 2, 224, 224, 96, 0, 0.0), RES7_DUO, layout="padded"),                          # longest 7-tile
]
DECODE = [case(f"decode-{B}x{H}x{sk}-hd{hd}" + ("-sqb" if sqb else ""), (B, H, 1, sk, hd, 0, 0.0),
               ("attn_decode_kernel<8>" if hd <= 64 else "attn_decode_kernel<16>", None, None), sqb=sqb)
          for (B, H, sk, hd) in ((3, 4, 1, 64), (2, 2, 2048, 64), (2, 3, 33, 96), (1, 2, 7, 8), (2, 2, 77, 80)) for sqb in (0, 1)]
ATTN_GROUPS = dict(streaming=STREAMING, one_shot=ONE_SHOT, paired=PAIRED, persistent=PERSISTENT, decode=DECODE)
ALL_ATTN = [c for g in ATTN_GROUPS.values() for c in g]
PAIR_KNOB_CASES = [dict(c, name=c["name"] + "-pairdkv", plan=PAIR5_ALL) for c in PAIRED if c["plan"] is PAIR5]       # MPV_ATTN_PAIR=2


# temporal: (n_outer, n_inner, T, heads, hd) -> the forward and the backward instance
def tcase(shape, fwd, bwd, long=False, tag=""):
    return dict(name="temporal-" + tag + "x".join(str(s) for s in shape), shape=shape, plan=(fwd, bwd), long=long)


TEMPORAL_B16 = [tcase((2, 6, T, 2, 96), f"temporal_attn_b16_kernel<false, {T}, 96>", f"temporal_attn_b16_kernel<true, {T}, 96>") for T in (4, 8, 16)]
TEMPORAL_F32_KNOB = [tcase((2, 6, T, 2, 96), f"temporal_attn_kernel<false, {T}, 96>", f"temporal_attn_kernel<true, {T}, 96>", tag="f32rows-") for T in (4, 8, 16)]
TEMPORAL_RUNTIME = [tcase(s, "temporal_attn_kernel<false>", "temporal_attn_kernel<true>")
                    for s in ((1, 3, 1, 2, 4), (1, 3, 5, 2, 64), (2, 6, 16, 2, 48), (2, 6, 3, 2, 96),
                              (1, 70000, 2, 1, 4))]      # 70000 problems of one wave: the 16384-workgroup cap, the stride loop runs
TEMPORAL_MFMA = [tcase((1, 5, T, 3, hd), f"temporal_attn_mfma_kernel<false, {32 if T <= 32 else 64}>",
                       f"temporal_attn_mfma_kernel<true, {32 if T <= 32 else 64}>", long=True)
                 for T in (17, 32, 33, 64) for hd in (16, 80, 96)]      # 15 problems: the last 4-wave workgroup is ragged
ALL_TEMPORAL = TEMPORAL_B16 + TEMPORAL_RUNTIME + TEMPORAL_MFMA
KNOB_ARMS = {"MPV_ATTN_PAIR=2": "pair", "MPV_TEMPORAL_ROWS=fp32": "temporal"}


def instances_named():
    """every instance the tables name, the knob arms' included: must be the whole variant table"""
    names = {n for c in ALL_ATTN + PAIR_KNOB_CASES for n in c["plan"] if n}
    return names | {n for c in ALL_TEMPORAL + TEMPORAL_F32_KNOB for n in c["plan"]}


# ------------------------------------------------------------------------------------------------------------------ buffers
class Arena:
    """A flat buffer filled with one bit pattern, out of which tensors are cut as strided views; check() compares every element no view
    owns with the pattern, on the raw bits, and names the first that differs."""

    def __init__(self, n, dtype, fill_bits, device):
        self.buf = torch.empty(n, dtype=dtype, device=device)
        self.bits = self.buf.view(torch.int16 if dtype == BF else torch.int32)
        self.fill = fill_bits
        self.bits.fill_(fill_bits)
        self.owned = torch.zeros(n, dtype=torch.bool, device=device)

    def view(self, offset, shape, strides):
        torch.as_strided(self.owned, shape, strides, offset).fill_(True)
        return torch.as_strided(self.buf, shape, strides, offset)

    def refill(self):
        self.bits.masked_fill_(self.owned, self.fill)

    def check(self, what, row=None):
        bad = (self.bits != self.fill) & ~self.owned
        if bool(bad.any()):
            i = int(bad.nonzero()[0].item())
            where = f" (row {i // row}, column {i % row} of the buffer)" if row else ""
            raise AssertionError(f"{what}: guard element {i}{where} of {int(bad.sum().item())} changed: bits {int(self.bits[i].item()) & 0xffffffff:#x}, "
                                 f"pattern {self.fill:#x}")


def strides_of(kind, S, H, hd, parts=1):
    """(batch, head, row) strides in elements and the column offset of part i"""
    if kind == "packed":
        rs, hs = H * parts * hd, parts * hd
        return (S * rs, hs, rs), hd
    if kind == "padded":
        rs = H * hd + 8
        return ((S + 3) * rs, hd, rs), 0
    rs = H * hd
    return (S * rs, hd, rs), 0


def cut(kind, B, S, H, hd, parts, fill, device, pad_items=0):
    """-> (arena, [views [B, H, S, hd]], strides): `parts` tensors of one layout out of one arena"""
    (bs, hs, rs), step = strides_of(kind, S, H, hd, parts)
    front = SLACK_ROWS * rs
    a = Arena(front + (B + pad_items) * bs + 2 * SLACK_ROWS * rs, BF, fill, device)
    a.row = rs
    if kind != "packed":
        assert parts == 1
    return a, [a.view(front + i * step, (B, H, S, hd), (bs, hs, rs, 1)) for i in range(parts)], (bs, hs, rs)


def stat(B, H, sq, device):
    """a guarded fp32 [B, H, sq] statistics tensor (lse, delta): room for the 7 padding items behind it"""
    n = B * H * sq
    a = Arena(SLACK_ROWS + n + 8 * H * sq + SLACK_ROWS, torch.float32, GUARD_BITS32, device)
    return a, a.view(SLACK_ROWS, (B, H, sq), (H * sq, sq, 1))


# ------------------------------------------------------------------------------------------------------------------ inputs
def rn(shape, seed, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF).to(device)


def make_inputs(c, klass, device, items=None):
    """-> q, k, v, dO as contiguous bf16 [B, H, S, hd], scale.  items: cap on batch and heads (the CPU test: items are independent)"""
    B, H, sq, sk, hd, causal, p = c["shape"]
    if items:
        B, H = min(B, items), min(H, items)
    scale = hd ** -0.5
    q, k, v, do = (rn((B, H, s, hd), 100 + i, device) for i, s in enumerate((sq, sk, sk, sq)))
    if klass == "needle":
        R.plant_needles(q, k, v, R.needle_pairs(sq, sk, causal), scale)
    if c["sqb"] == 2:
        q = (q.float() * torch.tensor(scale, dtype=torch.float32, device=device)).to(BF)
    return q, k, v, do, scale, (B, H)


def keep_of(c, B, H, device, deref=None, seed=None):
    _, _, sq, sk, _, _, p = c["shape"]
    if p == 0.0:
        return None, 1.0
    return R.attn_keep_mask(c["seed"] if seed is None else seed, c["offset"], B, H, sq, sk, p, device=device, deref=deref), R.drop_scale(p)


def references(c, klass, device, items=None, model=False):
    """the fp64 forward and backward of a case (the backward from bf16(o_ref) and fp32(lse_ref): a backward instance is judged on its own)"""
    q, k, v, do, scale, (B, H) = make_inputs(c, klass, device, items)
    causal = c["shape"][5]
    keep, ds = keep_of(c, B, H, device)
    fwd = R.attn_fwd_ref(q, k, v, causal, scale, c["sqb"], keep, ds)
    o_given, lse_given = R.rbf(fwd["o"]).to(BF), fwd["lse"].to(torch.float32)
    bwd = R.attn_bwd_ref(q, k, v, o_given, lse_given, do, causal, scale, c["sqb"], keep, ds)
    out = dict(q=q, k=k, v=v, do=do, scale=scale, keep=keep, ds=ds, fwd=fwd, bwd=bwd, o_given=o_given, lse_given=lse_given, B=B, H=H)
    if model:
        out["fwd_model"] = R.attn_fwd_ref(q, k, v, causal, scale, c["sqb"], keep, ds, model=True)
        out["bwd_model"] = R.attn_bwd_ref(q, k, v, o_given, lse_given, do, causal, scale, c["sqb"], keep, ds, model=True)
    return out


def compare(got, ref, what, names=("o", "lse", "dq", "dk", "dv")):
    """The one comparison of both tests: got[name] against the references of references(), every element, at GATES."""
    for n in names:
        if n not in got:
            continue
        src = ref["fwd"] if n in ("o", "lse") else ref["bwd"]
        R.close_gated(got[n], src[n], src["scale_" + n], GATES[n][:2], f"{what} {n}")


# ------------------------------------------------------------------------------------------------------------------ GPU runners
def _desc(ops, t, lse, lay, c, B, H, seed, scale):
    _, _, sq, sk, hd, causal, p = c["shape"]
    return ops._attn_desc(t["q"], t["k"], t["v"], t["o"], lse, lay, B, H, sq, sk, hd, causal, scale, c["sqb"], p, seed, c["offset"])


def planned(ops, t, lay, c, B, H, scale, roles=(0, 1, 2)):
    _, _, sq, sk, hd, causal, p = c["shape"]
    return tuple(ops.attn_plan(r, t["q"], t["k"], t["v"], t["o"], lay, B, H, sq, sk, hd, causal=causal, scale=scale, scale_q_bf16=c["sqb"],
                               dropout_p=p)["variant"] for r in roles)


def run_attention(ops, _lib, dev, c, klass):
    """One case, one input class, on the GPU: plan names, forward and backward against the fp64 references at GATES, guards, and under
    dropout a second run that must be bit-identical.  -> dict of the kernel's outputs."""
    B, H, sq, sk, hd, causal, p = c["shape"]
    what = f"{c['name']}[{klass}]"
    ref = references(c, klass, dev)
    scale, lib, st = ref["scale"], _lib.lib(), ops._stream()
    kind, packed = c["layout"], c["layout"] == "packed"
    assert not packed or sq == sk
    pad = (-B) % 8
    # operands (NaN slack) and outputs (pattern slack, room for the padding items)
    arenas = {}
    if packed:
        arenas["qkv"], (q, k, v), st_q = cut(kind, B, sq, H, hd, 3, NAN_BITS, dev)
        arenas["dqkv"], (dq, dk, dv), _ = cut(kind, B, sq, H, hd, 3, GUARD_BITS, dev, pad)
        st_k, okind = st_q, "bshd"
    else:
        arenas["q"], (q,), st_q = cut(kind, B, sq, H, hd, 1, NAN_BITS, dev)
        arenas["k"], (k,), st_k = cut(kind, B, sk, H, hd, 1, NAN_BITS, dev)
        arenas["v"], (v,), _ = cut(kind, B, sk, H, hd, 1, NAN_BITS, dev)
        arenas["dq"], (dq,), _ = cut(kind, B, sq, H, hd, 1, GUARD_BITS, dev, pad)
        arenas["dk"], (dk,), _ = cut(kind, B, sk, H, hd, 1, GUARD_BITS, dev, pad)
        arenas["dv"], (dv,), _ = cut(kind, B, sk, H, hd, 1, GUARD_BITS, dev, pad)
        okind = kind
    arenas["o"], (o,), st_o = cut(okind, B, sq, H, hd, 1, GUARD_BITS, dev, pad)
    arenas["do"], (do,), _ = cut(okind, B, sq, H, hd, 1, NAN_BITS, dev)
    arenas["og"], (og,), _ = cut(okind, B, sq, H, hd, 1, NAN_BITS, dev)          # the o GIVEN to the backward
    arenas["lse"], lse = stat(B, H, sq, dev)
    arenas["lseg"], lseg = stat(B, H, sq, dev)
    arenas["delta"], delta = stat(B, H, sq, dev)
    for dst, src in ((q, ref["q"]), (k, ref["k"]), (v, ref["v"]), (do, ref["do"]), (og, ref["o_given"])):
        dst.copy_(src)
    lseg.copy_(ref["lse_given"])
    lay = ops.AttnLayout(st_q, st_k, st_k, st_o)
    t = dict(q=q, k=k, v=v, o=o)
    seed = c["seed"]
    if c["seed_indirect"]:
        cell = torch.tensor([c["seed"]], dtype=torch.int64, device=dev)
        seed = R.SEED_INDIRECT_BIT | cell.data_ptr()
        again, _ = keep_of(c, B, H, dev, deref=lambda addr: cell.item() if addr == cell.data_ptr() else None, seed=seed)
        assert torch.equal(again, ref["keep"])
    backward = c["plan"][1] is not None
    assert planned(ops, t, lay, c, B, H, scale, (0, 1, 2) if backward else (0,)) == tuple(n for n in c["plan"] if n), what
    got = {}
    for rep in range(2 if p > 0 else 1):
        for a in ("o", "lse", "delta") + (("dqkv",) if packed else ("dq", "dk", "dv")):
            arenas[a].refill()
        d = _desc(ops, t, lse, lay, c, B, H, seed, scale)
        _lib.check(lib.mpv_attn_fwd(C.byref(d), st), "mpv_attn_fwd")
        if backward:
            d = _desc(ops, dict(t, o=og), lseg, lay, c, B, H, seed, scale)
            _lib.check(lib.mpv_attn_bwd(C.byref(d), do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), st), "mpv_attn_bwd")
        torch.cuda.synchronize()
        now = dict(o=o.clone(), lse=lse.clone())
        if backward:
            now.update(dq=dq.clone(), dk=dk.clone(), dv=dv.clone(), delta=delta.clone())
        if rep:
            for n in now:
                assert torch.equal(now[n].view(torch.int16 if now[n].dtype == BF else torch.int32),
                                   got[n].view(torch.int16 if got[n].dtype == BF else torch.int32)), f"{what}: {n} differs between two runs of one (seed, offset)"
        got = now
    for n, x in got.items():
        assert bool(torch.isfinite(x.float()).all()), f"{what}: {n} is not finite"
    for n, a in arenas.items():
        a.check(f"{what}: {n}", getattr(a, "row", None))
    compare(got, ref, what)
    return got


def temporal_describe(_binding, c):
    info, lib = _binding.AttnPlanInfo(), _binding.lib()
    no, ni, T, heads, hd = c["shape"]
    f = lib.mpv_temporal_attn_long_plan_describe if c["long"] else lib.mpv_temporal_attn_plan_describe
    out = []
    for bwd in (0, 1):
        _binding.check(f(no, ni, T, heads, hd, bwd, C.byref(info)), "temporal plan")
        out.append((info.variant.decode(), info.grid_x, info.block))
    return out


def temporal_inputs(c, device):
    B, N, T, heads, hd = c["shape"]
    D, N1 = heads * hd, N + 1
    Rr = B * T * N1
    return rn((Rr, 3 * D), 50, device), rn((Rr + SLACK_ROWS, D), 51, device), Rr


def run_temporal(ops, _lib, dev, c):
    """The layout and canaries of test_temporal_long_gpu.run_kernel_case (cls rows no problem owns between the sequences, 64 pre-filled
    rows behind out / dout / dqkv), the values against temporal_ref at TEMPORAL_GATES, every unowned row on the raw bits."""
    B, N, T, heads, hd = c["shape"]
    what = c["name"]
    D, N1, scale = heads * hd, N + 1, hd ** -0.5
    qkv, dout_all, Rr = temporal_inputs(c, dev)
    names = temporal_describe(_lib, c)
    assert (names[0][0], names[1][0]) == c["plan"], (what, names)
    if N >= 70000:
        assert names[0][1] == names[1][1] == 16384 and names[0][2] == 64, (what, names)
    ref = R.temporal_ref(qkv, dout_all[:Rr], B, N, T, heads, hd, scale)
    bits = lambda x: x.contiguous().view(torch.int16)      # noqa: E731
    out_all = rn((Rr + SLACK_ROWS, D), 52, dev)
    dqkv_all = rn((Rr + SLACK_ROWS, 3 * D), 53, dev)
    out0, dout0, dqkv0 = out_all.clone(), dout_all.clone(), dqkv_all.clone()
    args = (B, T * N1, N, 1, N1, T, heads, hd, scale)
    ops.temporal_attn_fwd(qkv, out_all, *args)
    ops.temporal_attn_bwd(qkv, dout_all, dqkv_all, *args)
    torch.cuda.synchronize()
    assert torch.equal(bits(out_all[Rr:]), bits(out0[Rr:])), f"{what}: forward wrote behind the last row"
    assert torch.equal(bits(out_all[:Rr].view(B, T, N1, D)[:, :, 0]), bits(out0[:Rr].view(B, T, N1, D)[:, :, 0])), f"{what}: forward wrote a cls row"
    assert torch.equal(bits(dout_all), bits(dout0)), f"{what}: backward wrote dout"
    assert torch.equal(bits(dqkv_all[Rr:]), bits(dqkv0[Rr:])), f"{what}: backward wrote behind the last row"
    assert torch.equal(bits(dqkv_all[:Rr].view(B, T, N1, 3 * D)[:, :, 0]), bits(dqkv0[:Rr].view(B, T, N1, 3 * D)[:, :, 0])), f"{what}: backward wrote a cls row"
    got = dict(out=R.temporal_rows(out_all[:Rr], B, N, T, heads, hd))
    got["dq"], got["dk"], got["dv"] = R.temporal_split(dqkv_all[:Rr], B, N, T, heads, hd)
    for n, x in got.items():
        assert bool(torch.isfinite(x.float()).all()), f"{what}: {n} is not finite"
        R.close_gated(x, ref[n], ref["scale_" + n], TEMPORAL_GATES[n][:2], f"{what} {n}")
    return got
