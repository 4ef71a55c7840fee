"""The cases, guarded buffers and runner of the packed shared-prefix TRAINING attention (tests/test_prefix_train_refs_cpu.py without
a GPU, tests/test_prefix_train_gpu.py on the MI355X), TEST INFRASTRUCTURE ONLY.

A case is (head_dim, heads, prefix_len, length list, continuations per group, accumulate_prefix).  The layouts are those of the
forward's sweep (caption_score_cases.LAYOUTS: every length list as one group and as all-ones groups, and mixes that put a group of more
than 128 rows beside smaller ones); 128 rows are a workgroup's tile of query rows (dQ) and of keys (dK/dV), 64 a chunk, 32 a wave's
tile.  Every layout runs twice per head_dim, overwriting and accumulating; heads (1 / 3) and prefix_len (0, 1, 33, 64, 65, 130: none /
one key / a ragged 32-tile / one chunk / one key over it / one key-tile workgroup and two keys of a second) rotate over the layouts so
that every value meets every head_dim: 60 problems.

Operands are views of real [rows, 3H] qkv buffers (head h's q / k / v at columns 3 h hd, + hd, + 2 hd, as the decoder's qkv product
writes them) inside guarded arenas (attention_cases.Arena): 64 rows of slack in front of and behind every tensor, NaN in the slack of
operands and a fixed bit pattern in the slack of outputs -- which includes the q columns of the prefix gradient buffer, which no kernel
owns.  Gates: attention_cases.GATES; dpk / dpv take the dk / dv gates."""
import torch

import attention_cases as A
import caption_score_cases as cs
import ref_attention as R
import ref_prefix_train as RP

BF = torch.bfloat16
PREFIX_LENS = [0, 1, 33, 64, 65, 130]
GATE_OF = dict(o="o", lse="lse", dq="dq", dk="dk", dv="dv", dpk="dk", dpv="dv")


def _cases():
    out = []
    for hd in (64, 80):
        for li, lay in enumerate(cs.LAYOUTS):
            for acc in (0, 1):
                P = PREFIX_LENS[(li + 3 * acc + (hd == 80)) % 6]
                heads = (1, 3)[(li + acc) % 2]
                out.append(dict(name=f"hd{hd}-h{heads}-P{P}-{cs.layout_id(lay)}" + ("-acc" if acc else ""), hd=hd, heads=heads, P=P,
                                cont_len=lay[0], groups=lay[1], acc=acc, seed=1000 * hd + 50 * li + acc))
    return out


CASES = _cases()


def inputs(c, device):
    """-> q, k, v, do [rows, heads, hd], pk, pv, dpk_in, dpv_in [G, heads, P, hd]: contiguous bf16, unit-variance"""
    rows, G, heads, hd, P = sum(c["cont_len"]), len(c["groups"]), c["heads"], c["hd"], c["P"]
    q, k, v, do = (A.rn((rows, heads, hd), c["seed"] + i, device) for i in range(4))
    pk, pv, dpk_in, dpv_in = (A.rn((G, heads, P, hd), c["seed"] + 4 + i, device) for i in range(4))
    return q, k, v, do, pk, pv, dpk_in, dpv_in


_refs = {}


def references(c, device, model=False):
    """the fp64 reference of a case, computed once per (case, device, model), shared and never modified"""
    key = (c["name"], str(device), model)
    if key not in _refs:
        q, k, v, do, pk, pv, dpk_in, dpv_in = inputs(c, device)
        ref = RP.reference(q, k, v, do, pk, pv, c["cont_len"], c["groups"], c["P"], c["hd"] ** -0.5,
                           dpk_in if c["acc"] else None, dpv_in if c["acc"] else None, model=model)
        _refs[key] = dict(ref, inputs=(q, k, v, do, pk, pv, dpk_in, dpv_in))
    return _refs[key]


def compare(got, ref, what, names=tuple(GATE_OF)):
    for n in names:
        if n in got and ref[n].numel():
            R.close_gated(got[n], ref[n], ref["scale_" + n], A.GATES[GATE_OF[n]][:2], f"{what} {n}")


# ------------------------------------------------------------------------------------------------------------------ GPU side
class Buffers:
    """The guarded device buffers of one case: qkv / dqkv [rows, 3H] and pqkv / dpqkv [G P, 3H] with the decoder's column order, o / og
    (the o given to the backward) / do [rows, H], lse / lseg [heads, rows]."""

    def __init__(self, c, dev):
        self.c = c
        rows, G, heads, hd, P = sum(c["cont_len"]), len(c["groups"]), c["heads"], c["hd"], c["P"]
        H = heads * hd
        self.rows, self.G, self.H = rows, G, H
        self.arenas = {}
        S = A.SLACK_ROWS

        def cut(name, n, width, fill, parts):
            a = A.Arena((n + 2 * S) * width, BF, fill, dev)
            a.row = width
            self.arenas[name] = a
            return [a.view(S * width + off, shape, strides) for off, shape, strides in parts]

        rowv = lambda w, off: (off, (rows, heads, hd), (w, w // heads, 1))                      # noqa: E731
        prev = lambda off: (off, (G, heads, P, hd), (P * 3 * H, 3 * hd, 3 * H, 1))              # noqa: E731
        self.q, self.k, self.v = cut("qkv", rows, 3 * H, A.NAN_BITS, [rowv(3 * H, i * hd) for i in range(3)])
        self.dq, self.dk, self.dv = cut("dqkv", rows, 3 * H, A.GUARD_BITS, [rowv(3 * H, i * hd) for i in range(3)])
        self.pk, self.pv = cut("pqkv", G * P, 3 * H, A.NAN_BITS, [prev(hd), prev(2 * hd)])
        self.dpk, self.dpv = cut("dpqkv", G * P, 3 * H, A.GUARD_BITS, [prev(hd), prev(2 * hd)])
        (self.o,) = cut("o", rows, H, A.GUARD_BITS, [rowv(H, 0)])
        (self.og,) = cut("og", rows, H, A.NAN_BITS, [rowv(H, 0)])
        (self.do,) = cut("do", rows, H, A.NAN_BITS, [rowv(H, 0)])
        for name in ("lse", "lseg"):
            a = A.Arena(2 * S + heads * rows, torch.float32, A.GUARD_BITS32, dev)
            self.arenas[name] = a
            setattr(self, name, a.view(S, (heads, rows), (rows, 1)))
        self.row_strides = ((3 * H, 3 * hd),) * 3 + ((H, hd),)
        pst = (P * 3 * H, 3 * hd, 3 * H)
        self.prefix_lay = (pst, pst)

    def load(self, q, k, v, do, pk, pv, og, lseg):
        for dst, src in ((self.q, q), (self.k, k), (self.v, v), (self.do, do), (self.pk, pk), (self.pv, pv), (self.og, og)):
            dst.copy_(src)
        self.lseg.copy_(lseg)

    def reset_outputs(self, dpk_in=None, dpv_in=None):
        for n in ("dqkv", "dpqkv", "o", "lse"):
            self.arenas[n].refill()
        if dpk_in is not None:
            self.dpk.copy_(dpk_in)
            self.dpv.copy_(dpv_in)

    def check(self, what):
        for n, a in self.arenas.items():
            a.check(f"{what}: {n}", getattr(a, "row", None))

    def forward(self, ops, layout, lse_entry=True):
        c = self.c
        args = (self.q, self.k, self.v, self.pk, self.pv, self.o, self.row_strides, self.prefix_lay, layout, c["heads"], c["P"], c["hd"])
        if lse_entry:
            ops.attn_prefix_packed_fwd_lse(*args, scale=c["hd"] ** -0.5, lse=self.lse)
        else:
            ops.attn_prefix_packed_fwd(*args, scale=c["hd"] ** -0.5)

    def backward(self, ops, layout, acc=None, **kw):
        c = self.c
        ops.attn_prefix_packed_bwd(self.q, self.k, self.v, self.pk, self.pv, self.og, self.lseg, self.do, self.dq, self.dk, self.dv, self.dpk,
                                   self.dpv, self.row_strides, self.prefix_lay, layout, c["heads"], c["P"], kw.pop("hd", c["hd"]),
                                   scale=kw.pop("scale", c["hd"] ** -0.5), accumulate_prefix=c["acc"] if acc is None else acc)

    def outputs(self):
        return {n: getattr(self, n).clone() for n in ("o", "lse", "dq", "dk", "dv", "dpk", "dpv")}


def bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF else torch.int32)
