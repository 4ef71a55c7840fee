"""The cases of the guidance tests (tests/test_guidance_cpu.py, tests/test_guidance_gpu.py): rows 1 / 3 / 5 x vocabularies 8 / 64 / 264 /
25600 x a leading dimension of the conditional matrix equal to the vocabulary, 8 and 24 columns wider, with POISON behind the
vocabulary; the unconditional matrix with a leading dimension of its own; the maximum in column 0, in the last column and in the last
16-byte chunk; rows that are all equal; ties at the maximum; scales 0 / 0.5 / 1 / 1.5 / 3; alpha 0, 0.1 and one just below 1 (only
ties with the maximum survive); values near the largest finite bf16; cond and uncond as the two halves of one allocation.  25600
columns are 3200 chunks: a thread of the 1024 holds three whole chunks and some a fourth, the kernel's partial last round.  The
data of a case is a function of the case alone (a seeded generator), built on the CPU."""
import itertools

import torch

POISON = -7.5                                      # behind the vocabulary: must stay as it is
BAN_INF = float("-inf")
BAN_FINITE = -float.fromhex("0x1.fep127")          # the lowest finite bf16
ALPHA_TIES = 1.0 - 2.0 ** -10                      # log(alpha) = -9.8e-4: closer to 0 than any non-zero difference of two bf16 logits near a
                                                   # maximum of at least 0.5 (2^-9), and further from 0 than the fp32 error of any c here
KINDS = ("random", "max_first", "max_last", "max_tail", "all_equal", "ties", "huge")
SCALES = (0.0, 0.5, 1.0, 1.5, 3.0)
ALPHAS = (0.0, 0.1, ALPHA_TIES)
PADS = (0, 8, 24)


def _grid():
    """every (rows, vocab, pad of cond); kind, pad of uncond, scale, alpha and ban value rotate through it with co-prime periods, so
    that every value of each meets every vocabulary"""
    out = []
    for i, (rows, V, pad_c) in enumerate(itertools.product((1, 3, 5), (8, 64, 264, 25600), PADS)):
        out.append(dict(rows=rows, V=V, pad_c=pad_c, pad_u=PADS[(PADS.index(pad_c) + 1 + i % 2) % 3],      # ld_u != ld_c, either way round
                        kind=KINDS[i % 7], scale=SCALES[i % 5], alpha=ALPHAS[(i + i // 3) % 3], ban=(BAN_INF, BAN_FINITE)[i % 2], shared=False))
    # what the rotation does not reach by itself: every kind at the big vocabulary under the strongest settings, and the shared allocation
    for k, kind in enumerate(KINDS):
        out.append(dict(rows=3, V=25600, pad_c=8, pad_u=24, kind=kind, scale=3.0, alpha=ALPHAS[k % 3], ban=BAN_INF, shared=False))
    for V, scale, alpha in ((8, 3.0, 0.1), (264, 1.5, 0.0), (25600, 3.0, ALPHA_TIES), (25600, 0.0, 0.1)):
        out.append(dict(rows=5, V=V, pad_c=8, pad_u=8, kind="random", scale=scale, alpha=alpha, ban=BAN_FINITE, shared=True))
    for c in out:                                  # near the largest finite bf16 the fp32 error of a difference dwarfs any log(alpha): no ban there
        if c["kind"] == "huge":
            c["alpha"] = 0.0
    return out


KERNEL_CASES = _grid()


def case_id(c):
    return (f"r{c['rows']}-V{c['V']}-c{c['pad_c']}-u{c['pad_u']}-{c['kind']}-s{c['scale']}-a{'ties' if c['alpha'] == ALPHA_TIES else c['alpha']}"
            f"-{'inf' if c['ban'] == BAN_INF else 'fin'}{'-shared' if c['shared'] else ''}")


def _rows(kind, rows, V, g):
    """fp32 [rows, V] of one matrix: values that are bf16 after the cast"""
    x = torch.randn(rows, V, generator=g) * 3.0
    if kind == "huge":                             # all within the top binades of bf16: the differences stay finite in fp32
        return 3.0e38 + torch.rand(rows, V, generator=g) * 3.8e37
    if kind == "all_equal":
        return torch.full((rows, V), 0.0) + torch.arange(rows)[:, None] * 1.25 - 1.25        # row 0: -1.25, row 1: all zeros, ...
    if kind == "ties":
        x = x.clamp(max=6.0)
        x[:, torch.randperm(V, generator=g)[:max(2, V // 16)]] = 6.0
        return x
    col = dict(max_first=0, max_last=V - 1, max_tail=V - 5).get(kind)
    if col is not None:
        x[:, col] = 17.0
    return x


def build(c, seed=0):
    """-> dict(cond [rows, V + pad_c] bf16, uncond [rows, V + pad_u] bf16, both with POISON behind the vocabulary; with shared=True the
    two are the halves of ONE [2 * rows, V + pad] tensor, `whole`)"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * c["rows"] + c["V"] + c["pad_c"] + 31 * KINDS.index(c["kind"]))
    rows, V = c["rows"], c["V"]
    a = _rows(c["kind"], rows, V, g)
    b = _rows(c["kind"] if c["kind"] in ("huge", "all_equal") else "random", rows, V, g)
    if c["shared"]:
        assert c["pad_c"] == c["pad_u"]
        whole = torch.full((2 * rows, V + c["pad_c"]), POISON, dtype=torch.bfloat16)
        whole[:rows, :V], whole[rows:, :V] = a.to(torch.bfloat16), b.to(torch.bfloat16)
        return dict(cond=whole[:rows], uncond=whole[rows:], whole=whole)
    cond = torch.full((rows, V + c["pad_c"]), POISON, dtype=torch.bfloat16)
    uncond = torch.full((rows, V + c["pad_u"]), POISON, dtype=torch.bfloat16)
    cond[:, :V], uncond[:, :V] = a.to(torch.bfloat16), b.to(torch.bfloat16)
    return dict(cond=cond, uncond=uncond, whole=None)
