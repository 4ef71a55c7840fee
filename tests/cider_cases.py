"""Token tables for the CIDEr tests (include/mpv.h: mpv_caption_cider; ops.caption_cider), shared by tests/test_cider_cpu.py (the
reference tests/ref_cider.py against the recorded scores of the reference project's scorer, generation.CiderStats, the stand-in) and
tests/test_cider_gpu.py (the kernel against the same reference).  TEST INFRASTRUCTURE ONLY.  Every case is a dict of CPU tensors and
host lists:
  tok_a / tok_b   int64 [rows, ld]: candidates / references; the first width_a / width_b columns are the row, what lies behind the
                  width is GUARD: a sentinel token that would lengthen a caption or change its n-grams if it were read
  start_a/_b      the first caption column per row;  begin_a/_b: the groups' (clips') CSR offsets;  term: the termination id
  groups_a/_b     the captions the tables were built from, per group (token lists; never holding `term`)
  corpus          the reference sets the corpus statistics are built from: the groups WITH references, in order (a group without
                  references is no document: its candidates score 0.0 by definition)
  vocab, capacity what generation.CiderStats gets (capacity None: its own choice)
The edges: caption lengths 0 .. 5 (an order without n-gram), 100 and 255; repeated tokens (tf > 1, the min clips); a candidate equal to
its reference; n-grams the corpus does not hold; a corpus of ONE clip (log_ref_len = 0: every weight, norm and value 0); a length
difference of 252 (the penalty underflows to 0); ragged groups, one without candidates and one without references; start columns > 0
and a start per row; a row stride above the width; `term` in the first column; ids 0 and 65534; a table forced to the smallest
capacity above its entry count (long probe chains that wrap past the last slot)."""
import random

import torch

TERM = 2
GUARD = 7             # behind the width: never `term`, and a token of the alphabets, so a read behind the width changes the result
MAX_LEN = 255
VOCAB = 65535
LENGTH_EDGES = [0, 1, 2, 3, 4, 5, 100, 255]


def _table(caps, starts, width, ld, rng, term=TERM):
    """rows [len(caps), ld]: row r = starts[r] prompt tokens (`term` among them), the caption, then -- when columns are left -- `term`
    and arbitrary tokens up to the width; behind the width the guard"""
    rows = torch.empty((len(caps), max(ld, 1)), dtype=torch.int64)
    for r, (c, s) in enumerate(zip(caps, starts)):
        assert term not in c and s + len(c) <= width and width - s <= MAX_LEN, (r, s, len(c), width)
        row = [rng.choice([term, 3, 4, 5, 6]) for _ in range(s)] + list(c)
        if len(row) < width:
            row += [term] + [rng.choice([term, 3, 4, 5, 6]) for _ in range(width - len(row) - 1)]
        row += [GUARD] * (rows.shape[1] - width)
        rows[r] = torch.tensor(row, dtype=torch.int64)
    return rows


def _begin(groups):
    out = [0]
    for g in groups:
        out.append(out[-1] + len(g))
    return out


def _case(name, groups_a, groups_b, rng, width_a, width_b, pad_a=0, pad_b=0, starts_a=None, starts_b=None, capacity=None):
    ca, cb = [c for g in groups_a for c in g], [c for g in groups_b for c in g]
    sa = starts_a if starts_a is not None else [0] * len(ca)
    sb = starts_b if starts_b is not None else [0] * len(cb)
    return dict(name=name, term=TERM, vocab=VOCAB, capacity=capacity, groups_a=groups_a, groups_b=groups_b, corpus=[g for g in groups_b if g],
                start_a=sa, start_b=sb, begin_a=_begin(groups_a), begin_b=_begin(groups_b), width_a=width_a, width_b=width_b,
                tok_a=_table(ca, sa, width_a, width_a + pad_a, rng), tok_b=_table(cb, sb, width_b, width_b + pad_b, rng))


def _draw(rng, n, alphabet):
    return [rng.choice(alphabet) for _ in range(n)]


def _cases():
    rng = random.Random(20241020)
    out = []
    al = [3, 4, 5, 6, 7, 9, 11]
    # 1. the short lengths, clipping, identity, unseen n-grams, ids 0 and 65534; ragged groups (no candidates: group 2; no references:
    #    group 3); a start per row; `term` in the first column (the empty candidate of group 0 starts at column 0); guard columns
    refs = [[[3, 4, 5, 6, 7], [3, 4, 3, 4, 9], [5]],
            [[0, 65534, 0, 65534, 9], [11, 11, 11, 11, 11, 11]],
            [[4, 5, 6], [9, 9]],
            [],
            [[3, 4, 5, 6, 7, 9, 11, 3], [7, 6, 5, 4]],
            [[6]]]
    cands = [[[], [3], [3, 4], [3, 4, 5], [3, 4, 5, 6], [3, 4, 5, 6, 7], [3, 4, 3, 4, 9], [3, 3, 3, 3, 3, 3, 4]],
             [[11, 11], [11, 11, 11, 11, 11, 11, 11, 11], [0, 65534, 0], [65534], [40000, 40001, 40002, 40003, 40004]],
             [],
             [[3, 4, 5], [9]],
             [[3, 4, 5, 6, 7, 9, 11, 3], [4, 5, 6, 7, 12, 13], [7, 6, 5, 4, 7, 6, 5, 4]],
             [[6], [6, 6], []]]
    na, nb = sum(len(g) for g in cands), sum(len(g) for g in refs)
    sa = [0] + [rng.randint(0, 5) for _ in range(na - 1)]
    sb = [rng.randint(0, 4) for _ in range(nb)]
    out.append(_case("edges", cands, refs, rng, 14, 13, pad_a=5, pad_b=3, starts_a=sa, starts_b=sb))
    # 2. a corpus of one clip: log_ref_len = 0, so every idf, norm and value is 0 -- and none is NaN
    out.append(_case("one_clip", [[[3, 4, 5, 6], [3, 4], []]], [[[3, 4, 5, 6], [4, 5, 6, 7, 9]]], rng, 8, 8, pad_a=2))
    # 3. lengths 255 and 100 over two symbols (tf up to hundreds), a reference of 3 tokens against a candidate of 255 (the penalty is
    #    exp(-882) = 0), rows that fill their table to the last column (no `term`), starts > 0 at full length
    two = [5, 9]
    long_refs = [[_draw(rng, 255, two), [5, 9, 5]], [_draw(rng, 100, two), _draw(rng, 254, [5, 9, 11])], [[11, 5, 9, 9, 5]]]
    long_cands = [[_draw(rng, 255, two), list(long_refs[0][0])], [_draw(rng, 100, two), [9, 5, 9]], [_draw(rng, 255, [5, 9, 11])]]
    out.append(_case("long", long_cands, long_refs, rng, 258, 257, starts_a=[3, 3, 158, 20, 3], starts_b=[2, 100, 157, 3, 7]))
    # 4. a few thousand distinct n-grams in a table forced to the smallest capacity above them: long probe chains, wrap-around
    big = list(range(100, 160))
    crefs = [[_draw(rng, rng.randint(6, 14), big) for _ in range(2)] for _ in range(40)]
    ccands = [[list(g[0][:5]) + _draw(rng, rng.randint(1, 6), big), _draw(rng, rng.randint(3, 12), big + [60000])] for g in crefs]
    case = _case("chains", ccands, crefs, rng, 16, 16, pad_b=1)
    entries = len({tuple(r[i:i + n]) for g in crefs for r in g for n in range(1, 5) for i in range(len(r) - n + 1)})
    cap = 2
    while cap <= entries:
        cap *= 2
    case["capacity"] = cap
    out.append(case)
    return out


CASES = _cases()
NAMES = [c["name"] for c in CASES]

# one hypothesis per clip against its references: the evaluation's corpus metric (df from these references, the mean over clips)
EVAL_REFS = [[[3, 4, 5, 6, 7, 9], [3, 4, 5, 9]], [[11, 12, 13, 14], [11, 12, 12, 14, 15]], [[3, 4, 20, 21, 22]], [[30, 31, 32, 33, 34, 35, 36]],
             [[9, 9, 9, 4], [9, 4]]]
EVAL_HYPS = [[3, 4, 5, 6, 7], [11, 12, 13, 14], [20, 21, 22, 3, 4], [30, 31, 40, 33, 34, 35], [9, 9, 4]]


def refused_table():
    """tables whose width - start is 256 for one candidate row: refused on the host before any launch
    -> (tok_a, start_a, begin_a, tok_b, start_b, begin_b)"""
    return torch.full((3, 260), 5, dtype=torch.int64), [10, 4, 30], [0, 3], torch.full((2, 8), 5, dtype=torch.int64), [0, 0], [0, 2]
