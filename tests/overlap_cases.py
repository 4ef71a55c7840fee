"""Token tables for the caption-overlap tests (include/mpv.h: mpv_caption_overlap; ops.caption_overlap), shared by
tests/test_overlap_cpu.py (the stand-in and the host code against tests/ref_overlap.py) and tests/test_overlap_gpu.py (the kernel
against the same reference).  Every case is a dict of CPU tensors and host lists:
  tok_a / tok_b   int64 [rows, ld]: the first width_a / width_b columns are the row (ld may exceed the width; what lies behind the
                  width is bait: tokens that would change the counts if they were read)
  start_a/_b      the first generated column per row;  begin_a/_b: the groups' CSR offsets;  term: the termination id
  same            True: tok_b IS tok_a (the call passes one table), the *_b entries repeat the *_a ones
  cands_a/_b      the candidates the tables were built from, for the reference (token lists; never holding `term`)
The edges: candidate lengths 0, 1, 3 (shorter than order 4), 4, 63, 64, 65 and 255; groups of 0, 1, 2, 8 (64 pairs: one full wave),
9 (81 pairs: a partial second wave) and 17 rows, ragged in one call; repeated tokens where clipping decides the count; identical rows;
disjoint alphabets; a two-symbol alphabet at length 255; ids up to 51199; rows without a `term`, with `term` at start, with a `term`
inside the prompt, with their own start each; a row stride above the width; two tables of different widths."""
import random

import torch

TERM = 2
MAX_LEN = 255
LENGTH_EDGES = [0, 1, 3, 4, 63, 64, 65, 255]
GROUP_EDGES = [0, 1, 2, 8, 9, 17]


def _table(cands, starts, width, ld, rng, term=TERM, prompt_term=(), vocab=51200):
    """rows [len(cands), ld]: row r = prompt of starts[r] tokens (holding `term` for r in prompt_term), the candidate, then -- when
    columns are left -- `term` and arbitrary tokens (`term` among them) up to the width; behind the width, bait"""
    rows = torch.empty((len(cands), ld), dtype=torch.int64)
    for r, (c, s) in enumerate(zip(cands, starts)):
        assert term not in c and s + len(c) <= width and width - s <= MAX_LEN, (r, s, len(c), width)
        prompt = [rng.choice([t for t in (3, 4, 5, 6, 7, 51199) if t != term]) for _ in range(s)]
        if r in prompt_term and s:
            prompt[rng.randrange(s)] = term
        row = prompt + list(c)
        if len(row) < width:
            row += [term] + [rng.choice([term, 3, 4, 5, 6]) for _ in range(width - len(row) - 1)]
        row += [rng.choice([3, 4, 5, 6, 7]) for _ in range(ld - width)]        # never term: a read behind the width lengthens a candidate
        rows[r] = torch.tensor(row, dtype=torch.int64)
    return rows


def _begin(sizes):
    out = [0]
    for n in sizes:
        out.append(out[-1] + n)
    return out


def _case(name, groups_a, starts_a, width_a, ld_a, rng, groups_b=None, starts_b=None, width_b=None, ld_b=None, prompt_term_a=(),
          prompt_term_b=()):
    cands_a = [c for g in groups_a for c in g]
    case = dict(name=name, term=TERM, same=groups_b is None, cands_a=cands_a, start_a=list(starts_a), begin_a=_begin([len(g) for g in groups_a]),
                width_a=width_a, tok_a=_table(cands_a, starts_a, width_a, ld_a, rng, prompt_term=prompt_term_a))
    if groups_b is None:
        case.update(cands_b=cands_a, start_b=case["start_a"], begin_b=case["begin_a"], width_b=width_a, tok_b=case["tok_a"])
    else:
        cands_b = [c for g in groups_b for c in g]
        case.update(cands_b=cands_b, start_b=list(starts_b), begin_b=_begin([len(g) for g in groups_b]), width_b=width_b,
                    tok_b=_table(cands_b, starts_b, width_b, ld_b, rng, prompt_term=prompt_term_b))
    return case


def _draw(rng, n, alphabet):
    return [rng.choice(alphabet) for _ in range(n)]


def _cases():
    rng = random.Random(20240611)
    out = []
    # 1. every group size and every length edge, one table against itself; a small alphabet makes the overlaps long, every row has
    #    its own start, the rows of 255 tokens fill their table to the last column (no term), the rows of 0 tokens have term at start
    sizes = [8, 0, 1, 2, 9, 17]
    lens = [0, 1, 3, 4, 63, 64, 65, 12, 5, 255, 7, 30]
    alphabet = [3, 4, 5, 6, 7, 9]
    W = 262
    groups, k = [], 0
    for n in sizes:
        g = []
        for _ in range(n):
            g.append(_draw(rng, lens[k % len(lens)], alphabet))
            k += 1
        groups.append(g)
    groups[5][3] = list(groups[5][1])                                           # identical rows inside the group of 17
    cands = [c for g in groups for c in g]
    starts = [W - MAX_LEN if len(c) > 240 else rng.randint(W - MAX_LEN, W - MAX_LEN + 9) for c in cands]
    out.append(_case("edges_self", groups, starts, W, W, rng, prompt_term_a=(0, 5, 11, 20)))
    # 2. a two-symbol alphabet at length 255 (and 254, 128): the LCS table at its largest, values up to 255 in the uint8 cells
    two = [_draw(rng, 255, [5, 9]), _draw(rng, 255, [5, 9]), _draw(rng, 254, [5, 9]), [5] * 255, _draw(rng, 128, [5, 9])]
    out.append(_case("two_symbols_255", [two], [4, 4, 5, 4, 100], 259, 259, rng))
    # 3. one full wave of 8 x 8 pairs: clipping (x x x x against x x), identical rows, disjoint alphabets, ids up to 51199; the row
    #    stride is larger than the width
    eight = [[7, 7, 7, 7], [7, 7], [7, 7, 7, 7], [10, 11, 12, 13, 14], [6, 8, 9, 15], [10, 11, 12, 13, 14], [51199, 51198, 51199], [51199],
             ]
    out.append(_case("clipping_identical_disjoint", [eight], [3, 1, 0, 2, 5, 2, 4, 6], 12, 19, rng, prompt_term_a=(0, 4)))
    # 4. candidates against references: two tables of different widths and strides, groups empty on either side, 9 x 8 pairs in one
    na, nb = [2, 0, 3, 1, 9, 2], [3, 2, 0, 1, 8, 0]
    ga = [[_draw(rng, rng.choice([0, 1, 3, 4, 9, 20]), alphabet) for _ in range(n)] for n in na]
    gb = [[_draw(rng, rng.choice([0, 2, 3, 5, 11, 33]), alphabet) for _ in range(n)] for n in nb]
    gb[4][2] = list(ga[4][2])                                                   # a reference equal to a candidate
    sa = [rng.randint(0, 6) for _ in range(sum(na))]
    sb = [rng.randint(2, 9) for _ in range(sum(nb))]
    out.append(_case("two_tables", ga, sa, 30, 37, rng, groups_b=gb, starts_b=sb, width_b=44, ld_b=44, prompt_term_a=(1, 6, 9),
                     prompt_term_b=(0, 3)))
    return out


CASES = _cases()
NAMES = [c["name"] for c in CASES]


def refused_table():
    """a table whose width - start is 256 for one row: refused on the host before any launch -> (tok, start, begin)"""
    tok = torch.full((3, 260), 5, dtype=torch.int64)
    return tok, [10, 4, 30], [0, 3]
