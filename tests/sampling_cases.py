"""The rows the fused sampler (mpv_sample_advance) is checked on, shared by tests/test_sampling_cpu.py and tests/test_sampling_gpu.py.

A case is (V, rows, ld, seed, T, filter, skip): `rows` rows of bf16 logits [rows, ld] (columns >= V are poison: +60, far above every
logit, so a kernel that read them would draw them), temperature T, filter one of ("plain",), ("greedy",), ("top_k", k), ("top_p", p).
Row r of the launch draws with u = standin_sampling.uniform(seed, POS, r).

Rows come from the candidate sequence i = 0, 1, 2, ... of the case: candidate i is make_row(V, seed * 100003 + i, variant) with the
variant cycling with seed + i (VARIANTS / VARIANTS_LARGE).  A candidate is LISTED only if the fp64 reference is unambiguous for it
(separation condition, everything as a fraction of the kept mass): no cumulative c_{j-1} of the top-p walk within DELTA of top_p, and
u * mass at least DELTA inside the selected token's CDF interval.  Candidates that fail are not listed: `skip` names them, and the
case's rows are the first `rows` candidates that are not in `skip`.  Nothing is decided at run time; test_sampling_cpu.py checks that
every listed row satisfies the condition.  `python tests/sampling_cases.py` recomputes the skip sets from PLAN (discover()).

Why DELTA = 1e-4: an entry that matters has |z - max| <= ~30, so its fp32 probability carries at most 30 * 2^-23 ~ 4e-6 relative error
plus a few ulp of exp; sums of positive terms keep that bound and add at most log2(65536) * 2^-24 ~ 1e-6.  Any partial sum over the mass
is therefore within about 1e-5 of the fp64 value, ten times inside DELTA: a disagreement on a listed row is a bug, not noise."""
import math

import torch

DELTA = 1e-4
POS = 5            # the token column the kernel tests fill (it keys the uniform)
ROW_LEN = 8
POISON = 60.0
VARIANTS = ("normal", "half_neg_inf", "all_equal", "normal", "one_hot", "cutoff_ties", "normal", "all_neg_inf")
VARIANTS_LARGE = ("normal", "half_neg_inf", "normal", "one_hot", "cutoff_ties", "normal", "normal", "all_neg_inf")      # V > 1000


def make_row(V, row_seed, variant):
    """-> bf16 [V]: a tail 2 * randn - 20 plus min(40, V // 2) hot entries uniform in [-6, 0] at random positions, rounded to bf16"""
    g = torch.Generator().manual_seed(row_seed)
    row = 2.0 * torch.randn(V, generator=g) - 20.0
    n_hot = min(40, V // 2)
    hot = torch.randperm(V, generator=g)[:n_hot]
    row[hot] = -6.0 * torch.rand(n_hot, generator=g)
    if variant == "all_equal":                       # ties decide everything
        row[:] = -3.5
    elif variant == "half_neg_inf":
        row[torch.randperm(V, generator=g)[:V // 2]] = float("-inf")
    elif variant == "all_neg_inf":
        row[:] = float("-inf")
    elif variant == "one_hot":                       # a nucleus of one
        row[hot[0]] = 12.0
    elif variant == "cutoff_ties":                   # at least four entries share the key the top-p walk / the k-th value stops at
        n_tie = max(4, (3 * n_hot) // 10)
        row[hot] = -3.0 - 3.0 * torch.rand(n_hot, generator=g)
        row[hot[:n_tie]] = -0.5
    else:
        assert variant == "normal", variant
    return row.to(torch.bfloat16)


def variant_of(V, seed, i):
    table = VARIANTS_LARGE if V > 1000 else VARIANTS
    return table[(seed + i) % len(table)]


def filter_args(filt):
    """-> (top_k, top_p) of a case's filter"""
    return {"plain": (0, 0.0), "greedy": (1, 0.0)}.get(filt[0]) or ((int(filt[1]), 0.0) if filt[0] == "top_k" else (0, float(filt[1])))


def candidate_ok(row, T, filt, u):
    import standin_sampling
    top_k, top_p = filter_args(filt)
    r = standin_sampling.sample_row(row.float(), T, top_k, top_p, u)
    return r["margin_p"] >= DELTA and r["margin_u"] >= DELTA, r


def case_rows(case):
    """-> (logits bf16 [rows, ld], candidate index of every row)"""
    V, rows, ld, seed, T, filt, skip = case
    out = torch.full((rows, ld), POISON, dtype=torch.bfloat16)
    taken, i = [], 0
    while len(taken) < rows:
        if i not in skip:
            out[len(taken), :V] = make_row(V, seed * 100003 + i, variant_of(V, seed, i))
            taken.append(i)
        i += 1
    return out, taken


def discover(plan):
    """PLAN entry (V, rows, ld, seed, T, filter) -> case with its skip set: the candidates, in order, that fail the separation condition
    at the launch position they would take"""
    import standin_sampling
    cases = []
    for V, rows, ld, seed, T, filt in plan:
        skip, n, i = [], 0, 0
        while n < rows:
            row = make_row(V, seed * 100003 + i, variant_of(V, seed, i))
            ok, _ = candidate_ok(row, T, filt, standin_sampling.uniform(seed, POS, n))
            if ok:
                n += 1
            else:
                skip.append(i)
            i += 1
            assert i < 4 * rows + 64, ("too few candidates pass", V, rows, seed, T, filt)
        cases.append((V, rows, ld, seed, T, filt, tuple(skip)))
    return cases


# V in {8, 64, 8000, 51200, 65536}; rows in {1, 3, 160}; ld = V and V + 64; T in {0.7, 1.0, 1.5}; plain / top-k in {2, 50, V} /
# top-p in {0.5, 0.9, 1.0} / greedy.  The 160-row launches are few (each is 160 reference rows on the CPU).
PLAN = [
    (8, 1, 8, 1, 1.0, ("plain",)), (8, 3, 72, 2, 0.7, ("top_p", 0.5)), (8, 160, 8, 3, 1.5, ("top_p", 0.9)), (8, 3, 8, 4, 1.0, ("top_k", 2)),
    (8, 3, 72, 5, 1.0, ("top_k", 8)), (8, 3, 8, 6, 0.7, ("greedy",)), (8, 3, 8, 7, 1.0, ("top_p", 1.0)),
    (64, 1, 64, 8, 0.7, ("top_p", 0.9)), (64, 3, 128, 9, 1.0, ("top_p", 0.5)), (64, 160, 128, 10, 1.0, ("top_p", 0.9)), (64, 3, 64, 11, 1.5, ("plain",)),
    (64, 3, 64, 12, 1.0, ("top_k", 2)), (64, 3, 128, 13, 0.7, ("top_k", 50)), (64, 3, 64, 14, 1.5, ("top_k", 64)), (64, 3, 64, 15, 1.0, ("greedy",)),
    (64, 8, 64, 16, 1.0, ("top_p", 1.0)), (64, 8, 64, 17, 1.3, ("plain",)),
    (8000, 1, 8000, 18, 1.0, ("top_p", 0.9)), (8000, 3, 8064, 19, 0.7, ("top_p", 0.5)), (8000, 3, 8000, 20, 1.5, ("plain",)),
    (8000, 3, 8064, 21, 1.0, ("top_k", 50)), (8000, 3, 8000, 22, 1.0, ("top_k", 2)), (8000, 8, 8000, 23, 1.5, ("top_p", 0.9)),
    (8000, 3, 8000, 24, 0.7, ("greedy",)), (8000, 1, 8000, 25, 1.0, ("top_k", 8000)),
    (51200, 1, 51200, 26, 1.0, ("top_p", 0.9)), (51200, 3, 51264, 27, 0.7, ("top_p", 0.9)), (51200, 160, 51200, 28, 1.0, ("top_p", 0.9)),
    (51200, 3, 51200, 29, 1.5, ("top_p", 0.5)), (51200, 3, 51264, 30, 1.3, ("plain",)), (51200, 160, 51264, 31, 1.0, ("top_k", 50)),
    (51200, 3, 51200, 32, 1.0, ("top_k", 2)), (51200, 1, 51200, 33, 0.7, ("top_k", 51200)), (51200, 3, 51200, 34, 1.0, ("greedy",)),
    (51200, 8, 51200, 35, 1.0, ("top_p", 1.0)), (51200, 8, 51200, 36, 1.5, ("top_p", 0.9)),
    (65536, 1, 65536, 37, 1.0, ("top_p", 0.9)), (65536, 3, 65600, 38, 0.7, ("top_p", 0.5)), (65536, 160, 65536, 39, 1.3, ("plain",)),
    (65536, 3, 65536, 40, 1.0, ("top_k", 50)), (65536, 3, 65600, 41, 1.5, ("top_k", 2)), (65536, 1, 65536, 42, 1.0, ("top_k", 65536)),
    (65536, 3, 65536, 43, 0.7, ("greedy",)), (65536, 8, 65536, 44, 1.0, ("top_p", 0.9)), (65536, 8, 65600, 45, 1.5, ("top_p", 1.0)),
]

CASES = [
    (8, 1, 8, 1, 1.0, ('plain',), ()),
    (8, 3, 72, 2, 0.7, ('top_p', 0.5), (0, 3)),
    (8, 160, 8, 3, 1.5, ('top_p', 0.9), ()),
    (8, 3, 8, 4, 1.0, ('top_k', 2), ()),
    (8, 3, 72, 5, 1.0, ('top_k', 8), ()),
    (8, 3, 8, 6, 0.7, ('greedy',), ()),
    (8, 3, 8, 7, 1.0, ('top_p', 1.0), ()),
    (64, 1, 64, 8, 0.7, ('top_p', 0.9), ()),
    (64, 3, 128, 9, 1.0, ('top_p', 0.5), (1,)),
    (64, 160, 128, 10, 1.0, ('top_p', 0.9), ()),
    (64, 3, 64, 11, 1.5, ('plain',), ()),
    (64, 3, 64, 12, 1.0, ('top_k', 2), ()),
    (64, 3, 128, 13, 0.7, ('top_k', 50), ()),
    (64, 3, 64, 14, 1.5, ('top_k', 64), ()),
    (64, 3, 64, 15, 1.0, ('greedy',), ()),
    (64, 8, 64, 16, 1.0, ('top_p', 1.0), ()),
    (64, 8, 64, 17, 1.3, ('plain',), ()),
    (8000, 1, 8000, 18, 1.0, ('top_p', 0.9), ()),
    (8000, 3, 8064, 19, 0.7, ('top_p', 0.5), ()),
    (8000, 3, 8000, 20, 1.5, ('plain',), ()),
    (8000, 3, 8064, 21, 1.0, ('top_k', 50), (1,)),
    (8000, 3, 8000, 22, 1.0, ('top_k', 2), ()),
    (8000, 8, 8000, 23, 1.5, ('top_p', 0.9), ()),
    (8000, 3, 8000, 24, 0.7, ('greedy',), ()),
    (8000, 1, 8000, 25, 1.0, ('top_k', 8000), ()),
    (51200, 1, 51200, 26, 1.0, ('top_p', 0.9), ()),
    (51200, 3, 51264, 27, 0.7, ('top_p', 0.9), ()),
    (51200, 160, 51200, 28, 1.0, ('top_p', 0.9), (2, 26, 65, 134)),
    (51200, 3, 51200, 29, 1.5, ('top_p', 0.5), ()),
    (51200, 3, 51264, 30, 1.3, ('plain',), ()),
    (51200, 160, 51264, 31, 1.0, ('top_k', 50), (97,)),
    (51200, 3, 51200, 32, 1.0, ('top_k', 2), ()),
    (51200, 1, 51200, 33, 0.7, ('top_k', 51200), ()),
    (51200, 3, 51200, 34, 1.0, ('greedy',), ()),
    (51200, 8, 51200, 35, 1.0, ('top_p', 1.0), ()),
    (51200, 8, 51200, 36, 1.5, ('top_p', 0.9), ()),
    (65536, 1, 65536, 37, 1.0, ('top_p', 0.9), ()),
    (65536, 3, 65600, 38, 0.7, ('top_p', 0.5), ()),
    (65536, 160, 65536, 39, 1.3, ('plain',), (42,)),
    (65536, 3, 65536, 40, 1.0, ('top_k', 50), ()),
    (65536, 3, 65600, 41, 1.5, ('top_k', 2), ()),
    (65536, 1, 65536, 42, 1.0, ('top_k', 65536), ()),
    (65536, 3, 65536, 43, 0.7, ('greedy',), ()),
    (65536, 8, 65536, 44, 1.0, ('top_p', 0.9), ()),
    (65536, 8, 65600, 45, 1.5, ('top_p', 1.0), ()),
]


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    print("CASES = [")
    for c in discover(PLAN):
        print(f"    {c!r},")
    print("]")
