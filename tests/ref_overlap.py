"""The reference of the caption-overlap tests, TEST INFRASTRUCTURE ONLY: what include/mpv.h (mpv_caption_overlap) and
generation.consensus_utility / consensus_choice define, written from the definitions with the standard library alone -- the textbook
two-dimensional LCS table, collections.Counter for the clipped n-gram matches, fractions.Fraction for the utilities and the expected
utility (b^2 = 36 / 25).  It shares no code with the product, nor with tests/standin_overlap.py."""
from collections import Counter
from fractions import Fraction

BETA2 = Fraction(36, 25)
ORDERS = (1, 2, 3, 4)


def candidate(row, start, term, width):
    """the tokens of `row` from column start up to the first `term` at or behind it, or to the width"""
    out = []
    for t in list(row)[start:width]:
        if t == term:
            break
        out.append(t)
    return out


def lcs(a, b):
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            table[i][j] = table[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(table[i - 1][j], table[i][j - 1])
    return table[len(a)][len(b)]


def clipped(a, b, n):
    ca = Counter(tuple(a[i:i + n]) for i in range(len(a) - n + 1))
    cb = Counter(tuple(b[i:i + n]) for i in range(len(b) - n + 1))
    return sum(min(c, cb[g]) for g, c in ca.items())


def pair_counts(a, b):
    return [lcs(a, b)] + [clipped(a, b, n) for n in ORDERS]


def table_counts(rows_a, start_a, begin_a, width_a, rows_b, start_b, begin_b, width_b, term):
    """-> (len_a, len_b, counts): counts holds group after group its nA x nB pairs row-major, five integers each"""
    ca = [candidate(r, s, term, width_a) for r, s in zip(rows_a, start_a)]
    cb = [candidate(r, s, term, width_b) for r, s in zip(rows_b, start_b)]
    memo, counts = {}, []
    for g in range(len(begin_a) - 1):
        for i in range(begin_a[g], begin_a[g + 1]):
            for j in range(begin_b[g], begin_b[g + 1]):
                key = (tuple(ca[i]), tuple(cb[j]))
                if key not in memo:
                    memo[key] = pair_counts(ca[i], cb[j])
                counts.append(memo[key])
    return [len(c) for c in ca], [len(c) for c in cb], counts


_cache = {}


def case_counts(case):
    """table_counts of a case of tests/overlap_cases.py, computed once per process and never changed"""
    if case["name"] not in _cache:
        _cache[case["name"]] = table_counts(case["tok_a"].tolist(), case["start_a"], case["begin_a"], case["width_a"], case["tok_b"].tolist(),
                                            case["start_b"], case["begin_b"], case["width_b"], case["term"])
    return _cache[case["name"]]


def utility(c, len_h, len_r, metric):
    """one pair's utility as an exact fraction: c = [lcs, m1, m2, m3, m4]"""
    if len_h == 0 and len_r == 0:
        return Fraction(1)
    if len_h == 0 or len_r == 0:
        return Fraction(0)
    if metric == "rouge_l":
        if c[0] == 0:
            return Fraction(0)
        p, r = Fraction(c[0], len_h), Fraction(c[0], len_r)
        return (1 + BETA2) * p * r / (r + BETA2 * p)
    assert metric == "ngram_f"
    terms = []
    for n in ORDERS:
        g = max(len_h - n + 1, 0) + max(len_r - n + 1, 0)
        if g > 0:
            terms.append(Fraction(2 * c[n], g))
    return sum(terms) / len(terms)


def group_utilities(counts, len_h, len_r, metric):
    """counts: nA * nB rows, row-major -> u[h][r] fractions"""
    nB = len(len_r)
    return [[utility(counts[h * nB + r], len_h[h], len_r[r], metric) for r in range(nB)] for h in range(len(len_h))]


def choice(u, weights=None):
    """-> (U fractions, argmax with ties to the lowest index; None without rows)"""
    if not u:
        return [], None
    w = [Fraction(1)] * len(u[0]) if weights is None else [Fraction(x) for x in weights]
    U = [sum(wr * x for wr, x in zip(w, row)) / sum(w) if w else Fraction(0) for row in u]
    best = 0
    for h in range(1, len(U)):
        if U[h] > U[best]:
            best = h
    return U, best


def clear_choice(U):
    """True when the best two U are exactly tied or more than 1e-9 apart: rounding cannot decide the choice"""
    top = sorted(U, reverse=True)[:2]
    return len(top) < 2 or top[0] == top[1] or top[0] - top[1] > Fraction(1, 10 ** 9)


def case_groups(case):
    """-> per group (counts rows, len_h, len_r) of a case"""
    la, lb, counts = case_counts(case)
    out, at = [], 0
    for g in range(len(case["begin_a"]) - 1):
        a0, a1, b0, b1 = case["begin_a"][g], case["begin_a"][g + 1], case["begin_b"][g], case["begin_b"][g + 1]
        n = (a1 - a0) * (b1 - b0)
        out.append((counts[at:at + n], la[a0:a1], lb[b0:b1]))
        at += n
    return out
