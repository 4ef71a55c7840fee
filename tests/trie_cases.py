"""The cases of the closed-vocabulary mask and search, shared by tests/test_trie_cpu.py and
tests/test_trie_gpu.py.

KERNEL_CASES: one launch each -- a vocabulary, a trie and a batch of rows whose histories cycle through every kind the contract
names (HISTORIES).  build(case) makes the tensors; every row of a launch works on the same column `pos`, the histories differ in
length through the rows' prompt lengths.

EXHAUSTIVE: phrase sets of P <= K phrases for the lockstep beam search on the stub decoder of oracle/gen_golden.py (StubLogits, the
clips of tests/test_beam_batched_cpu.py).  A set is the first one of a seeded search whose reference scores -- per clip the sum over
positions of the log-probability renormalised over the allowed tokens, fp64 -- differ by at least GAP between neighbours in the
ranking, so that the order is far above fp32 summation noise.  `python tests/trie_cases.py` recomputes the sets and compares them
with the committed ones."""
import random
import zlib

import torch

BAN_INF, BAN_FINITE = float("-inf"), -float.fromhex("0x1.fep127")
POISON = 1234.0                     # the sentinel of the columns behind vocab
EOS = 7
HISTORIES = ("empty", "mid", "leaf", "off", "oor", "eos_more", "forced")
TRIES = ("one", "prefix", "edges", "chunks", "all", "long", "random", "wave", "stage")

# (vocab, rows, trie, ban).  Every vocabulary meets every row count and every trie at least once; 51200 x 513 once.
KERNEL_CASES = [dict(V=V, rows=rows, trie=trie, ban=ban) for V, rows, trie, ban in [
    (8, 1, "one", "inf"), (8, 5, "prefix", "finite"), (8, 160, "all", "inf"), (8, 513, "edges", "finite"), (8, 5, "chunks", "inf"),
    (1000, 1, "prefix", "finite"), (1000, 5, "chunks", "inf"), (1000, 160, "random", "finite"), (1000, 513, "all", "inf"),
    (1000, 5, "long", "inf"), (1000, 5, "edges", "finite"), (1000, 5, "one", "inf"),
    (51200, 1, "random", "inf"), (51200, 5, "all", "finite"), (51200, 160, "chunks", "inf"), (51200, 513, "random", "finite"),
    (51200, 5, "long", "finite"), (51200, 5, "edges", "inf"), (51200, 5, "prefix", "inf"), (51200, 5, "one", "finite"),
    (1000, 160, "wave", "finite"), (51200, 160, "stage", "inf")]]


def case_id(c):
    return f"V{c['V']}-r{c['rows']}-{c['trie']}-{c['ban']}"


_PHRASES, _PREFIXES = {}, {}


def phrases_of(kind, V):
    """the phrase list of a trie kind over vocabulary V (no phrase holds EOS); made once per (kind, V)"""
    if (kind, V) in _PHRASES:
        return _PHRASES[(kind, V)]
    rng = random.Random(zlib.crc32(f"{kind}-{V}".encode()))
    free = [t for t in range(V) if t != EOS]
    if kind == "one":                                          # one phrase of one token
        ph = [[3]]
    elif kind == "prefix":                                     # a phrase that is the prefix of another: a terminal AND internal node
        ph = [[2, 5], [2, 5, 1], [2, 4], [2], [6, 6, 6]]
    elif kind == "edges":                                      # children at columns 0 and V - 1, at the root and below
        ph = [[0], [V - 1], [0, V - 1], [0, 0], [V - 1, 0, V - 1]]
    elif kind == "chunks":                                     # children that fill a chunk, straddle two, and sit alone
        base = 0 if V == 8 else 16
        fill = [t for t in range(base, base + 8) if t != EOS or V > 8]
        ph = [[t] for t in fill] + [[fill[0], t] for t in fill]
        if V > 8:
            ph += [[t] for t in (30, 31, 32, 33, 47, 48, V - 9, V - 8)] + [[30, t] for t in range(38, 42)]
        ph = [p for p in ph if EOS not in p]
    elif kind == "all":                                        # a root whose children are every token (but the termination id)
        ph = [[t] for t in free] + [[free[1], free[2]]]
    elif kind == "wave":                                       # 65 and 64 children: one narrowing round of the wave's search, and none
        ph = [[t] for t in free[:65]] + [[free[0], t] for t in free[100:164]]
    elif kind == "stage":                                      # 4096 children (staged in LDS) and 4097 (searched in global memory)
        ph = [[t] for t in free[:4096]] + [[free[0], t] for t in free[5000:9097]]
    elif kind == "long":                                       # a 255-token phrase, and a short one that leaves it half way
        long = [free[(7 * i) % len(free)] for i in range(255)]
        ph = [long, long[:100] + [free[0]]]
    else:                                                      # 10 000 random phrases of 2..6 tokens over a skewed alphabet
        ph = []
        for _ in range(10000):
            n = rng.randint(2, 6)
            ph.append([free[min(int(rng.expovariate(8.0 / len(free))), len(free) - 1)] for _ in range(n)])
    _PHRASES[(kind, V)] = ph
    _PREFIXES[(kind, V)] = {tuple(p[:i]) for p in ph for i in range(1, len(p) + 1)}
    return ph


def history(kind, phrases, V, rng, prefixes):
    """-> (the generated tokens of a row, is it teacher-forced); prefixes: every non-empty prefix of a phrase, as tuples"""
    ph = rng.choice(phrases)
    if kind == "empty":
        return [], False
    if kind == "mid":
        return ph[:rng.randint(0, len(ph) - 1)], False
    if kind == "leaf":
        return list(ph), False
    if kind == "off":                                          # a token that is in range and no child (if the root has one to spare)
        cut = rng.randint(0, len(ph) - 1)
        spare = [t for t in rng.sample(range(V), min(V, 40)) if t != EOS and tuple(ph[:cut] + [t]) not in prefixes]
        return (ph[:cut] + [rng.choice(spare)] + ph[cut:cut + 2], False) if spare else (list(ph) + [ph[0]] * 3, False)
    if kind == "oor":
        return ph[:rng.randint(0, len(ph))] + [rng.choice([-1, V, V + 5, 2 ** 40, -2 ** 40])] + ph[:1], False
    if kind == "eos_more":
        return list(ph) + [EOS] + ph[:2], False
    return list(ph), True


def build(c, seed=0):
    """-> dict(logits bf16 [rows, V + 8] (POISON behind V), tokens int64 [rows, row_len], prompt_len int64 [rows], pos, phrases, kinds)"""
    V, rows = c["V"], c["rows"]
    phrases = phrases_of(c["trie"], V)
    rng = random.Random(seed * 7919 + zlib.crc32(case_id(c).encode()))
    hists, kinds = [], []
    for r in range(rows):
        kind = HISTORIES[(r + seed) % len(HISTORIES)]
        h, forced = history(kind, phrases, V, rng, _PREFIXES[(c["trie"], V)])
        hists.append((h, forced))
        kinds.append(kind)
    pos = max(len(h) for h, _ in hists) + 2
    row_len = pos + 3
    tokens = torch.tensor([[rng.randrange(V) for _ in range(row_len)] for _ in range(rows)], dtype=torch.int64)
    prompt_len = torch.zeros(rows, dtype=torch.int64)
    for r, (h, forced) in enumerate(hists):
        if forced:
            prompt_len[r] = pos + 1 + (r % 2)
            continue
        prompt_len[r] = pos - len(h)
        if h:
            tokens[r, pos - len(h):pos] = torch.tensor(h, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed + 17)
    logits = torch.full((rows, V + 8), POISON, dtype=torch.bfloat16)
    logits[:, :V] = (torch.randn(rows, V, generator=g) * 3.0).to(torch.bfloat16)
    logits[:, 1:V:13] = float("-inf")                          # some columns are -inf already; allowed ones must stay so
    return dict(logits=logits, tokens=tokens, prompt_len=prompt_len, pos=pos, phrases=phrases, kinds=kinds, vocab=V,
                ban=BAN_INF if c["ban"] == "inf" else BAN_FINITE)


# ------------------------------------------------------------------------------ the exhaustive search cases
GAP = 1e-2
STUB_VOCAB, STUB_PAD, STUB_SEEDS, PROMPT = 37, 40, (1, 2), [5, 11, 3]
# K beams, P phrases; `phrases` is what find_set(K, P, first_seed) returns
EXHAUSTIVE = [
    dict(K=4, P=4, first_seed=0, phrases=[[25], [25, 27], [17, 2], [2, 33]]),
    dict(K=4, P=3, first_seed=100, phrases=[[10], [10, 30], [23, 10]]),
    dict(K=8, P=8, first_seed=200, phrases=[[2], [2, 14], [10], [14, 2, 10], [10, 10], [14], [2, 1, 10], [2, 10]]),
    dict(K=4, P=2, first_seed=300, phrases=[[23], [23, 0]]),              # fewer phrases than beams: the store sees non-phrases
]


def candidate_set(seed, P):
    """P distinct phrases of 1..3 tokens over a small alphabet, so that prefixes are shared; the first is a prefix of the second"""
    rng = random.Random(seed)
    alphabet = rng.sample([t for t in range(STUB_VOCAB) if t != EOS], 5)
    out = [[alphabet[0]], [alphabet[0], alphabet[1]]]
    while len(out) < P:
        ph = [rng.choice(alphabet) for _ in range(rng.randint(1, 3))]
        if ph not in out:
            out.append(ph)
    return out[:P]


def reference_scores(phrases, stub_seed):
    """per phrase the fp64 sum over its positions, the termination id included, of the log-probability renormalised over the allowed
    tokens, from a teacher-forced pass of the stub decoder"""
    import ref_trie
    from oracle.gen_golden import StubLogits
    stub, root = StubLogits(vocab=STUB_VOCAB, stop=EOS, seed=stub_seed), ref_trie.build(phrases)
    out = []
    for ph in phrases:
        total = 0.0
        for i, tok in enumerate(list(ph) + [EOS]):
            ok, _ = ref_trie.allowed_tokens(root, ph[:i], [EOS], STUB_VOCAB)
            lg = stub.row(PROMPT + list(ph[:i])).double()
            total += float(lg[tok] - torch.logsumexp(lg[ok], dim=0))
        out.append(total)
    return out


def find_set(K, P, first_seed):
    for seed in range(first_seed, first_seed + 100):
        phrases = candidate_set(seed, P)
        ok = True
        for s in STUB_SEEDS:
            sc = sorted(reference_scores(phrases, s), reverse=True)
            ok = ok and all(a - b >= GAP for a, b in zip(sc, sc[1:]))
        if ok:
            return phrases
    raise RuntimeError(f"no phrase set found from seed {first_seed}")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for e in EXHAUSTIVE:
        got = find_set(e["K"], e["P"], e["first_seed"])
        print(f"K={e['K']} P={e['P']} first_seed={e['first_seed']}: {got}" + ("" if got == e["phrases"] else "   <-- differs from the committed set"))
        for s in STUB_SEEDS:
            print("    clip", s, [round(x, 4) for x in reference_scores(got, s)])
