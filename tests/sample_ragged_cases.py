"""The launches the ragged sampling entries (mpv_sample_advance_ragged, mpv_logits_constrain_ragged, mpv_sample_score_ragged) are
checked on in tests/test_sample_ragged_gpu.py.  The inputs are those of tests/sampling_cases.py, constrain_cases.py and
sample_score_cases.py, laid out on a LEFT-ALIGNED table: row r has its own prompt length, and the launch one generation step t.

Sampler: 8 rows of ROW_LEN = 8 columns with PROMPT_LEN = [0, 1, 3, 5, 6, 7, 8, 2] at STEP = 2: columns 2, 3, 5, 7, three frozen rows
(the column lies behind the table) and 4.  Row r draws with u = standin_sampling.uniform(seed, c_r, r).  As in sampling_cases, row r is
the first candidate make_row(V, seed * 100003 + i, variant) that is not in the case's committed `skip` and, on a started row, the fp64
reference is unambiguous for it (sampling_cases.candidate_ok: DELTA = 1e-4 of the kept mass, derived there); nothing is decided at run
time, tests/test_sample_ragged_gpu.py checks the condition on every started row, and `python tests/sample_ragged_cases.py` recomputes
the skip sets from PLAN."""
import torch

import constrain_cases as cc
import sample_score_cases as qc
import sampling_cases as sc

ROW_LEN = 8
PROMPT_LEN = [0, 1, 3, 5, 6, 7, 8, 2]
STEP = 2
ROWS = len(PROMPT_LEN)


def column(pl, row_len, step):
    """c_r of a row, or None when the row is frozen"""
    c = min(max(int(pl), 0), row_len) + step
    return c if c < row_len else None


COLUMNS = [column(pl, ROW_LEN, STEP) for pl in PROMPT_LEN]          # [2, 3, 5, 7, None, None, None, 4]

# (V, ld, seed, T, filter): vocab 8, 520 and 51200; plain, greedy, top-k and top-p; ld = V and V + 64
PLAN = [(V, V + (64 if i % 2 else 0), 200 + 10 * j + i, T, filt)
        for j, V in enumerate((8, 520, 51200))
        for i, (T, filt) in enumerate(((1.0, ("plain",)), (0.7, ("greedy",)), (1.0, ("top_k", 2 if V == 8 else 50)), (1.3, ("top_p", 0.9))))]


def sampler_rows(case):
    """-> logits bf16 [ROWS, ld] (columns >= V hold sampling_cases.POISON)"""
    V, ld, seed, T, filt, skip = case
    out = torch.full((ROWS, ld), sc.POISON, dtype=torch.bfloat16)
    i = 0
    for r in range(ROWS):
        while i in skip:
            i += 1
        out[r, :V] = sc.make_row(V, seed * 100003 + i, sc.variant_of(V, seed, i))
        i += 1
    return out


def discover(plan):
    import standin_sampling
    cases = []
    for V, ld, seed, T, filt in plan:
        skip, i = [], 0
        for r in range(ROWS):
            while True:
                row = sc.make_row(V, seed * 100003 + i, sc.variant_of(V, seed, i))
                i += 1
                if COLUMNS[r] is None or sc.candidate_ok(row, T, filt, standin_sampling.uniform(seed, COLUMNS[r], r))[0]:
                    break
                skip.append(i - 1)
                assert i < 64, ("too few candidates pass", V, seed, T, filt)
        cases.append((V, ld, seed, T, filt, tuple(skip)))
    return cases


SAMPLER_CASES = [
    (8, 8, 200, 1.0, ('plain',), ()),
    (8, 72, 201, 0.7, ('greedy',), ()),
    (8, 8, 202, 1.0, ('top_k', 2), ()),
    (8, 72, 203, 1.3, ('top_p', 0.9), ()),
    (520, 520, 210, 1.0, ('plain',), ()),
    (520, 584, 211, 0.7, ('greedy',), ()),
    (520, 520, 212, 1.0, ('top_k', 50), ()),
    (520, 584, 213, 1.3, ('top_p', 0.9), ()),
    (51200, 51200, 220, 1.0, ('plain',), ()),
    (51200, 51264, 221, 0.7, ('greedy',), ()),
    (51200, 51200, 222, 1.0, ('top_k', 50), ()),
    (51200, 51264, 223, 1.3, ('top_p', 0.9), ()),
]


def sampler_id(c):
    return f"V{c[0]}-ld{c[1]}-seed{c[2]}-T{c[3]}-{'_'.join(str(x) for x in c[4])}"


# ---------------------------------------------------------------------------------------------- the constraint launches
NGRAM = 3
HIST = (0, 1, NGRAM - 1, NGRAM, 65, 257)              # the history lengths: none, one, below / at the n-gram size, past a wave, past 256
C_ROW_LEN = 300
EOS = cc.EOS


def constrain_build(V, step, include_prompt, seed, kind="few"):
    """-> (logits bf16 [rows, V + 8], tokens int64 [rows, C_ROW_LEN], prompt_len int64 [rows], frozen rows, LogitsConstraints keywords).
    include_prompt = 1: row i (i < 6) has the history tokens[0 : HIST[i]] (prompt_len = HIST[i] - step where that is not negative, else
    the row is dropped).  include_prompt = 0: every row's history is its `step` generated tokens, at prompt lengths 0, 1, 7, 40 and
    C_ROW_LEN - step - 1 (the last column of the table).  Then three frozen rows: the first column behind the table, a prompt as long as
    the table, 10**6; and one row with prompt_len = -3, which acts as 0."""
    if include_prompt:
        pls = [m - step for m in HIST if m - step >= 0]
    else:
        pls = [0, 1, 7, 40, C_ROW_LEN - step - 1]
    pls = pls + [C_ROW_LEN - step, C_ROW_LEN, 10 ** 6, -3]
    rows = len(pls)
    frozen = [r for r, pl in enumerate(pls) if column(pl, C_ROW_LEN, step) is None]
    g = torch.Generator().manual_seed(seed)
    logits = torch.full((rows, V + 8), sc.POISON, dtype=torch.bfloat16)
    tokens = torch.randint(0, V, (rows, C_ROW_LEN), generator=g)
    banned = [v for v in torch.randperm(V, generator=g)[:4].tolist() if v != EOS][:3]
    c = dict(V=V, kind=kind)
    for r, pl in enumerate(pls):
        logits[r, :V] = sc.make_row(V, seed * 100003 + r, sc.variant_of(V, seed, r))
        logits[r, banned[0]] = 2.5
        logits[r, EOS] = 1.5                                                 # finite and positive: an eos ban shows
        col = column(pl, C_ROW_LEN, step)
        if col is not None:
            start = 0 if include_prompt else max(pl, 0)
            tokens[r, start:col] = cc._history(c, r, col - start, g)
    ckw = dict(repetition_penalty=1.3, no_repeat_ngram_size=NGRAM, min_new_tokens=2, banned_token_ids=tuple(banned), include_prompt=bool(include_prompt))
    return logits, tokens, torch.tensor(pls, dtype=torch.int64), frozen, ckw


# (V, step, include_prompt, seed, history kind)
CONSTRAIN_CASES = ([(V, 0, 1, 300 + i, "few") for i, V in enumerate((64, 51200))] + [(64, 1, 1, 302, "overlap"), (51200, 2, 1, 303, "wide")] +
                   [(V, t, 0, 310 + 10 * i + j, "few" if V == 64 else "wide") for i, V in enumerate((64, 51200)) for j, t in enumerate(HIST)])


# ---------------------------------------------------------------------------------------------- the score launches
S_STEP = 2
# sample_score_cases' inputs, roles and variants at three vocabularies and two row widths, eight rows each
SCORE_CASES = [qc._case(V, ldx, 8, row_len, 0, seed) for V, ldx, row_len, seed in
               ((8, 8, 37, 400), (520, 0, 37, 401), (51200, 8, 37, 402), (520, 8, 2048, 403), (64, 0, 3, 404))]


def score_build(c):
    """sample_score_cases.build(c) re-laid: row r's scored token moves to its own column c_r = prompt_len[r] + S_STEP.  The role
    "forced" has no meaning without teacher forcing: those rows are FROZEN here (prompt lengths row_len - S_STEP, row_len and 10**6 in
    turn); "dead" rows keep live = 0; one live row gets prompt_len = -3 (acts as 0).  -> (the built namespace, columns)"""
    b = qc.build(c)
    rows, row_len = b.tokens.shape
    cols, n_frozen = [], 0
    for r in range(rows):
        t = int(b.tokens[r, c["pos"]])
        if qc.role_of(c, r) == "forced":
            b.prompt_len[r] = (row_len - S_STEP, row_len, 10 ** 6)[n_frozen % 3]
            n_frozen += 1
        else:
            b.prompt_len[r] = (5 * r) % (row_len - S_STEP)
        if r == rows - 1 and qc.role_of(c, r) != "forced":
            b.prompt_len[r] = -3
        col = column(int(b.prompt_len[r]), row_len, S_STEP)
        cols.append(col)
        if col is not None:
            b.tokens[r, col] = t
    return b, cols


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    print("SAMPLER_CASES = [")
    for case in discover(PLAN):
        print(f"    {case!r},")
    print("]")
