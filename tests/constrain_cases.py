"""The launches mpv_logits_constrain is checked on (tests/test_logits_constrain_gpu.py; tests/test_logits_constrain_cpu.py checks
that the list covers what it claims).  Everything is exact -- one fp32 multiply or IEEE divide and one bf16 rounding per edited logit --
so every comparison is bitwise on the whole [rows, ld] matrix and nothing has to be left out.

A case is a dict: V, rows, m (history length), kind (how the histories are drawn), penalty, ngram, min_new, n_banned, include_prompt,
ban ("inf": -inf, the sampling value; "finite": the lowest finite bf16, the beam value), seed, and optionally row_len / pos (default:
pos = PROMPT + m, or m with include_prompt; row_len = pos + 2), mixed (odd rows are still inside their prompt: prompt_len = pos + 1) and
scalar_prompt (prompt_len = None, prompt_len_all instead).  ld = V + 8: the extra columns hold sampling_cases.POISON.  Logit row r is
sampling_cases.make_row(V, seed * 100003 + r, variant) with the variant cycling as there (the -inf variants included); the first banned
id gets a POSITIVE logit in every row.

History kinds ("few" is the default; all of them depend on (seed, row) only):
  few      at most 5 distinct in-range tokens: repeats and n-gram matches are frequent
  same     one token throughout
  overlap  a b a b a b ...: overlapping n-gram matches
  pair     even tokens only: v ^ 1 is never in the history, so a 4-byte store of the pair would show in the neighbour
  oor      "few" with -1, V and 2**40 mixed in
  eos      "few" whose first distinct token is the eos id
  wide     uniform over the vocabulary"""
import torch

import sampling_cases as sc

PROMPT = 3
EOS = 5
BAN_INF, BAN_FINITE = float("-inf"), -float.fromhex("0x1.fep127")


def _case(V, rows, m, kind="few", penalty=1.3, ngram=2, min_new=0, n_banned=0, include_prompt=False, ban="inf", seed=0, **extra):
    return dict(V=V, rows=rows, m=m, kind=kind, penalty=penalty, ngram=ngram, min_new=min_new, n_banned=n_banned, include_prompt=include_prompt,
                ban=ban, seed=seed, **extra)


ALL = dict(penalty=1.3, ngram=2, min_new=10 ** 6, n_banned=3)               # every constraint on
HIST = (0, 1, 2, 63, 64, 65, 255, 256, 257)

CASES = (
    # every history length around the wave and workgroup sizes, all constraints together, both ban values, rows in {1, 3}
    [_case(64, 3 if i % 2 else 1, m, ban="finite" if i % 2 else "inf", seed=10 + i, **ALL) for i, m in enumerate(HIST)] +
    # each constraint alone
    [_case(64, 3, 65, penalty=1.3, ngram=0, seed=30), _case(64, 3, 65, penalty=0.8, ngram=0, seed=31), _case(64, 3, 65, penalty=2.0, ngram=0, seed=32),
     _case(64, 3, 65, penalty=1.0, ngram=0, min_new=10 ** 6, seed=33), _case(64, 3, 65, penalty=1.0, ngram=0, n_banned=3, seed=34),
     _case(64, 3, 65, penalty=1.0, ngram=0, min_new=2, seed=35)] +          # g = 65 >= min_new: the eos ban is over, nothing is launched
    # n-gram sizes, with m below, at and above n - 1 (m < n: nothing is banned)
    [_case(64, 3, m, penalty=1.0, ngram=n, seed=40 + 10 * n + m) for n in (1, 2, 3, 4, 8) for m in sorted({0, 1, n - 1, n, n + 1, 65} - {-1})] +
    # the special histories
    [_case(64, 3, 65, kind="same", seed=110, **ALL), _case(64, 3, 64, kind="overlap", ngram=3, seed=111), _case(64, 3, 65, kind="overlap", ngram=2, seed=112),
     _case(64, 3, 65, kind="pair", ngram=1, seed=113), _case(64, 3, 65, kind="pair", ngram=0, seed=114), _case(64, 3, 65, kind="oor", ngram=2, seed=115),
     _case(64, 3, 65, kind="oor", ngram=1, seed=116), _case(64, 3, 65, kind="eos", ngram=0, min_new=10 ** 6, seed=117),
     _case(64, 3, 65, kind="eos", ngram=2, min_new=10 ** 6, ban="finite", seed=118), _case(8, 3, 65, kind="wide", seed=119, **ALL)] +
    # pos = 0 (no history at all), with the prompt included and not; a launch that mixes teacher-forced and started rows; one scalar prompt length
    [_case(64, 3, 0, pos=0, row_len=4, include_prompt=True, seed=120, **ALL), _case(64, 3, 0, pos=0, row_len=1, scalar_prompt=True, seed=121, **ALL),
     _case(64, 4, 65, mixed=True, seed=122, **ALL), _case(64, 3, 64, scalar_prompt=True, ban="finite", seed=123, **ALL),
     _case(64, 3, 62, include_prompt=True, seed=124, **ALL)] +
    # the vocabularies; many rows; the longest table
    [_case(8, 1, 2, seed=130, **ALL), _case(8, 160, 63, seed=131, **ALL), _case(51200, 3, 257, kind="wide", seed=132, **ALL),
     _case(51200, 160, 65, seed=133, **ALL), _case(65536, 3, 256, kind="wide", ban="finite", seed=134, **ALL), _case(65536, 1, 64, kind="pair", ngram=1, seed=135),
     _case(64, 160, 257, seed=136, **ALL), _case(64, 3, 2047 - PROMPT, pos=2047, row_len=2048, seed=137, **ALL),
     _case(51200, 1, 2047, pos=2047, row_len=2048, include_prompt=True, kind="wide", ngram=3, seed=138)]
)


def case_id(c):
    return "-".join(f"{k}{c[k]}" for k in ("V", "rows", "m", "kind", "penalty", "ngram", "min_new", "n_banned", "ban", "seed"))


def _history(c, r, m, g):
    V, kind = c["V"], c["kind"]
    few = torch.randperm(V, generator=g)[:min(5, V)]
    if kind == "eos":
        few[0] = EOS
    if kind == "same":
        return few[:1].repeat(m)
    if kind == "overlap":
        return few[:2].repeat((m + 1) // 2)[:m]
    if kind == "pair":
        return (torch.randint(0, V // 2, (m,), generator=g) * 2).to(torch.int64)
    if kind == "wide":
        return torch.randint(0, V, (m,), generator=g)
    h = few[torch.randint(0, few.numel(), (m,), generator=g)]
    if kind == "oor" and m:
        odd = torch.tensor([-1, V, 2 ** 40])[torch.randint(0, 3, (m,), generator=g)]
        h = torch.where(torch.rand(m, generator=g) < 0.3, odd, h)
    return h


def build(c):
    """-> (logits bf16 [rows, V + 8], tokens int64 [rows, row_len], keywords of ops.logits_constrain without `constraints`, the keywords
    of generation.LogitsConstraints)"""
    V, rows, m, seed = c["V"], c["rows"], c["m"], c["seed"]
    pos = c.get("pos", m if c["include_prompt"] else PROMPT + m)
    prompt = 0 if pos == 0 else pos - m if not c["include_prompt"] else min(PROMPT, pos)
    row_len = c.get("row_len", pos + 2)
    logits = torch.full((rows, V + 8), sc.POISON, dtype=torch.bfloat16)
    tokens = torch.zeros((rows, row_len), dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    banned = torch.randperm(V, generator=g)[:c["n_banned"]].tolist()
    for r in range(rows):
        logits[r, :V] = sc.make_row(V, seed * 100003 + r, sc.variant_of(V, seed, r))
        if banned:
            logits[r, banned[0]] = 2.5
        tokens[r] = torch.randint(0, V, (row_len,), generator=g)             # the prompt and the columns from pos on: never read
        start = 0 if c["include_prompt"] else prompt
        tokens[r, start:pos] = _history(c, r, pos - start, g)
    prompt_len = torch.full((rows,), prompt, dtype=torch.int64)
    if c.get("mixed"):
        prompt_len[1::2] = pos + 1
    kw = dict(pos=pos, eos_ids=[EOS], ban_value=BAN_FINITE if c["ban"] == "finite" else BAN_INF)
    if c.get("scalar_prompt"):
        kw["prompt_len_all"] = prompt
    else:
        kw["prompt_len"] = prompt_len
    ckw = dict(repetition_penalty=c["penalty"], no_repeat_ngram_size=c["ngram"], min_new_tokens=c["min_new"], banned_token_ids=tuple(banned),
               include_prompt=c["include_prompt"])
    return logits, tokens, kw, ckw
