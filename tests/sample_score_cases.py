"""The launches mpv_sample_score is checked on (tests/test_sample_score_gpu.py; tests/test_sample_score_cpu.py runs the stand-in on the
same list and checks that the list covers what it claims).

A case is a dict: V, ldx (ld = V + ldx; the extra columns hold NaN, so a kernel that read them would show it), rows, row_len, pos, seed.
Everything else follows from (seed, row):
  role of row r, ROLES[(seed + r) % 4]:  "live" (started, scored), "forced" (prompt_len = pos + 1: teacher-forced, skipped), "dead"
    (live = 0: terminated earlier, skipped) and "ends" (scored, and done = 1: live flips to 0 in this very call);
  logits of row r, VARIANTS[(seed + r) % len(VARIANTS)], all finite values within |x| <= 64:
    normal / one_hot / half_neg_inf   sampling_cases.make_row (a tail around -20, hot entries in [-6, 0]; half the row -inf)
    wide                              uniform in [-64, 64]
    flat                              64 everywhere: S = V, the largest log S
    token_neg_inf                     "normal" with the chosen token's logit -inf: lp = -inf
    all_neg_inf                       -inf throughout, token 0 (what the sampler emits): lp = -inf, never NaN
  the token of row r: uniform over the columns whose logit is finite (token_neg_inf: any column, then banned).
The state before the launch is NOT the initial one, so that an untouched word shows: token_logprob is NaN everywhere (a canary, also in
a tail of TAIL words behind the rows * row_len table), sum_logprob[r] = -1.5 r, count[r] = r."""
import types

import torch

import sampling_cases as sc

ROLES = ("live", "forced", "dead", "ends")
VARIANTS = ("normal", "wide", "half_neg_inf", "flat", "token_neg_inf", "one_hot", "all_neg_inf")
TAIL = 16
GATE = 2e-5        # |lp - lp64|: derived in DESIGN.md section 19 (and the issue), not tuned


def _case(V, ldx, rows, row_len, pos, seed):
    return dict(V=V, ldx=ldx, rows=rows, row_len=row_len, pos=pos, seed=seed)


VOCABS = (8, 64, 520, 8192, 51200, 65536)

CASES = (
    # every vocabulary with ld == V and ld > V, three rows, both ends of a 37-column table
    [_case(V, ldx, 3, 37, 36 if (i + j) % 2 else 0, 10 + 2 * i + j) for i, V in enumerate(VOCABS) for j, ldx in enumerate((0, 8))] +
    # a launch of one row, in every role; the one-column table
    [_case(64, 8, 1, 1, 0, 30 + k) for k in range(4)] + [_case(520, 0, 1, 37, 36, 34 + k) for k in range(7)] +
    # many rows; the longest table, first and last column
    [_case(8, 8, 160, 37, 0, 50), _case(520, 8, 160, 2048, 2047, 51), _case(51200, 0, 160, 2048, 0, 52), _case(65536, 8, 160, 37, 36, 53),
     _case(8192, 0, 3, 2048, 2047, 54), _case(64, 0, 3, 1, 0, 55)]
)


def case_id(c):
    return "-".join(f"{k}{c[k]}" for k in ("V", "ldx", "rows", "row_len", "pos", "seed"))


def role_of(c, r):
    return ROLES[(c["seed"] + r) % len(ROLES)]


def variant_of(c, r):
    return VARIANTS[(c["seed"] + r) % len(VARIANTS)]


def make_row(V, row_seed, variant):
    """-> (bf16 [V], token)"""
    g = torch.Generator().manual_seed(row_seed)
    if variant == "wide":
        row = (128.0 * torch.rand(V, generator=g) - 64.0).to(torch.bfloat16)
    elif variant == "flat":
        row = torch.full((V,), 64.0, dtype=torch.bfloat16)
    elif variant == "all_neg_inf":
        return torch.full((V,), float("-inf"), dtype=torch.bfloat16), 0
    else:
        row = sc.make_row(V, row_seed, "normal" if variant == "token_neg_inf" else variant)
    finite = (row.float() > float("-inf")).nonzero().view(-1)
    t = int(finite[int(torch.randint(0, finite.numel(), (1,), generator=g))])
    if variant == "token_neg_inf":
        row[t] = float("-inf")
    return row, t


def build(c):
    """-> a namespace of CPU tensors: logits bf16 [rows, ld], tokens int64 [rows, row_len], prompt_len int64 [rows], done / live / count
    int32 [rows], sum_logprob fp32 [rows], table fp32 [rows * row_len + TAIL] (token_logprob is its head)"""
    V, rows, row_len, pos, seed = c["V"], c["rows"], c["row_len"], c["pos"], c["seed"]
    ld = V + c["ldx"]
    g = torch.Generator().manual_seed(seed)
    logits = torch.full((rows, ld), float("nan"), dtype=torch.bfloat16)
    tokens = torch.randint(0, V, (rows, row_len), generator=g)
    prompt_len = torch.randint(0, pos + 1, (rows,), generator=g)
    done, live = torch.zeros(rows, dtype=torch.int32), torch.ones(rows, dtype=torch.int32)
    for r in range(rows):
        row, t = make_row(V, seed * 100003 + r, variant_of(c, r))
        logits[r, :V], tokens[r, pos] = row, t
        role = role_of(c, r)
        if role == "forced":
            prompt_len[r] = pos + 1
        elif role == "dead":
            live[r], done[r] = 0, 1
        elif role == "ends":
            done[r] = 1
    return types.SimpleNamespace(logits=logits, tokens=tokens, prompt_len=prompt_len, done=done, live=live,
                                 table=torch.full((rows * row_len + TAIL,), float("nan"), dtype=torch.float32),
                                 sum_logprob=-1.5 * torch.arange(rows, dtype=torch.float32), count=torch.arange(rows, dtype=torch.int32))


def states(b, device="cpu"):
    """the (st, sc, table) of ops.sample_score / standin_sample_score.sample_score for a built case, as copies on `device`"""
    rows, row_len = b.tokens.shape
    mv = lambda t: t.clone().to(device)
    st = types.SimpleNamespace(rows=rows, row_len=row_len, tokens=mv(b.tokens), prompt_len=mv(b.prompt_len), done=mv(b.done))
    table = mv(b.table)
    sc_ = types.SimpleNamespace(rows=rows, row_len=row_len, live=mv(b.live), token_logprob=table[:rows * row_len].view(rows, row_len),
                                sum_logprob=mv(b.sum_logprob), count=mv(b.count))
    return st, sc_, table


def same_bits(a, b):
    """fp32 tensors equal bit for bit (NaN canaries included)"""
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))
