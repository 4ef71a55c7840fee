"""Torch restatement of ops.logits_constrain (include/mpv.h: mpv_logits_constrain), test-only, on any device and for bf16 or fp32
logits: the checker of the kernel (bitwise) and the constrain_fn of the loops when they run without a GPU.  It is written the way the
kernel is organised -- a first-occurrence mask over the history, a mask of the positions that end a repeat of the suffix -- and is
itself checked against a definition in sets and slices and against `transformers` in tests/test_logits_constrain_cpu.py."""
import math

import torch


def first_occurrence(h: torch.Tensor) -> torch.Tensor:
    """h int64 [m] -> bool [m]: no earlier position holds the same token"""
    m = h.numel()
    eq = h[:, None] == h[None, :]
    return ~(eq & torch.ones((m, m), dtype=torch.bool, device=h.device).tril(-1)).any(dim=1)


def repeat_ends(h: torch.Tensor, n: int) -> torch.Tensor:
    """h int64 [m] -> bool [m]: position p ends an n-gram whose first n - 1 tokens equal the last n - 1 tokens of h (n == 1: every
    position; n == 0 or m < n: none)"""
    m = h.numel()
    hit = torch.zeros(m, dtype=torch.bool, device=h.device)
    if n == 1:
        hit[:] = True
    elif n >= 2 and m >= n:
        win = h.unfold(0, n - 1, 1)[:m - n + 1]                             # the windows that start at i = 0 .. m - n
        hit[n - 1:] = (win == h[m - n + 1:][None]).all(dim=1)
    return hit


def constrain_row(row: torch.Tensor, h: torch.Tensor, g: int, constraints, eos_ids, ban_value: float):
    """row [vocab] (a view: edited in place), h int64 [m] the history, g tokens generated so far"""
    vocab, dev = row.numel(), row.device
    listed = list(constraints.banned_token_ids) + (list(eos_ids) if g < constraints.min_new_tokens else [])
    listed = torch.tensor(listed, dtype=torch.int64, device=dev)
    in_range = (h >= 0) & (h < vocab)
    own = first_occurrence(h) & in_range
    hit = repeat_ends(h, constraints.no_repeat_ngram_size)
    banned = ((h[:, None] == h[None, :]) & hit[None, :]).any(dim=1) | torch.isin(h, listed)
    pen = h[own & ~banned]
    if constraints.repetition_penalty != 1.0 and pen.numel():
        p = torch.tensor(constraints.repetition_penalty, dtype=torch.float32, device=dev)
        x = row[pen].float()
        row[pen] = torch.where(x < 0, x * p, x / p).to(row.dtype)
    ban = torch.cat([h[own & banned], listed[(listed >= 0) & (listed < vocab)]])
    if ban.numel():
        row[ban] = torch.tensor(ban_value, dtype=torch.float32, device=dev).to(row.dtype)


def logits_constrain(logits, tokens, *, pos, constraints, prompt_len=None, prompt_len_all=0, eos_ids=(), ban_value=float("-inf"), vocab=None,
                     ld=None):
    """ops.logits_constrain: edits logits [rows, ld] in place (the first `vocab` columns) and returns it; refuses what the kernel refuses"""
    rows = logits.shape[0]
    vocab = logits.shape[-1] if vocab is None else int(vocab)
    assert logits.ndim == 2 and tokens.ndim == 2 and tokens.shape[0] == rows and tokens.dtype == torch.int64
    assert 8 <= vocab <= 65536 and vocab % 8 == 0 and logits.shape[1] >= vocab, vocab
    row_len = tokens.shape[1]
    assert 1 <= row_len <= 2048 and 0 <= pos < row_len, (pos, row_len)
    assert math.isfinite(constraints.repetition_penalty) and constraints.repetition_penalty > 0
    assert 0 <= constraints.no_repeat_ngram_size <= 8 and constraints.min_new_tokens >= 0
    assert len(eos_ids) <= 8 and len(constraints.banned_token_ids) <= 1024
    assert ban_value < 0 and not math.isnan(ban_value)
    pl = [int(prompt_len_all)] * rows if prompt_len is None else [int(v) for v in prompt_len.tolist()]
    for r in range(rows):
        if pl[r] > pos:
            continue                                                        # teacher-forced: untouched
        start = 0 if constraints.include_prompt else max(pl[r], 0)
        constrain_row(logits[r, :vocab], tokens[r, start:pos], pos - pl[r], constraints, [int(t) for t in eos_ids], float(ban_value))
    return logits
