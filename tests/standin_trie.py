"""Torch restatement of ops.logits_trie_mask / _ragged / _steps (include/mpv.h: mpv_logits_trie_mask), test-only, on any device and
for bf16 or fp32 logits: the trie_fn of the loops when they run without a GPU, and the host mask the GPU loop tests compare against.
It works on the CSR arrays of generation.PhraseTrie, as the kernel does; tests/ref_trie.py, which never sees them, checks it."""
import math

import torch


def _column(prompt_len, r, row_len, step):
    """c_r of the ragged / steps entries, or None for a frozen row"""
    pl = min(max(int(prompt_len[r]), 0), row_len)
    return None if int(step) < 0 or pl + int(step) >= row_len else pl + int(step)


def walk(trie, hist, vocab):
    """-> the node the history leads to on the CSR arrays, or -1"""
    cb, ct, cn = trie.child_begin, trie.child_tok, trie.child_node
    u = 0
    for t in hist:
        t = int(t)
        if not 0 <= t < vocab:
            return -1
        kids = ct[cb[u]:cb[u + 1]]
        lo, hi = 0, len(kids)
        while lo < hi:
            mid = (lo + hi) // 2
            if kids[mid] < t:
                lo = mid + 1
            else:
                hi = mid
        if lo == len(kids) or kids[lo] != t:
            return -1
        u = cn[cb[u] + lo]
    return u


def _mask_one(row, trie, hist, eos_ids, ban_value):
    """row [vocab], a view: edited in place -> the node"""
    vocab = row.numel()
    u = walk(trie, hist, vocab)
    ok = [] if u < 0 else trie.child_tok[trie.child_begin[u]:trie.child_begin[u + 1]]
    if u < 0 or trie.terminal[u] >= 0:
        ok = list(ok) + [int(e) for e in eos_ids if 0 <= int(e) < vocab]
    keep = torch.zeros(vocab, dtype=torch.bool, device=row.device)
    if len(ok):
        keep[torch.tensor(ok, dtype=torch.long, device=row.device)] = True
    row[~keep] = torch.tensor(ban_value, dtype=torch.float32, device=row.device).to(row.dtype)
    return u


def _check(logits, tokens, vocab, eos_ids, ban_value):
    rows = logits.shape[0]
    vocab = logits.shape[-1] if vocab is None else int(vocab)
    assert logits.ndim == 2 and tokens.ndim == 2 and tokens.shape[0] == rows and tokens.dtype == torch.int64
    assert 8 <= vocab <= 65536 and vocab % 8 == 0 and logits.shape[1] >= vocab, vocab
    assert 1 <= tokens.shape[1] <= 2048 and 1 <= len(eos_ids) <= 8
    assert ban_value < 0 and not math.isnan(ban_value)
    return rows, vocab


def _apply(logits, tokens, columns, pls, trie, eos_ids, ban_value, node_out, vocab):
    for r, c in enumerate(columns):
        node = -2
        if c is not None and pls[r] <= c:
            node = _mask_one(logits[r, :vocab], trie, tokens[r, max(pls[r], 0):c].tolist(), eos_ids, float(ban_value))
        if node_out is not None:
            node_out[r] = node
    return logits


def logits_trie_mask(logits, tokens, *, pos, trie, prompt_len=None, prompt_len_all=0, eos_ids, ban_value=float("-inf"), node_out=None, vocab=None,
                     ld=None):
    rows, vocab = _check(logits, tokens, vocab, eos_ids, ban_value)
    assert 0 <= pos < tokens.shape[1], (pos, tokens.shape)
    pls = [int(prompt_len_all)] * rows if prompt_len is None else [int(v) for v in prompt_len.tolist()]
    return _apply(logits, tokens, [pos] * rows, pls, trie, eos_ids, ban_value, node_out, vocab)


def logits_trie_mask_ragged(logits, tokens, *, step, trie, prompt_len, eos_ids, ban_value=float("-inf"), node_out=None, vocab=None, ld=None):
    rows, vocab = _check(logits, tokens, vocab, eos_ids, ban_value)
    assert prompt_len is not None and 0 <= step < tokens.shape[1]
    pls = [min(max(int(v), 0), tokens.shape[1]) for v in prompt_len.tolist()]
    return _apply(logits, tokens, [_column(prompt_len, r, tokens.shape[1], step) for r in range(rows)], pls, trie, eos_ids, ban_value, node_out, vocab)


def logits_trie_mask_steps(logits, tokens, *, row_step, trie, prompt_len, eos_ids, ban_value=float("-inf"), node_out=None, vocab=None, ld=None):
    rows, vocab = _check(logits, tokens, vocab, eos_ids, ban_value)
    assert prompt_len is not None and row_step.dtype == torch.int32 and row_step.numel() == rows
    pls = [min(max(int(v), 0), tokens.shape[1]) for v in prompt_len.tolist()]
    cols = [_column(prompt_len, r, tokens.shape[1], row_step[r]) for r in range(rows)]
    return _apply(logits, tokens, cols, pls, trie, eos_ids, ban_value, node_out, vocab)


def install(monkeypatch):
    """the three stand-ins behind youku_mplug_amd.ops"""
    from youku_mplug_amd import ops
    for fn in (logits_trie_mask, logits_trie_mask_ragged, logits_trie_mask_steps):
        monkeypatch.setattr(ops, fn.__name__, fn)
