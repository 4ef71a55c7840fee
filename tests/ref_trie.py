"""Independent reference of the closed-vocabulary mask (include/mpv.h: mpv_logits_trie_mask), test-only: plain Python over a
dict-of-dicts trie built from the phrase list.  It never sees the CSR arrays of generation.PhraseTrie; the only thing it shares with
them is the numbering of the nodes, which is part of the contract: node 0 is the root and a node gets the next number when the
phrases, inserted in the order given, first reach it."""
import torch


class Node:
    __slots__ = ("kids", "phrase", "number")

    def __init__(self, number):
        self.kids, self.phrase, self.number = {}, -1, number


def build(phrases):
    """-> the root of the trie of `phrases` (lists of ints)"""
    root, n = Node(0), 1
    for idx, ph in enumerate(phrases):
        u = root
        for t in ph:
            t = int(t)
            if t not in u.kids:
                u.kids[t] = Node(n)
                n += 1
            u = u.kids[t]
        if u.phrase < 0:
            u.phrase = idx
    return root


def lookup(root, seq):
    u = root
    for t in seq:
        u = u.kids.get(int(t))
        if u is None:
            return -1
    return u.phrase


def walk(root, hist):
    """-> the node the history leads to, or None (dead)"""
    u = root
    for t in hist:
        u = u.kids.get(int(t))
        if u is None:
            return None
    return u


def allowed_tokens(root, hist, eos_ids, vocab):
    """-> (the allowed columns as a sorted list, node number or -1)"""
    u = walk(root, hist)
    if u is None:
        return sorted({int(e) for e in eos_ids if 0 <= int(e) < vocab}), -1
    ok = {t for t in u.kids if 0 <= t < vocab}
    if u.phrase >= 0:
        ok |= {int(e) for e in eos_ids if 0 <= int(e) < vocab}
    return sorted(ok), u.number


def mask_row(row, allowed, ban_value):
    """row [vocab] -> a new row: the allowed columns keep their bits, every other one is ban_value in the row's dtype"""
    out = torch.full_like(row, ban_value)
    if allowed:
        idx = torch.tensor(allowed, dtype=torch.long, device=row.device)
        out[idx] = row[idx]
    return out


def trie_mask(logits, tokens, root, *, columns, prompt_len, eos_ids, ban_value, vocab):
    """logits [rows, ld], tokens [rows, row_len] (host tensors); columns[r]: the column row r works on, or None for a row that is
    left alone (teacher-forced or frozen); prompt_len[r] ints -> (the masked copy of logits, node per row: number, -1 dead, -2
    untouched)"""
    out, nodes = logits.clone(), []
    for r in range(logits.shape[0]):
        c = columns[r]
        if c is None or prompt_len[r] > c:
            nodes.append(-2)
            continue
        hist = tokens[r, max(int(prompt_len[r]), 0):c].tolist()
        ok, node = allowed_tokens(root, hist, eos_ids, vocab)
        out[r, :vocab] = mask_row(logits[r, :vocab], ok, ban_value)
        nodes.append(node)
    return out, nodes
