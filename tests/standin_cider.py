"""Torch / host restatement of ops.caption_cider (include/mpv.h: mpv_caption_cider), test-only, on any device: what
DistributedGPT3_Caption.forward_scst and the caption entry point's corpus metric call when they run without a GPU.  It restates the
KERNEL's scheme, not the textbook's -- per row the packed 64-bit key of the four tokens from every position, an order's key its low
fields, tf by comparing a row's keys with each other, a weight only at an n-gram's first occurrence, idf by PROBING the corpus table
(the table's own arrays, slot by slot, the slot rule restated), then per pair a search of the candidate's keys among the
reference's -- and is itself checked against tests/ref_cider.py on every case.  It refuses what the wrapper refuses (ValueError for a
caption that could exceed 255 tokens, AssertionError otherwise)."""
import math

import torch

MAX_LEN, ORDERS = 255, 4
calls = []       # (rows_a, rows_b, groups) of every call: "was the stand-in reached at all?"


def _probe(key, keys, idf, log_ref_len):
    """idf of a packed key: the probe sequence of the kernel over the table's arrays (keys: Python ints, unsigned)"""
    cap = len(keys)
    slot = _slot(key, cap)
    for _ in range(cap):
        if keys[slot] == key:
            return idf[slot]
        if keys[slot] == 0:
            break
        slot = (slot + 1) & (cap - 1)
    return log_ref_len


def _slot(key, cap):
    x = key
    x ^= x >> 30
    x = x * 0xbf58476d1ce4e5b9 & (1 << 64) - 1
    x ^= x >> 27
    x = x * 0x94d049bb133111eb & (1 << 64) - 1
    return (x ^ x >> 31) & (cap - 1)


def _row(tokens, table):
    """one caption -> (per order: {key: vec} at first occurrences, in position order; norms)"""
    keys, idf, log_ref_len = table
    L = len(tokens)
    field = [t + 1 for t in tokens] + [0] * 4
    full = [field[i] | field[i + 1] << 16 | field[i + 2] << 32 | field[i + 3] << 48 for i in range(L)]
    vec, norm = [], []
    for n in range(ORDERS):
        mask = (1 << 16 * (n + 1)) - 1
        mine, sq = {}, 0.0
        for i in range(L - n):
            k = full[i] & mask
            if k in mine:
                continue
            tf = sum(1 for j in range(L) if (full[j] ^ full[i]) & mask == 0)
            mine[k] = float(tf) * _probe(k, keys, idf, log_ref_len)
            sq += mine[k] * mine[k]
        vec.append(mine)
        norm.append(math.sqrt(sq))
    return vec, norm


def caption_cider(tok_a, start_a, begin_a, tok_b, start_b, begin_b, *, term, stats, sigma=6.0, width_a=None, width_b=None):
    dev = tok_a.device
    keys_t, idf_t, log_ref_len = stats.arrays("cpu") if hasattr(stats, "arrays") else stats
    assert keys_t.numel() >= 2 and keys_t.numel() & (keys_t.numel() - 1) == 0
    table = ([k & (1 << 64) - 1 for k in keys_t.cpu().view(torch.int64).tolist()], idf_t.cpu().tolist(), float(log_ref_len))
    sides = []
    for tok, start, begin, width in ((tok_a, start_a, begin_a, width_a), (tok_b, start_b, begin_b, width_b)):
        assert tok.dtype == torch.int64 and tok.ndim == 2
        width = tok.shape[1] if width is None else int(width)
        start = [int(s) for s in (start.tolist() if torch.is_tensor(start) else start)]
        begin = [int(s) for s in (begin.tolist() if torch.is_tensor(begin) else begin)]
        assert len(start) == tok.shape[0] and width <= tok.shape[1]
        if start and width - min(start) > MAX_LEN:
            raise ValueError(f"caption_cider: a candidate of {width - min(start)} tokens (at most {MAX_LEN})")
        assert all(0 <= s <= width for s in start)
        assert begin[0] == 0 and begin[-1] == tok.shape[0] and all(x <= y for x, y in zip(begin, begin[1:]))
        caps = []
        for row, s in zip(tok.cpu().tolist(), start):
            gen = row[s:width]
            caps.append(gen[:gen.index(int(term))] if int(term) in gen else gen)
        memo = {}
        rows = [memo.setdefault(tuple(c), _row(c, table)) for c in caps]
        sides.append((caps, begin, rows))
    (ca, ba, ra), (cb, bb, rb) = sides
    assert len(ba) == len(bb)
    calls.append((len(ca), len(cb), len(ba) - 1))
    pair, score = [], []
    for g in range(len(ba) - 1):
        nb = bb[g + 1] - bb[g]
        for i in range(ba[g], ba[g + 1]):
            total = [0.0] * ORDERS
            for j in range(bb[g], bb[g + 1]):
                penalty = math.exp(-float(len(ca[i]) - len(cb[j])) ** 2 / (2.0 * sigma * sigma))
                vals = []
                for n in range(ORDERS):
                    val = 0.0
                    for k, vc in ra[i][0][n].items():
                        vr = rb[j][0][n].get(k, 0.0)
                        val += min(vc, vr) * vr
                    if ra[i][1][n] != 0.0 and rb[j][1][n] != 0.0:
                        val /= ra[i][1][n] * rb[j][1][n]
                    vals.append(val * penalty)
                    total[n] += vals[n]
                pair.append(vals)
            score.append(10.0 * (sum(total) / ORDERS / nb) if nb else 0.0)
    return (torch.tensor(pair, dtype=torch.float64, device=dev).reshape(-1, ORDERS), torch.tensor(score, dtype=torch.float64, device=dev))


def install(monkeypatch):
    from youku_mplug_amd import ops
    monkeypatch.setattr(ops, "caption_cider", caption_cider)
