"""Test-only restatements of the two entries behind beam search in flight (include/mpv.h: mpv_beam_advance_steps,
mpv_kv_suffix_reorder_steps) on host tensors, written the way the header states them: a clip at step s IS the uniform stand-in
advance (tests/standin_beam_groups.py; one group: tests/standin_beam.py's iteration) on that clip alone at pos = clamp(prompt_len, 0,
row_len) + s, cur_len = s + 1, first = (s == 0), a clip with a negative step or a column behind the table is frozen; the re-order is
a torch gather of every clip's first rows.  install() puts them behind `ops` on top of tests/standin_inflight.install."""
import types

import torch

import beam_groups_cases as bg
import standin_beam_groups as sg
import standin_inflight as si

PER_ROW = ("src_row", "next_tok")


def clip_view(st, c, G, clone=True):
    """clip c of a BeamState of (clip, group) pseudo-clips as a state of its own (copies, or views with clone=False)"""
    K = st.beams
    sub = types.SimpleNamespace(batch=G, beams=K, row_len=st.row_len)
    for n in bg.STATE_ARRAYS:
        t = getattr(st, n)
        t = t[c * G * K:(c + 1) * G * K] if n in PER_ROW else t[c * G:(c + 1) * G]
        setattr(sub, n, t.clone() if clone else t)
    return sub


def beam_advance_steps(cand_val, cand_idx, st, *, groups=1, diversity_penalty=0.0, vocab, clip_prompt_len, clip_step, stop_token):
    G, K, Lt = int(groups), st.beams, st.row_len
    B = st.batch // G
    assert clip_prompt_len.dtype == clip_step.dtype == torch.int32 and clip_prompt_len.numel() == clip_step.numel() == B
    st.tokens_alt.copy_(st.tokens)                                           # a frozen clip's rows go to the other table unchanged
    for c in range(B):
        s, pl = int(clip_step[c]), min(max(int(clip_prompt_len[c]), 0), Lt)
        rows = slice(c * G * K, (c + 1) * G * K)
        if s < 0 or pl + s >= Lt:                                            # frozen: no candidate read, nothing else written
            st.src_row[rows] = torch.arange(rows.start, rows.stop)
            st.next_tok[rows] = int(stop_token)
            continue
        sub = clip_view(st, c, G)
        sg.beam_advance_groups(cand_val[rows], cand_idx[rows], sub, groups=G, diversity_penalty=diversity_penalty, vocab=vocab, pos=pl + s,
                               cur_len=s + 1, first=s == 0, stop_token=stop_token)
        sub.src_row += rows.start                                            # the one-clip call numbers its rows from 0
        whole = clip_view(st, c, G, clone=False)
        for n in bg.STATE_ARRAYS:
            if n not in ("tokens", "tokens_alt"):
                getattr(whole, n).copy_(getattr(sub, n))
        whole.tokens_alt.copy_(sub.tokens)                                   # the stand-in has swapped: tokens is the table it wrote
    st.tokens, st.tokens_alt = st.tokens_alt, st.tokens
    return st.src_row, st.next_tok


def kv_suffix_reorder_steps(src, dst, idx, group_rows, *, fan, suffix_rows, max_rows):
    assert idx.dtype == torch.int64 and group_rows.dtype == torch.int32 and 0 <= max_rows <= suffix_rows
    n_seq = idx.numel()
    s, d = src.view(src.shape[0], n_seq, suffix_rows, -1), dst.view(dst.shape[0], n_seq, suffix_rows, -1)
    for j in range(n_seq):
        r = min(max(int(group_rows[j // fan]), 0), max_rows)
        assert int(idx[j]) // fan == j // fan                                # a source row never leaves the clip
        d[:, j, :r] = s[:, int(idx[j]), :r]
    return dst


def install(monkeypatch):
    """standin_inflight.install and the two stand-ins above behind youku_mplug_amd.ops"""
    from youku_mplug_amd import ops
    si.install(monkeypatch)
    monkeypatch.setattr(ops, "beam_advance_steps", beam_advance_steps)
    monkeypatch.setattr(ops, "kv_suffix_reorder_steps", kv_suffix_reorder_steps)
