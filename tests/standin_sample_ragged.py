"""Test-only restatements of the ragged sampling entries (include/mpv.h: mpv_sample_advance_ragged, mpv_logits_constrain_ragged,
mpv_sample_score_ragged; youku_mplug_amd.ops.sample_advance_ragged / logits_constrain_ragged / sample_score_ragged) on host tensors.
Each is written the way the header states the invariant: row r of a ragged call IS the uniform stand-in (tests/standin_sampling.py,
standin_constrain.py, standin_sample_score.py) run on that row alone at pos = c_r = clamp(prompt_len[r], 0, row_len) + step; a row
with c_r >= row_len is frozen.  install() puts them, with the uniform stand-ins, behind `ops` on top of
tests/standin_decode_ragged.install (the ragged prefill and step, and products that do not depend on the row count)."""
import types

import torch

import standin_constrain as sk
import standin_sample_score as sq
import standin_sampling as ss


def column(prompt_len, r, row_len, step):
    """c_r, or None for a frozen row"""
    c = min(max(int(prompt_len[r]), 0), row_len) + int(step)
    return c if c < row_len else None


def _one(t, r):
    return None if t is None else t[r:r + 1]


def _row_state(st, r, prompt_len):
    """row r of a generation.SampleState as a one-row state on VIEWS of its tensors: what the uniform stand-in writes lands in st"""
    return types.SimpleNamespace(rows=1, row_len=st.row_len, tokens=st.tokens[r:r + 1], prompt_len=torch.tensor([prompt_len]), done=st.done[r:r + 1],
                                 next_tok=st.next_tok[r:r + 1], stream=st.stream[r:r + 1], n_done=torch.zeros(1, dtype=torch.int32))


def sample_advance_ragged(logits, st, *, step, u_override=None, out_kept=None, out_mass=None, out_token=None, **kw):
    assert 0 <= int(step) < st.row_len and st.prompt_len is not None
    for r in range(st.rows):
        c = column(st.prompt_len, r, st.row_len, step)
        if c is None:                                                        # frozen: no logit read, no token written
            for out in (out_token, out_kept, out_mass):
                if out is not None:
                    out[r] = 0
            st.next_tok[r] = st.tokens[r, st.row_len - 1]
            st.done[r] = 1
            continue
        ss.sample_advance(logits[r:r + 1], _row_state(st, r, 0), pos=c, u_override=_one(u_override, r), out_kept=_one(out_kept, r),
                          out_mass=_one(out_mass, r), out_token=_one(out_token, r), **kw)
    st.n_done[0] = int((st.done != 0).sum())
    return st.next_tok


def logits_constrain_ragged(logits, tokens, *, step, constraints, prompt_len, **kw):
    assert prompt_len is not None and 0 <= int(step) < tokens.shape[1]
    for r in range(logits.shape[0]):
        c = column(prompt_len, r, tokens.shape[1], step)
        if c is not None:
            sk.logits_constrain(logits[r:r + 1], tokens[r:r + 1], pos=c, constraints=constraints, prompt_len=torch.tensor([c - int(step)]), **kw)
    return logits


def sample_score_ragged(logits, st, sc, *, step, **kw):
    assert 0 <= int(step) < st.row_len and st.prompt_len is not None
    for r in range(st.rows):
        c = column(st.prompt_len, r, st.row_len, step)
        if c is None:
            continue
        one = types.SimpleNamespace(rows=1, row_len=sc.row_len, live=sc.live[r:r + 1], token_logprob=sc.token_logprob[r:r + 1],
                                    sum_logprob=sc.sum_logprob[r:r + 1], count=sc.count[r:r + 1])
        sq.sample_score(logits[r:r + 1], _row_state(st, r, 0), one, pos=c, **kw)
    return sc


def install(monkeypatch):
    """standin_decode_ragged.install, the uniform sampling stand-ins and the three ragged ones behind youku_mplug_amd.ops"""
    import standin_decode_ragged as sr
    from youku_mplug_amd import ops
    sr.install(monkeypatch)
    for name, fn in (("sample_advance", ss.sample_advance), ("logits_constrain", sk.logits_constrain), ("sample_score", sq.sample_score),
                     ("sample_advance_ragged", sample_advance_ragged), ("logits_constrain_ragged", logits_constrain_ragged),
                     ("sample_score_ragged", sample_score_ragged)):
        monkeypatch.setattr(ops, name, fn)
