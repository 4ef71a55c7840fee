"""Test-only restatements of the in-flight entries (include/mpv.h: mpv_sample_advance_steps, mpv_logits_constrain_steps,
mpv_sample_score_steps, mpv_attn_decode_shared_steps_fwd, mpv_gpt_decode_step_shared_steps / _q8) on host tensors.  Each is written the
way the header states the invariant: row r of a _steps call IS the uniform stand-in run on that row alone at
pos = c_r = clamp(prompt_len[r], 0, row_len) + row_step[r], a row with a negative step or a column behind the table is frozen; a live
group of the step IS the ragged stand-in step (tests/standin_decode_ragged.py) on that group alone at its own suffix position, an idle
group writes nothing.  install() puts them behind `ops` and generation.InflightDecodeState on top of tests/standin_sample_ragged.install."""
import types

import torch

import standin_constrain as sk
import standin_decode_ragged as sr
import standin_sample_ragged as sra
import standin_sample_score as sq
import standin_sampling as ss
import standin_w8 as sw

BF = torch.bfloat16


def column(prompt_len, r, row_len, step):
    """c_r, or None for a frozen row"""
    return None if int(step) < 0 else sra.column(prompt_len, r, row_len, step)


def sample_advance_steps(logits, st, *, row_step, u_override=None, out_kept=None, out_mass=None, out_token=None, **kw):
    assert row_step.dtype == torch.int32 and row_step.numel() == st.rows and st.prompt_len is not None
    for r in range(st.rows):
        c = column(st.prompt_len, r, st.row_len, row_step[r])
        if c is None:                                                        # frozen: no logit read, no token written
            for out in (out_token, out_kept, out_mass):
                if out is not None:
                    out[r] = 0
            st.next_tok[r] = st.tokens[r, st.row_len - 1]
            st.done[r] = 1
            continue
        ss.sample_advance(logits[r:r + 1], sra._row_state(st, r, 0), pos=c, u_override=sra._one(u_override, r), out_kept=sra._one(out_kept, r),
                          out_mass=sra._one(out_mass, r), out_token=sra._one(out_token, r), **kw)
    st.n_done[0] = int((st.done != 0).sum())
    return st.next_tok


def logits_constrain_steps(logits, tokens, *, row_step, constraints, prompt_len, **kw):
    assert prompt_len is not None and row_step.dtype == torch.int32 and row_step.numel() == logits.shape[0]
    for r in range(logits.shape[0]):
        c = column(prompt_len, r, tokens.shape[1], row_step[r])
        if c is not None:
            sk.logits_constrain(logits[r:r + 1], tokens[r:r + 1], pos=c, constraints=constraints, prompt_len=torch.tensor([c - int(row_step[r])]),
                                **kw)
    return logits


def sample_score_steps(logits, st, sc, *, row_step, **kw):
    assert row_step.dtype == torch.int32 and row_step.numel() == st.rows and st.prompt_len is not None
    for r in range(st.rows):
        c = column(st.prompt_len, r, st.row_len, row_step[r])
        if c is None:
            continue
        one = types.SimpleNamespace(rows=1, row_len=sc.row_len, live=sc.live[r:r + 1], token_logprob=sc.token_logprob[r:r + 1],
                                    sum_logprob=sc.sum_logprob[r:r + 1], count=sc.count[r:r + 1])
        sq.sample_score(logits[r:r + 1], sra._row_state(st, r, 0), one, pos=c, **kw)
    return sc


def attn_decode_shared_steps_ref(q, k, v, pk, pv, lay, prefix_lay, n_seq, group_size, heads, lengths, own_lengths, hd, scale):
    """fp32: group g attends to lengths[g] prefix rows and own_lengths[g] own rows -> [n_seq, heads, hd]; q of sequence s at
    q + s * lay.q[0]; an idle group (own length 0) is zeros"""
    import standin_decode_shared as sds
    out = []
    (pks, _, _), (pvs, _, _) = prefix_lay
    for g, (plen, own) in enumerate(zip(lengths, own_lengths)):
        s0 = g * group_size
        n = min(group_size, n_seq - s0)
        if int(own) <= 0:
            out.append(torch.zeros(n, heads, hd, device=q.device))
            continue
        out.append(sds.attn_decode_shared_ref(sr._at(q, s0 * lay.q[0]), sr._at(k, s0 * lay.k[0]), sr._at(v, s0 * lay.v[0]), sr._at(pk, g * pks),
                                              sr._at(pv, g * pvs), lay, prefix_lay, n, group_size, heads, int(plen), int(own), hd, scale))
    return torch.cat(out, dim=0)


def steps_step(self, tokens, group_t, max_t):
    """mpv_gpt_decode_step_shared_steps(_q8) behind generation.InflightDecodeState._steps_step: every live slot is the ragged stand-in
    step on that slot alone (a one-group state over VIEWS of the caches, at the slot's own suffix position); an idle slot's logits
    are zeros and nothing of it is written"""
    st = self.prefix
    real = st.gpt
    if st.q8 is not None:
        st.gpt = sw._dequantised_decoder(st.gpt, st.q8)
    try:
        fan, P, S, nl = self.fan, self.P, self.S, self.nl
        logits = torch.zeros((self.batch, st.V), dtype=BF)
        for g, t in enumerate(group_t.tolist()):
            if t < 0 or t > max_t:
                continue
            prefix = types.SimpleNamespace(gpt=st.gpt, H=st.H, np_=st.np_, hn=st.hn, V=st.V, cache=[st.cache[li][g * P:(g + 1) * P] for li in range(nl)])
            one = types.SimpleNamespace(prefix=prefix, batch=fan, S=S, P=P, t=t, fan=fan, group_prefix_len=self.group_prefix_len[g:g + 1],
                                        suffix=[self.suffix[li][g * fan * S:(g + 1) * fan * S] for li in range(nl)])
            logits[g * fan:(g + 1) * fan] = sr._ragged_step(one, tokens[g * fan:(g + 1) * fan])
        return logits
    finally:
        st.gpt = real


def install(monkeypatch):
    """standin_sample_ragged.install, the three _steps sampler stand-ins behind youku_mplug_amd.ops and the in-flight step"""
    from youku_mplug_amd import generation, ops
    sra.install(monkeypatch)
    for name, fn in (("sample_advance_steps", sample_advance_steps), ("logits_constrain_steps", logits_constrain_steps),
                     ("sample_score_steps", sample_score_steps)):
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(generation.InflightDecodeState, "_steps_step", steps_step)
