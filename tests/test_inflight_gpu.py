"""The in-flight entries on the GPU: mpv_attn_decode_shared_steps_fwd against the fp32 softmax and, bit for bit,
against the uniform and ragged entries; mpv_gpt_decode_step_shared_steps / _q8 on the tiny decoder against the ragged driver; the three
sampler-side _steps entries on the launches of tests/sample_ragged_cases.py, every row bit for bit the uniform entry on that row alone;
and generation.sample_inflight_loop on the tiny decoder against the lockstep mixed loop at the same row count."""
import types

import pytest
import torch

import decode_ragged_cases as drc
import sample_ragged_cases as rc
import sample_score_cases as qc
import sampling_cases as sc
import standin_decode_shared as sd
import standin_inflight as si
from test_kernels_gpu import close, rel_err
from test_sample_ragged_gpu import OUTS, _bits, _same, _sampler_kw, _table

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")

# ------------------------------------------------------------------------------------------------ the attention
PREFIX = [1, 33, 65]
OWN = ([1, 33, 0], [2, 70, 33])


def _attn_case(hd, group_size, own, dev, seed=7, poison=True):
    """3 groups x group_size sequences, 2 heads, prefix lengths 1 / 33 / 65 at a pitch of 65, a suffix cache of max(own) + 3 rows and a
    DENSE q [n_seq, 3H] as the steps driver passes it.  poison: NaN in the prefix rows behind every group's length, in the suffix rows
    behind every group's own length, and in ALL operands of an idle group (its q, its suffix rows, its prefix rows)"""
    from youku_mplug_amd import ops
    heads, top = 2, max(own)
    c = drc.make_case(hd, heads, group_size, PREFIX, top, 0, seed=seed, device=dev, prefix_pad=NAN if poison else 0.0)
    H, S, n_seq = heads * hd, c["S"], c["n_seq"]
    qbuf = torch.randn(n_seq, 3 * H, generator=torch.Generator().manual_seed(seed + 1)).to(BF).to(dev)
    suffix = c["suffix"].view(n_seq, S, 3 * H)
    prefix = c["prefix"].view(len(PREFIX), max(PREFIX), 3 * H)
    if poison:
        for g, o in enumerate(own):
            rows = slice(g * group_size, (g + 1) * group_size)
            suffix[rows, o:] = NAN
            if o == 0:
                qbuf[rows] = NAN
                prefix[g] = NAN
    lay = ops.AttnLayout((3 * H, 3 * hd, 3 * H), c["lay"].k, c["lay"].v, c["lay"].o)
    return dict(c, q=qbuf.view(-1), lay=lay, own=list(own), own_len=top, qbuf=qbuf,
                group_own_len=torch.tensor(own, dtype=torch.int32, device=dev))


def _run_steps(c, **over):
    from youku_mplug_amd import ops
    c = {**c, **over}
    ops.attn_decode_shared_steps_fwd(c["q"], c["k"], c["v"], c["pk"], c["pv"], c["o"], c["lay"], c["prefix_lay"], c["n_seq"], c["group_size"],
                                     c["heads"], c["prefix_len"], c["group_prefix_len"], c["own_len"], c["group_own_len"], c["hd"], scale=c["scale"])
    torch.cuda.synchronize()
    return c["o"]


def _group_alone(c, g):
    """the uniform entry on group g alone with its two lengths (the operands are views of c's)"""
    from youku_mplug_amd import ops
    gs, S, P, H = c["group_size"], c["S"], c["prefix_len"], c["heads"] * c["hd"]
    o = torch.full((gs, H), 5.0, dtype=BF, device=c["o"].device)
    off = g * gs * S * 3 * H
    ops.attn_decode_shared_fwd(c["q"][g * gs * 3 * H:], c["k"][off:], c["v"][off:], c["pk"][g * P * 3 * H:], c["pv"][g * P * 3 * H:], o, c["lay"],
                               c["prefix_lay"], gs, gs, c["heads"], PREFIX[g], c["own"][g], c["hd"], scale=c["scale"])
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("own", OWN, ids=lambda o: "own" + "_".join(map(str, o)))
@pytest.mark.parametrize("group_size", [1, 5, 33])
@pytest.mark.parametrize("hd", [64, 80])
def test_steps_attention_is_the_uniform_entry_group_by_group(dev, hd, group_size, own):
    """NaN behind every length and in the idle group's operands: the output is finite, within 1e-2 (the gate of
    tests/test_decode_shared_gpu.py) of the fp32 softmax over each group's own keys, every live group bit for bit the uniform entry on
    that group alone with its two lengths, the idle group's rows zeros"""
    c = _attn_case(hd, group_size, own, dev)
    c["o"].fill_(7.0)
    got = _run_steps(c).clone()
    assert torch.isfinite(got.float()).all()
    want = si.attn_decode_shared_steps_ref(*[c[n] for n in ("q", "k", "v", "pk", "pv", "lay", "prefix_lay", "n_seq", "group_size", "heads")],
                                           PREFIX, own, c["hd"], c["scale"])
    e = rel_err(got.view(c["n_seq"], c["heads"], hd), want)
    print(f"    hd{hd} g{group_size} own{own}: max-abs error / max-abs ref = {e:.3e}")
    close(got.view(c["n_seq"], c["heads"], hd), want, 1e-2, f"hd{hd}-g{group_size}")
    for g, o in enumerate(own):
        rows = got[g * group_size:(g + 1) * group_size]
        if o == 0:
            assert (rows == 0).all(), g
        else:
            assert torch.equal(_group_alone(c, g), rows), (g, o)


@pytest.mark.parametrize("hd,group_size,own", [(64, 5, 12), (80, 33, 33), (64, 1, 1)])
def test_equal_own_lengths_are_the_ragged_entry_bit_for_bit(dev, hd, group_size, own):
    from youku_mplug_amd import ops
    c = _attn_case(hd, group_size, [own] * 3, dev, seed=9)
    steps = _run_steps(c).clone()
    c["o"].zero_()
    ops.attn_decode_shared_ragged_fwd(c["q"], c["k"], c["v"], c["pk"], c["pv"], c["o"], c["lay"], c["prefix_lay"], c["n_seq"], group_size, c["heads"],
                                      c["prefix_len"], c["group_prefix_len"], own, hd, scale=c["scale"])
    torch.cuda.synchronize()
    assert torch.equal(c["o"], steps)


def test_a_bad_own_length_touches_only_its_group(dev):
    """a negative length is idle, a length above the bound is the bound: the neighbours' rows are what they were"""
    c = _attn_case(64, 5, [4, 4, 4], dev, seed=10, poison=False)
    bad = torch.tensor([-5, 10 ** 6, 2], dtype=torch.int32, device=dev)
    got = _run_steps(c, group_own_len=bad).clone()
    c["o"].fill_(3.0)
    want = _run_steps(c, group_own_len=torch.tensor([0, 4, 2], dtype=torch.int32, device=dev))
    assert torch.equal(got, want) and (got[:5] == 0).all()


def test_steps_attention_refusals_leave_the_output_untouched(dev):
    from youku_mplug_amd import _lib
    c = _attn_case(64, 5, [4, 2, 0], dev, poison=False)
    c["o"].fill_(7.0)
    for over in (dict(group_own_len=None), dict(group_prefix_len=None), dict(hd=96), dict(own_len=0), dict(own_len=2049)):
        with pytest.raises(_lib.MpvError, match="mpv_attn_decode_shared_steps_fwd"):
            _run_steps(c, **over)
    with pytest.raises(ValueError, match="group_own_len"):
        _run_steps(c, group_own_len=c["group_own_len"].long())
    torch.cuda.synchronize()
    assert (c["o"] == 7.0).all()


# ------------------------------------------------------------------------------------------------ the driver on the tiny decoder
G, FAN, Q, S = len(drc.PROMPTS), drc.FAN, drc.Q, drc.STEPS


def _inflight_state(gpt, qe, prompt, weights):
    from youku_mplug_amd.generation import InflightDecodeState
    st = InflightDecodeState(gpt, G, FAN, Q + max(drc.PROMPTS), S, weights)
    first = st.install([0, 1, 2], prompt, qe, drc.PROMPTS)
    return st, first


def _t(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev)


@pytest.fixture(scope="module")
def tiny(dev):
    from test_decode_shared_cpu import _tiny_decoder
    cfg, gpt = _tiny_decoder(dev)
    qe, prompt, toks = drc.state_inputs(cfg, dev)
    return types.SimpleNamespace(cfg=cfg, gpt=gpt, qe=qe, prompt=prompt, toks=toks)


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_steps_driver_with_one_position_is_the_ragged_driver_bit_for_bit(tiny, weights):
    """three clips with prompts of 2 / 5 / 9 tokens, fan 3: install equals the ragged prefill, and three steps with every group at the
    same position equal SharedPrefixDecodeState's ragged steps -- logits and suffix cache, bit for bit -- on bf16 and on FP8 weights"""
    from youku_mplug_amd.generation import SharedPrefixDecodeState
    dev = tiny.qe.device
    ref = SharedPrefixDecodeState(tiny.gpt, G * FAN, Q + max(drc.PROMPTS) + S, weights)
    want = [ref.prefill_fan_out(tiny.prompt, tiny.qe, FAN, prompt_len=torch.tensor(drc.PROMPTS))]
    st, first = _inflight_state(tiny.gpt, tiny.qe, tiny.prompt, weights)
    got = [first.repeat_interleave(FAN, dim=0)]
    for t in range(3):
        want.append(ref.step(tiny.toks[t]))
        got.append(st.step(tiny.toks[t], _t([t] * G, dev), t))
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape == (G * FAN, tiny.cfg.vocab) and torch.equal(a, b), i
    assert st.S == ref.S and torch.equal(st.suffix, ref.suffix) and torch.equal(st.prefix.cache, ref.prefix.cache)
    assert st.group_prefix_len.tolist() == ref.group_prefix_len.tolist() == [Q + n for n in drc.PROMPTS]
    assert (st.steps, st.prefills) == (3, 1)
    assert st.kv_bytes() == tiny.cfg.layers * (G * st.P + G * FAN * S) * 3 * tiny.cfg.hidden * 2


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_steps_driver_with_groups_at_different_positions(tiny, weights):
    """group_t = [2, 0, -1]: group 0 (two positions cached, its neighbours idle meanwhile) is, bit for bit, group 0 of a state in which
    ALL groups sit at position 2; group 1 is group 1 of a state in which all sit at position 0; of the idle group 2 nothing is written
    into the suffix cache (a sentinel stays) and its logits are finite"""
    dev = tiny.qe.device
    toks = tiny.toks
    all2, _ = _inflight_state(tiny.gpt, tiny.qe, tiny.prompt, weights)
    for t in range(2):
        all2.step(toks[t], _t([t] * G, dev), t)
    want2 = all2.step(toks[2], _t([2] * G, dev), 2)
    all0, _ = _inflight_state(tiny.gpt, tiny.qe, tiny.prompt, weights)
    want0 = all0.step(toks[2], _t([0] * G, dev), 0)
    st, _ = _inflight_state(tiny.gpt, tiny.qe, tiny.prompt, weights)
    idle_rows = st.suffix.view(st.nl, G, FAN * S, -1)[:, 2]
    idle_rows.fill_(3.0)
    for t in range(2):
        st.step(toks[t], _t([t, -1, -1], dev), t)
    assert (st.suffix.view(st.nl, G, FAN * S, -1)[:, 1] == 0).all()                 # idle so far: group 1's rows are still the zeros
    got = st.step(toks[2], _t([2, 0, -1], dev), 2)
    torch.cuda.synchronize()
    assert torch.equal(got[:FAN], want2[:FAN])
    assert torch.equal(got[FAN:2 * FAN], want0[FAN:2 * FAN])
    assert torch.isfinite(got.float()).all()
    assert (idle_rows == 3.0).all()
    sfx, sfx2, sfx0 = (x.suffix.view(x.nl, G, FAN, S, -1) for x in (st, all2, all0))
    assert torch.equal(sfx[:, 0], sfx2[:, 0]) and torch.equal(sfx[:, 1], sfx0[:, 1])
    # a position outside [0, max_t] is idle too, and stays inside its group
    again = st.step(toks[2], _t([2, 0, 10 ** 6], dev), 2)
    torch.cuda.synchronize()
    assert torch.equal(again[:2 * FAN], got[:2 * FAN]) and (idle_rows == 3.0).all()


# ------------------------------------------------------------------------------------------------ the three sampler-side entries
ROW_STEP = [2, 0, 1, 3, -1, 5, 0, 2]


def _column(pl, row_len, step):
    return None if step < 0 else rc.column(pl, row_len, step)


def _advance(dev, logits, table, prompt_len, streams, row_step=None, pos=None, **kw):
    from youku_mplug_amd import ops
    from youku_mplug_amd.generation import SampleState
    st = SampleState(table.to(dev), torch.as_tensor(prompt_len).to(dev), streams=streams)
    st.n_done.fill_(-5)
    outs = {n: torch.full((st.rows,), -1, dtype=dt, device=dev) for n, dt in OUTS}
    if row_step is not None:
        ops.sample_advance_steps(logits, st, row_step=torch.tensor(row_step, dtype=torch.int32, device=dev), **outs, **kw)
    else:
        ops.sample_advance(logits, st, pos=pos, **outs, **kw)
    torch.cuda.synchronize()
    return types.SimpleNamespace(tokens=st.tokens.cpu(), next_tok=st.next_tok.cpu(), done=st.done.cpu(), n_done=int(st.n_done.item()),
                                 **{n: t.cpu() for n, t in outs.items()})


@pytest.mark.parametrize("case", rc.SAMPLER_CASES, ids=rc.sampler_id)
def test_sampler_rows_at_their_own_step_equal_the_uniform_entry_alone(dev, case):
    """8 rows, prompt_len [0, 1, 3, 5, 6, 7, 8, 2] at steps [2, 0, 1, 3, -1, 5, 0, 2]: columns 2, 1, 4, frozen (8), frozen (idle), frozen
    (12), frozen (8), 4.  Every started row is, bit for bit, the uniform entry on that row alone at its column; the frozen rows read
    nothing (their logits are NaN), keep their table row, are done and counted, and report token 0 / kept 0 / mass 0"""
    V = case[0]
    logits = rc.sampler_rows(case)
    cols = [_column(pl, rc.ROW_LEN, s) for pl, s in zip(rc.PROMPT_LEN, ROW_STEP)]
    assert cols == [2, 1, 4, None, None, None, None, 4]
    for r, col in enumerate(cols):
        if col is None:
            logits[r, :V] = NAN
    table, kw = _table(seed=case[2]), _sampler_kw(case)
    got = _advance(dev, logits.to(dev), table, rc.PROMPT_LEN, torch.arange(rc.ROWS), row_step=ROW_STEP, **kw)
    for r, col in enumerate(cols):
        if col is None:
            assert torch.equal(got.tokens[r], table[r]) and int(got.done[r]) == 1 and int(got.next_tok[r]) == int(table[r, -1]), r
            assert int(got.out_token[r]) == 0 and int(got.out_kept[r]) == 0 and float(got.out_mass[r]) == 0.0, r
            continue
        one = _advance(dev, logits[r:r + 1].to(dev), table[r:r + 1], [min(rc.PROMPT_LEN[r], col)], torch.tensor([r]), pos=col, **kw)
        for name in ("tokens", "next_tok", "done", "out_token", "out_kept", "out_mass"):
            assert _same(getattr(got, name)[r:r + 1], getattr(one, name)), (r, name)
        keep = [c for c in range(rc.ROW_LEN) if c != col]
        assert torch.equal(got.tokens[r, keep], table[r, keep]) and int(got.tokens[r, col]) == int(got.next_tok[r])
    assert got.n_done == 4


def test_sampler_with_one_step_is_the_ragged_entry_bit_for_bit(dev):
    from test_sample_ragged_gpu import _sample
    case = rc.SAMPLER_CASES[7]
    logits, kw, table = rc.sampler_rows(case).to(dev), _sampler_kw(case), _table(seed=1)
    a = _advance(dev, logits, table, rc.PROMPT_LEN, torch.arange(rc.ROWS), row_step=[rc.STEP] * rc.ROWS, **kw)
    b = _sample(dev, "ragged", logits, table, rc.PROMPT_LEN, rc.STEP, torch.arange(rc.ROWS), **kw)
    for name in ("tokens", "next_tok", "done", "out_token", "out_kept", "out_mass"):
        assert _same(getattr(a, name), getattr(b, name)), name
    assert a.n_done == b.n_done == 3


CONSTRAIN = [rc.CONSTRAIN_CASES[i] for i in (0, 2, 3, 5, 9, 15)]


@pytest.mark.parametrize("case", CONSTRAIN, ids=lambda c: f"V{c[0]}-t{c[1]}-prompt{c[2]}-seed{c[3]}-{c[4]}")
def test_constraint_rows_at_their_own_step_equal_the_uniform_entry_alone(dev, case):
    """the tables of the ragged constraint launches with the steps [2, 0, 1, 3, -1, 5, 0, 2, ...] row by row: every started row
    bit-identical to mpv_logits_constrain on that row alone at pos = c_r with g = row_step[r] generated tokens; frozen rows (a negative
    step or a column behind the table), the columns behind the vocabulary and the token table untouched; with one step for every row
    the launch is the ragged entry's, bit for bit"""
    from youku_mplug_amd import ops
    from youku_mplug_amd.generation import LogitsConstraints
    V, t, include_prompt, seed, kind = case
    logits, tokens, pls, _, ckw = rc.constrain_build(V, t, include_prompt, seed, kind)
    rows = logits.shape[0]
    steps = (ROW_STEP * 2)[:rows]
    cons = LogitsConstraints(**ckw)
    dl, dt = logits.to(dev), tokens.to(dev)
    kw = dict(constraints=cons, eos_ids=[rc.EOS], vocab=V)
    assert ops.logits_constrain_steps(dl, dt, row_step=torch.tensor(steps, dtype=torch.int32, device=dev), prompt_len=pls.to(dev), **kw) is dl
    torch.cuda.synchronize()
    got = dl.cpu()
    assert torch.equal(dt.cpu(), tokens) and (got[:, V:] == sc.POISON).all()
    n_frozen = 0
    for r, pl in enumerate(pls.tolist()):
        col = _column(pl, rc.C_ROW_LEN, steps[r])
        if col is None:
            n_frozen += 1
            assert _same(got[r], logits[r]), r
            continue
        one = logits[r:r + 1].to(dev)
        ops.logits_constrain(one, dt[r:r + 1], pos=col, prompt_len=torch.tensor([col - steps[r]], device=dev), **kw)
        assert _same(got[r], one[0]), r
        if steps[r] < 2:
            assert float(got[r, rc.EOS]) == float("-inf"), r                  # min_new_tokens = 2 counts row_step[r]
    assert 3 <= n_frozen < rows
    a, b = logits.to(dev), logits.to(dev)
    ops.logits_constrain_steps(a, dt, row_step=torch.full((rows,), t, dtype=torch.int32, device=dev), prompt_len=pls.to(dev), **kw)
    ops.logits_constrain_ragged(b, dt, step=t, prompt_len=pls.to(dev), **kw)
    assert _same(a, b)


@pytest.mark.parametrize("c", rc.SCORE_CASES, ids=qc.case_id)
def test_score_rows_at_their_own_step_equal_the_uniform_entry_alone(dev, c):
    """the tables of the ragged score launches with the steps [2, 0, 1, 3, -1, 5, 0, 2]: every scored row bit-identical to
    mpv_sample_score on that row alone at pos = c_r; frozen and dead rows and every other cell untouched; with one step for every row
    the launch is the ragged entry's, bit for bit"""
    from youku_mplug_amd import ops
    b, _ = rc.score_build(c)
    V, rows, L = c["V"], c["rows"], c["row_len"]
    assert rows == len(ROW_STEP)
    cols = [_column(int(b.prompt_len[r]), L, ROW_STEP[r]) for r in range(rows)]
    st, sc_, table = qc.states(b, dev)
    logits = b.logits.to(dev)
    assert ops.sample_score_steps(logits, st, sc_, row_step=torch.tensor(ROW_STEP, dtype=torch.int32, device=dev), vocab=V) is sc_
    torch.cuda.synchronize()
    assert _same(logits, b.logits) and torch.equal(st.tokens.cpu(), b.tokens) and torch.equal(st.done.cpu(), b.done)
    scored = torch.tensor([cols[r] is not None and int(b.live[r]) == 1 for r in range(rows)])
    assert any(col is None for col in cols)
    cell = torch.zeros(rows * L + qc.TAIL, dtype=torch.bool)
    for r in range(rows):
        if scored[r]:
            cell[r * L + cols[r]] = True
    got_table = table.cpu()
    assert qc.same_bits(got_table[~cell], b.table[~cell]), "a cell of a frozen or dead row, another column or the tail was written"
    got_sum, got_cnt, got_live = sc_.sum_logprob.cpu(), sc_.count.cpu(), sc_.live.cpu()
    for r in range(rows):
        if not scored[r]:
            assert qc.same_bits(got_sum[r:r + 1], b.sum_logprob[r:r + 1]) and int(got_cnt[r]) == int(b.count[r]) and int(got_live[r]) == int(b.live[r]), r
            continue
        assert int(got_cnt[r]) == int(b.count[r]) + 1 and int(got_live[r]) == (0 if int(b.done[r]) else 1), r
        one = types.SimpleNamespace(logits=b.logits[r:r + 1], tokens=b.tokens[r:r + 1], prompt_len=torch.tensor([min(max(int(b.prompt_len[r]), 0), cols[r])]),
                                    done=b.done[r:r + 1], live=b.live[r:r + 1], table=b.table[:L + qc.TAIL], sum_logprob=b.sum_logprob[r:r + 1],
                                    count=b.count[r:r + 1])
        st1, sc1, table1 = qc.states(one, dev)
        ops.sample_score(one.logits.to(dev), st1, sc1, pos=cols[r], vocab=V)
        assert qc.same_bits(table1[:L], got_table[r * L:(r + 1) * L]) and qc.same_bits(sc1.sum_logprob, got_sum[r:r + 1]), r
    b2, _ = rc.score_build(c)
    st2, sc2, table2 = qc.states(b2, dev)
    b3, _ = rc.score_build(c)
    st3, sc3, table3 = qc.states(b3, dev)
    ops.sample_score_steps(logits, st2, sc2, row_step=torch.full((rows,), rc.S_STEP, dtype=torch.int32, device=dev), vocab=V)
    ops.sample_score_ragged(logits, st3, sc3, step=rc.S_STEP, vocab=V)
    assert qc.same_bits(table2, table3) and qc.same_bits(sc2.sum_logprob, sc3.sum_logprob) and torch.equal(sc2.count, sc3.count)


def test_steps_entries_refuse_a_bad_row_step(dev):
    from youku_mplug_amd import _lib, ops
    from youku_mplug_amd.generation import LogitsConstraints, SampleScores, SampleState
    logits = sc.make_row(64, 1, "normal")[None].repeat(2, 1).to(dev)
    st = SampleState(_table(2, 8).to(dev), torch.tensor([1, 2]).to(dev))
    scs = SampleScores(2, 8, dev)
    before = {n: getattr(st, n).clone() for n in SampleState.ARRAYS}
    for bad in (None, torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)):
        with pytest.raises(_lib.MpvError, match="row_step"):
            ops.sample_advance_steps(logits, st, row_step=bad)
        with pytest.raises(_lib.MpvError, match="row_step"):
            ops.logits_constrain_steps(logits, st.tokens, row_step=bad, constraints=LogitsConstraints(repetition_penalty=1.2), prompt_len=st.prompt_len)
        with pytest.raises(_lib.MpvError, match="row_step"):
            ops.sample_score_steps(logits, st, scs, row_step=bad)
    torch.cuda.synchronize()
    assert all(torch.equal(getattr(st, n), before[n]) for n in SampleState.ARRAYS) and int(scs.count.sum()) == 0


# ------------------------------------------------------------------------------------------------ the loop on the tiny decoder
LENGTHS, BUDGETS, N, QL = [3, 1, 4, 2, 3], [2, 5, 3, 1, 4], 3, 16


@pytest.fixture(scope="module")
def clips(tiny):
    """five clips in rows 6 wide behind 16 query slots: a prefill of one clip has 20 rows and one of two has 40, so both run the tile
    kernel of the products (at most 16 rows take the weight-streaming one, whose sums run in another order)"""
    g = torch.Generator().manual_seed(91)
    dev = tiny.qe.device
    ids = torch.randint(8, tiny.cfg.vocab, (5, 6), generator=g).to(dev)
    qe = (torch.randn(5, QL, tiny.cfg.hidden, generator=g) * 0.5).to(dev).to(BF)
    return types.SimpleNamespace(ids=ids, qe=qe)


def _inflight(tiny, clips, order, slots=2, refill_min=1, **kw):
    tiny.gpt.config.extra.update(tokens_to_generate=5)
    sel = torch.tensor(order, device=clips.ids.device)
    streams = (sel[:, None] * N + torch.arange(N, device=sel.device)[None]).reshape(-1)
    out = tiny.gpt.sample_inflight(clips.ids[sel], query_embeds=clips.qe[sel].contiguous(), prompt_length=[LENGTHS[c] for c in order], num_samples=N,
                                   slots=slots, seed=21, streams=streams, max_new_tokens=[BUDGETS[c] for c in order], refill_min=refill_min,
                                   top_p=0.9, temperature=1.1, return_scores=True, termination_id=-1, **kw)
    torch.cuda.synchronize()
    return out


def _lockstep_pair(tiny, clips, c, **kw):
    """clip c with a partner (clip 2, the longest prompt, or clip 0 for clip 2 itself) in the lockstep mixed loop: 2 clips x 3 samples,
    the in-flight loop's 6 rows, and a prefill over rows as wide as the in-flight one's -> clip c's rows and scores"""
    tiny.gpt.config.extra.update(tokens_to_generate=5)
    pair = [c, 2 if c != 2 else 0]
    sel = torch.tensor(pair, device=clips.ids.device)
    streams = (sel[:, None] * N + torch.arange(N, device=sel.device)[None]).reshape(-1)
    toks, scs = tiny.gpt.sample_batched(clips.ids[sel], query_embeds=clips.qe[sel].contiguous(), prompt_length=[LENGTHS[i] for i in pair],
                                        num_samples=N, seed=21, streams=streams, top_p=0.9, temperature=1.1, kv="shared_prefix", mixed_prompts=True,
                                        return_scores=True, use_eod_token_for_early_termination=False, termination_id=-1, **kw)
    torch.cuda.synchronize()
    return toks[:N], scs.token_logprob[:N]


@pytest.fixture(scope="module")
def runs(tiny, clips):
    """the in-flight runs once for the module: input order twice, and a permuted order; nothing here is modified by the tests"""
    ident = list(range(5))
    return types.SimpleNamespace(a=_inflight(tiny, clips, ident), b=_inflight(tiny, clips, ident), perm=[4, 2, 0, 3, 1],
                                 p=_inflight(tiny, clips, [4, 2, 0, 3, 1]))


def test_inflight_loop_equals_the_lockstep_mixed_loop_at_its_row_count(tiny, clips, runs):
    """5 clips (prompts 3 / 1 / 4 / 2 / 3, budgets 2 / 5 / 3 / 1 / 4) through 2 slots x 3 samples, nothing terminates: every clip's
    tokens and token scores are, bit for bit and on every column both wrote, those of a lockstep mixed call of the same 6 rows that
    holds the clip; 7 decode steps and 3 prefills, as the budgets imply"""
    out = runs.a
    assert (out.steps, out.prefills) == (7, 3) and out.written == [pl + b for pl, b in zip(LENGTHS, BUDGETS)]
    for c in range(5):
        want, wlp = _lockstep_pair(tiny, clips, c)
        w = min(out.written[c], want.shape[1])
        rows = slice(c * N, (c + 1) * N)
        assert torch.equal(out.tokens[rows, :w], want[:, :w]), (c, out.tokens[rows].tolist(), want.tolist())
        assert _same(out.scores.token_logprob[rows, :w], wlp[:, :w]), c
        assert (out.scores.token_logprob[rows, LENGTHS[c]:w] < 0).all() and (out.scores.token_logprob[rows, w:] == 0).all()
        assert out.scores.count[rows].tolist() == [BUDGETS[c]] * N
        assert (out.tokens[rows, :LENGTHS[c]] == clips.ids[c, :LENGTHS[c]]).all()
    assert len({tuple(r) for r in out.tokens[3:6].tolist()}) > 1               # the three streams of a clip draw different rows


def test_a_clips_rows_do_not_depend_on_when_or_where_it_runs(runs):
    """input order [4, 2, 0, 3, 1] instead of [0 .. 4]: every clip enters at another time (at the start or mid-flight), in another slot
    and beside other neighbours, alone in its prefill or with a second clip; its rows and scores are bit-identical.  Two runs of one
    call are bit-identical"""
    a, b, p = runs.a, runs.b, runs.p
    assert torch.equal(a.tokens, b.tokens) and a.written == b.written
    for name in ("token_logprob", "sum_logprob", "count", "live"):
        assert _same(getattr(a.scores, name), getattr(b.scores, name)), name
    for i, c in enumerate(runs.perm):
        ra, rp = slice(c * N, (c + 1) * N), slice(i * N, (i + 1) * N)
        w = a.written[c]
        assert p.written[i] == w
        assert torch.equal(a.tokens[ra, :w], p.tokens[rp, :w]), c
        for name in ("token_logprob", "sum_logprob", "count"):
            assert _same(getattr(a.scores, name)[ra], getattr(p.scores, name)[rp]), (c, name)


def test_inflight_loop_on_fp8_weights_with_constraints_and_a_termination(tiny, clips):
    """decode_weights="fp8", a repetition penalty with min_new_tokens = 2 and a termination id the model draws, 3 slots with refills
    that wait for two free ones: two runs are bit-identical, no row terminates before its third token, and every row is scored up to
    and including its terminating token and nowhere else"""
    from youku_mplug_amd.generation import LogitsConstraints
    probe = _inflight(tiny, clips, list(range(5)), decode_weights="fp8")
    tid = int(probe.tokens[1 * N, LENGTHS[1] + 2])                              # clip 1's third token, sample 0
    kw = dict(decode_weights="fp8", constraints=LogitsConstraints(repetition_penalty=1.3, min_new_tokens=2), slots=3)
    outs = []
    for _ in range(2):
        tiny.gpt.config.extra.update(tokens_to_generate=5)
        out = tiny.gpt.sample_inflight(clips.ids, query_embeds=clips.qe, prompt_length=LENGTHS, num_samples=N, seed=21, max_new_tokens=BUDGETS,
                                       refill_min=2, top_p=0.9, temperature=1.1, return_scores=True, termination_id=tid, **kw)
        torch.cuda.synchronize()
        outs.append(out)
    a, b = outs
    assert torch.equal(a.tokens, b.tokens) and _same(a.scores.token_logprob, b.scores.token_logprob) and a.written == b.written
    for c in range(5):
        for s in range(N):
            r, pl = c * N + s, LENGTHS[c]
            gen = a.tokens[r, pl:a.written[c]].tolist()
            n = gen.index(tid) + 1 if tid in gen else len(gen)
            assert tid not in gen[:2]                                           # min_new_tokens = 2
            assert int(a.scores.count[r]) == n and (a.scores.token_logprob[r, pl:pl + n] < 0).all()
            assert (a.scores.token_logprob[r, pl + n:] == 0).all() and (a.scores.token_logprob[r, :pl] == 0).all()
