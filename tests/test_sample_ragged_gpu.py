"""The ragged sampling entries on the GPU: mpv_sample_advance_ragged, mpv_logits_constrain_ragged and
mpv_sample_score_ragged on the launches of tests/sample_ragged_cases.py -- every row bit for bit what the UNIFORM entry gives on that
row alone at pos = c_r, and equal to the stand-ins (token-exact / bitwise / within sample_score_cases.GATE of fp64) --, frozen rows,
bad lengths, the refusals; then the mixed loop on the tiny decoder and DistributedGPT3_Caption.generate(sample_mixed_prompts=True)."""
import ctypes as C
import types

import pytest
import torch

import sample_ragged_cases as rc
import sample_score_cases as qc
import sampling_cases as sc
import standin_constrain as sk
import standin_sample_score as sq
import standin_sampling as ss

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FILL = 3
OUTS = (("out_token", torch.int64), ("out_kept", torch.int32), ("out_mass", torch.float32))


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ the sampler
def _table(rows=rc.ROWS, row_len=rc.ROW_LEN, seed=0):
    return torch.randint(8, 600, (rows, row_len), generator=torch.Generator().manual_seed(900 + seed))


def _sample(dev, entry, logits, table, prompt_len, at, streams, done=None, **kw):
    """one launch of ops.sample_advance (at = pos) or ops.sample_advance_ragged (at = step) -> a namespace of CPU tensors"""
    from youku_mplug_amd import ops
    from youku_mplug_amd.generation import SampleState
    st = SampleState(table.to(dev), torch.as_tensor(prompt_len).to(dev), streams=streams)
    if done is not None:
        st.done.copy_(done.to(dev))
    st.n_done.fill_(-5)
    outs = {n: torch.full((st.rows,), -1, dtype=dt, device=dev) for n, dt in OUTS}
    fn, key = (ops.sample_advance_ragged, "step") if entry == "ragged" else (ops.sample_advance, "pos")
    fn(logits, st, **{key: at}, **outs, **kw)
    torch.cuda.synchronize()
    return types.SimpleNamespace(tokens=st.tokens.cpu(), next_tok=st.next_tok.cpu(), done=st.done.cpu(), n_done=int(st.n_done.item()),
                                 **{n: t.cpu() for n, t in outs.items()})


def _sampler_kw(case, **more):
    V, ld, seed, T, filt, _ = case
    top_k, top_p = sc.filter_args(filt)
    return dict(temperature=T, top_k=top_k, top_p=top_p, seed=seed, vocab=V, termination_id=-1, **more)


def _row_alone(dev, logits, table, r, col, pl, kw, done=None):
    """the uniform entry on row r alone at pos = col, with the row's (clamped) prompt length and its stream"""
    return _sample(dev, "uniform", logits[r:r + 1], table[r:r + 1], [min(max(pl, 0), col)], col, torch.tensor([r]),
                   done=None if done is None else done[r:r + 1], **kw)


@pytest.mark.parametrize("case", rc.SAMPLER_CASES, ids=rc.sampler_id)
def test_sampler_rows_equal_the_uniform_entry_alone_and_the_standin(dev, case):
    """8 rows, prompt_len [0, 1, 3, 5, 6, 7, 8, 2] at step 2: every started row is, bit for bit, the uniform entry on that row alone at
    its column (token, table row, next_tok, done, kept, mass) and draws the stand-in's token; the three frozen rows read nothing (their
    logits are NaN here), keep their table row, are done and counted, and report token 0 / kept 0 / mass 0"""
    V = case[0]
    logits = rc.sampler_rows(case)
    for r, col in enumerate(rc.COLUMNS):
        if col is None:
            logits[r, :V] = float("nan")
    table, kw = _table(seed=case[2]), _sampler_kw(case)
    got = _sample(dev, "ragged", logits.to(dev), table, rc.PROMPT_LEN, rc.STEP, torch.arange(rc.ROWS), **kw)
    n_frozen = 0
    for r, col in enumerate(rc.COLUMNS):
        if col is None:
            n_frozen += 1
            assert torch.equal(got.tokens[r], table[r]) and int(got.done[r]) == 1 and int(got.next_tok[r]) == int(table[r, -1]), r
            assert int(got.out_token[r]) == 0 and int(got.out_kept[r]) == 0 and float(got.out_mass[r]) == 0.0, r
            continue
        one = _row_alone(dev, logits.to(dev), table, r, col, rc.PROMPT_LEN[r], kw)
        for name in ("tokens", "next_tok", "done", "out_token", "out_kept", "out_mass"):
            assert _same(getattr(got, name)[r:r + 1], getattr(one, name)), (r, name)
        ok, ref = sc.candidate_ok(logits[r, :V], case[3], case[4], ss.uniform(case[2], col, r))
        assert ok, ("a listed row fails the separation condition", r)
        assert int(got.out_token[r]) == ref["token"] and int(got.out_kept[r]) == ref["kept"], (r, int(got.out_token[r]), ref["token"])
        assert int(got.tokens[r, col]) == ref["token"] == int(got.next_tok[r])
        keep = [c for c in range(rc.ROW_LEN) if c != col]
        assert torch.equal(got.tokens[r, keep], table[r, keep])
    assert n_frozen == 3 and got.n_done == 3


def test_sampler_equal_lengths_bad_lengths_and_place_in_the_launch(dev):
    case = rc.SAMPLER_CASES[7]                                                # V = 520, top-p
    logits, kw = rc.sampler_rows(case).to(dev), _sampler_kw(case)
    table = _table(seed=1)
    done = torch.tensor([0, 1, 0, 0, 0, 1, 0, 0], dtype=torch.int32)
    streams = torch.arange(rc.ROWS)
    # every length equal: the uniform entry at pos = p + t, n_done included
    a = _sample(dev, "ragged", logits, table, [3] * rc.ROWS, 2, streams, done=done, **kw)
    b = _sample(dev, "uniform", logits, table, [3] * rc.ROWS, 5, streams, done=done, **kw)
    for name in ("tokens", "next_tok", "done", "out_token", "out_kept", "out_mass"):
        assert _same(getattr(a, name), getattr(b, name)), name
    assert a.n_done == b.n_done == 2
    # lengths -3 and 10**6 act as 0 and frozen, and touch only their own rows
    base = _sample(dev, "ragged", logits, table, rc.PROMPT_LEN, rc.STEP, streams, **kw)
    bad = list(rc.PROMPT_LEN)
    bad[0], bad[3] = -3, 10 ** 6
    got = _sample(dev, "ragged", logits, table, bad, rc.STEP, streams, **kw)
    for name in ("tokens", "next_tok", "done", "out_token", "out_kept", "out_mass"):
        keep = [r for r in range(rc.ROWS) if r != 3]
        assert _same(getattr(got, name)[keep], getattr(base, name)[keep]), name      # row 0: -3 is 0, which it was
    assert torch.equal(got.tokens[3], table[3]) and int(got.done[3]) == 1 and got.n_done == base.n_done + 1
    # rows shuffled, lengths and streams with them; and a row alone in a launch of one
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4])
    moved = _sample(dev, "ragged", logits[perm.to(dev)].contiguous(), table[perm], [rc.PROMPT_LEN[i] for i in perm.tolist()], rc.STEP, perm, **kw)
    for name in ("tokens", "next_tok", "done", "out_token", "out_kept", "out_mass"):
        assert _same(getattr(moved, name), getattr(base, name)[perm]), name
    alone = _sample(dev, "ragged", logits[7:8], table[7:8], [rc.PROMPT_LEN[7]], rc.STEP, torch.tensor([7]), **kw)
    assert _same(alone.tokens, base.tokens[7:8]) and _same(alone.out_mass, base.out_mass[7:8])


def test_sampler_double_eol_looks_at_the_rows_own_previous_column(dev):
    """termination mode 2, every row drawing 198 (a nucleus of one): only the row with a 198 at c_r - 1 terminates; a row at column 0
    has no previous token"""
    V = 640
    logits = torch.stack([sc.make_row(V, 60 + r, "normal").float() for r in range(4)])
    logits[:, 198] = 12.0
    table = _table(4, 8, seed=2)
    table[:, :] = 7
    table[1, 3] = 198                                                         # row 1: prompt 4 at step 0 -> column 4, previous 198
    table[2, 2] = 198                                                         # row 2: column 4 too (prompt 4), its 198 two columns back
    got = _sample(dev, "ragged", logits.to(BF).to(dev), table, [0, 4, 4, 5], 0, torch.arange(4), temperature=1.0, top_p=0.9, seed=1, vocab=V,
                  termination_mode=2)
    assert got.out_token.tolist() == [198] * 4 and got.done.tolist() == [0, 1, 0, 0] and got.n_done == 1
    assert got.tokens[0, 0] == 198 and got.tokens[3, 5] == 198


def test_sampler_refusals_leave_every_output_untouched(dev):
    from youku_mplug_amd import _lib, ops
    from youku_mplug_amd.generation import SampleState
    logits = sc.make_row(64, 1, "normal")[None].repeat(2, 1).to(dev)
    st = SampleState(_table(2, 8).to(dev), torch.tensor([1, 2]).to(dev))
    outs = {n: torch.full((2,), -1, dtype=dt, device=dev) for n, dt in OUTS}
    st.n_done.fill_(-5)
    before = {n: getattr(st, n).clone() for n in SampleState.ARRAYS}
    good = dict(pos=1, temperature=1.0, top_k=0, top_p=0.0, **outs)
    lib = _lib.lib()
    for bad in (dict(vocab=60), dict(ld=56), dict(temperature=0.0), dict(top_k=5, top_p=0.9), dict(top_k=1, top_p=0.9), dict(top_k=65), dict(top_p=1.5),
                dict(pos=8), dict(pos=-1), dict(pos=10 ** 6), dict(termination_mode=3)):
        d = ops.sample_advance_desc(logits, st, **{**good, **bad})
        assert lib.mpv_sample_advance_ragged(C.byref(d), ops._stream()) < 0 and b"mpv_sample_advance_ragged" in lib.mpv_last_error(), bad
    for field in ("logits", "tokens", "prompt_len", "done", "next_tok", "n_done"):
        d = ops.sample_advance_desc(logits, st, **good)
        setattr(d, field, None)
        assert lib.mpv_sample_advance_ragged(C.byref(d), ops._stream()) < 0, field
    with pytest.raises(_lib.MpvError, match="mpv_sample_advance_ragged"):
        ops.sample_advance_ragged(logits, st, step=8)
    torch.cuda.synchronize()
    assert all(torch.equal(getattr(st, n), before[n]) for n in SampleState.ARRAYS) and all((t == -1).all() for t in outs.values())


# ------------------------------------------------------------------------------------------------ the constraint kernel
def _constraints(ckw):
    from youku_mplug_amd.generation import LogitsConstraints
    return LogitsConstraints(**ckw)


@pytest.mark.parametrize("case", rc.CONSTRAIN_CASES, ids=lambda c: f"V{c[0]}-t{c[1]}-prompt{c[2]}-seed{c[3]}-{c[4]}")
def test_constraint_rows_equal_the_uniform_entry_alone_and_the_standin(dev, case):
    """every started row bit-identical to mpv_logits_constrain on that row alone at pos = c_r and to standin_constrain.constrain_row on
    its history with g = t generated tokens (min_new_tokens = 2 bans the eos id at t < 2 only); frozen rows, the columns behind the
    vocabulary and the token table untouched"""
    from youku_mplug_amd import ops
    V, t, include_prompt, seed, kind = case
    logits, tokens, pls, frozen, ckw = rc.constrain_build(V, t, include_prompt, seed, kind)
    cons = _constraints(ckw)
    dl, dt = logits.to(dev), tokens.to(dev)
    kw = dict(constraints=cons, eos_ids=[rc.EOS], vocab=V)
    assert ops.logits_constrain_ragged(dl, dt, step=t, prompt_len=pls.to(dev), **kw) is dl
    torch.cuda.synchronize()
    got = dl.cpu()
    assert torch.equal(dt.cpu(), tokens) and (got[:, V:] == sc.POISON).all()
    assert len(frozen) == 3
    for r, pl in enumerate(pls.tolist()):
        col = rc.column(pl, rc.C_ROW_LEN, t)
        if col is None:
            assert r in frozen and _same(got[r], logits[r]), r
            continue
        pl = min(max(pl, 0), rc.C_ROW_LEN)
        want = logits[r, :V].clone()
        sk.constrain_row(want, tokens[r, (0 if include_prompt else pl):col], t, cons, [rc.EOS], float("-inf"))
        assert _same(got[r, :V], want), (r, (_bits(got[r, :V]) != _bits(want)).nonzero().view(-1)[:8].tolist())
        one = logits[r:r + 1].to(dev)
        ops.logits_constrain(one, dt[r:r + 1], pos=col, prompt_len=torch.tensor([pl], device=dev), **kw)
        assert _same(got[r], one[0]), r
        if t < 2:
            assert float(got[r, rc.EOS]) == float("-inf"), r                  # min_new_tokens counts t: the eos id is banned
        elif not bool((tokens[r, (0 if include_prompt else pl):col] == rc.EOS).any()):
            assert float(got[r, rc.EOS]) == 1.5, r                            # past min_new_tokens: the eos logit is left alone


def test_constraint_refusals(dev):
    from youku_mplug_amd import _lib, ops
    logits, tokens, pls, _, ckw = rc.constrain_build(64, 1, 0, 5)
    dl, dt = logits.to(dev), tokens.to(dev)
    kw = dict(constraints=_constraints(ckw), eos_ids=[rc.EOS], vocab=64)
    for step in (-1, rc.C_ROW_LEN, 10 ** 6):
        with pytest.raises(_lib.MpvError, match="mpv_logits_constrain_ragged: step"):
            ops.logits_constrain_ragged(dl, dt, step=step, prompt_len=pls.to(dev), **kw)
    with pytest.raises(_lib.MpvError, match="prompt_len"):
        ops.logits_constrain_ragged(dl, dt, step=1, prompt_len=None, **kw)
    with pytest.raises(_lib.MpvError, match="mpv_logits_constrain_ragged"):
        ops.logits_constrain_ragged(dl, dt, step=1, prompt_len=pls.to(dev), **dict(kw, vocab=60))
    torch.cuda.synchronize()
    assert _same(dl, logits)


# ------------------------------------------------------------------------------------------------ the score kernel
@pytest.mark.parametrize("c", rc.SCORE_CASES, ids=qc.case_id)
def test_score_rows_within_the_gate_and_equal_the_uniform_entry_alone(dev, c):
    """lp within sample_score_cases.GATE (2e-5, derived in DESIGN.md section 19) of the fp64 definition; every scored row bit-identical
    to mpv_sample_score on that row alone at pos = c_r; frozen and dead rows, every other cell and the tail untouched (NaN canaries)"""
    from youku_mplug_amd import ops
    b, cols = rc.score_build(c)
    V, rows, L = c["V"], c["rows"], c["row_len"]
    st, sc_, table = qc.states(b, dev)
    logits = b.logits.to(dev)
    assert ops.sample_score_ragged(logits, st, sc_, step=rc.S_STEP, vocab=V) is sc_
    torch.cuda.synchronize()
    assert _same(logits, b.logits) and torch.equal(st.tokens.cpu(), b.tokens) and torch.equal(st.done.cpu(), b.done)
    scored = torch.tensor([cols[r] is not None and int(b.live[r]) == 1 for r in range(rows)])
    assert bool(scored.any()) and any(col is None for col in cols)
    cell = torch.zeros(rows * L + qc.TAIL, dtype=torch.bool)
    for r in range(rows):
        if scored[r]:
            cell[r * L + cols[r]] = True
    got_table = table.cpu()
    assert qc.same_bits(got_table[~cell], b.table[~cell]), "a cell of a frozen or dead row, another column or the tail was written"
    got_sum, got_cnt, got_live = sc_.sum_logprob.cpu(), sc_.count.cpu(), sc_.live.cpu()
    worst = 0.0
    for r in range(rows):
        if not scored[r]:
            assert qc.same_bits(got_sum[r:r + 1], b.sum_logprob[r:r + 1]) and int(got_cnt[r]) == int(b.count[r]) and int(got_live[r]) == int(b.live[r]), r
            continue
        lp = float(got_table[r * L + cols[r]])
        want = sq.logprob_row_fp64(b.logits[r, :V], int(b.tokens[r, cols[r]]))
        if want == float("-inf"):
            assert lp == want, r
        else:
            worst = max(worst, abs(lp - want))
        assert int(got_cnt[r]) == int(b.count[r]) + 1 and int(got_live[r]) == (0 if int(b.done[r]) else 1), r
        # the uniform entry on this row alone
        one = types.SimpleNamespace(logits=b.logits[r:r + 1], tokens=b.tokens[r:r + 1], prompt_len=torch.tensor([min(max(int(b.prompt_len[r]), 0), cols[r])]),
                                    done=b.done[r:r + 1], live=b.live[r:r + 1], table=b.table[:L + qc.TAIL], sum_logprob=b.sum_logprob[r:r + 1],
                                    count=b.count[r:r + 1])
        st1, sc1, table1 = qc.states(one, dev)
        ops.sample_score(one.logits.to(dev), st1, sc1, pos=cols[r], vocab=V)
        assert qc.same_bits(table1[:L], got_table[r * L:(r + 1) * L]) and qc.same_bits(sc1.sum_logprob, got_sum[r:r + 1]), r
    print(f"    {qc.case_id(c)}: max |lp - lp64| = {worst:.3e} (gate {qc.GATE:.0e})")
    assert worst <= qc.GATE, worst


def test_score_refusals(dev):
    from youku_mplug_amd import _lib, ops
    b, _ = rc.score_build(rc.SCORE_CASES[1])
    st, sc_, table = qc.states(b, dev)
    for step in (-1, 37, 10 ** 6):
        with pytest.raises(_lib.MpvError, match="mpv_sample_score_ragged: step"):
            ops.sample_score_ragged(b.logits.to(dev), st, sc_, step=step, vocab=520)
    torch.cuda.synchronize()
    assert qc.same_bits(table, b.table) and torch.equal(sc_.count.cpu(), b.count) and torch.equal(sc_.live.cpu(), b.live)


# ------------------------------------------------------------------------------------------------ the loop on the tiny decoder
PROMPTS, N = [2, 5, 9], 3


@pytest.fixture(scope="module")
def tiny(dev):
    import decode_ragged_cases as drc
    from test_decode_shared_cpu import _tiny_decoder
    cfg, gpt = _tiny_decoder(dev)
    qe, prompt, _ = drc.state_inputs(cfg, dev)                              # three clips, Q = 8 query slots, rows 9 wide
    return types.SimpleNamespace(cfg=cfg, gpt=gpt, qe=qe, prompt=prompt)


def _loop(tiny, tokens, qe, lengths, mixed, tokens_to_generate=5, streams=None, termination_id=-1, **kw):
    """sample_batched with top-p 0.9 and early termination off (termination_id -1: no row ever terminates) -> (tokens, SampleScores
    or None)"""
    tiny.gpt.config.extra.update(tokens_to_generate=tokens_to_generate)
    dev = tokens.device
    pl = lengths if mixed else torch.as_tensor(lengths, device=dev)
    out = tiny.gpt.sample_batched(tokens, query_embeds=qe.contiguous(), prompt_length=pl, num_samples=N, seed=21, top_p=0.9, temperature=1.1,
                                  kv="shared_prefix", use_eod_token_for_early_termination=False, termination_id=termination_id, streams=streams,
                                  **(dict(mixed_prompts=True) if mixed else {}), **kw)
    torch.cuda.synchronize()
    return out if isinstance(out, tuple) else (out, None)


def _cons(**kw):
    from youku_mplug_amd.generation import LogitsConstraints
    return LogitsConstraints(**kw)


@pytest.mark.parametrize("extra", ["plain", "penalty_min_new", "return_scores", "fp8"])
def test_mixed_loop_with_equal_prompts_is_the_uniform_loop_bit_for_bit(tiny, extra):
    """prompt_length = [5, 5, 5] with mixed_prompts=True against prompt_length = 5 in today's loop, the same 9 rows: prefill plus four
    steps (tokens_to_generate = 1 in rows 9 wide: columns 5 .. 9); tokens and scores bit-identical"""
    kw = {"plain": {}, "penalty_min_new": dict(constraints=_cons(repetition_penalty=1.3, min_new_tokens=3), return_scores=True, termination_id=7),
          "return_scores": dict(return_scores=True), "fp8": dict(decode_weights="fp8", return_scores=True)}[extra]
    want, wsc = _loop(tiny, tiny.prompt, tiny.qe, [5, 5, 5], False, tokens_to_generate=1, **kw)
    got, gsc = _loop(tiny, tiny.prompt, tiny.qe, [5, 5, 5], True, tokens_to_generate=1, **kw)
    assert got.shape == want.shape == (9, 10) and torch.equal(got, want), (got.tolist(), want.tolist())
    assert (got[:, :5] == tiny.prompt[:, :5].repeat_interleave(N, 0)).all()
    if wsc is not None:
        for name in ("token_logprob", "sum_logprob", "count", "live"):
            assert _same(getattr(gsc, name), getattr(wsc, name)), name
        if "termination_id" not in kw:
            assert int(gsc.count.min()) == 5


def test_a_clips_samples_do_not_depend_on_its_neighbour_or_its_place(tiny):
    """[A, B, A] against [A, C, A], B and C of one common length (9) longer than A (2): A's rows and scores are bit-identical in all
    four places; the two A clips share their streams inside each call"""
    A, B = tiny.prompt[0], tiny.prompt[2]
    Cc = B.clone()
    Cc[1] = (Cc[1] + 11) % 200 + 8
    streams = torch.tensor([0, 1, 2, 10, 11, 12, 0, 1, 2])
    places = []
    for mid, q in ((B, tiny.qe[2]), (Cc, tiny.qe[1])):
        toks, sc_ = _loop(tiny, torch.stack([A, mid, A]), torch.stack([tiny.qe[0], q, tiny.qe[0]]), [2, 9, 2], True, streams=streams, return_scores=True,
                          constraints=_cons(no_repeat_ngram_size=2))
        assert (toks[3:6, :9] == mid).all()
        places += [(toks[rows], sc_.token_logprob[rows], sc_.sum_logprob[rows], sc_.count[rows]) for rows in (slice(0, 3), slice(6, 9))]
    for other in places[1:]:
        assert all(_same(a, b) for a, b in zip(places[0], other))
    assert len({tuple(r) for r in places[0][0].tolist()}) > 1                 # the three streams draw different rows


@pytest.mark.parametrize("lengths", [[2, 5, 9], [7, 9, 7]], ids=["2-5-9", "7-9-7"])
def test_the_longest_prompt_is_frozen_by_the_kernels_and_the_others_run_on(tiny, lengths):
    """tokens_to_generate = 3 in rows 9 wide: final_len 12, so the 9-token prompt has 3 columns -- with lengths 7 / 9 / 7 it freezes two
    steps before the others, with 2 / 5 / 9 four and seven.  Its rows and scores are those of a call that holds only that clip; the
    other clips fill every column of their budget; the loop runs final_len - P_min positions with one host read each and no bookkeeping"""
    from youku_mplug_amd import generation
    at = lengths.index(9)
    steps = []
    orig = generation.SharedPrefixDecodeState.step
    generation.SharedPrefixDecodeState.step = lambda self, *a, **k: (steps.append(1), orig(self, *a, **k))[1]
    try:
        toks, sc_ = _loop(tiny, tiny.prompt, tiny.qe, lengths, True, tokens_to_generate=3, return_scores=True, streams=torch.arange(9))
    finally:
        generation.SharedPrefixDecodeState.step = orig
    assert len(steps) == 12 - min(lengths) - 1 and toks.shape == (9, 12)
    rows = slice(at * N, (at + 1) * N)
    one, osc = _loop(tiny, tiny.prompt[at:at + 1], tiny.qe[at:at + 1], [9], True, tokens_to_generate=3, return_scores=True, streams=torch.arange(9)[rows])
    assert torch.equal(toks[rows], one) and _same(sc_.token_logprob[rows], osc.token_logprob) and _same(sc_.sum_logprob[rows], osc.sum_logprob)
    assert sc_.count.tolist() == [12 - n for n in lengths for _ in range(N)]
    for c, n in enumerate(lengths):
        assert (toks[c * N:(c + 1) * N, :n] == tiny.prompt[c, :n]).all()
        assert (sc_.token_logprob[c * N:(c + 1) * N, n:] < 0).all() and (sc_.token_logprob[c * N:(c + 1) * N, :n] == 0).all()


# ------------------------------------------------------------------------------------------------ the caption model
def test_caption_generate_sample_mixed_prompts_on_the_tiny_model(dev):
    """ONE generate(do_sample=True, sample_mixed_prompts=True, num_samples=3, return_scores=True) call on the golden's two clips
    (prompts of 5 and 3 tokens): one lockstep loop with both clips; every returned row's token_logprob is re-derived by score_captions
    on the same tokens under the gate of tests/test_caption_score_gpu.py for that comparison: both deviate from
    the fp32 restatement's teacher-forced log-probabilities, e_packed <= 1.5 * e_sampled + 1e-6, with equal counts.
    A row-for-row comparison against the grouped call is NOT made on the device: decode steps of different row counts (3 rows per
    group there, 6 here) differ in the last bf16 digit of a logit, which can move a draw; the stand-ins of
    tests/test_sample_ragged_cpu.py, whose products do not depend on the row count, carry that comparison."""
    import caption_score_cases as cs
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    term = g["meta"]["eod_id"]
    vid = video.to(dev).to(BF)
    text = cs.text_of(ids, mask, [0, 1], dev)
    calls = []
    td = model.text_decoder
    orig = td.sample_batched
    td.sample_batched = lambda tokens, **k: (calls.append((tokens.shape[0], k.get("prompt_length"), k.get("mixed_prompts"))), orig(tokens, **k))[1]
    try:
        out, scores = model.generate(vid, text, termination_id=term, do_sample=True, sample_mixed_prompts=True, num_samples=3, return_scores=True,
                                     seed=11, kv_cache="shared_prefix")
    finally:
        td.sample_batched = orig
    assert calls == [(2, [5, 3], True)]
    Lt = ids.shape[1] + g["meta"]["tokens_to_generate"]
    e_pk = e_smp = 0.0
    n_checked = 0
    for ended in (True, False):
        cl, where = [], []
        for i in range(2):
            pl = int(mask[i].sum()) - 1
            assert out[i].shape == (3, Lt) and (out[i][:, :pl] == ids[i, :pl]).all()
            cl.append([])
            for s in range(3):
                gen = out[i][s, pl:].tolist()
                if (term in gen) != ended:
                    continue
                cl[-1].append(gen[:gen.index(term)] if ended else gen)
                where.append((i, s, pl))
        if not where:
            continue
        rs = model.score_captions(vid, text, cl, termination_id=term, score_termination=ended)
        at = [0, 0]
        for i, s, pl in where:
            j = at[i]
            at[i] += 1
            n = int(scores[i]["count"][s])
            assert int(rs[i]["count"][j]) == n, (i, s, ended)
            toks = out[i][s, pl:pl + n].tolist()
            ref = cs.restated_logprobs(("gpu-ragged", i, s), video[i], ids[i, :pl].tolist(), [toks[:-1]], toks[-1], sd, cfg)[0]
            e_smp = max(e_smp, (scores[i]["token_logprob"][s, pl:pl + n].double() - ref).abs().max().item())
            e_pk = max(e_pk, (rs[i]["token_logprob"][j, :n].double() - ref).abs().max().item())
            assert (scores[i]["token_logprob"][s, :pl] == 0).all() and (scores[i]["token_logprob"][s, pl + n:] == 0).all()
            n_checked += 1
    print(f"    the mixed sampler's own scores: e_packed {e_pk:.3e} e_sampled {e_smp:.3e}")
    assert n_checked == 6 and e_pk <= 1.5 * e_smp + 1e-6, (e_pk, e_smp)
