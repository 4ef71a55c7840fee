"""Beam search in flight on the GPU: mpv_beam_advance_steps on the launches of tests/beam_groups_cases.py, every
started clip bit for bit the uniform entry on that clip alone; mpv_kv_suffix_reorder_steps against a torch gather and
mpv_gather_rows_ld; and generation.beam_inflight_loop on the tiny decoder against the lockstep mixed search at the same row count."""
import types

import pytest
import torch

import beam_groups_cases as bg
import standin_beam_inflight as sbi
from test_inflight_gpu import LENGTHS, clips, tiny                                  # the fixtures: the tiny decoder and its five clips

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
VOCAB, STOP, CLIPS = 37, 7, 4
PROMPT_LEN, CLIP_STEP = [3, 1, 4, 2], [2, 0, -1, 5]
SHAPES = [(1, 1), (1, 3), (1, 8), (2, 8), (8, 2), (3, 2)]


def _i32(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev)


def _uniform(vals, idxs, st, G, lam, **step):
    from youku_mplug_amd import ops
    if G == 1:
        return ops.beam_advance(vals, idxs, st, vocab=VOCAB, stop_token=STOP, **step)
    return ops.beam_advance_groups(vals, idxs, st, groups=G, diversity_penalty=lam, vocab=VOCAB, stop_token=STOP, **step)


def _column(pl, step, Lt):
    return None if step < 0 or min(max(pl, 0), Lt) + step >= Lt else min(max(pl, 0), Lt) + step


def _check_call(dev, st, vals, idxs, G, K, Lt, lam, prompt_len, steps):
    """one _steps call on the carried state `st` (on the device): every started clip against the uniform entry on that clip alone, every
    frozen clip against what it was.  The frozen clips' candidates are NaN with indices far outside the vocabulary."""
    from youku_mplug_amd import ops
    cols = [_column(pl, s, Lt) for pl, s in zip(prompt_len, steps)]
    vals, idxs = vals.clone(), idxs.clone()
    for c, col in enumerate(cols):
        if col is None:
            vals[c * G * K:(c + 1) * G * K] = float("nan")
            idxs[c * G * K:(c + 1) * G * K] = 10 ** 12
    vals, idxs = vals.to(dev), idxs.to(dev)
    before = bg.clone_state(st)
    ops.beam_advance_steps(vals, idxs, st, groups=G, diversity_penalty=lam, vocab=VOCAB, clip_prompt_len=_i32(prompt_len, dev),
                           clip_step=_i32(steps, dev), stop_token=STOP)
    torch.cuda.synchronize()
    for c, col in enumerate(cols):
        rows = slice(c * G * K, (c + 1) * G * K)
        got, was = sbi.clip_view(st, c, G), sbi.clip_view(before, c, G)
        if col is None:
            assert torch.equal(got.tokens, was.tokens) and got.src_row.tolist() == list(range(rows.start, rows.stop)), c
            assert (got.next_tok == STOP).all(), c
            for n in ("scores", "hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "hyp_next", "worst", "done"):
                assert torch.equal(getattr(got, n), getattr(was, n)), (c, n)
            continue
        _uniform(vals[rows].contiguous(), idxs[rows].contiguous(), was, G, lam, pos=col, cur_len=steps[c] + 1, first=steps[c] == 0)
        was.src_row += rows.start
        bg.assert_states_equal(got, was, (G, K, Lt, c, steps[c]))
    return before


@pytest.mark.parametrize("Lt", [7, 70])
@pytest.mark.parametrize("G,K", SHAPES, ids=lambda v: str(v))
def test_a_clip_at_its_own_step_is_the_uniform_entry_on_that_clip_alone(dev, G, K, Lt):
    """4 clips with prompts of 3 / 1 / 4 / 2 tokens at steps 2 / 0 / -1 / 5, the state carried over three calls in which every started
    clip goes one step further: at row_len 7 clip 3 starts behind the table and clip 0 runs out of it in the third call (frozen by the
    column test), at 70 (the 64-lane row loop wraps) all three run; the hypothesis stores fill on the way and clip 1's last group is
    built to become done in the first call.  All state arrays and outputs, bit for bit"""
    lam = 0.5
    fin = (1 * G + G - 1,)
    st0, _, _ = bg.random_state(CLIPS, G, K, Lt, vocab=VOCAB, stop=STOP, pos=0, seed=100 * G + K + Lt, finishing=fin)
    st = bg.clone_state(st0, dev)
    events = [0, 0, 0]
    for call in range(3):
        # fresh candidates every call (built for the same shape; `finishing` rows carry the low values that close clip 1's group)
        _, vals, idxs = bg.random_state(CLIPS, G, K, Lt, vocab=VOCAB, stop=STOP, pos=0, seed=100 * G + K + Lt + 1000 * call,
                                        finishing=fin if call == 0 else (), stop_rate=0.9)
        steps = [s + call if s >= 0 else s for s in CLIP_STEP]
        before = _check_call(dev, st, vals, idxs, G, K, Lt, lam, PROMPT_LEN, steps)
        events = [a + b for a, b in zip(events, bg.store_events(before, st))]
        if call == 0:
            assert int(st.done[fin[0]]) == 1 and int(before.done[fin[0]]) == 0
    print(f"    (G, K', row_len) = ({G}, {K}, {Lt}): additions {events[0]}, evictions {events[1]}")
    assert Lt == 7 or events[0] > 0, events                                        # where three clips run, hypotheses were stored on the way


def test_a_step_far_outside_acts_as_frozen_and_touches_only_its_clip(dev):
    from youku_mplug_amd import ops
    G, K, Lt = 2, 3, 12
    st0, vals, idxs = bg.random_state(CLIPS, G, K, Lt, vocab=VOCAB, stop=STOP, pos=0, seed=5)
    a, b = bg.clone_state(st0, dev), bg.clone_state(st0, dev)
    kw = dict(groups=G, diversity_penalty=0.5, vocab=VOCAB, clip_prompt_len=_i32(PROMPT_LEN, dev), stop_token=STOP)
    ops.beam_advance_steps(vals.to(dev), idxs.to(dev), a, clip_step=_i32([10 ** 6, 0, 1, 2], dev), **kw)
    ops.beam_advance_steps(vals.to(dev), idxs.to(dev), b, clip_step=_i32([-1, 0, 1, 2], dev), **kw)
    torch.cuda.synchronize()
    bg.assert_states_equal(a, b)
    assert torch.equal(a.tokens[:G].cpu(), st0.tokens[:G]) and torch.equal(a.done.cpu()[:G], st0.done[:G])


@pytest.mark.parametrize("G,K,step", [(1, 3, 0), (1, 8, 2), (2, 8, 2), (3, 2, 0)])
def test_one_common_step_is_the_uniform_entry_on_the_whole_batch(dev, G, K, step):
    from youku_mplug_amd import ops
    Lt = 70
    st0, vals, idxs = bg.random_state(CLIPS, G, K, Lt, vocab=VOCAB, stop=STOP, pos=0, seed=9 + G + K, frozen=(1,))
    a, b = bg.clone_state(st0, dev), bg.clone_state(st0, dev)
    ops.beam_advance_steps(vals.to(dev), idxs.to(dev), a, groups=G, diversity_penalty=0.75, vocab=VOCAB, clip_prompt_len=_i32([3] * CLIPS, dev),
                           clip_step=_i32([step] * CLIPS, dev), stop_token=STOP)
    _uniform(vals.to(dev), idxs.to(dev), b, G, 0.75, pos=3 + step, cur_len=step + 1, first=step == 0)
    torch.cuda.synchronize()
    bg.assert_states_equal(a, b, (G, K, step))


@pytest.mark.parametrize("over", [dict(K=9, G=1), dict(G=9, K=1), dict(K=5, G=4), dict(lam=-1.0), dict(lam=float("nan")), dict(Lt=4096),
                                  dict(vocab=0), dict(clip_step=None), dict(clip_prompt_len=None), dict(clip_step="int64"), dict(clip_step="short")],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_advance_refusals_leave_the_outputs_untouched(dev, over):
    from youku_mplug_amd import _lib, ops
    from youku_mplug_amd.generation import BeamState
    c = dict(dict(K=2, G=2, lam=0.5, Lt=12, vocab=VOCAB, clip_step="ok", clip_prompt_len="ok"), **over)
    K, G = c["K"], c["G"]
    st = BeamState(torch.randint(0, VOCAB, (2 * G, c["Lt"]), generator=torch.Generator().manual_seed(1)).to(dev), K)
    for n in ("src_row", "next_tok", "tokens_alt", "scores", "hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "hyp_next", "worst"):
        getattr(st, n).fill_(bg.CANARY[getattr(st, n).dtype])
    before = {n: getattr(st, n).clone() for n in bg.STATE_ARRAYS}
    tokens_id = id(st.tokens)
    rows, m = 2 * G * K, (G + 1) * K
    arrays = {"ok": _i32([1, 0], dev), None: None, "int64": torch.zeros(2, dtype=torch.int64, device=dev), "short": _i32([1], dev)}
    with pytest.raises(_lib.MpvError, match="beam_advance_steps"):
        ops.beam_advance_steps(torch.zeros((rows, m), dtype=torch.float32, device=dev), torch.arange(m, device=dev).repeat(rows, 1), st, groups=G,
                               diversity_penalty=c["lam"], vocab=c["vocab"], clip_prompt_len=arrays[c["clip_prompt_len"]],
                               clip_step=arrays[c["clip_step"]], stop_token=STOP)
    torch.cuda.synchronize()
    assert id(st.tokens) == tokens_id
    for n, t in before.items():
        assert torch.equal(getattr(st, n), t), n


# ------------------------------------------------------------------------------------------------ the re-order
NL, FAN, GROUPS, S, H3 = 2, 3, 3, 5, 48
IDX = [2, 0, 1, 4, 3, 5, 8, 7, 6]                                                   # a permutation inside every clip


def _caches(dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(NL, GROUPS * FAN * S, H3, generator=g).to(BF).to(dev)
    return src, torch.full_like(src, -9.0)


def _expected(src, rows):
    want = torch.full_like(src, -9.0).view(NL, GROUPS * FAN, S, H3)
    s = src.view(NL, GROUPS * FAN, S, H3)
    for j, i in enumerate(IDX):
        want[:, j, :rows[j // FAN]] = s[:, i, :rows[j // FAN]]
    return want.view_as(src)


@pytest.mark.parametrize("counts,max_rows,clamped", [([2, 0, 5], 5, [2, 0, 5]), ([-3, 10 ** 6, 2], 4, [0, 4, 2])], ids=["2_0_5", "clamped"])
def test_reorder_copies_every_clips_own_rows_and_nothing_else(dev, counts, max_rows, clamped):
    """the copied region equals a torch gather; the rows at or behind a clip's count, and all rows of a clip with count 0, keep the
    sentinel; a count of -3 is 0 and one of 10^6 is max_rows"""
    from youku_mplug_amd import ops
    src, dst = _caches(dev)
    keep = src.clone()
    assert ops.kv_suffix_reorder_steps(src, dst, torch.tensor(IDX, device=dev), _i32(counts, dev), fan=FAN, suffix_rows=S, max_rows=max_rows) is dst
    torch.cuda.synchronize()
    assert torch.equal(dst, _expected(src, clamped)) and torch.equal(src, keep)


def test_reorder_with_equal_counts_is_the_lockstep_gather(dev):
    from youku_mplug_amd import ops
    src, a = _caches(dev, seed=4)
    b = a.clone()
    t = 3
    ops.kv_suffix_reorder_steps(src, a, torch.tensor(IDX, device=dev), _i32([t] * GROUPS, dev), fan=FAN, suffix_rows=S, max_rows=S)
    idx = (torch.arange(NL, device=dev)[:, None] * (GROUPS * FAN) + torch.tensor(IDX, device=dev)[None]).reshape(-1)
    ops.gather_rows_ld(src.view(-1), idx, b.view(-1), NL * GROUPS * FAN, t * H3, S * H3, S * H3)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_reorder_refusals_leave_the_destination_untouched(dev):
    from youku_mplug_amd import _lib, ops
    src, dst = _caches(dev)
    idx, rows = torch.tensor(IDX, device=dev), _i32([2, 0, 5], dev)
    call = lambda **o: ops.kv_suffix_reorder_steps(o.get("src", src), o.get("dst", dst), o.get("idx", idx), o.get("rows", rows), fan=FAN,
                                                   suffix_rows=S, max_rows=o.get("max_rows", 5))
    odd = torch.zeros(NL * GROUPS * FAN * S * 36, dtype=BF, device=dev).view(NL, GROUPS * FAN * S, 36)       # hidden 12
    off = torch.zeros(NL * GROUPS * FAN * S * H3 + 4, dtype=BF, device=dev)[4:].view(NL, GROUPS * FAN * S, H3)   # 8 bytes off
    for o in (dict(idx=None), dict(rows=None), dict(max_rows=6), dict(max_rows=-1), dict(src=odd, dst=torch.zeros_like(odd)), dict(src=off),
              dict(dst=src), dict(idx=idx.int()), dict(rows=rows.long()), dict(rows=rows[:2].contiguous())):
        with pytest.raises(_lib.MpvError, match="kv_suffix_reorder_steps"):
            call(**o)
    torch.cuda.synchronize()
    assert (dst == -9.0).all()


# ------------------------------------------------------------------------------------------------ the loop on the tiny decoder
K, NRET = 3, 3


def _inflight(tiny, clips, order, stop=STOP, slots=2, **kw):
    tiny.gpt.config.extra.update(tokens_to_generate=5)
    sel = torch.tensor(order, device=clips.ids.device)
    kw = dict(dict(beam_size=K, num_return_gen=NRET), **kw)
    out = tiny.gpt.beam_search_inflight(clips.ids[sel], query_embeds=clips.qe[sel].contiguous(), prompt_length=[LENGTHS[c] for c in order],
                                        stop_token=stop, slots=slots, refill_min=1, **kw)
    torch.cuda.synchronize()
    return out


def _lockstep_pair(tiny, clips, c, stop=STOP, **kw):
    """clip c with a partner (clip 2, the longest prompt, or clip 0 for clip 2 itself) in the lockstep mixed search: the in-flight
    loop's row count, and a prefill over rows as wide as the in-flight one's -> clip c's result"""
    tiny.gpt.config.extra.update(tokens_to_generate=5)
    pair = [c, 2 if c != 2 else 0]
    sel = torch.tensor(pair, device=clips.ids.device)
    kw = dict(dict(beam_size=K, num_return_gen=NRET), **kw)
    out = tiny.gpt.beam_search_batched(clips.ids[sel], query_embeds=clips.qe[sel].contiguous(), prompt_length=[LENGTHS[i] for i in pair],
                                       stop_token=stop, kv="shared_prefix", **kw)
    torch.cuda.synchronize()
    return out[0]


def _same_result(a, b):
    return torch.equal(a.sequences, b.sequences) and torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32)) and \
        (not hasattr(b, "group") or torch.equal(a.group, b.group))


def _full_budget_steps(slots):
    import test_inflight_cpu as ti
    return ti.simulate([6 + 5 - pl for pl in LENGTHS], slots, 1)


@pytest.fixture(scope="module")
def runs(tiny, clips):
    """the in-flight runs once for the module: input order twice, and a permuted order; nothing here is modified by the tests"""
    ident = list(range(5))
    return types.SimpleNamespace(a=_inflight(tiny, clips, ident), b=_inflight(tiny, clips, ident), perm=[4, 2, 0, 3, 1],
                                 p=_inflight(tiny, clips, [4, 2, 0, 3, 1]))


def test_inflight_search_equals_the_lockstep_mixed_search_at_its_row_count(tiny, clips, runs):
    """5 clips (prompts 3 / 1 / 4 / 2 / 3 in rows 6 wide, 16 query slots) through 2 slots x 3 beams, tokens_to_generate 5, default
    budgets: every clip's sequences are equal, and its scores bit-equal, to those of a lockstep mixed search over the same 6 rows
    that holds the clip"""
    out = runs.a
    print(f"    advances {out.advances} steps {out.steps} prefills {out.prefills}")
    assert len(out.results) == 5
    for c in range(5):
        want = _lockstep_pair(tiny, clips, c)
        got = out.results[c]
        assert _same_result(got, want), (c, got, want)
        assert (got.sequences[:, :LENGTHS[c]] == clips.ids[c, :LENGTHS[c]]).all() and got.sequences.shape == (NRET, 11)


def test_a_clips_result_does_not_depend_on_when_or_where_it_runs(runs):
    """input order [4, 2, 0, 3, 1]: every clip gets another entry time, slot and neighbour, and bit-identical results; two runs of one
    call are bit-identical"""
    for x, y in zip(runs.a.results, runs.b.results):
        assert _same_result(x, y)
    assert (runs.a.steps, runs.a.prefills, runs.a.advances) == (runs.b.steps, runs.b.prefills, runs.b.advances)
    for i, c in enumerate(runs.perm):
        assert _same_result(runs.p.results[i], runs.a.results[c]), c
        assert runs.p.advances[i] == runs.a.advances[c]


def test_a_stop_token_the_search_emits_lets_clips_leave_at_their_own_steps(tiny, clips, runs):
    """the stop token is taken from the first run: of the tokens its sequences generated, most frequent first (at most sixteen are
    tried: the tiny decoder has random weights and few tokens ever close a hypothesis store), the first that closes searches early enough to save a decode step.  Clips then leave at different steps, before their
    budgets, the results still equal the lockstep pair's, and fewer decode steps are issued than the budgets alone imply"""
    gen = torch.cat([r.sequences[:, LENGTHS[c]:].reshape(-1) for c, r in enumerate(runs.a.results)]).cpu()
    tokens, counts = torch.unique(gen[gen != STOP], return_counts=True)
    by_frequency = tokens[torch.argsort(counts, descending=True, stable=True)].tolist()[:16]
    full = _full_budget_steps(2)[0]
    assert runs.a.steps == full and runs.a.advances == [6 + 5 - pl for pl in LENGTHS]      # the default stop token closed nothing
    out = stop = None
    for stop in by_frequency:
        out = _inflight(tiny, clips, list(range(5)), stop=stop)
        print(f"    stop {stop}: advances {out.advances} steps {out.steps} prefills {out.prefills}; budgets alone {full}")
        if out.steps < full:
            break
    assert out.steps < full and len(set(out.advances)) > 1
    assert any(a < 6 + 5 - pl for a, pl in zip(out.advances, LENGTHS))
    for c in range(5):
        assert _same_result(out.results[c], _lockstep_pair(tiny, clips, c, stop=stop)), c


def test_inflight_group_search_equals_the_lockstep_pair(tiny, clips):
    kw = dict(beam_groups=2, beam_size=2, diversity_penalty=0.5, num_return_gen=4)
    out = _inflight(tiny, clips, list(range(5)), **kw)
    for c in range(5):
        want = _lockstep_pair(tiny, clips, c, **kw)
        assert out.results[c].group.tolist() == [0, 0, 1, 1] and _same_result(out.results[c], want), c


def test_inflight_search_on_fp8_weights_with_constraints(tiny, clips):
    from youku_mplug_amd.generation import LogitsConstraints
    kw = dict(decode_weights="fp8", constraints=LogitsConstraints(repetition_penalty=1.3, min_new_tokens=2))
    out = _inflight(tiny, clips, list(range(5)), **kw)
    for c in range(5):
        assert _same_result(out.results[c], _lockstep_pair(tiny, clips, c, **kw)), c
