"""Diverse (group) beam search in lockstep, on the GPU: mpv_beam_advance_groups (csrc/beam_search.hip, the kernel it shares with
mpv_beam_advance) against its restatement tests/standin_beam_groups.py bit for bit on every state array, against mpv_beam_advance at one group, its refusals, the stub-driven
search of tests/test_beam_groups_cpu.py on the real kernel against the reference's golden, the exact statements that hold on the tiny
model in both KV modes, and the re-ranked scores of DistributedGPT3_Caption.generate(rerank_by_logprob=True) against the fp32
restatement under section 20's gate."""
import itertools
import re
import types

import pytest
import torch

import beam_groups_cases as bg
import caption_score_cases as cs
import standin_beam_groups as sg

pytestmark = pytest.mark.gpu
VOCAB, STOP = 41, 7
BATCHES, ROW_LENS, LAMBDAS = (1, 3, 33), (1, 63, 64, 65, 130), (0.0, 0.5, 1e4)


def _special(B, G):
    """(frozen, finishing) pseudo-clips: a frozen group between two live ones where there are three groups, and a group that becomes
    done in the call in front of a live group of its clip"""
    if G == 1:
        return ((1,) if B > 1 else ()), ((2,) if B > 2 else ())
    frozen = (1,) if G >= 3 else ()
    return frozen, ((B - 1) * G,)


@pytest.mark.parametrize("K,G", [(1, 2), (1, 8), (2, 4), (4, 2), (8, 2), (5, 1), (2, 8)])
def test_kernel_equals_the_restatement_bit_for_bit(dev, K, G):
    """batch {1, 3, 33} x row_len {1, 63, 64, 65, 130} (the 64-lane row copies) x first on / off x lambda {0, 0.5, 1e4}: 90 cases per
    (K', G).  Every case has tied values within and across beams, stop tokens at ranks below and at K', a frozen group between live ones
    (G >= 3), a group that becomes done in the call in front of a live one, rows of -inf candidates, and hypothesis stores -- about
    half of them full -- whose scores lie on the grid of the candidates' scores: additions, refusals below and AT `worst`, evictions
    and (K' > 1) evictions out of a store whose lowest score is tied, counted below.  All state arrays and outputs, bit for bit; at
    G = 1 also against mpv_beam_advance."""
    from youku_mplug_amd import ops
    events = [0, 0, 0]
    for idx, (B, Lt, first, lam) in enumerate(itertools.product(BATCHES, ROW_LENS, (True, False), LAMBDAS)):
        frozen, finishing = _special(B, G)
        pos = (0, Lt - 1, Lt // 2)[idx % 3]
        rows = B * G * K
        st, vals, idxs = bg.random_state(B, G, K, Lt, vocab=VOCAB, stop=STOP, pos=pos, seed=1000 * K + 37 * G + idx, first=first, frozen=frozen,
                                         finishing=finishing, banned_rows=(rows - 1, 0) if idx % 4 == 1 else (rows - 1,))
        ref, mine = bg.clone_state(st), bg.clone_state(st, dev)
        step = dict(groups=G, diversity_penalty=lam, vocab=VOCAB, pos=pos, cur_len=Lt, first=first, stop_token=STOP)
        sg.beam_advance_groups(vals, idxs, ref, **step)
        ops.beam_advance_groups(vals.to(dev), idxs.to(dev), mine, **step)
        bg.assert_states_equal(mine, ref, (K, G, B, Lt, first, lam))
        events = [a + b for a, b in zip(events, bg.store_events(st, ref))]
        assert torch.equal(ref.src_row // K, torch.arange(rows) // K)              # a source row never leaves its (clip, group)
        for p in finishing:
            assert int(ref.done[p]) == 1 and p not in frozen
        if G == 1:
            plain = bg.clone_state(st, dev)
            ops.beam_advance(vals.to(dev), idxs.to(dev), plain, vocab=VOCAB, pos=pos, cur_len=Lt, first=first, stop_token=STOP)
            bg.assert_states_equal(mine, plain, ("G = 1", K, B, Lt, first, lam))
    print(f"    (K', G) = ({K}, {G}): additions {events[0]}, evictions {events[1]}, of them out of a tied lowest score {events[2]}")
    assert events[0] > events[1] > 100 and (K == 1 or events[2] > 0), events


@pytest.mark.parametrize("K", [1, 2, 8])
def test_one_group_equals_mpv_beam_advance_bit_for_bit(dev, K):
    from youku_mplug_amd import ops
    events = [0, 0, 0]
    for idx, (B, Lt, first, lam) in enumerate(((3, 65, True, 0.5), (33, 12, False, 1e4), (1, 130, False, 0.0), (17, 5, False, 2.0))):
        frozen, finishing = _special(B, 1)
        st, vals, idxs = bg.random_state(B, 1, K, Lt, vocab=VOCAB, stop=STOP, pos=Lt // 3, seed=77 * K + idx, first=first, frozen=frozen,
                                         finishing=finishing)
        a, b = bg.clone_state(st, dev), bg.clone_state(st, dev)
        step = dict(vocab=VOCAB, pos=Lt // 3, cur_len=Lt, first=first, stop_token=STOP)
        ops.beam_advance(vals.to(dev), idxs.to(dev), a, **step)
        ops.beam_advance_groups(vals.to(dev), idxs.to(dev), b, groups=1, diversity_penalty=lam, **step)
        bg.assert_states_equal(a, b, (K, idx))
        events = [x + y for x, y in zip(events, bg.store_events(st, a))]
    assert events[0] > events[1] > 0, events                                       # additions and evictions went through both kernels


@pytest.mark.parametrize("over", [dict(K=9, G=1), dict(G=9, K=1), dict(K=5, G=4), dict(K=8, G=3), dict(lam=-1.0), dict(lam=float("nan")),
                                  dict(lam=float("inf")), dict(Lt=4096), dict(pos=12), dict(pos=-1), dict(cur_len=0), dict(vocab=0)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_refusals_leave_the_outputs_untouched(dev, over):
    from youku_mplug_amd import _lib, ops
    from youku_mplug_amd.generation import BeamState
    c = dict(dict(K=2, G=2, lam=0.5, Lt=12, pos=3, cur_len=1, vocab=37), **over)
    K, G = c["K"], c["G"]
    st = BeamState(torch.randint(0, 37, (2 * G, c["Lt"]), generator=torch.Generator().manual_seed(1)).to(dev), K)
    for n in ("src_row", "next_tok", "tokens_alt", "scores", "hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "hyp_next", "worst"):
        getattr(st, n).fill_(bg.CANARY[getattr(st, n).dtype])
    before = {n: getattr(st, n).clone() for n in bg.STATE_ARRAYS}
    tokens_id = id(st.tokens)
    rows, m = 2 * G * K, (G + 1) * K
    val = torch.zeros((rows, m), dtype=torch.float32, device=dev)
    tok = torch.arange(m, device=dev).repeat(rows, 1)
    with pytest.raises(_lib.MpvError) as e:
        ops.beam_advance_groups(val, tok, st, groups=G, diversity_penalty=c["lam"], vocab=c["vocab"], pos=c["pos"], cur_len=c["cur_len"], first=True,
                                stop_token=STOP)
    assert re.search(r"failed \(-\d+\)", str(e.value)), str(e.value)
    torch.cuda.synchronize()
    assert id(st.tokens) == tokens_id
    for n, t in before.items():
        assert torch.equal(getattr(st, n), t), n


@pytest.mark.parametrize("Q", [0, 3])
def test_stub_driven_group_search_on_the_real_kernel_matches_the_golden(dev, Q):
    """The CPU suite's anchor with the bookkeeping on the device: seeds (1, 2, 3, 4) as one batch, beam_groups 2 x beam_size 4 at
    diversity_penalty 0, 6 returned: every group of every clip is the reference's beam_search (beam 4, 3 returned).  Stub logits
    have no KV memory, so neither real KV state runs here: the stub state only asserts what both of them rely on (a source row never
    leaves its clip, the promised shared prefix is shared).  The two real KV states, "per_sequence" and "shared_prefix", run under the
    group search in test_exact_statements_on_the_tiny_model below."""
    import test_beam_batched_cpu as tc
    import test_beam_groups_cpu as tg
    from oracle.gen_golden import StubLogits
    from youku_mplug_amd import ops
    seeds = (1, 2, 3, 4)
    vocab, _, _ = tc._case(Q)
    stubs = [StubLogits(vocab=vocab, stop=STOP, seed=s) for s in seeds]

    class DevStub(tc._BatchedStubState):
        def prefill_fan_out(self, tokens, query_embeds, fan):
            return super().prefill_fan_out(tokens.cpu(), query_embeds, fan).to(dev)

        def step(self, tokens, query_embeds=None):
            return super().step(tokens.cpu(), query_embeds).to(dev)

        def reorder(self, idx, shared_prefix=0):
            super().reorder(idx.cpu(), shared_prefix)
    out = tg.run_stub_groups(seeds, Q, advance=ops.beam_advance_groups, make_state=lambda b, m: DevStub(stubs, b, m), device=dev)
    tg.check_groups_against_golden([types.SimpleNamespace(sequences=o.sequences.cpu(), scores=o.scores.cpu(), group=o.group.cpu()) for o in out],
                                   seeds, Q)


@pytest.mark.parametrize("kv", ["per_sequence", "shared_prefix"])
def test_exact_statements_on_the_tiny_model(dev, kv):
    """Statements that need no tolerance (the lockstep kernels give a row the same bits wherever it stands, at an equal row count):
    at lambda = 0 all groups of a clip return identical sequences and scores; at lambda > 0 group 0 equals group 0 of the lambda = 0 run
    of the same shape; the same clip twice in one batch and next to a different neighbour gives identical results.  Token equality with
    a plain K'-beam search is NOT asserted: the row count differs, and the GEMM dispatch moves near-ties."""
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    term = g["meta"]["eod_id"]
    vid = video.to(dev).to(torch.bfloat16)
    K, G, pl = 2, 3, 5
    td = model.text_decoder

    def search(sel, lam):
        qf = model.encode_video(vid[sel]).view(len(sel), -1, model.text_width)
        return td.beam_search_batched(ids[[0] * len(sel)].to(dev), query_embeds=qf.contiguous(), beam_size=K, num_return_gen=G * K, stop_token=term,
                                      prompt_length=pl, kv=kv, beam_groups=G, diversity_penalty=lam)
    zero, div, other = search([0, 0, 1], 0.0), search([0, 0, 1], 0.75), search([0, 1, 0], 0.75)
    for o in zero:
        assert o.group.tolist() == [x for x in range(G) for _ in range(K)] and (o.sequences[:, :pl].cpu() == ids[0, :pl]).all()
        for x in range(1, G):
            assert torch.equal(o.sequences[o.group == x], o.sequences[o.group == 0]) and torch.equal(o.scores[o.group == x], o.scores[o.group == 0])
    differs = 0
    for z, d in zip(zero, div):
        assert torch.equal(d.sequences[d.group == 0], z.sequences[z.group == 0]) and torch.equal(d.scores[d.group == 0], z.scores[z.group == 0])
        differs += int(not torch.equal(d.sequences, z.sequences))
    assert differs > 0                                                             # the penalty moved the later groups
    for a, b in ((div[0], div[1]), (div[0], other[0]), (div[0], other[2]), (div[2], other[1])):
        assert torch.equal(a.sequences, b.sequences) and torch.equal(a.scores, b.scores) and torch.equal(a.group, b.group)


def test_reranked_scores_against_the_restatement_under_the_existing_gate(dev):
    """generate(batched=True, beam_groups=2, rerank_by_logprob=True) on the golden's two clips (ragged prompts): the returned per-token
    log-probabilities against the fp32 restatement's teacher-forced ones of the same tokens, under DESIGN.md section 20's gate for that
    quantity -- at most 1.5 x the padded forward_continuation's own deviation on the same candidates + 1e-6 (measured there: 4.2e-3 for
    both).  The rows are ordered by the normalised score, the first is best_sample's choice."""
    from youku_mplug_amd.downstream import best_sample
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    term = g["meta"]["eod_id"]
    vid = video.to(dev).to(torch.bfloat16)
    text = cs.text_of(ids, mask, [0, 1], dev)
    res, scores = model.generate(vid, text, termination_id=term, batched=True, beam_groups=2, diversity_penalty=1.0, beam_size=3, num_return_gen=4,
                                 rerank_by_logprob=True)
    qf = model.encode_video(vid).view(2, -1, model.text_width)
    e_rerank = e_padded = 0.0
    for i in range(2):
        pl = int(mask[i].sum()) - 1
        sc = scores[i]
        assert res[i].shape[0] == 4 and sorted(sc["group"].tolist()) == [0, 0, 1, 1] and sc["best"] == 0
        norm = [s / float(c) for s, c in zip(sc["sum_logprob"].tolist(), sc["count"].tolist())]
        assert norm == sorted(norm, reverse=True) and best_sample(sc["sum_logprob"], sc["count"], 1.0) == 0
        cands = [row[:row.index(term)] if term in row else row for row in res[i][:, pl:].tolist()]
        assert sc["count"].tolist() == [len(c) + 1 for c in cands]
        ref = cs.restated_logprobs(("groups-gpu", i), video[i], ids[i, :pl].tolist(), cands, term, sd, cfg)
        pad = cs.padded_logprobs(model, qf[i:i + 1].contiguous(), text.input_ids[i:i + 1], pl, [cands], term)[0]
        for j, lp in enumerate(pad):
            n = len(lp)
            e_padded = max(e_padded, (lp.double() - ref[j]).abs().max().item())
            e_rerank = max(e_rerank, (sc["token_logprob"][j, :n].double() - ref[j]).abs().max().item())
    print(f"    re-ranked scores: e_rerank {e_rerank:.3e} e_padded {e_padded:.3e}")
    assert e_rerank <= 1.5 * e_padded + 1e-6, (e_rerank, e_padded)
