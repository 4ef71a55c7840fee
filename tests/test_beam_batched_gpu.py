"""Lockstep beam search over a batch of clips, on the GPU: mpv_beam_advance (csrc/beam_search.hip: the groups = 1 case of the kernel it
shares with mpv_beam_advance_groups) against its restatement tests/standin_beam.py bit for bit, its refusals, the stub-driven search
of tests/test_beam_batched_cpu.py on the real kernel against the reference's golden, DistributedGPT3_Caption.generate(batched=True) on
the tiny model, and DecodeState.prefill_fan_out."""
import os
import re
import types

import pytest
import torch

import standin_beam

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STOP = 7


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _candidates(g, B, K, V, step):
    """[B * K, 2K] candidates as mpv_logprob_topk writes them (distinct tokens per row, value descending, ties to the lower token).  The
    values are multiples of 0.25 in a narrow range, so ties occur within and across beams.  Forced per clip and step: the stop token as
    the clip's best candidate (rank 0 < K: a hypothesis is added; its value 1 + 0.25 * ((step + 1) // 2) repeats, so the store sees
    additions, refusals of an equal score, evictions and evictions with tied scores, and positive values keep the done test false); on
    even steps after the first and K >= 2 a second stop token from the last beam at rank exactly K (skipped), behind K - 1 tied others."""
    rows, K2 = B * K, 2 * K
    tok = torch.stack([torch.randperm(V, generator=g)[:K2] for _ in range(rows)])
    val = -0.25 * torch.randint(1, 9, (rows, K2), generator=g).float() - 0.5 * step

    def put_stop(row, col, v):
        at = (tok[row] == STOP).nonzero()
        if len(at):
            tok[row, at[0, 0]] = tok[row, col]
        tok[row, col], val[row, col] = STOP, v
    top = 1.0 + 0.25 * ((step + 1) // 2)
    for b in range(B):
        lo, hi = b * K, b * K + K - 1
        put_stop(lo, 0, top)
        if step % 2 == 0 and step > 0 and K >= 2:
            put_stop(hi, K - 1, top - 0.5)
            val[hi, :K - 1] = top - 0.25
    order = torch.argsort(val * -1e4 + tok.float(), dim=1, stable=True)      # value descending, then token ascending
    return torch.gather(val, 1, order).contiguous(), torch.gather(tok, 1, order).contiguous()


@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_kernel_equals_the_standin_bit_for_bit(dev, K):
    """6 consecutive steps (the `first` step included) of B = 3 clips, V = 37, Lt = 12; one clip is made done before step 2.  Every
    state array and both outputs are compared after every step."""
    from youku_mplug_amd import ops
    from youku_mplug_amd.generation import BeamState
    B, V, Lt, P = 3, 37, 12, 3
    g = torch.Generator().manual_seed(100 + K)
    prompt = torch.randint(0, V, (B, Lt), generator=g)
    ref, mine = BeamState(prompt, K), BeamState(prompt.to(dev), K)
    added = 0
    for step in range(6):
        if step == 2:
            ref.done[1] = 1
            mine.done[1] = 1
        val, tok = _candidates(g, B, K, V, step)
        kw = dict(vocab=V, pos=P + step, cur_len=step + 1, first=step == 0, stop_token=STOP)
        before = int(ref.hyp_next.sum())
        standin_beam.beam_advance(val, tok, ref, **kw)
        ops.beam_advance(val.to(dev), tok.to(dev), mine, **kw)
        added += int(ref.hyp_next.sum()) - before
        for n in BeamState.ARRAYS + ("tokens_alt",):
            a, b = getattr(mine, n).cpu(), getattr(ref, n)
            assert a.dtype == b.dtype and torch.equal(a, b), (K, step, n, a.tolist(), b.tolist())
        assert torch.equal(ref.src_row // K, torch.arange(B * K) // K)          # a source row never leaves its clip
    assert int(ref.done[1]) == 1 and int(ref.done[0]) == 0 and int(ref.done[2]) == 0          # only the clip that was made done
    assert added > 2 * min(K, 6) and int(ref.hyp_count[0]) == min(K, 6)                        # additions, and evictions where K < 6


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("B", [1, 33])
def test_plain_entry_equals_the_standin_at_the_row_copy_and_rank_edges(dev, K, B):
    """mpv_beam_advance runs the kernel it shares with mpv_beam_advance_groups (groups = 1); tests/standin_beam.py shares no code with
    it.  row_len 63 / 64 / 65 / 130 lie below, at, one over and two passes over the 64-lane row copies, K = 8 ranks 128 candidates,
    B = 33 is more than one workgroup and an odd count.  4 steps from `first`, one clip made done before step 2 where B > 1; every
    state array and tokens_alt bit for bit after every step (no tolerance: both sides are exact)."""
    from youku_mplug_amd import ops
    from youku_mplug_amd.generation import BeamState
    V, P = 37, 3
    for Lt in (63, 64, 65, 130):
        g = torch.Generator().manual_seed(1000 * K + 10 * B + Lt)
        prompt = torch.randint(0, V, (B, Lt), generator=g)
        ref, mine = BeamState(prompt, K), BeamState(prompt.to(dev), K)
        for step in range(4):
            if step == 2 and B > 1:
                ref.done[1] = 1
                mine.done[1] = 1
            val, tok = _candidates(g, B, K, V, step)
            kw = dict(vocab=V, pos=P + step, cur_len=step + 1, first=step == 0, stop_token=STOP)
            standin_beam.beam_advance(val, tok, ref, **kw)
            ops.beam_advance(val.to(dev), tok.to(dev), mine, **kw)
            for n in BeamState.ARRAYS + ("tokens_alt",):
                a, b = getattr(mine, n).cpu(), getattr(ref, n)
                assert a.dtype == b.dtype and torch.equal(a, b), (K, B, Lt, step, n)
        assert int(ref.hyp_next.sum()) >= B and int(ref.done.sum()) == (1 if B > 1 else 0)      # hypotheses were added; only the clip made done is


@pytest.mark.parametrize("K,Lt", [(9, 12), (4, 4096)])
def test_refusals_leave_the_outputs_untouched(dev, K, Lt):
    from youku_mplug_amd import _lib, ops
    from youku_mplug_amd.generation import BeamState
    st = BeamState(torch.randint(0, 37, (2, Lt), generator=torch.Generator().manual_seed(1)).to(dev), K)
    st.src_row.fill_(-5)
    st.next_tok.fill_(-6)
    st.tokens_alt.fill_(-7)
    before = {n: getattr(st, n).clone() for n in BeamState.ARRAYS + ("tokens_alt",)}
    tokens_id = id(st.tokens)
    val = torch.zeros((2 * K, 2 * K), dtype=torch.float32, device=dev)
    tok = torch.arange(2 * K, device=dev).repeat(2 * K, 1)
    with pytest.raises(_lib.MpvError) as e:
        ops.beam_advance(val, tok, st, vocab=37, pos=3, cur_len=1, first=True, stop_token=STOP)
    assert re.search(r"failed \(-\d+\)", str(e.value)), str(e.value)
    torch.cuda.synchronize()
    assert id(st.tokens) == tokens_id
    for n, t in before.items():
        assert torch.equal(getattr(st, n), t), n


@pytest.mark.parametrize("Q", [0, 3])
def test_stub_driven_search_on_the_real_kernel_matches_the_golden(dev, Q):
    """The CPU suite's stub-driven batch of seeds (1, 2, 3, 4) with the bookkeeping on the device: candidates computed by torch in fp32
    on the device, ops.beam_advance as the advance_fn, the stub state downloading the step's tokens."""
    import test_beam_batched_cpu as tc
    from oracle.gen_golden import StubLogits
    from youku_mplug_amd import generation, ops
    seeds = (1, 2, 3, 4)
    vocab, cfg, tokens = tc._case(Q)
    stubs = [StubLogits(vocab=vocab, stop=STOP, seed=s) for s in seeds]

    class DevStub(tc._BatchedStubState):
        def prefill_fan_out(self, tokens, query_embeds, fan):
            return super().prefill_fan_out(tokens.cpu(), query_embeds, fan).to(dev)

        def step(self, tokens, query_embeds=None):
            return super().step(tokens.cpu(), query_embeds).to(dev)

        def reorder(self, idx, shared_prefix=0):
            super().reorder(idx.cpu(), shared_prefix)
    qe = torch.zeros(len(seeds), Q, 4, device=dev) if Q else None
    out = generation.beam_search_batched_loop(cfg, lambda b, m: DevStub(stubs, b, m), tokens.repeat(len(seeds), 1).to(dev), query_embeds=qe,
                                              beam_size=tc.K, num_return_gen=tc.N_RET, prompt_length=tc.PROMPT, topk_fn=tc._torch_topk,
                                              advance_fn=ops.beam_advance)
    tc._check_against_golden([types.SimpleNamespace(sequences=o.sequences.cpu(), scores=o.scores.cpu()) for o in out], seeds, Q)


def _caption_model(dev):
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict
    from youku_mplug_amd.downstream import synthetic_gencls_model
    g = torch.load(os.path.join(GOLD, "caption_tiny.pt"))
    m = g["meta"]
    model = synthetic_gencls_model(CONFIG_TINY, "caption", device=dev)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in make_state_dict(CONFIG_TINY, m["weight_seed"]).items()}, strict=True)
    model.text_decoder.config.extra.update(tokens_to_generate=m["tokens_to_generate"], eod_id=m["eod_id"])
    video, ids, mask = make_inputs(CONFIG_TINY, m["batch"], m["text_len"], seed=m["input_seed"], ragged=False)
    mask[1, 4:] = 0
    return g, model, video.to(dev).to(torch.bfloat16), ids, mask


def test_caption_generate_batched_on_the_tiny_model(dev):
    """generate(batched=True) on the golden's two clips (ragged prompts: two groups).  Gate on the best hypothesis' score against the
    golden's fp32 score: 1.5 x the larger of the reference's own bf16 deviation (stored in the golden) and the deviation of the unchanged
    per-clip generate in this run; both are printed.  Random weights make near-ties and the GEMM dispatch depends on the row count, so
    token equality with the per-clip path is not asserted.  Then the same clip three times in one search: bit-identical results, equal to
    that clip's result next to a different neighbour."""
    g, model, video, ids, mask = _caption_model(dev)
    m, f32, b16 = g["meta"], g["fp32"], g["bf16"]
    text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    td = model.text_decoder
    plain_scores, batched = [], []
    orig, orig_b = td.beam_search, td.beam_search_batched

    def spy(*a, **k):
        out = orig(*a, **k)
        plain_scores.append(out.scores[0].item())
        return out

    def spy_b(tokens, **k):
        outs = orig_b(tokens, **k)
        batched.append((tokens.shape[0], k["prompt_length"], [o.scores[0].item() for o in outs], outs))
        return outs
    td.beam_search, td.beam_search_batched = spy, spy_b
    try:
        plain = model.generate(video, text, termination_id=m["eod_id"])
        res = model.generate(video, text, termination_id=m["eod_id"], batched=True)
        assert [(c[0], c[1]) for c in batched] == [(1, 3), (1, 5)]                 # two prompt lengths: two groups
        scores = {0: batched[1][2][0], 1: batched[0][2][0]}
        assert len(res) == len(plain) == m["batch"]
        for i, (r, p) in enumerate(zip(res, plain)):
            ref, refb = f32["scores"][i][0].item(), b16["scores"][i][0].item()
            assert r.shape == p.shape == f32["sequences"][i].shape and r.dtype == p.dtype
            n_prompt = int(mask[i].sum()) - 1
            assert torch.equal(r[0, :n_prompt], ids[i, :n_prompt])                    # the prompt is kept, in input order
            dev_ref, dev_plain, dev_batched = abs(refb - ref) / abs(ref), abs(plain_scores[i] - ref) / abs(ref), abs(scores[i] - ref) / abs(ref)
            print(f"    clip {i}: batched {dev_batched:.3e} <= 1.5 * max(reference bf16 {dev_ref:.3e}, per-clip generate {dev_plain:.3e})")
            assert dev_batched <= 1.5 * max(dev_ref, dev_plain), (i, dev_batched, dev_ref, dev_plain)
        # one clip three times / next to a different neighbour (same row count, so the same GEMM dispatch)
        ids0, mask0 = ids[[0, 0, 0]].to(dev), mask[[0, 0, 0]].to(dev)
        text0 = types.SimpleNamespace(input_ids=ids0, attention_mask=mask0)
        batched.clear()
        same = model.generate(video[[0, 0, 0]], text0, termination_id=m["eod_id"], batched=True)
        other = model.generate(video[[0, 1, 0]], text0, termination_id=m["eod_id"], batched=True)
        assert [(c[0], c[1]) for c in batched] == [(3, 5), (3, 5)]
        (_, _, s_same, o_same), (_, _, s_other, o_other) = batched
        assert torch.equal(same[0], same[1]) and torch.equal(same[0], same[2]) and s_same[0] == s_same[1] == s_same[2]
        assert torch.equal(o_same[0].scores, o_same[1].scores) and torch.equal(o_same[0].scores, o_same[2].scores)
        assert torch.equal(other[0], same[0]) and torch.equal(other[2], same[0]) and s_other[0] == s_other[2] == s_same[0]
    finally:
        td.beam_search, td.beam_search_batched = orig, orig_b


def test_prefill_fan_out_matches_a_prefill_on_repeated_rows(dev):
    """Prefill at B = 2 + fan-out to K = 3 against a prefill at batch 6 on repeated rows: the logits of the prefill and of the next two
    steps agree within 1e-2 (the gate of test_kv_cache_decode_matches_full_forward); after re-orders with and without shared_prefix
    two fanned-out states stay bit-identical to each other."""
    from oracle.weights import CONFIG_TINY, make_state_dict
    from youku_mplug_amd.generation import DecodeState
    from youku_mplug_amd.pretrain import synthetic_model
    cfg = CONFIG_TINY
    model = synthetic_model(cfg, device=dev)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in make_state_dict(cfg, 6).items()}, strict=True)
    model.eval()
    gpt = model.text_decoder
    B, K, Q, P, H = 2, 3, 8, 3, cfg.hidden
    g = torch.Generator().manual_seed(21)
    qe = (torch.randn(B, Q, H, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    prompt = torch.randint(0, cfg.vocab, (B, P), generator=g).to(dev)
    fan, fan2, rep = (DecodeState(gpt, B * K, Q + P + 6) for _ in range(3))
    la, la2 = fan.prefill_fan_out(prompt, qe, K), fan2.prefill_fan_out(prompt, qe, K)
    lb = rep.step(prompt.repeat_interleave(K, 0).contiguous(), qe.repeat_interleave(K, 0).contiguous())
    assert la.shape == lb.shape and torch.equal(la, la2) and fan.pos == rep.pos == Q + P
    assert torch.equal(la[0], la[K - 1]) and torch.equal(la[K], la[2 * K - 1])
    assert rel(la, lb) <= 1e-2
    for t in range(2):
        tok = torch.randint(0, cfg.vocab, (B * K, 1), generator=g).to(dev)
        la, la2, lb = fan.step(tok), fan2.step(tok), rep.step(tok)
        assert rel(la, lb) <= 1e-2, t
        assert torch.equal(la, la2), t
    for t, perm in enumerate([[0, 0, 1, 5, 3, 3], [2, 1, 1, 4, 4, 3], [1, 2, 0, 3, 5, 4]]):      # sources stay inside their group of K
        perm = torch.tensor(perm, device=dev)
        fan.reorder(perm)                                   # whole cache
        fan2.reorder(perm, shared_prefix=Q + P)             # generated rows only
        rep.reorder(perm)
        tok = torch.randint(0, cfg.vocab, (B * K, 1), generator=g).to(dev)
        la, la2, lb = fan.step(tok), fan2.step(tok), rep.step(tok)
        assert torch.equal(la, la2), t
        assert rel(la, lb) <= 1e-2, t
