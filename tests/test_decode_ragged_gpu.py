"""Lockstep decode over prompts of different lengths, on the GPU: mpv_attn_decode_shared_ragged_fwd (csrc/decode_shared_attention.hip)
against the fp32 softmax over each group's own keys and, bit for bit, against the uniform entry; mpv_gpt_embed_rows_w8_fwd; the ragged
generation.SharedPrefixDecodeState against uniform states run clip by clip on the tiny decoder; DistributedGPT3_Caption.generate(
mixed_prompts=True) on the caption_tiny golden."""
import copy
import types

import pytest
import torch

import decode_ragged_cases as rc
import standin_decode_shared as sd
from test_kernels_gpu import close, rel_err

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _lay(c):
    from youku_mplug_amd import ops
    return ops.AttnLayout(c["lay"].q, c["lay"].k, c["lay"].v, c["lay"].o)


def _run_ragged(c, **over):
    from youku_mplug_amd import ops
    c = {**c, **over}
    ops.attn_decode_shared_ragged_fwd(c["q"], c["k"], c["v"], c["pk"], c["pv"], c["o"], _lay(c), c["prefix_lay"], c["n_seq"], c["group_size"],
                                      c["heads"], c["prefix_len"], c["group_prefix_len"], c["own_len"], c["hd"], scale=c["scale"])
    return c["o"]


def _run_uniform(c):
    from youku_mplug_amd import ops
    sd.run_case(ops.attn_decode_shared_fwd, {**c, "lay": _lay(c)})
    return c["o"]


@pytest.mark.parametrize("case", rc.SWEEP, ids=rc.case_id)
def test_ragged_kernel_matches_the_fp32_softmax_and_the_uniform_entry(dev, case):
    """1e-2 in max-abs error over max-abs reference (the gate of test_attention_decode_step, as tests/test_decode_shared_gpu.py uses
    it); then every group, bit for bit, against the uniform entry run on that group alone with prefix_len = its length"""
    c = rc.make_case(*case, seed=3, device=dev)
    want = rc.reference(c)
    got = _run_ragged(c).clone()
    e = rel_err(got.view(c["n_seq"], c["heads"], c["hd"]), want)
    print(f"    {rc.case_id(case)}: max-abs error / max-abs ref = {e:.3e}")
    close(got.view(c["n_seq"], c["heads"], c["hd"]), want, 1e-2, rc.case_id(case))
    gs = c["group_size"]
    for g in range(len(c["lengths"])):
        alone = _run_uniform(rc.group_alone(c, g))
        assert torch.equal(alone, got[g * gs:g * gs + alone.shape[0]]), (g, c["lengths"][g])


@pytest.mark.parametrize("case", [(64, 3, 5, [264] * 3, 12, 0), (80, 1, 8, [65] * 2, 33, 3), (64, 1, 33, [33], 1, 0)], ids=rc.case_id)
def test_equal_lengths_are_the_uniform_entry_bit_for_bit(dev, case):
    c = rc.make_case(*case, seed=4, device=dev)
    ragged = _run_ragged(c).clone()
    c["o"].zero_()
    assert torch.equal(_run_uniform(c), ragged)


@pytest.mark.parametrize("case", [rc.SWEEP[1], rc.SWEEP[2], rc.SWEEP[4]], ids=rc.case_id)
def test_rows_beyond_a_length_are_never_read(dev, case):
    """prefix rows at and beyond a group's length and suffix rows at and beyond own_len hold NaN: the output is bit-identical to the
    run with zeros there"""
    zero = _run_ragged(rc.make_case(*case, seed=5, device=dev))
    nan = _run_ragged(rc.make_case(*case, seed=5, device=dev, prefix_pad=float("nan"), suffix_pad=float("nan")))
    assert torch.isfinite(nan.float()).all() and torch.equal(zero, nan)


def test_a_length_outside_its_range_is_clamped_into_the_group_s_rows(dev):
    """0 and a negative length read one row, a length above the bound reads the bound's rows: never another group's"""
    case = (64, 1, 5, [40, 40, 40], 2, 0)
    c = rc.make_case(*case, seed=6, device=dev)
    bad = torch.tensor([0, 10 ** 6, -5], dtype=torch.int32, device=dev)
    got = _run_ragged(c, group_prefix_len=bad).clone()
    c["o"].zero_()
    want = _run_ragged(c, group_prefix_len=torch.tensor([1, 40, 1], dtype=torch.int32, device=dev))
    assert torch.equal(got, want)


def test_ragged_refusals_leave_the_output_untouched(dev):
    from youku_mplug_amd import _lib
    c = rc.make_case(64, 3, 5, [33, 20, 7], 4, device=dev)
    c["o"].fill_(7.0)
    for over in (dict(group_prefix_len=None), dict(hd=96), dict(own_len=0)):
        with pytest.raises(_lib.MpvError):
            _run_ragged(c, **over)
    torch.cuda.synchronize()
    assert (c["o"] == 7.0).all()


@pytest.mark.parametrize("rows,H", [(7, 64), (33, 2048)])
def test_embed_rows_w8_is_the_dequantised_row_plus_the_position_row(dev, rows, H):
    from youku_mplug_amd import ops
    g = torch.Generator().manual_seed(rows + H)
    vocab, max_pos = 50, 40
    wte = (torch.randn(vocab, H, generator=g) * 0.3).to(BF).to(dev)
    wpe = (torch.randn(max_pos, H, generator=g) * 0.3).to(BF).to(dev)
    ids = torch.randint(0, vocab, (rows,), generator=g).to(dev)
    pos_host = torch.randint(0, max_pos, (rows,), generator=g).tolist()
    pos_host[0], pos_host[-1] = 0, max_pos - 1
    pos = torch.tensor(pos_host, dtype=torch.int32, device=dev)
    codes, scale = ops.quantize_rows_e4m3(wte)
    deq = (codes.view(torch.float8_e4m3fn).float() * scale[:, None]).to(BF)
    want = (deq[ids].float() + wpe[pos.long()].float()).to(BF)
    got = ops.gpt_embed_rows_w8_fwd(ids, pos, pos_host, codes, scale, wpe, rows, H)
    assert got.shape == (rows, H) and torch.equal(got, want)
    # the uniform FP8 embedding of one row per sequence at one position: the same conversion, bit for bit
    h = torch.empty((rows, H), dtype=BF, device=dev)
    from youku_mplug_amd import _lib
    ops.check(_lib.lib().mpv_gpt_embed_w8_fwd(None, ids.data_ptr(), codes.data_ptr(), scale.data_ptr(), wpe[5:].data_ptr(), h.data_ptr(), rows, 0, 1,
                                              H, ops._stream()), "mpv_gpt_embed_w8_fwd")
    five = torch.full((rows,), 5, dtype=torch.int32, device=dev)
    assert torch.equal(ops.gpt_embed_rows_w8_fwd(ids, five, [5] * rows, codes, scale, wpe, rows, H), h)


# ------------------------------------------------------------------------------------------------ the state on the tiny decoder
@pytest.fixture(scope="module")
def state_runs(dev):
    """the ragged state case once for the module: the reference logits (uniform states clip by clip), two ragged runs and one with
    the pad rows' KV poisoned; nothing here is modified by the tests"""
    from test_decode_shared_cpu import _tiny_decoder
    cfg, gpt = _tiny_decoder(dev)
    qe, prompt, toks = rc.state_inputs(cfg, dev)
    want = rc.run_uniform_states(gpt, dev, qe, prompt, toks)
    a, st = rc.run_ragged_state(gpt, dev, qe, prompt, toks)
    b, _ = rc.run_ragged_state(gpt, dev, qe, prompt, toks)
    p, _ = rc.run_ragged_state(gpt, dev, qe, prompt, toks, poison=True)
    return types.SimpleNamespace(cfg=cfg, gpt=gpt, inputs=(qe, prompt, toks), want=want, a=a, b=b, poisoned=p, state=st)


def test_ragged_state_matches_uniform_states_clip_by_clip(state_runs):
    """prefill, two steps, three steps after in-group re-orders: every call's logits within 1e-2 (the project's KV-cache gate) of
    uniform SharedPrefixDecodeStates run clip by clip; two ragged states are bit-identical"""
    r = state_runs
    G, K = len(rc.PROMPTS), rc.FAN
    assert len(r.a) == len(r.want) == 6
    for i, (got, want, again) in enumerate(zip(r.a, r.want, r.b)):
        assert got.shape == want.shape == (G * K, r.cfg.vocab) and got.dtype == BF
        for c in range(G):
            e = rel_err(got[c * K:(c + 1) * K], want[c * K:(c + 1) * K])
            print(f"    call {i} clip {c} (prompt {rc.PROMPTS[c]}): ragged vs uniform logits {e:.3e}")
            assert e <= 1e-2, (i, c, e)
        assert torch.equal(got, again), i
    st = r.state
    assert st.P == rc.Q + max(rc.PROMPTS) and st.t == 5 and st.group_prefix_len.tolist() == [rc.Q + n for n in rc.PROMPTS]
    assert st.kv_bytes() == r.cfg.layers * (G * st.P + 2 * G * K * rc.STEPS) * 3 * r.cfg.hidden * 2


def test_the_pad_rows_of_the_prefill_are_never_read(state_runs):
    """the KV the prefill wrote for the pad rows behind each prompt, overwritten with NaN: every logit unchanged, bit for bit"""
    for i, (a, p) in enumerate(zip(state_runs.a, state_runs.poisoned)):
        assert torch.isfinite(p.float()).all() and torch.equal(a, p), i


def test_ragged_state_on_fp8_weights_is_the_dequantised_model(state_runs):
    """weights="fp8" against bf16 ragged states on a copy of the decoder with dequantized_state_dict() loaded: 1e-2, as
    tests/test_w8_gpu.py gates the FP8 steps; two FP8 states are bit-identical"""
    r = state_runs
    gpt = copy.deepcopy(r.gpt)
    twin = copy.deepcopy(r.gpt)
    twin.load_state_dict(gpt.dequantized_state_dict(), strict=False)
    got, _ = rc.run_ragged_state(gpt, r.inputs[0].device, *r.inputs, weights="fp8")
    again, _ = rc.run_ragged_state(gpt, r.inputs[0].device, *r.inputs, weights="fp8")
    want, _ = rc.run_ragged_state(twin, r.inputs[0].device, *r.inputs)
    for i, (a, b, w) in enumerate(zip(got, again, want)):
        e = rel_err(a, w)
        print(f"    call {i}: fp8 ragged vs dequantised bf16 ragged logits {e:.3e}")
        assert e <= 1e-2, (i, e)
        assert torch.equal(a, b), i


# ------------------------------------------------------------------------------------------------ the caption model
def _spied(model):
    """-> (calls, restore): every beam_search / beam_search_batched call of the model's decoder, recorded"""
    td = model.text_decoder
    calls = types.SimpleNamespace(plain=[], batched=[])
    orig, orig_b = td.beam_search, td.beam_search_batched

    def spy(*a, **k):
        out = orig(*a, **k)
        calls.plain.append(out.scores[0].item())
        return out

    def spy_b(tokens, **k):
        outs = orig_b(tokens, **k)
        calls.batched.append((tokens.shape[0], k["prompt_length"], k.get("kv"), outs))
        return outs
    td.beam_search, td.beam_search_batched = spy, spy_b

    def restore():
        td.beam_search, td.beam_search_batched = orig, orig_b
    return calls, restore


def test_caption_generate_mixed_prompts_on_the_tiny_model(dev):
    """generate(batched=True, kv_cache="shared_prefix", mixed_prompts=True) on the golden's two clips (prompts of 5 and 3 tokens): ONE
    lockstep search with both clips, under the gate of test_caption_generate_shared_prefix_on_the_tiny_model -- the best hypothesis'
    score deviates from the golden's fp32 score by at most 1.5 x the larger of the reference's own bf16 deviation and the deviation
    of the unchanged per-clip generate in this run (the three numbers are printed)."""
    from test_beam_batched_gpu import _caption_model
    g, model, video, ids, mask = _caption_model(dev)
    m, f32, b16 = g["meta"], g["fp32"], g["bf16"]
    text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    calls, restore = _spied(model)
    try:
        plain = model.generate(video, text, termination_id=m["eod_id"])
        res = model.generate(video, text, termination_id=m["eod_id"], batched=True, kv_cache="shared_prefix", mixed_prompts=True)
        assert [(c[0], c[1], c[2]) for c in calls.batched] == [(2, [5, 3], "shared_prefix")]      # one search, both clips
        outs = calls.batched[0][3]
        assert len(res) == len(plain) == m["batch"]
        for i, (r, p) in enumerate(zip(res, plain)):
            ref, refb = f32["scores"][i][0].item(), b16["scores"][i][0].item()
            assert r.shape == p.shape == f32["sequences"][i].shape and r.dtype == p.dtype
            n_prompt = int(mask[i].sum()) - 1
            assert torch.equal(r[0, :n_prompt], ids[i, :n_prompt])                    # the prompt is kept, in input order
            score = outs[i].scores[0].item()
            dev_ref, dev_plain, dev_mixed = abs(refb - ref) / abs(ref), abs(calls.plain[i] - ref) / abs(ref), abs(score - ref) / abs(ref)
            print(f"    clip {i}: mixed prompts {dev_mixed:.3e} <= 1.5 * max(reference bf16 {dev_ref:.3e}, per-clip generate {dev_plain:.3e})")
            assert dev_mixed <= 1.5 * max(dev_ref, dev_plain), (i, dev_mixed, dev_ref, dev_plain)
    finally:
        restore()


def test_mixed_mode_with_equal_prompts_is_the_uniform_loop_bit_for_bit(dev):
    """beam_search_batched on three clips with EQUAL prompts: prompt_length = [5, 5, 5] against prompt_length = 5, same row count.  The
    mixed mode's table is twice as wide with cur_len doubled and the scores doubled back at the finish; both sides of every
    comparison of the advance kernel are then exactly halved, so rows AND scores equal the uniform loop's bit for bit -- plain
    search, 3-best, two beam groups and with a repetition penalty and a minimum length."""
    from test_beam_batched_gpu import _caption_model
    from youku_mplug_amd import generation
    g, model, video, ids, mask = _caption_model(dev)
    m = g["meta"]
    td = model.text_decoder
    tokens = ids[[0, 0, 0]].clone().to(dev)
    tokens[1, 1] = (tokens[1, 1] + 11) % 1000 + 8                       # three different clips of one prompt length
    qf = (torch.randn(3, model.num_learnable_token, model.text_width, generator=torch.Generator().manual_seed(12)) * 0.5).to(dev).to(BF)
    for extra in (dict(), dict(num_return_gen=3), dict(beam_groups=2, diversity_penalty=1.5, beam_size=3, num_return_gen=4),
                  dict(constraints=generation.LogitsConstraints(repetition_penalty=1.3, min_new_tokens=4))):
        kw = dict(query_embeds=qf.contiguous(), stop_token=m["eod_id"], kv="shared_prefix", **extra)
        want = td.beam_search_batched(tokens, prompt_length=5, **kw)
        got = td.beam_search_batched(tokens, prompt_length=[5, 5, 5], **kw)
        assert len(got) == len(want) == 3
        for a, b in zip(got, want):
            assert a.sequences.shape == b.sequences.shape and torch.equal(a.sequences, b.sequences), extra
            assert torch.equal(a.scores, b.scores), (extra, a.scores, b.scores)
            if "beam_groups" in extra:
                assert torch.equal(a.group, b.group)


def _aba(ids, mask, video, dev):
    """clips [A, B, A] and [A, C, A]: A the golden's clip with the 3-token prompt, B and C two different clips with 5-token prompts"""
    a_ids, a_mask, b_ids, b_mask = ids[1], mask[1], ids[0], mask[0]
    c_ids = b_ids.clone()
    c_ids[1] = (c_ids[1] + 11) % 1000 + 8
    def text(mid):
        return types.SimpleNamespace(input_ids=torch.stack([a_ids, mid, a_ids]).to(dev), attention_mask=torch.stack([a_mask, b_mask, a_mask]).to(dev))
    return (video[[1, 0, 1]], text(b_ids)), (video[[1, 1, 1]], text(c_ids))


@pytest.mark.parametrize("extra", [dict(), dict(beam_groups=2, diversity_penalty=1.5, beam_size=3, num_return_gen=4), dict(no_repeat_ngram_size=2)],
                         ids=["plain", "beam_groups2", "no_repeat_ngram2"])
def test_a_clip_does_not_depend_on_its_longer_neighbour(dev, extra):
    """[A, B, A] and [A, C, A] with B and C equally long and longer than A, one mixed search each: A's rows and scores are bit-identical
    in all four places -- neither the neighbour's content nor A's place in the chunk reaches them.  Also with two beam groups and
    with no_repeat_ngram_size=2 (the constraint kernel on the left-padded table)."""
    from test_beam_batched_gpu import _caption_model
    g, model, video, ids, mask = _caption_model(dev)
    m = g["meta"]
    calls, restore = _spied(model)
    try:
        kw = dict(termination_id=m["eod_id"], batched=True, kv_cache="shared_prefix", mixed_prompts=True, **extra)
        cases = _aba(ids, mask, video, dev)
        results = [model.generate(v, t, **kw) for v, t in cases]
        assert [(c[0], c[1]) for c in calls.batched] == [(3, [3, 5, 3]), (3, [3, 5, 3])]
        places = [(results[s][i], calls.batched[s][3][i]) for s in range(2) for i in (0, 2)]
        rows0, ns0 = places[0]
        n_rows = extra.get("num_return_gen", 1)
        assert rows0.shape == (n_rows, ids.shape[1] + m["tokens_to_generate"]) and (rows0[:, :3] == ids[1, :3]).all()
        for rows, ns in places[1:]:
            assert torch.equal(rows, rows0) and torch.equal(ns.scores, ns0.scores)
            if "beam_groups" in extra:
                assert torch.equal(ns.group, ns0.group) and ns.group.tolist() == [0, 0, 1, 1]
        for s, (_, t) in enumerate(cases):
            mid = results[s][1]
            assert mid.shape == rows0.shape and (mid[:, :5] == t.input_ids[1, :5].cpu()).all()      # the neighbour keeps ITS prompt
    finally:
        restore()
