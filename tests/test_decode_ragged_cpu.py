"""Lockstep beam search over clips whose prompts differ in length, on CPU: generate(mixed_prompts=True) on the stand-ins
(tests/standin_decode_ragged.py) against the grouped batched=True, kv_cache="shared_prefix" call -- token-equal rows and equal scores
clip by clip --, the budget rule, the refusals, the exported symbols and what the new entries refuse on the host."""
import ctypes
import types

import pytest
import torch

import standin_decode_ragged as sr

BF = torch.bfloat16
LENGTHS = [1, 4, 4, 7, 2]
SEL = [0, 1, 0, 1, 0]
NEW_SYMBOLS = ("mpv_attn_decode_shared_ragged_fwd", "mpv_gpt_embed_rows_w8_fwd", "mpv_gpt_decode_step_shared_ragged",
               "mpv_gpt_decode_step_shared_ragged_q8", "mpv_gpt_prefill_ragged", "mpv_gpt_prefill_ragged_q8")


def _on_cpu(monkeypatch):
    import test_w8_cpu as tw
    dev = tw._on_cpu(monkeypatch)
    sr.install(monkeypatch)
    return dev


def _setup(dev, lengths=LENGTHS, width=9, tokens_to_generate=None):
    """the tiny caption model; clips SEL with prompts of `lengths` tokens in rows `width` wide (the prompt of clip i is
    input_ids[i, :mask.sum() - 1]; what lies behind it in the row is arbitrary, as a tokenizer's padding is)"""
    import caption_score_cases as cs
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    term = g["meta"]["eod_id"]
    if tokens_to_generate is not None:
        model.text_decoder.config.extra.update(tokens_to_generate=tokens_to_generate)
    gen = torch.Generator().manual_seed(77)
    ids = torch.randint(8, cfg.vocab, (len(lengths), width), generator=gen)
    mask = torch.zeros_like(ids)
    for i, n in enumerate(lengths):
        mask[i, :n + 1] = 1
    text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    return model, cfg, term, video[SEL[:len(lengths)]].to(BF), text


def _with_scores(model, monkeypatch):
    """records what every beam_search_batched call of the model got and returned: [(prompt_length, [namespace per clip])]"""
    calls = []
    gpt = model.text_decoder
    orig = gpt.beam_search_batched

    def spy(tokens, **kw):
        outs = orig(tokens, **kw)
        calls.append((kw.get("prompt_length"), outs))
        return outs
    monkeypatch.setattr(gpt, "beam_search_batched", spy)
    return calls


def _per_clip(calls, lengths, per_chunk, mixed):
    """the recorded namespaces back in input order"""
    from youku_mplug_amd.downstream import _prompt_length_chunks
    n = len(lengths)
    chunks = [list(range(c, min(c + per_chunk, n))) for c in range(0, n, per_chunk)] if mixed else \
        [chunk for _, chunk in _prompt_length_chunks(lengths, per_chunk)]
    assert len(chunks) == len(calls)
    res = [None] * n
    for chunk, (_, outs) in zip(chunks, calls):
        assert len(outs) == len(chunk)
        for i, o in zip(chunk, outs):
            res[i] = o
    return res


CASES = {
    "plain": dict(),
    "n_best": dict(num_return_gen=3),
    "groups": dict(beam_groups=2, diversity_penalty=1.5, beam_size=3, num_return_gen=4),
    "penalty_min_new": dict(repetition_penalty=1.3, min_new_tokens=4),
    "fp8": dict(decode_weights="fp8"),
}


@pytest.mark.parametrize("per_chunk", [2, 32])
@pytest.mark.parametrize("case", list(CASES))
def test_mixed_prompts_equal_the_grouped_search_on_standins(monkeypatch, case, per_chunk):
    """five clips with prompts of 1 / 4 / 4 / 7 / 2 tokens: mixed_prompts=True returns, clip by clip, the rows AND the scores of the
    grouped call; it makes one search per chunk of clips in input order, with the chunk's lengths"""
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev)
    kw = dict(termination_id=term, batched=True, kv_cache="shared_prefix", clips_per_search=per_chunk, **CASES[case])
    calls = _with_scores(model, monkeypatch)
    want = model.generate(vid, text, **kw)
    want_ns = _per_clip(calls, LENGTHS, per_chunk, mixed=False)
    assert all(isinstance(pl, int) for pl, _ in calls)
    calls.clear()
    got = model.generate(vid, text, mixed_prompts=True, **kw)
    got_ns = _per_clip(calls, LENGTHS, per_chunk, mixed=True)
    assert [pl for pl, _ in calls] == [LENGTHS[c:c + per_chunk] for c in range(0, len(LENGTHS), per_chunk)]
    assert len(got) == len(want) == len(LENGTHS)
    for i, (a, b, na, nb) in enumerate(zip(got, want, got_ns, want_ns)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (i, a, b)
        assert (a[:, :LENGTHS[i]] == text.input_ids[i, :LENGTHS[i]].cpu()).all()
        assert torch.equal(na.scores, nb.scores), (i, na.scores, nb.scores)
        assert torch.equal(na.sequences, nb.sequences)
        if "beam_groups" in CASES[case]:
            assert torch.equal(na.group, nb.group)


def test_mixed_prompts_rerank_equals_the_grouped_call_on_standins(monkeypatch):
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev)
    kw = dict(termination_id=term, batched=True, kv_cache="shared_prefix", num_return_gen=3, rerank_by_logprob=True)
    want, want_sc = model.generate(vid, text, **kw)
    got, got_sc = model.generate(vid, text, mixed_prompts=True, **kw)
    for a, b, sa, sb in zip(got, want, got_sc, want_sc):
        assert torch.equal(a, b) and sa.keys() == sb.keys()
        assert all(torch.equal(sa[k], sb[k]) if torch.is_tensor(sa[k]) else sa[k] == sb[k] for k in sa)


@pytest.mark.parametrize("ban_stop", [True, False])
def test_the_longest_prompt_runs_out_of_positions_first(monkeypatch, ban_stop):
    """tokens_to_generate = 2: the clip with the 7-token prompt has final_len - 7 = 4 positions, the one with 1 token has 10.  Every
    clip gets exactly the budget the grouped path gives it (with the stop token banned no clip is ever done: every budget ends, the
    longest prompt's first, and its beams are flushed while the others run on)."""
    from youku_mplug_amd import generation
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev, tokens_to_generate=2)
    kw = dict(termination_id=term, batched=True, kv_cache="shared_prefix", num_return_gen=2)
    if ban_stop:
        kw["min_new_tokens"] = 100
    steps = []
    orig = generation.SharedPrefixDecodeState.step
    monkeypatch.setattr(generation.SharedPrefixDecodeState, "step", lambda self, *a, **k: (steps.append(self), orig(self, *a, **k))[1])
    calls = _with_scores(model, monkeypatch)
    want = model.generate(vid, text, **kw)
    want_ns = _per_clip(calls, LENGTHS, 32, mixed=False)
    calls.clear()
    steps.clear()
    got = model.generate(vid, text, mixed_prompts=True, **kw)
    got_ns = _per_clip(calls, LENGTHS, 32, mixed=True)
    width = text.input_ids.shape[1] + 2
    if ban_stop:
        assert len(steps) == width - min(LENGTHS) - 1                  # the loop runs to the end of the SHORTEST prompt's budget
    for i, (a, b, na, nb) in enumerate(zip(got, want, got_ns, want_ns)):
        assert a.shape == (2, width) and torch.equal(a, b), (i, a, b)
        assert torch.equal(na.scores, nb.scores), (i, na.scores, nb.scores)
        if ban_stop:                                                   # every generated column is filled, none holds the stop token
            assert (a[:, LENGTHS[i]:] != term).all()


def test_mixed_prompts_refusals(monkeypatch):
    from youku_mplug_amd import generation
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev)
    ok = dict(termination_id=term, batched=True, kv_cache="shared_prefix", mixed_prompts=True)
    for bad, word in ((dict(batched=False), "batched"), (dict(do_sample=True), "do_sample"), (dict(kv_cache="per_sequence"), "shared_prefix"),
                      (dict(constrain_prompt=True, repetition_penalty=1.2), "constrain_prompt")):
        with pytest.raises(ValueError, match=word):
            model.generate(vid, text, **dict(ok, **bad))
    with pytest.raises(ValueError, match="mixed_prompts"):
        model.generate(vid, text, termination_id=term, mixed_prompts=True)              # kv_cache default: per_sequence, no batched
    gpt = model.text_decoder
    ids = text.input_ids
    with pytest.raises(ValueError, match="shared_prefix"):
        gpt.beam_search_batched(ids, prompt_length=LENGTHS, stop_token=term)             # kv="per_sequence": a DecodeState
    with pytest.raises(ValueError, match="include_prompt"):
        gpt.beam_search_batched(ids, prompt_length=LENGTHS, stop_token=term, kv="shared_prefix",
                                constraints=generation.LogitsConstraints(repetition_penalty=1.2, include_prompt=True))
    for lens in (LENGTHS[:4], [0] + LENGTHS[1:], [ids.shape[1] + 1] + LENGTHS[1:]):
        with pytest.raises(ValueError, match="prompt_length"):
            gpt.beam_search_batched(ids, prompt_length=lens, stop_token=term, kv="shared_prefix")
    gpt.config.extra.update(tokens_to_generate=250)                                   # frozen clips would step past the position table
    with pytest.raises(ValueError, match="position table"):
        gpt.beam_search_batched(ids, prompt_length=LENGTHS, stop_token=term, kv="shared_prefix")
    gpt.config.extra.update(tokens_to_generate=12)
    # an int stays the uniform path: the state is never asked for prompt_len
    seen = []
    orig = generation.SharedPrefixDecodeState.prefill_fan_out
    monkeypatch.setattr(generation.SharedPrefixDecodeState, "prefill_fan_out",
                        lambda self, *a, **k: (seen.append(k), orig(self, *a, **k))[1])
    gpt.beam_search_batched(ids[:2], prompt_length=4, stop_token=term, kv="shared_prefix")
    assert seen == [{}]


def test_caption_entrypoint_mixed_prompts_flag_on_standins(tmp_path, monkeypatch):
    """downstream/run_caption_distributed_gpt3.py --evaluate_only: --eval_mixed_prompts defaults off, implies nothing else, and reaches
    the lockstep beam-search call of model.generate as mixed_prompts=True -- not the sampling call; the result file keeps its format."""
    import json
    import os
    import test_entrypoint_gpu as t
    from test_engine_cpu import _stub_optimizer_kernels
    from youku_mplug_amd import downstream
    orig = t._write_configs

    def write(d, update_freq=1):
        path = orig(d, update_freq)
        cfg = json.load(open(os.path.join(d, "txt.json")))
        cfg.update(hidden_dropout=0.0, attention_dropout=0.0)
        json.dump(cfg, open(os.path.join(d, "txt.json"), "w"))
        return path
    monkeypatch.setattr(t, "_write_configs", write)
    _stub_optimizer_kernels(monkeypatch)
    monkeypatch.setenv("MASTER_PORT", str(44000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    seen = []
    gen = downstream.DistributedGPT3_Caption.generate

    def spy(self, image, text, *a, **kw):
        seen.append((kw.get("batched", False), kw.get("do_sample", False), kw.get("kv_cache"), kw.get("mixed_prompts", False)))
        return gen(self, image, text, *a, **kw)
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    try:
        out = str(tmp_path / "mixed")
        base = ["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only",
                "--eval_batched_beam", "--eval_shared_kv", "--eval_sample", "2"]
        assert entry.get_args(base)[0].eval_mixed_prompts is False
        alone = entry.get_args(["--config", cfg, "--output_dir", out, "--evaluate_only", "--eval_mixed_prompts"])[0]
        assert alone.eval_mixed_prompts is True and alone.eval_batched_beam is False and alone.eval_shared_kv is False
        args, config = entry.get_args(base + ["--eval_mixed_prompts"])
        entry.main(args, config)
        assert seen and set(seen) == {(True, False, "shared_prefix", True), (False, True, "shared_prefix", False)}, seen
        merged = json.load(open(os.path.join(out, "result", "val_caption_result.json")))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert len(merged) == 5
    for rec in merged:
        assert set(rec) == {"video_id", "pred_caption", "gold_caption", "sampled_captions"}


# ------------------------------------------------------------------------------------------------ the state and the reference
def test_ragged_state_matches_uniform_states_on_standins(monkeypatch):
    """the state case of tests/test_decode_ragged_gpu.py on the stand-ins: three clips with prompts of 2 / 5 / 9 tokens, fan 3 -- every
    call's logits within 1e-2 (the KV-cache gate) of uniform states run clip by clip, two ragged states bit-identical, the pad rows'
    KV never read, and the same on FP8 weights"""
    import decode_ragged_cases as rc
    import test_decode_shared_cpu as tds
    sr.install(monkeypatch)
    dev = torch.device("cpu")
    cfg, gpt = tds._tiny_decoder(dev)
    qe, prompt, toks = rc.state_inputs(cfg, dev)
    want = rc.run_uniform_states(gpt, dev, qe, prompt, toks)
    for weights in ("bf16", "fp8"):
        got, st = rc.run_ragged_state(gpt, dev, qe, prompt, toks, weights=weights)
        again, _ = rc.run_ragged_state(gpt, dev, qe, prompt, toks, weights=weights)
        poisoned, _ = rc.run_ragged_state(gpt, dev, qe, prompt, toks, weights=weights, poison=True)
        assert len(got) == len(want) == 6
        for i, (a, w, b, p) in enumerate(zip(got, want, again, poisoned)):
            assert a.shape == w.shape == (9, cfg.vocab) and a.dtype == BF
            assert torch.equal(a, b) and torch.equal(a, p), (weights, i)
            if weights == "bf16":
                assert tds.rel(a, w) <= 1e-2, (i, tds.rel(a, w))
        assert st.P == rc.Q + 9 and st.t == 5 and st.pos == rc.Q + 9 + 5 and st.group_prefix_len.tolist() == [rc.Q + 2, rc.Q + 5, rc.Q + 9]
        assert st.kv_bytes() == cfg.layers * (3 * st.P + 2 * 9 * rc.STEPS) * 3 * cfg.hidden * 2
    from youku_mplug_amd.generation import SharedPrefixDecodeState
    for bad in ([2, 5], [0, 5, 9], [2, 5, 10]):
        with pytest.raises(ValueError):
            SharedPrefixDecodeState(gpt, 9, 40).prefill_fan_out(prompt, qe, 3, prompt_len=bad)


def test_standin_products_do_not_depend_on_the_row_count(monkeypatch):
    """what the equal-scores comparisons above rest on: under the fixture a row of a stand-in product, of the shared-prefix attention
    and of the prefill attention is bit-identical whether it is computed alone or among 24 others -- through `@`, torch.matmul,
    torch.mm / bmm and F.linear alike"""
    import torch.nn.functional as F
    import standin_ops as so
    sr.install(monkeypatch)
    g = torch.Generator().manual_seed(5)
    a = torch.randn(25, 256, generator=g).to(BF)
    w = torch.randn(1024, 256, generator=g).to(BF)
    full = so.gemm(a, w, 25, 1024, 256)
    for r in (0, 7, 24):
        assert torch.equal(so.gemm(a[r:r + 1].contiguous(), w, 1, 1024, 256)[0], full[r]), r
    af, wf = a.float(), w.float()
    want = (af.double() @ wf.double().t()).float()
    for got in (af @ wf.t(), torch.matmul(af, wf.t()), torch.mm(af, wf.t()), F.linear(af, wf), torch.bmm(af[None], wf.t()[None])[0]):
        assert torch.equal(got, want)


def test_ragged_reference_matches_the_fp64_definition():
    """the reference of the GPU kernel test, group by group, against the element-by-element fp64 definition at that group's length"""
    import decode_ragged_cases as rc
    import standin_decode_shared as sd
    c = rc.make_case(64, 2, 3, [1, 33, 5], 2, short_last=1, seed=9, prefix_pad=float("nan"), suffix_pad=float("nan"))
    got = rc.reference(c)
    assert got.shape == (8, 2, 64) and torch.isfinite(got).all()
    for g in range(3):
        one = rc.group_alone(c, g)
        want = sd.reference_fp64(*[one[n] for n in ("q", "k", "v", "pk", "pv", "lay", "prefix_lay", "n_seq", "group_size", "heads", "prefix_len",
                                                    "own_len", "hd", "scale")])
        assert ((got[g * 3:g * 3 + one["n_seq"]].double() - want).abs().max() / want.abs().max()).item() <= 1e-6


# ------------------------------------------------------------------------------------------------ the library on the host
def test_library_exports_the_ragged_entries_and_refuses_on_the_host():
    """every refusal is a negative code from host-side checks: no device is needed (and none is touched) to get it"""
    import test_decode_shared_cpu as tds
    from youku_mplug_amd import _lib
    lib = _lib.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(lib, sym)
    glen = 0x70000                                                                     # never dereferenced on the host
    for over in (dict(head_dim=96), dict(own_len=0), dict(own_len=2049), dict(prefix_len=0), dict(group_size=0), dict(n_groups=3),
                 dict(pv_gs=11 * 768 + 2), dict(o_ss=258), dict(q=0x10008), dict(pk=0), dict(scale=0.0), dict(n_seq=0)):
        rc = lib.mpv_attn_decode_shared_ragged_fwd(ctypes.byref(tds._desc(**over)), glen, None)
        assert rc < 0, (over, rc)
        assert rc == lib.mpv_attn_decode_shared_fwd(ctypes.byref(tds._desc(**over)), None), over      # the uniform entry's refusal
        lib.mpv_attn_decode_shared_ragged_fwd(ctypes.byref(tds._desc(**over)), glen, None)
        assert b"mpv_attn_decode_shared_ragged_fwd" in lib.mpv_last_error()
    assert lib.mpv_attn_decode_shared_ragged_fwd(ctypes.byref(tds._desc()), None, None) == -5
    assert b"group_prefix_len" in lib.mpv_last_error()
    P = 0x10000
    assert lib.mpv_gpt_embed_rows_w8_fwd(None, P, P, P, P, P, 4, 64, 16, None) == -5
    for rows, H, mp in ((0, 64, 16), (4, 60, 16), (4, 64, 0)):
        assert lib.mpv_gpt_embed_rows_w8_fwd(P, P, P, P, P, P, rows, H, mp, None) == -1
        assert b"mpv_gpt_embed_rows_w8_fwd" in lib.mpv_last_error()
    w = _lib.GptWeights()
    w.layers, w.hidden, w.heads, w.ffn, w.vocab, w.max_positions = 2, 256, 4, 1024, 1024, 64
    q8 = _lib.GptWeightsQ8()
    q8.layers = 1
    tab = (ctypes.c_void_p * 2)(P, P)
    big = 1 << 40                                                                      # (a workspace size: never touched)
    # the ragged step: a NULL length array, a pitch below the longest prefix, a position past the table, t outside the suffix
    step = lambda **o: lib.mpv_gpt_decode_step_shared_ragged(ctypes.byref(w), tab, tab, 2, 3, o.get("stride", 20), o.get("glen", P),
                                                             o.get("maxp", 20), 8, o.get("t", 0), P, P, big, P, None)
    assert step(glen=None) == -5 and b"mpv_gpt_decode_step_shared_ragged: null group_prefix_len" in lib.mpv_last_error()
    assert step(stride=19) == -1 and b"mpv_gpt_decode_step_shared_ragged: max_prefix_len" in lib.mpv_last_error()
    assert step(maxp=60, stride=60, t=4) == -1 and b"position" in lib.mpv_last_error()
    assert step(t=8) == -1
    assert lib.mpv_gpt_decode_step_shared_ragged_q8(ctypes.byref(w), ctypes.byref(q8), tab, tab, 2, 3, 20, P, 20, 8, 0, P, P, big, P, None) == -5
    assert b"mpv_gpt_decode_step_shared_ragged_q8" in lib.mpv_last_error()
    # the ragged prefill: a NULL last_row; rows that do not fit the cache
    assert lib.mpv_gpt_prefill_ragged(ctypes.byref(w), tab, 2, 16, None, 0, P, 4, None, P, big, P, None) == -5
    assert b"last_row" in lib.mpv_last_error()
    assert lib.mpv_gpt_prefill_ragged(ctypes.byref(w), tab, 2, 3, None, 0, P, 4, P, P, big, P, None) == -1
    assert b"mpv_gpt_prefill_ragged: positions" in lib.mpv_last_error()                # the shared body names the entry it serves
    assert lib.mpv_gpt_prefill_ragged_q8(ctypes.byref(w), ctypes.byref(q8), tab, 2, 16, None, 0, P, 4, P, P, big, P, None) == -5
    assert b"mpv_gpt_prefill_ragged_q8" in lib.mpv_last_error()
