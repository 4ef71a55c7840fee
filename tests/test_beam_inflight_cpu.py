"""Beam search with the finished clips' slots refilled in flight, on CPU: generation.beam_inflight_loop on the stand-ins
(tests/standin_beam_inflight.py) against beam_search_batched_loop on every clip ALONE and the per-clip beam_search_loop, whatever the
slots, refill_min or the input order; short budgets against an oracle written here; the decode steps and prefills the refill rules
imply; generate(beam_inflight=True) against generate(mixed_prompts=True); the refusals, the entry point's flag, and what the two new
exports refuse on the host."""
import ctypes
import types

import pytest
import torch

import standin_beam
import standin_beam_inflight as sbi
import test_inflight_cpu as ti

LENGTHS, BUDGETS = ti.LENGTHS, ti.BUDGETS
K, NRET = 3, 2
NEW_SYMBOLS = ("mpv_beam_advance_steps", "mpv_kv_suffix_reorder_steps")
# the stop token of the three runs of a schedule and the bonus its logit gets in front of every top-k (the tiny model has random
# weights: without help its search never closes a hypothesis store): nothing ends early / some clips do / every clip does
STOPS = {"none": (-1, 0.0), "some": (7, 1.0), "all": (7, 1.25)}


def _on_cpu(monkeypatch, stop_mode="none"):
    from youku_mplug_amd import ops
    dev = ti._on_cpu(monkeypatch)
    sbi.install(monkeypatch)
    stop, bonus = STOPS[stop_mode]
    if bonus:
        plain = ops.logprob_topk

        def boosted(logits, k, add=None, **kw):
            lg = logits.clone()
            lg[:, stop] += bonus
            return plain(lg, k, add=add, **kw)
        monkeypatch.setattr(ops, "logprob_topk", boosted)
    return dev


def _inputs(dev):
    model, cfg, term, vid, text = ti._setup(dev)
    return model, model.text_decoder, text.input_ids, ti._query(model, len(LENGTHS)), vid, text


_ALONE = {}


def _alone(gpt, ids, qf, mode):
    """every clip ALONE through the lockstep loop (one prompt length, shared-prefix KV) and through the per-clip loop, once per stop
    mode for the module; nothing modifies them"""
    if mode not in _ALONE:
        stop = STOPS[mode][0]
        kw = dict(beam_size=K, num_return_gen=NRET, stop_token=stop)
        _ALONE[mode] = [(gpt.beam_search_batched(ids[c:c + 1], query_embeds=qf[c:c + 1], prompt_length=LENGTHS[c], kv="shared_prefix", **kw)[0],
                         gpt.beam_search(ids[c:c + 1], query_embeds=qf[c:c + 1], prompt_length=LENGTHS[c], **kw)) for c in range(len(LENGTHS))]
    return _ALONE[mode]


def _oracle(gpt, ids, qf, c, budget, stop):
    """clip c alone, advanced `budget` times by the UNIFORM stand-in advance, finished by the module's own _ranked_hypotheses"""
    from youku_mplug_amd import generation, ops
    cfg, pl = generation._gen_config(gpt), LENGTHS[c]
    table, final_len, Q = generation._pad_for_generation(cfg, ids[c:c + 1], stop, pl, qf)
    state = generation.make_state_fn(gpt, "shared_prefix")(K, final_len + Q)
    bs = generation.BeamState(table, K)
    for n in range(min(budget, final_len - pl)):
        logits = state.prefill_fan_out(table[:, :pl].contiguous(), qf[c:c + 1], K) if n == 0 else state.step(bs.next_tok.view(-1, 1))
        vals, idxs = ops.logprob_topk(logits, 2 * K, add=bs.scores.view(-1))
        standin_beam.beam_advance(vals, idxs, bs, vocab=logits.size(-1), pos=pl + n, cur_len=n + 1, first=n == 0, stop_token=stop)
        if bool(bs.done.all()):
            break
        state.reorder(bs.src_row, shared_prefix=Q + pl)
    h = types.SimpleNamespace(**{k: getattr(bs, k) for k in generation.BeamState.ARRAYS})
    ranked = generation._ranked_hypotheses(h, 0, K)[:NRET]
    return torch.stack([r[1] for r in ranked]), torch.tensor([r[0] for r in ranked], dtype=torch.float32)


def _run(gpt, ids, qf, order, slots, refill_min, stop, **kw):
    sel = torch.tensor(order)
    return gpt.beam_search_inflight(ids[sel], query_embeds=qf[sel], prompt_length=[LENGTHS[c] for c in order], beam_size=K, num_return_gen=NRET,
                                    stop_token=stop, slots=slots, refill_min=refill_min, **kw)


@pytest.mark.parametrize("slots,refill_min,order", ti.SCHEDULES)
@pytest.mark.parametrize("mode", list(STOPS))
def test_inflight_beams_equal_each_clip_alone(monkeypatch, slots, refill_min, order, mode):
    """5 clips (prompts of 3 / 1 / 4 / 2 / 3 tokens) through `slots` slots x 3 beams.  Full budgets: every clip's sequences and scores
    are those of beam_search_batched_loop on that clip alone (bit for bit); the per-clip beam_search_loop returns the same sequences,
    and scores within 1e-2, the project's bf16 gate (it keeps a cache per beam, whose stand-in rounds the bf16 logits on another
    route than the shared-prefix one).  Budgets 2 / 5 / 3 / 1 / 4: every clip equals the oracle above.  The decode
    steps and prefills are those the refill rules give for the positions every clip was advanced by.  "some" / "all": the stop token
    closes some / all of the clips' searches before their budgets"""
    from youku_mplug_amd.generation import refill_min_default
    dev = _on_cpu(monkeypatch, mode)
    model, gpt, ids, qf, _, _ = _inputs(dev)
    stop = STOPS[mode][0]
    order = list(range(len(LENGTHS))) if order is None else order
    rm = refill_min_default(slots) if refill_min is None else refill_min
    alone = _alone(gpt, ids, qf, mode)
    out = _run(gpt, ids, qf, order, slots, refill_min, stop)
    full = [ids.shape[1] + gpt.config.extra["tokens_to_generate"] - LENGTHS[c] for c in order]
    assert len(out.results) == len(order)
    for i, c in enumerate(order):
        got, (want, one) = out.results[i], alone[c]
        assert torch.equal(got.sequences, want.sequences) and torch.equal(got.scores, want.scores), (c, got, want)
        assert torch.equal(got.sequences, one.sequences) and torch.allclose(got.scores, one.scores, rtol=0, atol=1e-2), c
        assert 1 <= out.advances[i] <= full[i]
    early = sum(a < f for a, f in zip(out.advances, full))
    assert {"none": early == 0, "some": 0 < early < len(order), "all": early == len(order)}[mode], (out.advances, full)
    assert (out.steps, out.prefills) == ti.simulate(out.advances, slots, rm)
    short = _run(gpt, ids, qf, order, slots, refill_min, stop, max_new_tokens=[BUDGETS[c] for c in order])
    for i, c in enumerate(order):
        seqs, scores = _oracle(gpt, ids, qf, c, BUDGETS[c], stop)
        assert torch.equal(short.results[i].sequences, seqs) and torch.equal(short.results[i].scores, scores), c
        assert short.advances[i] <= BUDGETS[c]
    assert (short.steps, short.prefills) == ti.simulate(short.advances, slots, rm)
    if mode == "none":
        assert short.advances == [BUDGETS[c] for c in order]


def test_inflight_beams_issue_fewer_decode_steps_than_the_lockstep_chunks(monkeypatch):
    """2 slots, budgets 2 / 5 / 3 / 1 / 4: 7 decode steps and 3 prefills against the 9 steps of lockstep chunks of 2"""
    dev = _on_cpu(monkeypatch)
    model, gpt, ids, qf, _, _ = _inputs(dev)
    out = _run(gpt, ids, qf, list(range(5)), 2, 1, -1, max_new_tokens=BUDGETS)
    assert (out.steps, out.prefills) == (7, 3) and out.steps < ti.lockstep_steps(BUDGETS, 2)


CASES = {
    "plain": dict(),
    "n_best": dict(num_return_gen=3),
    "groups": dict(beam_groups=2, diversity_penalty=1.5, beam_size=3, num_return_gen=4),
    "rerank": dict(beam_groups=2, diversity_penalty=1.0, beam_size=2, num_return_gen=4, rerank_by_logprob=True),
    "min_new": dict(repetition_penalty=1.3, min_new_tokens=4),
    "fp8": dict(decode_weights="fp8"),
}


@pytest.mark.parametrize("slots", [2, 32])
@pytest.mark.parametrize("case", list(CASES))
def test_generate_beam_inflight_equals_mixed_prompts_on_standins(monkeypatch, case, slots):
    """generate(batched=True, beam_inflight=True) with full budgets returns what mixed_prompts=True returns, clip by clip"""
    import test_w8_cpu as tw
    dev = _on_cpu(monkeypatch, "some")
    model, gpt, ids, qf, vid, text = _inputs(dev)
    kw = dict(termination_id=7, batched=True, kv_cache="shared_prefix", clips_per_search=slots, **CASES[case])
    want = model.generate(vid, text, mixed_prompts=True, **kw)
    got = model.generate(vid, text, beam_inflight=True, refill_min=1, **kw)
    assert tw._same(got, want), (got, want)


def test_generate_beam_inflight_with_constrain_prompt_equals_the_grouped_call(monkeypatch):
    """constrain_prompt=True has no mixed counterpart (the left padding would count as prompt): against the call grouped by length"""
    import test_w8_cpu as tw
    dev = _on_cpu(monkeypatch, "some")
    model, gpt, ids, qf, vid, text = _inputs(dev)
    kw = dict(termination_id=7, batched=True, kv_cache="shared_prefix", clips_per_search=2, repetition_penalty=1.3, no_repeat_ngram_size=2,
              constrain_prompt=True)
    want = model.generate(vid, text, **kw)
    got = model.generate(vid, text, beam_inflight=True, **kw)
    assert tw._same(got, want), (got, want)
    assert not tw._same(got, model.generate(vid, text, beam_inflight=True, **dict(kw, constrain_prompt=False)))


def test_beam_inflight_refusals(monkeypatch):
    from youku_mplug_amd import generation, ops
    dev = _on_cpu(monkeypatch)
    model, gpt, ids, qf, vid, text = _inputs(dev)
    ok = dict(termination_id=7, batched=True, kv_cache="shared_prefix", beam_inflight=True)
    for bad, word in ((dict(do_sample=True), "do_sample"), (dict(batched=False), "batched"), (dict(kv_cache="per_sequence"), "shared_prefix"),
                      (dict(mixed_prompts=True), "mixed_prompts")):
        with pytest.raises(ValueError, match=word):
            model.generate(vid, text, **dict(ok, **bad))
    with pytest.raises(ValueError, match="do_sample"):                             # the sampling keyword keeps its refusal
        model.generate(vid, text, termination_id=7, batched=True, kv_cache="shared_prefix", inflight=True)
    for alone in (dict(max_new_tokens=3), dict(refill_min=2)):
        with pytest.raises(ValueError, match="inflight"):
            model.generate(vid, text, termination_id=7, batched=True, kv_cache="shared_prefix", **alone)
    call = lambda **kw: gpt.beam_search_inflight(ids, **dict(dict(query_embeds=qf, prompt_length=LENGTHS, stop_token=7, beam_size=K), **kw))
    for lens in (4, None, LENGTHS[:4], [0] + LENGTHS[1:], [ids.shape[1] + 1] + LENGTHS[1:]):
        with pytest.raises(ValueError, match="prompt_length"):
            call(prompt_length=lens)
    for kw, word in ((dict(slots=0), "slots"), (dict(beam_size=0), "beam_size"), (dict(refill_min=0), "refill_min"),
                     (dict(max_new_tokens=0), "max_new_tokens"), (dict(max_new_tokens=[1, 2]), "max_new_tokens"),
                     (dict(beam_groups=2, num_return_gen=3), "num_return_gen"), (dict(beam_groups=2, num_return_gen=2, diversity_penalty=-1.0), "diversity"),
                     (dict(decode_weights="int4"), "decode_weights"), (dict(return_scores=True), "return_scores")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    with pytest.raises(ValueError, match="constrain_fn"):
        generation.beam_inflight_loop(generation._gen_config(gpt), generation.make_inflight_state_fn(gpt), ids, prompt_length=LENGTHS,
                                      topk_fn=ops.logprob_topk, advance_fn=sbi.beam_advance_steps,
                                      constraints=generation.LogitsConstraints(min_new_tokens=2))
    installs = []                                                                  # the position table is checked before the first launch
    orig = generation.InflightDecodeState.install
    monkeypatch.setattr(generation.InflightDecodeState, "install", lambda self, *a, **k: (installs.append(a), orig(self, *a, **k))[1])
    gpt.config.extra.update(tokens_to_generate=10 ** 4)
    with pytest.raises(ValueError, match="position table"):
        call()
    assert not installs
    gpt.config.extra.update(tokens_to_generate=12)
    st = generation.make_inflight_state_fn(gpt)(2, K, model.num_learnable_token + 4, 3)
    with pytest.raises(ValueError, match="group_rows"):
        st.reorder(torch.arange(2 * K), torch.zeros(2, dtype=torch.int64), 1)
    with pytest.raises(ValueError, match="suffix"):
        st.reorder(torch.arange(2 * K), torch.zeros(2, dtype=torch.int32), 4)
    assert st.twin is None
    # the default stays today's loops: no new op and no in-flight state without the keyword
    for name in ("beam_advance_steps", "kv_suffix_reorder_steps", "logits_constrain_steps"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("an in-flight entry without beam_inflight=True"))
    monkeypatch.setattr(generation, "InflightDecodeState", lambda *a, **k: pytest.fail("an in-flight state without beam_inflight=True"))
    monkeypatch.setattr(generation, "beam_inflight_loop", lambda *a, **k: pytest.fail("the in-flight loop without beam_inflight=True"))
    model.generate(vid, text, termination_id=7, batched=True, kv_cache="shared_prefix", mixed_prompts=True, repetition_penalty=1.2)
    model.generate(vid, text, termination_id=7, batched=True, beam_groups=2, beam_size=2, num_return_gen=2)


def test_a_sampling_call_allocates_no_twin(monkeypatch):
    from youku_mplug_amd import generation
    dev = _on_cpu(monkeypatch)
    model, gpt, ids, qf, _, _ = _inputs(dev)
    states = []
    make = generation.make_inflight_state_fn(gpt)
    generation.sample_inflight_loop(generation._sampler_config(gpt, top_k=1), lambda *a: (states.append(make(*a)), states[-1])[1], ids, query_embeds=qf,
                                    prompt_length=LENGTHS, slots=2, max_new_tokens=3, **generation._sampler_fns("steps", False))
    assert len(states) == 1 and states[0].twin is None


def test_caption_entrypoint_beam_inflight_flag_on_standins(tmp_path, monkeypatch):
    """downstream/run_caption_distributed_gpt3.py --evaluate_only: --eval_beam_inflight defaults off, needs --eval_batched_beam and
    --eval_shared_kv, is refused with --eval_mixed_prompts and the sampling flags, and reaches the BEAM-search call of model.generate as
    beam_inflight=True; the result file keeps its format."""
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
    monkeypatch.setenv("MASTER_PORT", str(50000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    seen = []
    gen = downstream.DistributedGPT3_Caption.generate

    def spy(self, image, text, *a, **kw):
        seen.append((kw.get("batched", False), kw.get("beam_inflight", False), kw.get("kv_cache")))
        return gen(self, image, text, *a, **kw)
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    try:
        out = str(tmp_path / "beam_inflight")
        head = ["--config", cfg, "--output_dir", out, "--evaluate_only"]
        base = ["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only",
                "--eval_batched_beam", "--eval_shared_kv"]
        assert entry.get_args(base)[0].eval_beam_inflight is False
        for bad in (["--eval_beam_inflight"], ["--eval_beam_inflight", "--eval_batched_beam"], ["--eval_beam_inflight", "--eval_shared_kv"],
                    ["--eval_beam_inflight", "--eval_batched_beam", "--eval_shared_kv", "--eval_mixed_prompts"],
                    ["--eval_beam_inflight", "--eval_batched_beam", "--eval_shared_kv", "--eval_sample", "2"],
                    ["--eval_beam_inflight", "--eval_batched_beam", "--eval_shared_kv", "--eval_sample_best_of", "2"]):
            with pytest.raises(ValueError, match="eval_beam_inflight"):
                entry.get_args(head + bad)
        args, config = entry.get_args(base + ["--eval_beam_inflight"])
        assert args.eval_beam_inflight is True
        entry.main(args, config)
        assert seen and set(seen) == {(True, True, "shared_prefix")}, seen
        merged = json.load(open(os.path.join(out, "result", "val_caption_result.json")))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert len(merged) == 5
    for rec in merged:
        assert set(rec) == {"video_id", "pred_caption", "gold_caption"}


# ------------------------------------------------------------------------------------------------ the stand-ins themselves
def test_steps_standin_is_the_uniform_one_at_a_common_step():
    """the tests' own apparatus: with one step for every clip the _steps stand-in is the uniform stand-in on the whole batch; a
    negative step and a column behind the table freeze a clip"""
    import beam_groups_cases as bg
    import standin_beam_groups as sg
    st, vals, idxs = bg.random_state(3, 2, 2, 9, vocab=37, stop=5, pos=6, seed=3)
    a, b, c = bg.clone_state(st), bg.clone_state(st), bg.clone_state(st)
    kw = dict(groups=2, diversity_penalty=0.5, vocab=37, stop_token=5)
    sg.beam_advance_groups(vals, idxs, a, pos=6, cur_len=3, first=False, **kw)
    sbi.beam_advance_steps(vals, idxs, b, clip_prompt_len=torch.tensor([4, 4, 4], dtype=torch.int32), clip_step=torch.tensor([2, 2, 2], dtype=torch.int32), **kw)
    bg.assert_states_equal(a, b)
    sbi.beam_advance_steps(vals, idxs, c, clip_prompt_len=torch.tensor([4, 4, 4], dtype=torch.int32), clip_step=torch.tensor([2, -1, 5], dtype=torch.int32), **kw)
    for n in bg.STATE_ARRAYS:
        if n in ("tokens_alt",):
            continue
        x, y, z = getattr(c, n), getattr(a, n), getattr(st, n)
        per = x.shape[0] // 3
        assert torch.equal(x[:per], y[:per]), n
        if n == "tokens":
            assert torch.equal(x[per:], st.tokens[per:])
        elif n == "src_row":
            assert x[per:].tolist() == list(range(per, 3 * per))
        elif n == "next_tok":
            assert (x[per:] == 5).all()
        else:
            assert torch.equal(x[per:], z[per:]), n


# ------------------------------------------------------------------------------------------------ the library on the host
def test_library_exports_the_entries_and_refuses_on_the_host():
    """every refusal is a negative code from host-side checks, before any launch: no device is needed (and none is touched)"""
    from youku_mplug_amd import _lib
    lib = _lib.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(lib, sym)
    P = 0x10000
    ptrs = ("cand_val", "cand_idx", "tokens_in", "tokens_out", "scores", "hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "hyp_next", "worst",
            "done", "src_row", "next_tok")

    def desc(**over):
        d = _lib.BeamAdvanceGroupsDesc(batch=2, beams=2, row_len=12, vocab=37, pos=10 ** 6, cur_len=0, first=0, groups=2, diversity_penalty=0.5,
                                       stop_token=7)
        for i, n in enumerate(ptrs):
            setattr(d, n, P + 0x1000 * i)
        for k, v in over.items():
            setattr(d, k, v)
        return d
    refused = [dict(beams=9), dict(beams=0), dict(groups=9), dict(groups=0), dict(beams=5, groups=4), dict(diversity_penalty=-1.0),
               dict(diversity_penalty=float("nan")), dict(diversity_penalty=float("inf")), dict(row_len=4096), dict(row_len=0), dict(batch=0),
               dict(vocab=0), dict(tokens_out=P + 0x2000)] + [{n: 0} for n in ptrs]
    for over in refused:
        rc = lib.mpv_beam_advance_steps(ctypes.byref(desc(**over)), P, P, None)
        assert rc < 0, (over, rc)
        assert b"mpv_beam_advance_steps:" in lib.mpv_last_error(), (over, lib.mpv_last_error())
        d = desc(**over)
        d.pos, d.cur_len = 3, 1                                                    # what the uniform entry refuses it refuses with the same code
        assert rc == lib.mpv_beam_advance_groups(ctypes.byref(d), None), over
    assert lib.mpv_beam_advance_steps(ctypes.byref(desc()), None, P, None) == -5 and b"null clip_prompt_len" in lib.mpv_last_error()
    assert lib.mpv_beam_advance_steps(ctypes.byref(desc()), P, None, None) == -5 and b"null clip_step" in lib.mpv_last_error()
    assert lib.mpv_beam_advance_steps(None, P, P, None) == -5
    reorder = lambda **o: lib.mpv_kv_suffix_reorder_steps(o.get("src", P), o.get("dst", 2 * P), o.get("layers", 2), 3, 3, o.get("S", 5), o.get("idx", P),
                                                          o.get("rows", P), o.get("max_rows", 5), o.get("hidden", 16), None)
    for o in (dict(src=None), dict(dst=None), dict(idx=None), dict(rows=None), dict(dst=P), dict(hidden=12), dict(hidden=0), dict(max_rows=6),
              dict(max_rows=-1), dict(src=P + 8), dict(dst=2 * P + 2), dict(layers=0), dict(S=0)):
        assert reorder(**o) < 0, o
        assert b"mpv_kv_suffix_reorder_steps:" in lib.mpv_last_error(), o
    assert reorder(max_rows=0) == 0                                                # nothing to move: no launch
