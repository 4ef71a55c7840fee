"""Lockstep beam search over a batch of clips, on CPU: generation.beam_search_batched_loop driven by oracle/gen_golden.py's StubLogits
(one stub per clip) with tests/standin_beam.py as the advance_fn, against tests/golden/search_stub.pt -- written by the reference's
own beam_search, one clip at a time.  The four seeds of BEAM_CASES share vocab, prompt, config and Q: a batch of four clips whose
per-clip answers are committed.  The search logic is discrete: sequences must agree token for token.  Then DistributedGPT3_Caption
.generate(batched=True) and the caption entry point's --eval_batched_beam on the stand-ins of tests/standin_ops.py."""
import json
import os
import types

import pytest
import torch

import standin_beam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
K, N_RET, PROMPT = 4, 3, 3


class _BatchedStubState:
    """The decode state of a batch of clips as token prefixes: sequence j belongs to clip j // fan and gets that clip's stub logits."""

    def __init__(self, stubs, batch, max_len):
        self.stubs, self.batch, self.prefix, self.q, self.fan = stubs, batch, None, 0, None
        self.steps = 0

    def _logits(self):
        return torch.stack([self.stubs[j // self.fan].row(self.prefix[:, j].tolist()) for j in range(self.batch)])

    def prefill_fan_out(self, tokens, query_embeds, fan):
        assert self.prefix is None and tokens.shape[0] * fan == self.batch == len(self.stubs) * fan
        self.fan = fan
        self.q += 0 if query_embeds is None else query_embeds.size(1)
        assert query_embeds is None or query_embeds.shape[0] == tokens.shape[0]          # the prefill runs once per clip
        self.prefix = tokens.t().contiguous().repeat_interleave(fan, dim=1)
        self.steps += 1
        return self._logits()

    def step(self, tokens, query_embeds=None):
        assert query_embeds is None and tuple(tokens.shape) == (self.batch, 1)
        self.prefix = torch.cat([self.prefix, tokens.t().contiguous()], dim=0)
        self.steps += 1
        return self._logits()

    def reorder(self, idx, shared_prefix=0):
        n = shared_prefix - self.q
        groups = self.prefix[:n].view(n, -1, self.fan)
        assert n >= 0 and (groups == groups[:, :, :1]).all(), "the promised shared prefix is not shared within a clip's sequences"
        assert torch.equal(idx // self.fan, torch.arange(self.batch) // self.fan), "a source row left its clip"
        self.prefix = self.prefix[:, idx]


def _torch_topk(logits, k, add):
    lp = torch.log_softmax(logits.float(), dim=-1) + (add.view(-1, 1) if add is not None else 0.0)
    v, i = torch.sort(lp, dim=-1, descending=True, stable=True)
    return v[:, :k].contiguous(), i[:, :k].contiguous()


def _case(Q):
    from oracle.gen_golden import BEAM_CASES
    vocab, _, cfgd, tokens, _, _ = BEAM_CASES[(1, Q)]
    return vocab, types.SimpleNamespace(**cfgd, top_k=1, top_p=0.0, vocab_size=vocab), torch.tensor(tokens)


_RUNS = {}


def _run(seeds, Q):
    """-> (results, per clip the first step after which it was done or None, per clip its state when it became done, the final state);
    computed once per (seeds, Q) and shared"""
    if (seeds, Q) in _RUNS:
        return _RUNS[(seeds, Q)]
    from oracle.gen_golden import StubLogits
    from youku_mplug_amd import generation
    vocab, cfg, tokens = _case(Q)
    stubs = [StubLogits(vocab=vocab, stop=7, seed=s) for s in seeds]
    B = len(seeds)
    qe = torch.zeros(B, Q, 4) if Q else None
    done_at, frozen, last = [None] * B, [None] * B, {}

    def advance(vals, idxs, bs, **kw):
        r = standin_beam.beam_advance(vals, idxs, bs, **kw)
        for b in range(B):
            if done_at[b] is None and int(bs.done[b]):
                done_at[b] = kw["cur_len"]
                frozen[b] = {n: getattr(bs, n)[b].clone() for n in ("tokens", "scores", "hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "worst")}
        last["bs"], last["steps"] = bs, kw["cur_len"]
        return r
    out = generation.beam_search_batched_loop(cfg, lambda b, m: _BatchedStubState(stubs, b, m), tokens.repeat(B, 1), query_embeds=qe,
                                              beam_size=K, num_return_gen=N_RET, prompt_length=PROMPT, topk_fn=_torch_topk, advance_fn=advance)
    _RUNS[(seeds, Q)] = (out, done_at, frozen, last)
    return _RUNS[(seeds, Q)]


def _check_against_golden(out, seeds, Q):
    ref = torch.load(os.path.join(GOLD, "search_stub.pt"))["beam"]
    assert len(out) == len(seeds)
    for o, s in zip(out, seeds):
        r = ref[(s, Q)]
        assert o.sequences.shape == r["sequences"].shape
        assert torch.equal(o.sequences, r["sequences"]), (s, Q, o.sequences.tolist(), r["sequences"].tolist())
        assert torch.allclose(o.scores, r["scores"], atol=1e-5), (s, Q)


@pytest.mark.parametrize("Q", [0, 3])
def test_batched_beam_search_matches_the_reference_golden_per_clip(Q):
    """batch = seeds (1, 2, 3, 4): every clip's sequences equal the reference's, token for token; scores within the golden's 1e-5"""
    out, _, _, _ = _run((1, 2, 3, 4), Q)
    _check_against_golden(out, (1, 2, 3, 4), Q)


@pytest.mark.parametrize("Q", [0, 3])
def test_batch_order_duplicates_and_batch_of_one(Q):
    from oracle.gen_golden import StubLogits
    from youku_mplug_amd import generation
    base, _, _, _ = _run((1, 2, 3, 4), Q)
    by_seed = dict(zip((1, 2, 3, 4), base))
    out, _, _, _ = _run((3, 1, 4, 2), Q)                       # another order: the same per-clip results, bit for bit
    for o, s in zip(out, (3, 1, 4, 2)):
        assert torch.equal(o.sequences, by_seed[s].sequences) and torch.equal(o.scores, by_seed[s].scores), s
    out, _, _, _ = _run((1, 1, 3), Q)                          # duplicates: clips 0 and 1 are identical
    assert torch.equal(out[0].sequences, out[1].sequences) and torch.equal(out[0].scores, out[1].scores)
    _check_against_golden(out, (1, 1, 3), Q)
    vocab, cfg, tokens = _case(Q)
    for s in (1, 2, 3, 4):                                     # B = 1 equals beam_search_loop exactly
        one, _, _, _ = _run((s,), Q)
        import test_host_cpu as th
        stub = StubLogits(vocab=vocab, stop=7, seed=s)
        ref = generation.beam_search_loop(cfg, lambda b, m: th._StubState(stub, b, m), tokens.clone(), query_embeds=torch.zeros(1, Q, 4) if Q else None,
                                          beam_size=K, num_return_gen=N_RET, prompt_length=PROMPT, topk_fn=_torch_topk)
        assert torch.equal(one[0].sequences, ref.sequences) and torch.equal(one[0].scores, ref.scores), s


@pytest.mark.parametrize("Q", [0, 3])
def test_a_clip_that_finishes_early_keeps_its_result(Q):
    """The seeds finish at different positions.  A finished clip is frozen -- its hypotheses, token rows and scores do not change while
    the others run on (it keeps stepping as padding rows: no compaction) -- and its result is the golden's."""
    out, done_at, frozen, last = _run((1, 2, 3, 4), Q)
    print("done after step", done_at, "of", last["steps"])
    finished = [d for d in done_at if d is not None]
    assert finished and len(set(done_at)) > 1, done_at
    _, cfg, tokens = _case(Q)
    assert last["steps"] == (max(finished) if len(finished) == len(done_at) else tokens.size(1) + cfg.tokens_to_generate - PROMPT)
    early = [b for b, d in enumerate(done_at) if d is not None and d < last["steps"]]
    assert early, done_at
    for b in early:
        for n, t in frozen[b].items():
            assert torch.equal(getattr(last["bs"], n)[b], t), (b, n)
    _check_against_golden(out, (1, 2, 3, 4), Q)


def test_advance_standin_refuses_what_the_kernel_refuses():
    from youku_mplug_amd.generation import BeamState
    for beams, row_len in ((9, 12), (4, 4096)):
        st = BeamState(torch.zeros(1, row_len, dtype=torch.long), beams)
        with pytest.raises(AssertionError):
            standin_beam.beam_advance(torch.zeros(beams, 2 * beams), torch.zeros(beams, 2 * beams, dtype=torch.long), st, vocab=37, pos=1, cur_len=1,
                                      first=True, stop_token=7)


# ------------------------------------------------------------------------------ the model and the entry point on the stand-ins
def _on_cpu(monkeypatch):
    import test_pipeline_cpu as tp
    from youku_mplug_amd import ops
    dev = tp._on_cpu(monkeypatch)
    monkeypatch.setattr(ops, "beam_advance", standin_beam.beam_advance)
    return dev


def test_caption_generate_batched_on_standins(monkeypatch):
    """DistributedGPT3_Caption.generate(batched=True) in the setup of test_caption_generate_on_standins (ragged prompts: two groups):
    the same list, shapes and order as batched=False, prompts kept; clips_per_search = 1 walks the same groups one clip at a time."""
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict
    from youku_mplug_amd import generation
    from youku_mplug_amd.downstream import synthetic_gencls_model
    dev = _on_cpu(monkeypatch)
    m = torch.load(os.path.join(GOLD, "caption_tiny.pt"))["meta"]
    model = synthetic_gencls_model(CONFIG_TINY, "caption", device=dev)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in make_state_dict(CONFIG_TINY, m["weight_seed"]).items()}, strict=True)
    model.text_decoder.config.extra.update(tokens_to_generate=m["tokens_to_generate"], eod_id=m["eod_id"])
    video, ids, mask = make_inputs(CONFIG_TINY, m["batch"], m["text_len"], seed=m["input_seed"], ragged=False)
    mask[1, 4:] = 0
    text = types.SimpleNamespace(input_ids=ids, attention_mask=mask)
    video = video.to(torch.bfloat16)
    plain = model.generate(video, text, termination_id=m["eod_id"])
    calls = []
    orig = generation.beam_search_batched_loop

    def spy(cfg, make_state, tokens, **kw):
        calls.append((tokens.shape[0], kw["prompt_length"]))
        return orig(cfg, make_state, tokens, **kw)
    monkeypatch.setattr(generation, "beam_search_batched_loop", spy)
    for cps, want_calls in ((32, [(1, 3), (1, 5)]), (1, [(1, 3), (1, 5)])):
        calls.clear()
        res = model.generate(video, text, termination_id=m["eod_id"], batched=True, clips_per_search=cps)
        assert calls == want_calls, calls                                      # grouped by prompt length
        assert isinstance(res, list) and len(res) == len(plain) == m["batch"]
        for i, (r, p) in enumerate(zip(res, plain)):
            assert r.shape == p.shape and r.dtype == p.dtype and r.device == p.device
            n_prompt = int(mask[i].sum()) - 1
            assert torch.equal(r[0, :n_prompt], ids[i, :n_prompt]), i          # clip i's own prompt: input order is kept
    # three clips of one prompt length, two clips per search: chunks of 2 + 1, results in input order
    text3 = types.SimpleNamespace(input_ids=ids[[0, 0, 0]], attention_mask=mask[[0, 0, 0]])
    calls.clear()
    res = model.generate(video[[0, 1, 0]], text3, termination_id=m["eod_id"], batched=True, clips_per_search=2)
    assert calls == [(2, 5), (1, 5)] and len(res) == 3
    assert torch.equal(res[0], res[2])                                         # the same clip in two different chunks
    with pytest.raises(ValueError):
        model.generate(video, text, termination_id=m["eod_id"], batched=True, clips_per_search=0)


def test_caption_entrypoint_batched_flag_on_standins(tmp_path, monkeypatch):
    """downstream/run_caption_distributed_gpt3.py --evaluate_only with and without --eval_batched_beam on the stand-ins: the flag
    defaults off, reaches model.generate, and the result files have the same format, clips and order."""
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
    monkeypatch.setenv("MASTER_PORT", str(38000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    seen = []
    gen = downstream.DistributedGPT3_Caption.generate

    def spy(self, image, text, *a, **kw):
        seen.append((kw.get("batched", False), kw.get("clips_per_search")))
        return gen(self, image, text, *a, **kw)
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    merged = {}
    try:
        for name, flags in (("plain", []), ("batched", ["--eval_batched_beam", "--clips_per_search", "3"])):
            out = str(tmp_path / name)
            args, config = entry.get_args(["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7",
                                           "--evaluate_only"] + flags)
            assert args.eval_batched_beam is bool(flags) and args.clips_per_search == (3 if flags else 32)
            seen.clear()
            res = entry.main(args, config)
            assert seen and all(s == ((True, 3) if flags else (False, None)) for s in seen), seen
            merged[name] = json.load(open(os.path.join(out, "result", "val_caption_result.json")))
            assert os.path.isfile(os.path.join(out, "result", "val_caption_result_rank0.json"))
            assert all(0.0 <= res[f"val_{k}"] <= 1.0 for k in ("Bleu_1", "Bleu_4", "ROUGE_L"))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    a, b = merged["plain"], merged["batched"]
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert set(x) == set(y) == {"video_id", "pred_caption", "gold_caption"}
        assert x["video_id"] == y["video_id"] and x["gold_caption"] == y["gold_caption"] and isinstance(y["pred_caption"], str)
