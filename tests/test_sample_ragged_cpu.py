"""Sampled captions over clips whose prompts differ in length, on CPU: generate(do_sample=True, sample_mixed_prompts=True) on the
stand-ins (tests/standin_sample_ragged.py on tests/standin_decode_ragged.py) against the grouped generate(do_sample=True) call --
token-equal rows and equal scores clip by clip --, the budget rule, the refusals, the entry point's flag, the exported symbols and
what the three ragged entries refuse on the host."""
import ctypes
import types

import pytest
import torch

import standin_sample_ragged as sra

BF = torch.bfloat16
LENGTHS = [1, 4, 4, 7, 2]
NEW_SYMBOLS = ("mpv_sample_advance_ragged", "mpv_logits_constrain_ragged", "mpv_sample_score_ragged")


def _on_cpu(monkeypatch):
    import test_w8_cpu as tw
    dev = tw._on_cpu(monkeypatch)
    sra.install(monkeypatch)
    return dev


def _setup(dev, **kw):
    import test_decode_ragged_cpu as tdr
    return tdr._setup(dev, **kw)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _spy_sample_batched(model, monkeypatch):
    """records prompt_length, the row count and mixed_prompts of every sample_batched call of the model"""
    calls = []
    gpt = model.text_decoder
    orig = gpt.sample_batched

    def spy(tokens, **kw):
        pl = kw.get("prompt_length")
        calls.append((pl.tolist() if torch.is_tensor(pl) else pl, tokens.shape[0], kw.get("mixed_prompts", False)))
        return orig(tokens, **kw)
    monkeypatch.setattr(gpt, "sample_batched", spy)
    return calls


SCORED = dict(return_scores=True)
CASES = {
    "plain": dict(top_p=1.0),
    "top_k": dict(top_k=5),
    "top_p": dict(top_p=0.9, temperature=1.2),
    "return_scores": dict(top_p=0.9, **SCORED),
    "best_of": dict(top_p=0.9, best_of=True, length_penalty=1.0, **SCORED),
    "penalty_ngram": dict(top_p=0.9, repetition_penalty=1.3, no_repeat_ngram_size=2, **SCORED),
    "min_new": dict(top_p=0.9, min_new_tokens=4, **SCORED),
    "fp8": dict(top_p=0.9, decode_weights="fp8", **SCORED),
    "constrain_prompt": dict(top_p=0.9, repetition_penalty=1.3, no_repeat_ngram_size=2, constrain_prompt=True, **SCORED),
}


@pytest.mark.parametrize("per_chunk", [2, 32])
@pytest.mark.parametrize("case", list(CASES))
def test_sample_mixed_prompts_equal_the_grouped_call_on_standins(monkeypatch, case, per_chunk):
    """five clips with prompts of 1 / 4 / 4 / 7 / 2 tokens, 3 samples each: sample_mixed_prompts=True returns, clip by clip, the rows
    AND the scores of the grouped call (constrain_prompt=True against a grouped call with the same flag); it makes one loop per chunk
    of clips in input order, with the chunk's lengths"""
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev)
    kw = dict(termination_id=term, do_sample=True, num_samples=3, seed=11, kv_cache="shared_prefix", clips_per_search=per_chunk, **CASES[case])
    calls = _spy_sample_batched(model, monkeypatch)
    want = model.generate(vid, text, **kw)
    assert calls and all(not mixed and len(set(pl)) == 1 for pl, _, mixed in calls)         # today's call: one length per loop
    calls.clear()
    got = model.generate(vid, text, sample_mixed_prompts=True, **kw)
    assert calls == [(LENGTHS[c:c + per_chunk], len(LENGTHS[c:c + per_chunk]), True) for c in range(0, len(LENGTHS), per_chunk)]
    assert _same(got, want), (got, want)
    rows = got[0] if "return_scores" in CASES[case] else got
    width = text.input_ids.shape[1] + model.text_decoder.config.extra["tokens_to_generate"]
    for i, a in enumerate(rows):
        assert a.shape == (1 if "best_of" in CASES[case] else 3, width)
        assert (a[:, :LENGTHS[i]] == text.input_ids[i, :LENGTHS[i]].cpu()).all()
    if "return_scores" in CASES[case] and "best_of" not in CASES[case]:
        assert any(int(s["count"].max()) > 0 for s in got[1])                                # something was scored


def test_a_clips_samples_do_not_depend_on_its_neighbours(monkeypatch):
    """the reason for the left-aligned table: clip 0's samples in a chunk with a 7-token neighbour are those it gets alone"""
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev)
    kw = dict(termination_id=term, do_sample=True, num_samples=3, seed=3, kv_cache="shared_prefix", sample_mixed_prompts=True, return_scores=True,
              top_p=0.9)
    rows, scores = model.generate(vid, text, **kw)
    one = types.SimpleNamespace(input_ids=text.input_ids[:1], attention_mask=text.attention_mask[:1])
    rows1, scores1 = model.generate(vid[:1], one, **kw)
    assert _same(rows[0], rows1[0]) and _same(scores[0], scores1[0])


@pytest.mark.parametrize("ban_stop", [True, False])
def test_the_longest_prompt_runs_out_of_columns_first(monkeypatch, ban_stop):
    """tokens_to_generate = 2 in rows 9 wide: the clip with the 7-token prompt has 11 - 7 = 4 columns, the one with 1 token has 10.
    Every clip gets exactly the budget the grouped path gives it; with the stop token banned no row ever terminates, the loop runs to
    the end of the SHORTEST prompt's budget and the kernels' frozen rows are what ends the longer ones"""
    from youku_mplug_amd import generation
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev, tokens_to_generate=2)
    kw = dict(termination_id=term, do_sample=True, num_samples=2, seed=5, kv_cache="shared_prefix", return_scores=True, top_p=0.9)
    if ban_stop:
        kw["min_new_tokens"] = 100
    steps = []
    orig = generation.SharedPrefixDecodeState.step
    want = model.generate(vid, text, **kw)
    monkeypatch.setattr(generation.SharedPrefixDecodeState, "step", lambda self, *a, **k: (steps.append(self), orig(self, *a, **k))[1])
    got = model.generate(vid, text, sample_mixed_prompts=True, **kw)
    width = text.input_ids.shape[1] + 2
    assert _same(got, want), (got, want)
    if ban_stop:
        assert len(steps) == width - min(LENGTHS) - 1
        for i, (a, s) in enumerate(zip(*got)):
            assert a.shape == (2, width) and (a[:, LENGTHS[i]:] != term).all()               # every column of the budget is filled
            assert s["count"].tolist() == [width - LENGTHS[i]] * 2                          # and scored, none behind it


def test_sample_mixed_prompts_refusals(monkeypatch):
    from youku_mplug_amd import generation
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev)
    ok = dict(termination_id=term, do_sample=True, kv_cache="shared_prefix", sample_mixed_prompts=True)
    for bad, word in ((dict(do_sample=False), "do_sample"), (dict(do_sample=False, batched=True), "do_sample"),
                      (dict(kv_cache="per_sequence"), "shared_prefix")):
        with pytest.raises(ValueError, match=word):
            model.generate(vid, text, **dict(ok, **bad))
    with pytest.raises(ValueError, match="shared_prefix"):
        model.generate(vid, text, termination_id=term, do_sample=True, sample_mixed_prompts=True)          # kv_cache default: per_sequence
    with pytest.raises(ValueError, match="do_sample"):                                   # the pinned refusal of the beam keyword stays
        model.generate(vid, text, termination_id=term, batched=True, kv_cache="shared_prefix", mixed_prompts=True, do_sample=True)
    gpt = model.text_decoder
    ids = text.input_ids
    with pytest.raises(ValueError, match="shared_prefix"):
        gpt.sample_batched(ids, prompt_length=LENGTHS, termination_id=term, mixed_prompts=True)             # kv="per_sequence"
    with pytest.raises(ValueError, match="prompt_len"):                                  # a state whose prefill takes no prompt_len
        generation.sample_batched_loop(generation._gen_config(gpt), generation.make_state_fn(gpt, "per_sequence"), ids, prompt_length=LENGTHS,
                                       mixed_prompts=True, advance_fn=sra.sample_advance_ragged)
    for lens in (4, None, LENGTHS[:4], [0] + LENGTHS[1:], [ids.shape[1] + 1] + LENGTHS[1:]):
        with pytest.raises(ValueError, match="prompt_length"):
            gpt.sample_batched(ids, prompt_length=lens, termination_id=term, kv="shared_prefix", mixed_prompts=True)
    gpt.config.extra.update(tokens_to_generate=250)                                      # frozen rows would step past the position table
    with pytest.raises(ValueError, match="position table"):
        gpt.sample_batched(ids, prompt_length=LENGTHS, termination_id=term, kv="shared_prefix", mixed_prompts=True)
    gpt.config.extra.update(tokens_to_generate=12)
    # the default stays today's loop: the state is never asked for prompt_len, and no ragged entry is called
    seen = []
    orig = generation.SharedPrefixDecodeState.prefill_fan_out
    monkeypatch.setattr(generation.SharedPrefixDecodeState, "prefill_fan_out", lambda self, *a, **k: (seen.append(k), orig(self, *a, **k))[1])
    from youku_mplug_amd import ops
    for name in ("sample_advance_ragged", "logits_constrain_ragged", "sample_score_ragged"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a ragged entry in the uniform loop"))
    gpt.sample_batched(ids[:2], prompt_length=torch.tensor([4, 2]), termination_id=term, kv="shared_prefix", return_scores=True,
                       constraints=generation.LogitsConstraints(repetition_penalty=1.2))
    assert seen == [{}]


def test_pad_after_termination_takes_a_length_per_row():
    from youku_mplug_amd.generation import pad_after_termination
    t = torch.tensor([[7, 1, 7, 3, 4], [1, 2, 7, 3, 4], [1, 2, 3, 4, 5]])
    assert pad_after_termination(t, 1, 7, 6, 9).tolist() == [[7, 1, 7, 9, 9, 9], [1, 2, 7, 9, 9, 9], [1, 2, 3, 4, 5, 9]]       # an int: as before
    for lens in ([1, 3, 0], torch.tensor([1, 3, 0])):
        assert pad_after_termination(t, lens, 7, 6, 9).tolist() == [[7, 1, 7, 9, 9, 9], [1, 2, 7, 3, 4, 9], [1, 2, 3, 4, 5, 9]]
    assert pad_after_termination(t, torch.tensor(1), 7, 6, 9).tolist() == pad_after_termination(t, 1, 7, 6, 9).tolist()


def test_caption_entrypoint_sample_mixed_prompts_flag_on_standins(tmp_path, monkeypatch):
    """downstream/run_caption_distributed_gpt3.py --evaluate_only: --eval_sample_mixed_prompts defaults off, needs --eval_sample (or
    --eval_sample_best_of) and --eval_shared_kv, and reaches the SAMPLING call of model.generate as sample_mixed_prompts=True -- not
    the beam-search call; --eval_mixed_prompts still does not touch the sampling call; the result file keeps its format."""
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
    monkeypatch.setenv("MASTER_PORT", str(46000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    seen = []
    gen = downstream.DistributedGPT3_Caption.generate

    def spy(self, image, text, *a, **kw):
        seen.append((kw.get("do_sample", False), kw.get("mixed_prompts", False), kw.get("sample_mixed_prompts", False)))
        return gen(self, image, text, *a, **kw)
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    try:
        out = str(tmp_path / "mixed")
        base = ["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only",
                "--eval_batched_beam", "--eval_shared_kv", "--eval_sample", "2"]
        assert entry.get_args(base)[0].eval_sample_mixed_prompts is False
        for alone in (["--eval_sample_mixed_prompts"], ["--eval_sample_mixed_prompts", "--eval_sample", "2"],
                      ["--eval_sample_mixed_prompts", "--eval_shared_kv"]):
            with pytest.raises(ValueError, match="eval_sample_mixed_prompts"):
                entry.get_args(["--config", cfg, "--output_dir", out, "--evaluate_only"] + alone)
        assert entry.get_args(["--config", cfg, "--output_dir", out, "--evaluate_only", "--eval_shared_kv", "--eval_sample_best_of", "2",
                               "--eval_sample_mixed_prompts"])[0].eval_sample_mixed_prompts is True
        args, config = entry.get_args(base + ["--eval_mixed_prompts", "--eval_sample_mixed_prompts"])
        entry.main(args, config)
        assert seen and set(seen) == {(False, True, False), (True, False, True)}, seen
        merged = json.load(open(os.path.join(out, "result", "val_caption_result.json")))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert len(merged) == 5
    for rec in merged:
        assert set(rec) == {"video_id", "pred_caption", "gold_caption", "sampled_captions"}
        assert len(rec["sampled_captions"]) == 2


# ------------------------------------------------------------------------------------------------ the stand-ins themselves
def test_ragged_standins_are_the_uniform_ones_row_by_row():
    """the tests' own apparatus: a ragged stand-in call equals the uniform stand-in at the common column when every length is equal,
    freezes the rows whose column lies behind the table, and treats lengths -3 and 10**6 as 0 and frozen"""
    import standin_sampling as ss
    from youku_mplug_amd.generation import SampleScores, SampleState
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(4, 16, generator=g).to(BF)
    table = torch.randint(0, 16, (4, 6), generator=g)
    a, b = SampleState(table, torch.tensor([2])), SampleState(table, torch.tensor([2]))
    sra.sample_advance_ragged(logits, a, step=1, top_p=0.9, seed=4, termination_id=3)
    ss.sample_advance(logits, b, pos=3, top_p=0.9, seed=4, termination_id=3)
    assert all(torch.equal(getattr(a, n), getattr(b, n)) for n in SampleState.ARRAYS)
    c = SampleState(table, torch.tensor([-3, 10 ** 6, 5, 0]))
    sc = SampleScores(4, 6, "cpu")
    sra.sample_advance_ragged(logits, c, step=1, seed=4, termination_id=-1)
    sra.sample_score_ragged(logits, c, sc, step=1)
    assert c.done.tolist() == [0, 1, 1, 0] and int(c.n_done) == 2
    assert torch.equal(c.tokens[1:3], table[1:3]) and c.next_tok[1:3].tolist() == table[1:3, -1].tolist()
    assert sc.count.tolist() == [1, 0, 0, 1] and (sc.token_logprob[[0, 3], 1] < 0).all() and (sc.token_logprob[1:3] == 0).all()


# ------------------------------------------------------------------------------------------------ the kernels' budget
def test_ragged_kernels_fit_the_uniform_kernels_budget():
    """the three ragged instantiations in the gfx950 code object: 1024 threads, no scratch, at most 128 registers, and each with the
    registers and the static LDS of its uniform instantiation (the per-row column lives in scalar registers).  Register, LDS and
    scratch figures only, read the way tests/test_isa_cpu.py reads them."""
    import os
    import re
    import subprocess
    import tempfile
    import test_isa_cpu as isa
    from test_sampling_cpu import LLVM
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    pairs = {"sa_rows": ("sa_ragged_entry", "sample_advance_kernel"), "lc_rows": ("lc_ragged_entry", "logits_constrain_kernel"),
             "ss_rows": ("ss_ragged_entry", "sample_score_kernel")}
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for i, blob in enumerate(isa._code_objects()):
            f = os.path.join(d, f"co_{i}.elf")
            open(f, "wb").write(blob)
            txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
            for blk in txt.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                for body, tags in pairs.items():
                    for tag in tags:
                        if body in name and tag in name:
                            g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                            found[(body, tag)] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), scratch=g("private_segment_fixed_size"),
                                                      lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    assert len(found) == 6, sorted(found)
    for body, (ragged, uniform) in pairs.items():
        r, u = found[(body, ragged)], found[(body, uniform)]
        print(f"    {body}: ragged {r}  uniform {u}")
        assert r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 128 and r["threads"] == 1024, (body, r)
        assert (r["vgpr"], r["agpr"], r["lds"]) == (u["vgpr"], u["agpr"], u["lds"]), (body, r, u)


# ------------------------------------------------------------------------------------------------ the library on the host
def _descs(_lib):
    P = 0x10000                                                                          # never dereferenced on the host
    sa = dict(logits=P, prompt_len=P, tokens=P, done=P, next_tok=P, n_done=P, ld=64, rows=2, vocab=64, row_len=8, pos=0, top_k=0, top_p=0.9,
              temperature=1.0)
    lc = dict(logits=P, tokens=P, prompt_len=P, eos_ids=P, banned_ids=P, ld=64, rows=2, vocab=64, row_len=8, pos=0, n_eos=1, n_banned=1, ngram=2,
              min_new_tokens=1, include_prompt=0, penalty=1.2, ban_value=float("-inf"))
    sq = dict(logits=P, tokens=P, prompt_len=P, done=P, live=P, token_logprob=P, sum_logprob=P, count=P, ld=64, rows=2, vocab=64, row_len=8, pos=0)
    return {"sample_advance": (_lib.SampleAdvanceDesc, sa), "logits_constrain": (_lib.LogitsConstrainDesc, lc),
            "sample_score": (_lib.SampleScoreDesc, sq)}


REFUSED = {
    "sample_advance": [dict(logits=0), dict(tokens=0), dict(done=0), dict(next_tok=0), dict(n_done=0), dict(rows=0), dict(vocab=60), dict(vocab=65544, ld=65544),
                       dict(ld=56), dict(ld=68), dict(logits=0x10008), dict(temperature=0.0), dict(temperature=float("inf")), dict(top_k=-1),
                       dict(top_k=65), dict(top_p=1.5), dict(top_k=4), dict(top_k=1), dict(row_len=0), dict(termination_mode=3), dict(vocab_size=-1)],
    "logits_constrain": [dict(logits=0), dict(tokens=0), dict(rows=0), dict(vocab=60), dict(ld=56), dict(logits=0x10008), dict(row_len=0),
                         dict(row_len=2049), dict(penalty=0.0), dict(penalty=float("nan")), dict(ngram=9), dict(ngram=-1), dict(min_new_tokens=-1),
                         dict(include_prompt=2), dict(n_eos=9), dict(eos_ids=0), dict(n_banned=1025), dict(banned_ids=0), dict(ban_value=0.0),
                         dict(ban_value=float("nan"))],
    "sample_score": [dict(logits=0), dict(tokens=0), dict(done=0), dict(live=0), dict(token_logprob=0), dict(sum_logprob=0), dict(count=0), dict(rows=0),
                     dict(vocab=60), dict(ld=56), dict(logits=0x10008), dict(row_len=0), dict(row_len=2049)],
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_library_exports_the_ragged_entries_and_refuses_on_the_host(name):
    """every refusal is a negative code from host-side checks, before any launch: no device is needed (and none is touched).  What the
    uniform entry refuses the ragged one refuses with the same code, under its own name; a step outside [0, row_len) and a NULL
    prompt_len are refused too"""
    from youku_mplug_amd import _lib
    lib = _lib.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(lib, sym)
    cls, base = _descs(_lib)[name]
    uniform, ragged = getattr(lib, "mpv_" + name), getattr(lib, "mpv_" + name + "_ragged")

    def desc(**over):
        d = cls()
        for k, v in dict(base, **over).items():
            setattr(d, k, v)
        return d
    for over in REFUSED[name]:
        rc = ragged(ctypes.byref(desc(**over)), None)
        assert rc < 0, (over, rc)
        assert f"mpv_{name}_ragged:".encode() in lib.mpv_last_error(), (over, lib.mpv_last_error())
        assert rc == uniform(ctypes.byref(desc(**over)), None), over
        assert f"mpv_{name}:".encode() in lib.mpv_last_error()
    for t in (-1, 8, 10 ** 6):
        assert ragged(ctypes.byref(desc(pos=t)), None) == -1, t
        assert f"mpv_{name}_ragged: step".encode() in lib.mpv_last_error()
    assert ragged(ctypes.byref(desc(prompt_len=0)), None) == -5
    assert f"mpv_{name}_ragged: null".encode() in lib.mpv_last_error()
    assert ragged(None, None) == -5
