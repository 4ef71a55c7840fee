"""Sampled captions with the finished clips' slots refilled in flight, on CPU: generation.sample_inflight_loop on the stand-ins
(tests/standin_inflight.py) against sample_batched(mixed_prompts=True) on every clip ALONE with the same streams -- equal tokens and
scores on every column both wrote, whatever the slots, refill_min or the input order --, the number of decode steps the budgets
imply, generate(inflight=True) against sample_mixed_prompts=True, the refusals, the entry point's flag, what the new exports refuse on
the host and the budgets of the new kernel instantiations."""
import ctypes
import types

import pytest
import torch

import standin_inflight as si

BF = torch.bfloat16
LENGTHS = [3, 1, 4, 2, 3]
BUDGETS = [2, 5, 3, 1, 4]
N = 3
NEW_SYMBOLS = ("mpv_attn_decode_shared_steps_fwd", "mpv_gpt_decode_shared_steps_workspace_size", "mpv_gpt_decode_step_shared_steps",
               "mpv_gpt_decode_step_shared_steps_q8", "mpv_sample_advance_steps", "mpv_logits_constrain_steps", "mpv_sample_score_steps")


def _on_cpu(monkeypatch):
    import test_w8_cpu as tw
    dev = tw._on_cpu(monkeypatch)
    si.install(monkeypatch)
    return dev


def _setup(dev, **kw):
    import test_decode_ragged_cpu as tdr
    return tdr._setup(dev, lengths=LENGTHS, **kw)


def _query(model, n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, model.num_learnable_token, model.text_width, generator=g).to(BF)


def simulate(budgets, slots, refill_min):
    """the loop's schedule when no row ever terminates, from its documented rules alone -> (decode steps, prefill passes): a refill
    when refill_min slots are free or nothing runs; a decode step whenever a slot holds a clip that has drawn at least once; a clip
    leaves after `budget` draws"""
    refill_min = min(refill_min, slots)
    steps = prefills = nxt = 0
    running = [None] * slots                                   # per slot: [draws so far, budget]
    while nxt < len(budgets) or any(r is not None for r in running):
        free = [s for s in range(slots) if running[s] is None]
        if nxt < len(budgets) and free and (len(free) >= refill_min or len(free) == slots):
            for s in free[:len(budgets) - nxt]:
                running[s] = [0, budgets[nxt]]
                nxt += 1
            prefills += 1
        if any(r is not None and r[0] >= 1 for r in running):
            steps += 1
        for s in range(slots):
            if running[s] is not None:
                running[s][0] += 1
                if running[s][0] >= running[s][1]:
                    running[s] = None
    return steps, prefills


def lockstep_steps(budgets, per_chunk):
    """decode steps of the lockstep chunks in input order, each run to its longest budget (a chunk's first logits are its prefill's)"""
    return sum(max(budgets[c:c + per_chunk]) - 1 for c in range(0, len(budgets), per_chunk))


def _alone(gpt, ids, qf, c, term, **kw):
    """clip c alone in the lockstep mixed loop, with the streams it has in the call over all clips"""
    return gpt.sample_batched(ids[c:c + 1], query_embeds=qf[c:c + 1], prompt_length=[LENGTHS[c]], num_samples=N, seed=11,
                              streams=torch.arange(c * N, (c + 1) * N), kv="shared_prefix", mixed_prompts=True, return_scores=True,
                              termination_id=term, **kw)


SCHEDULES = [(2, 1, None), (2, 2, None), (3, 1, [4, 2, 0, 3, 1]), (5, 4, None), (1, 1, [1, 0, 2, 4, 3]), (4, None, None)]


@pytest.mark.parametrize("slots,refill_min,order", SCHEDULES)
@pytest.mark.parametrize("terminate", [None, "a row", "a clip"])
def test_inflight_rows_equal_each_clip_alone(monkeypatch, slots, refill_min, order, terminate):
    """5 clips (prompts of 3 / 1 / 4 / 2 / 3 tokens, budgets 2 / 5 / 3 / 1 / 4) through `slots` slots x 3 samples: every clip's rows and
    scores are those of the lockstep mixed loop on that clip alone with the same streams, on every column both wrote; results come
    back in input order; with no termination the loop issues exactly the decode steps and prefills its rules imply.  "a row": a
    termination id that one sample of clip 1 draws ends that row (it is not scored behind it); "a clip": under top_k = 1 all three
    samples draw it, and the clip leaves before its budget"""
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev)
    gpt, ids = model.text_decoder, text.input_ids
    qf = _query(model, len(LENGTHS))
    kw = dict(top_k=1) if terminate == "a clip" else dict(top_p=0.9, temperature=1.1)
    tid = -1                                                                       # no token is -1: nothing ever terminates
    if terminate:                                                                  # a token the model emits: clip 1's second token, sample 0
        probe, _ = _alone(gpt, ids, qf, 1, -1, **kw)
        tid = int(probe[0, LENGTHS[1] + 1])
    order = list(range(len(LENGTHS))) if order is None else order
    sel = torch.tensor(order)
    streams = (sel[:, None] * N + torch.arange(N)[None]).reshape(-1)
    out = gpt.sample_inflight(ids[sel], query_embeds=qf[sel], prompt_length=[LENGTHS[c] for c in order], num_samples=N, slots=slots, seed=11,
                              streams=streams, max_new_tokens=[BUDGETS[c] for c in order], refill_min=refill_min, return_scores=True,
                              termination_id=tid, **kw)
    assert out.tokens.shape[0] == len(order) * N and len(out.written) == len(order)
    ended_early = rows_ended = 0
    for i, c in enumerate(order):
        want, wsc = _alone(gpt, ids, qf, c, tid, **kw)
        pl, b = LENGTHS[c], BUDGETS[c]
        assert pl < out.written[i] <= pl + b
        ended_early += out.written[i] < pl + b
        w = min(out.written[i], want.shape[1])
        rows = slice(i * N, (i + 1) * N)
        assert torch.equal(out.tokens[rows, :w], want[:, :w]), (c, out.tokens[rows], want)
        assert torch.equal(out.scores.token_logprob[rows, :w], wsc.token_logprob[:, :w]), c
        assert (out.scores.token_logprob[rows, w:] == 0).all()                     # nothing behind the clip's last column
        assert torch.equal(out.tokens[rows, :pl], ids[c, :pl].expand(N, -1))
        gen = out.scores.token_logprob[rows, pl:w]
        assert torch.equal(out.scores.count[rows], (gen != 0).sum(1).to(torch.int32))
        rows_ended += int((out.scores.count[rows] < w - pl).sum())
        assert torch.allclose(out.scores.sum_logprob[rows], gen.sum(1), rtol=1e-5, atol=1e-6)
    if not terminate:
        from youku_mplug_amd.generation import refill_min_default
        rm = refill_min_default(slots) if refill_min is None else refill_min
        assert (out.steps, out.prefills) == simulate([BUDGETS[c] for c in order], slots, rm)
        assert all(out.written[i] == LENGTHS[c] + BUDGETS[c] for i, c in enumerate(order))
    elif terminate == "a row":
        assert rows_ended >= 1                                                     # the termination id did end a row before its clip left
    else:
        assert ended_early >= 1                                                    # ... and here a clip before its budget


def test_inflight_issues_fewer_decode_steps_than_the_lockstep_chunks(monkeypatch):
    """2 slots, refills as soon as a slot is free, budgets 2 / 5 / 3 / 1 / 4 in input order: 7 decode steps and 3 prefills, against the 9
    steps of the lockstep chunks of 2 that are held to their longest budget (4 + 2 + 3)"""
    assert simulate(BUDGETS, 2, 1) == (7, 3) and lockstep_steps(BUDGETS, 2) == 9
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev)
    out = model.text_decoder.sample_inflight(text.input_ids, query_embeds=_query(model, 5), prompt_length=LENGTHS, num_samples=N, slots=2,
                                             max_new_tokens=BUDGETS, refill_min=1, termination_id=-1, top_k=1)
    assert (out.steps, out.prefills) == (7, 3) and out.steps < lockstep_steps(BUDGETS, 2)
    assert out.scores is None
    rows = out.tokens.view(5, N, -1)
    assert (rows == rows[:, :1]).all()                                             # top_k = 1: a greedy captioner, every sample the same


CASES = {
    "plain": dict(top_p=1.0),
    "top_k": dict(top_k=5),
    "return_scores": dict(top_p=0.9, temperature=1.2, return_scores=True),
    "best_of": dict(top_p=0.9, best_of=True, length_penalty=1.0, return_scores=True),
    "min_new": dict(top_p=0.9, min_new_tokens=4, return_scores=True),
    "fp8": dict(top_p=0.9, decode_weights="fp8", return_scores=True),
    "constrain_prompt": dict(top_p=0.9, repetition_penalty=1.3, no_repeat_ngram_size=2, constrain_prompt=True, return_scores=True),
    "double_eol": dict(top_p=0.9, stop_on_double_eol=True),
}


@pytest.mark.parametrize("slots", [2, 32])
@pytest.mark.parametrize("case", list(CASES))
def test_generate_inflight_equals_sample_mixed_prompts_on_standins(monkeypatch, case, slots):
    """generate(inflight=True) with every clip's budget open to the end of the table returns what sample_mixed_prompts=True returns:
    rows, scores and the best-of choice, clip by clip"""
    import test_sample_ragged_cpu as tsr
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev)
    kw = dict(termination_id=term, do_sample=True, num_samples=N, seed=11, kv_cache="shared_prefix", clips_per_search=slots, **CASES[case])
    want = model.generate(vid, text, sample_mixed_prompts=True, **kw)
    got = model.generate(vid, text, inflight=True, max_new_tokens=10 ** 6, refill_min=1, **kw)
    assert tsr._same(got, want), (got, want)


def test_generate_inflight_budget_pads_behind_it(monkeypatch):
    """a clip's row behind its budget is padding (the termination id), whatever the input row held there"""
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev)
    res, sc = model.generate(vid, text, termination_id=term, do_sample=True, num_samples=2, kv_cache="shared_prefix", clips_per_search=2,
                             inflight=True, max_new_tokens=BUDGETS, min_new_tokens=100, return_scores=True, top_p=0.9)
    for i, (rows, s) in enumerate(zip(res, sc)):
        assert (rows[:, LENGTHS[i] + BUDGETS[i]:] == term).all() and (rows[:, LENGTHS[i]:LENGTHS[i] + BUDGETS[i]] != term).all()
        assert s["count"].tolist() == [BUDGETS[i]] * 2


def test_inflight_refusals(monkeypatch):
    from youku_mplug_amd import generation
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = _setup(dev)
    ok = dict(termination_id=term, do_sample=True, kv_cache="shared_prefix", inflight=True)
    for bad, word in ((dict(do_sample=False), "do_sample"), (dict(do_sample=False, batched=True), "do_sample"),
                      (dict(kv_cache="per_sequence"), "shared_prefix")):
        with pytest.raises(ValueError, match=word):
            model.generate(vid, text, **dict(ok, **bad))
    with pytest.raises(ValueError, match="shared_prefix"):
        model.generate(vid, text, termination_id=term, do_sample=True, inflight=True)                  # kv_cache default: per_sequence
    for alone in (dict(max_new_tokens=3), dict(refill_min=2)):
        with pytest.raises(ValueError, match="inflight"):
            model.generate(vid, text, termination_id=term, do_sample=True, kv_cache="shared_prefix", **alone)
    gpt, ids = model.text_decoder, text.input_ids
    qf = _query(model, 5)
    call = lambda **kw: gpt.sample_inflight(ids, **dict(dict(query_embeds=qf, prompt_length=LENGTHS, termination_id=term), **kw))
    for lens in (4, None, LENGTHS[:4], [0] + LENGTHS[1:], [ids.shape[1] + 1] + LENGTHS[1:]):
        with pytest.raises(ValueError, match="prompt_length"):
            call(prompt_length=lens)
    for kw, word in ((dict(slots=0), "slots"), (dict(num_samples=0), "num_samples"), (dict(refill_min=0), "refill_min"),
                     (dict(max_new_tokens=0), "max_new_tokens"), (dict(max_new_tokens=[1, 2]), "max_new_tokens"),
                     (dict(streams=torch.arange(4)), "streams"), (dict(decode_weights="int4"), "decode_weights")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    with pytest.raises(ValueError, match="min_new_tokens"):
        call(constraints=generation.LogitsConstraints(min_new_tokens=2), stop_on_double_eol=True)
    with pytest.raises(ValueError, match="score_fn"):
        generation.sample_inflight_loop(generation._gen_config(gpt), generation.make_inflight_state_fn(gpt), ids, prompt_length=LENGTHS,
                                        advance_fn=si.sample_advance_steps, return_scores=True)
    # the position table is checked before the first launch: nothing is installed
    installs = []
    orig = generation.InflightDecodeState.install
    monkeypatch.setattr(generation.InflightDecodeState, "install", lambda self, *a, **k: (installs.append(a), orig(self, *a, **k))[1])
    gpt.config.extra.update(tokens_to_generate=10 ** 4)
    with pytest.raises(ValueError, match="position table"):
        call(max_new_tokens=10 ** 4)
    assert not installs
    gpt.config.extra.update(tokens_to_generate=12)
    st = generation.make_inflight_state_fn(gpt)(2, N, model.num_learnable_token + 4, 3)
    with pytest.raises(ValueError, match="prefix rows"):
        st.install([0], ids[:1, :3], qf[:1], [2])
    with pytest.raises(ValueError, match="distinct"):
        st.install([1, 1], ids[:2, :4], qf[:2], [2, 2])
    with pytest.raises(ValueError, match="suffix"):
        st.step(torch.zeros(2 * N, 1, dtype=torch.long), torch.zeros(2, dtype=torch.int32), 3)
    # the default stays today's loops: no _steps entry and no in-flight state without the keyword
    from youku_mplug_amd import ops
    for name in ("sample_advance_steps", "logits_constrain_steps", "sample_score_steps"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a _steps entry without inflight=True"))
    monkeypatch.setattr(generation, "InflightDecodeState", lambda *a, **k: pytest.fail("an in-flight state without inflight=True"))
    model.generate(vid, text, termination_id=term, do_sample=True, num_samples=2, kv_cache="shared_prefix", sample_mixed_prompts=True,
                   return_scores=True, repetition_penalty=1.2)


def test_caption_entrypoint_sample_inflight_flag_on_standins(tmp_path, monkeypatch):
    """downstream/run_caption_distributed_gpt3.py --evaluate_only: --eval_sample_inflight defaults off, needs --eval_sample (or
    --eval_sample_best_of) and --eval_shared_kv, is refused with --eval_sample_mixed_prompts, and reaches the SAMPLING call of
    model.generate as inflight=True -- not the beam-search call; the result file keeps its format."""
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
    monkeypatch.setenv("MASTER_PORT", str(48000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    seen = []
    gen = downstream.DistributedGPT3_Caption.generate

    def spy(self, image, text, *a, **kw):
        seen.append((kw.get("do_sample", False), kw.get("inflight", False), kw.get("sample_mixed_prompts", False)))
        return gen(self, image, text, *a, **kw)
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    try:
        out = str(tmp_path / "inflight")
        base = ["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only",
                "--eval_batched_beam", "--eval_shared_kv", "--eval_sample", "2"]
        assert entry.get_args(base)[0].eval_sample_inflight is False
        for alone in (["--eval_sample_inflight"], ["--eval_sample_inflight", "--eval_sample", "2"], ["--eval_sample_inflight", "--eval_shared_kv"],
                      ["--eval_sample_inflight", "--eval_shared_kv", "--eval_sample", "2", "--eval_sample_mixed_prompts"]):
            with pytest.raises(ValueError, match="eval_sample_inflight"):
                entry.get_args(["--config", cfg, "--output_dir", out, "--evaluate_only"] + alone)
        assert entry.get_args(["--config", cfg, "--output_dir", out, "--evaluate_only", "--eval_shared_kv", "--eval_sample_best_of", "2",
                               "--eval_sample_inflight"])[0].eval_sample_inflight is True
        args, config = entry.get_args(base + ["--eval_sample_inflight"])
        entry.main(args, config)
        assert seen and set(seen) == {(False, False, False), (True, True, False)}, seen
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
def test_steps_standins_are_the_ragged_ones_at_a_common_step():
    """the tests' own apparatus: a _steps stand-in call equals the ragged stand-in when every row_step is that step, and freezes rows
    with a negative step or a column behind the table"""
    import standin_sample_ragged as sra
    from youku_mplug_amd.generation import SampleScores, SampleState
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(4, 16, generator=g).to(BF)
    table = torch.randint(0, 16, (4, 6), generator=g)
    a, b = SampleState(table, torch.tensor([2, 1, 0, 3])), SampleState(table, torch.tensor([2, 1, 0, 3]))
    sa, sb = SampleScores(4, 6, "cpu"), SampleScores(4, 6, "cpu")
    si.sample_advance_steps(logits, a, row_step=torch.full((4,), 2, dtype=torch.int32), top_p=0.9, seed=4, termination_id=3)
    si.sample_score_steps(logits, a, sa, row_step=torch.full((4,), 2, dtype=torch.int32))
    sra.sample_advance_ragged(logits, b, step=2, top_p=0.9, seed=4, termination_id=3)
    sra.sample_score_ragged(logits, b, sb, step=2)
    assert all(torch.equal(getattr(a, n), getattr(b, n)) for n in SampleState.ARRAYS)
    assert all(torch.equal(getattr(sa, n), getattr(sb, n)) for n in SampleScores.ARRAYS)
    c = SampleState(table, torch.tensor([2, 1, 0, 3]))
    sc = SampleScores(4, 6, "cpu")
    steps = torch.tensor([2, -1, 6, 0], dtype=torch.int32)
    si.sample_advance_steps(logits, c, row_step=steps, seed=4, termination_id=-1)
    si.sample_score_steps(logits, c, sc, row_step=steps)
    assert c.done.tolist() == [0, 1, 1, 0] and int(c.n_done) == 2
    assert torch.equal(c.tokens[1:3], table[1:3]) and c.next_tok[1:3].tolist() == table[1:3, -1].tolist()
    assert sc.count.tolist() == [1, 0, 0, 1] and sc.token_logprob[0, 4] < 0 and sc.token_logprob[3, 3] < 0


# ------------------------------------------------------------------------------------------------ the kernels' budget
def test_steps_kernels_fit_their_siblings_budget():
    """the new instantiations in the gfx950 code object -- the three sampler-side _steps entries and the decode attention's steps
    kernel at head_dim 64 and 80 --: no scratch, and the registers and static LDS of their uniform siblings (the per-row step and the
    per-group own length live in scalar registers).  Read the way tests/test_isa_cpu.py reads them."""
    import os
    import re
    import subprocess
    import tempfile
    import test_isa_cpu as isa
    if not os.path.isfile(os.path.join(isa.LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    pairs = {("sa_rows", "sa_steps_entry"): ("sa_rows", "sample_advance_kernel"), ("lc_rows", "lc_steps_entry"): ("lc_rows", "logits_constrain_kernel"),
             ("ss_rows", "ss_steps_entry"): ("ss_rows", "sample_score_kernel"),
             ("attn_decode_shared_steps_kernel", "ILi64E"): ("attn_decode_shared_kernel", "ILi64E"),
             ("attn_decode_shared_steps_kernel", "ILi80E"): ("attn_decode_shared_kernel", "ILi80E")}
    keys = set(pairs) | set(pairs.values())
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for i, blob in enumerate(isa._code_objects()):
            f = os.path.join(d, f"co_{i}.elf")
            open(f, "wb").write(blob)
            txt = subprocess.run([os.path.join(isa.LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
            for blk in txt.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                for body, tag in keys:
                    if body in name and tag in name:
                        g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                        assert (body, tag) not in found, name
                        found[(body, tag)] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), scratch=g("private_segment_fixed_size"),
                                                  lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    assert len(found) == 10, sorted(found)
    for new, old in pairs.items():
        a, b = found[new], found[old]
        print(f"    {new}: {a}  {old}: {b}")
        assert a["scratch"] == 0 and a == b, (new, a, b)


# ------------------------------------------------------------------------------------------------ the library on the host
@pytest.mark.parametrize("name", ["sample_advance", "logits_constrain", "sample_score"])
def test_library_exports_the_steps_entries_and_refuses_on_the_host(name):
    """every refusal is a negative code from host-side checks, before any launch: no device is needed (and none is touched).  What the
    ragged entry refuses the _steps one refuses with the same code, under its own name (d->pos is ignored: the step comes per row); a
    NULL row_step and a NULL prompt_len are refused too"""
    import test_sample_ragged_cpu as tsr
    from youku_mplug_amd import _lib
    lib = _lib.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(lib, sym)
    cls, base = tsr._descs(_lib)[name]
    ragged, steps = getattr(lib, "mpv_" + name + "_ragged"), getattr(lib, "mpv_" + name + "_steps")
    P = 0x10000

    def desc(**over):
        d = cls()
        for k, v in dict(base, **over).items():
            setattr(d, k, v)
        return d
    for over in tsr.REFUSED[name]:
        rc = steps(ctypes.byref(desc(**over)), P, None)
        assert rc < 0, (over, rc)
        assert f"mpv_{name}_steps:".encode() in lib.mpv_last_error(), (over, lib.mpv_last_error())
        assert rc == ragged(ctypes.byref(desc(**over)), None), over
        rc8 = steps(ctypes.byref(desc(pos=10 ** 6, **over)), P, None)                 # d->pos does not matter to the refusal either
        assert rc8 == rc, over
    assert steps(ctypes.byref(desc()), None, None) == -5
    assert f"mpv_{name}_steps: null row_step".encode() in lib.mpv_last_error()
    assert steps(ctypes.byref(desc(prompt_len=0)), P, None) == -5
    assert f"mpv_{name}_steps: null".encode() in lib.mpv_last_error()
    assert steps(None, P, None) == -5


def test_library_refuses_the_steps_attention_and_driver_on_the_host():
    """mpv_attn_decode_shared_steps_fwd refuses what the ragged entry refuses, with its code and under its own name, and a NULL own
    length array; the two drivers refuse what the ragged drivers refuse with max_t in t's place, and a NULL group_t"""
    import test_decode_shared_cpu as tds
    from youku_mplug_amd import _lib
    lib = _lib.lib()
    P = 0x10000
    for over in (dict(head_dim=96), dict(own_len=0), dict(own_len=2049), dict(prefix_len=0), dict(group_size=0), dict(n_groups=3),
                 dict(pv_gs=11 * 768 + 2), dict(o_ss=258), dict(q=0x10008), dict(pk=0), dict(scale=0.0), dict(n_seq=0)):
        rc = lib.mpv_attn_decode_shared_steps_fwd(ctypes.byref(tds._desc(**over)), P, P, None)
        assert rc < 0, (over, rc)
        assert b"mpv_attn_decode_shared_steps_fwd" in lib.mpv_last_error()
        assert rc == lib.mpv_attn_decode_shared_ragged_fwd(ctypes.byref(tds._desc(**over)), P, None), over
    assert lib.mpv_attn_decode_shared_steps_fwd(ctypes.byref(tds._desc()), None, P, None) == -5
    assert b"mpv_attn_decode_shared_steps_fwd: null group_prefix_len" in lib.mpv_last_error()
    assert lib.mpv_attn_decode_shared_steps_fwd(ctypes.byref(tds._desc()), P, None, None) == -5
    assert b"mpv_attn_decode_shared_steps_fwd: null group_own_len" in lib.mpv_last_error()
    w = _lib.GptWeights()
    w.layers, w.hidden, w.heads, w.ffn, w.vocab, w.max_positions = 2, 256, 4, 1024, 1024, 64
    q8 = _lib.GptWeightsQ8()
    q8.layers = 1
    tab = (ctypes.c_void_p * 2)(P, P)
    big = 1 << 40                                                                      # (a workspace size: never touched)
    assert lib.mpv_gpt_decode_shared_steps_workspace_size(ctypes.byref(w), 6) == \
        lib.mpv_gpt_decode_shared_workspace_size(ctypes.byref(w), 6) + 6 * 3 * 256 * 2 + 256
    step = lambda **o: lib.mpv_gpt_decode_step_shared_steps(ctypes.byref(w), tab, tab, 2, 3, o.get("stride", 20), o.get("glen", P),
                                                            o.get("maxp", 20), 8, o.get("gt", P), o.get("t", 0), P, P, o.get("ws", big), P, None)
    ragged = lambda **o: lib.mpv_gpt_decode_step_shared_ragged(ctypes.byref(w), tab, tab, 2, 3, o.get("stride", 20), o.get("glen", P),
                                                               o.get("maxp", 20), 8, o.get("t", 0), P, P, big, P, None)
    for o in (dict(glen=None), dict(stride=19), dict(maxp=60, stride=60, t=4), dict(t=8), dict(t=-1)):
        rc = step(**o)
        assert rc < 0 and rc == ragged(**o), o
        step(**o)
        assert b"mpv_gpt_decode_step_shared_steps:" in lib.mpv_last_error()
    assert step(gt=None) == -5 and b"mpv_gpt_decode_step_shared_steps: null group_t" in lib.mpv_last_error()
    assert step(ws=lib.mpv_gpt_decode_shared_workspace_size(ctypes.byref(w), 6)) == -5 and b"workspace too small" in lib.mpv_last_error()
    assert lib.mpv_gpt_decode_step_shared_steps_q8(ctypes.byref(w), ctypes.byref(q8), tab, tab, 2, 3, 20, P, 20, 8, P, 0, P, P, big, P, None) == -5
    assert b"mpv_gpt_decode_step_shared_steps_q8" in lib.mpv_last_error()
