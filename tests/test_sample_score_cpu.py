"""Sequence scores of sampled generation, checked without a GPU: the restatement tests/standin_sample_score.py
against an fp64 definition on the committed launches of tests/sample_score_cases.py; sample_batched_loop with the restatement as
score_fn (same tokens, exactly the positions in [prompt_len, first termination] scored, in every termination mode and with early
termination off, never called and nothing allocated without return_scores, today's call sequence); the refusals of the other loops;
DistributedGPT3_Caption.generate (return shapes, the best_of rule) and the caption entry point's flag on the stand-ins; the library's
refusals on the host, the ctypes mirror of the descriptor and the kernel's register / LDS / scratch figures in the built code object."""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import sample_score_cases as cases
import standin_constrain as sk
import standin_sample_score as sq
import standin_sampling as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LLVM = "/opt/rocm/lib/llvm/bin"


# ------------------------------------------------------------------------------ the committed launches
def test_case_list_covers_what_it_claims():
    C = cases.CASES
    assert len({cases.case_id(c) for c in C}) == len(C)
    assert {c["V"] for c in C} == {8, 64, 520, 8192, 51200, 65536} and {c["rows"] for c in C} == {1, 3, 160} and {c["row_len"] for c in C} == {1, 37, 2048}
    for V in (8, 64, 520, 8192, 51200, 65536):
        assert {c["ldx"] for c in C if c["V"] == V} == {0, 8}, V
    for L in (1, 37, 2048):
        assert {c["pos"] for c in C if c["row_len"] == L} == {0, L - 1}, L
    assert {cases.role_of(c, 0) for c in C if c["rows"] == 1} == set(cases.ROLES)
    pairs = {(cases.role_of(c, r), cases.variant_of(c, r)) for c in C for r in range(c["rows"])}
    assert pairs == {(a, b) for a in cases.ROLES for b in cases.VARIANTS}                             # every kind of row is scored, ends, is skipped
    assert all({cases.role_of(c, r) for r in range(160)} == set(cases.ROLES) and {cases.variant_of(c, r) for r in range(160)} == set(cases.VARIANTS)
               for c in C if c["rows"] == 160)
    b = cases.build(C[1])
    assert b.logits.shape[1] == C[1]["V"] + 8 and torch.isnan(b.logits[:, C[1]["V"]:].float()).all()
    finite = b.logits[:, :C[1]["V"]].float()
    assert (finite[finite > float("-inf")].abs() <= 64).all()


@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_standin_equals_the_fp64_definition(c):
    b = cases.build(c)
    st, sc_, table = cases.states(b)
    assert sq.sample_score(b.logits, st, sc_, pos=c["pos"], vocab=c["V"]) is sc_
    pos, V = c["pos"], c["V"]
    keep = torch.ones_like(b.table, dtype=torch.bool)
    worst = 0.0
    for r in range(c["rows"]):
        role = cases.role_of(c, r)
        if role in ("forced", "dead"):
            assert int(sc_.count[r]) == int(b.count[r]) and int(sc_.live[r]) == int(b.live[r]) and float(sc_.sum_logprob[r]) == float(b.sum_logprob[r])
            continue
        keep[r * c["row_len"] + pos] = False
        lp, want = float(sc_.token_logprob[r, pos]), sq.logprob_row_fp64(b.logits[r, :V], int(b.tokens[r, pos]))
        if cases.variant_of(c, r) in ("token_neg_inf", "all_neg_inf"):
            assert want == -math.inf and lp == -math.inf, (r, lp, want)
        else:
            assert math.isfinite(want) and abs(lp - want) <= cases.GATE, (r, lp, want)
            worst = max(worst, abs(lp - want))
        assert int(sc_.count[r]) == int(b.count[r]) + 1 and int(sc_.live[r]) == (0 if role == "ends" else 1)
        assert float(sc_.sum_logprob[r]) == float(b.sum_logprob[r] + sc_.token_logprob[r, pos])
    assert cases.same_bits(table[keep], b.table[keep])                       # the canaries: skipped rows, other columns, the tail
    print(f"    stand-in vs fp64: max |lp - lp64| = {worst:.3e}")


def test_standin_misuse_and_refusals():
    from youku_mplug_amd.generation import SampleScores, SampleState
    st = SampleState(torch.tensor([[1, 99, 0], [2, -1, 0]]), torch.zeros(2, dtype=torch.long))
    sc_ = SampleScores(2, 3, "cpu")
    assert sc_.live.tolist() == [1, 1] and sc_.count.tolist() == [0, 0] and not sc_.token_logprob.any() and not sc_.sum_logprob.any()
    assert SampleScores.ARRAYS == ("live", "token_logprob", "sum_logprob", "count") and sc_.live.dtype == torch.int32 and sc_.count.dtype == torch.int32
    sq.sample_score(torch.zeros(2, 16), st, sc_, pos=1)
    assert torch.isnan(sc_.token_logprob[:, 1]).all() and torch.isnan(sc_.sum_logprob).all()      # a token outside [0, vocab): loud
    ok = dict(pos=1)
    for logits, bad in ((torch.zeros(2, 12), {}), (torch.zeros(2, 4), {}), (torch.zeros(2, 16), dict(vocab=8, ld=4)), (torch.zeros(2, 16), dict(vocab=8, ld=12)),
                        (torch.zeros(2, 16), dict(pos=3)), (torch.zeros(2, 16), dict(pos=-1)), (None, {})):
        with pytest.raises(AssertionError):
            sq.sample_score(logits, st, SampleScores(2, 3, "cpu"), **{**ok, **bad})
    big = types.SimpleNamespace(rows=1, row_len=2049, tokens=torch.zeros(1, 2049, dtype=torch.long), prompt_len=torch.zeros(1, dtype=torch.long),
                                done=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(AssertionError):
        sq.sample_score(torch.zeros(1, 16), big, SampleScores(1, 2049, "cpu"), pos=0)


# ------------------------------------------------------------------------------ the loop
def _terminated(tok, prev, mode, tid):
    return ss._terminated(tok, prev, mode, tid)


def _expected_mask(tokens, lengths, mode, tid):
    """bool [R, n]: the positions in [prompt_len, first termination] of every row of the loop's output"""
    R, n = tokens.shape
    mask = torch.zeros((R, n), dtype=torch.bool)
    for r in range(R):
        for c in range(int(lengths[r]), n):
            mask[r, c] = True
            if _terminated(int(tokens[r, c]), int(tokens[r, c - 1]) if c > 0 else -1, mode, tid):
                break
    return mask


def _scored_run(make_state, cfg, tokens, lengths, record=None, constraints=None, **kw):
    """sample_batched_loop with return_scores=True on the stand-ins; the score_fn notes, per call, which rows it scored and the fp64
    log-probability of the token from a CLONE of the logits it was handed -> (tokens, scores, mask, lp64)"""
    from youku_mplug_amd import generation
    seen = {}

    def constrain(logits, toks, **k):
        if record is not None:
            record.append(("constrain", logits))
        return sk.logits_constrain(logits, toks, **k)

    def advance(logits, st, **k):
        if record is not None:
            record.append(("advance", logits))
        return ss.sample_advance(logits, st, **k)

    def score(logits, st, sc_, *, pos):
        if record is not None:
            record.append(("score", logits))
        before, lg = sc_.count.clone(), logits.clone()
        out = sq.sample_score(logits, st, sc_, pos=pos)
        assert torch.equal(lg, logits)                                       # the score reads, never edits
        seen[pos] = (sc_.count != before, [sq.logprob_row_fp64(lg[r], int(st.tokens[r, pos])) for r in range(st.rows)])
        return out
    toks, sc_ = generation.sample_batched_loop(cfg, make_state, tokens.clone(), prompt_length=lengths.clone(), advance_fn=advance,
                                               constraints=constraints, constrain_fn=constrain, return_scores=True, score_fn=score, **kw)
    R, n = toks.shape
    mask, lp64 = torch.zeros((R, n), dtype=torch.bool), torch.zeros((R, n), dtype=torch.float64)
    for pos, (m, lp) in seen.items():
        mask[:, pos], lp64[:, pos] = m, torch.tensor(lp, dtype=torch.float64)
    return toks, sc_, mask, lp64


def _check_scores(toks, sc_, mask, lp64, lengths_rows, mode, tid):
    want = _expected_mask(toks, lengths_rows, mode, tid)
    assert torch.equal(mask, want), (mask.int().tolist(), want.int().tolist())
    assert sc_.token_logprob.shape == toks.shape and sc_.token_logprob.dtype == torch.float32
    assert torch.equal(sc_.count, want.sum(dim=1).to(torch.int32))
    assert (sc_.token_logprob[~want] == 0).all()                             # teacher-forced positions and those behind the termination
    assert ((sc_.token_logprob.double() - lp64)[want].abs() <= cases.GATE).all()
    for r in range(toks.shape[0]):                                           # the sum runs in position order, in fp32
        acc = torch.zeros((), dtype=torch.float32)
        for c in want[r].nonzero().view(-1).tolist():
            acc = acc + sc_.token_logprob[r, c]
        assert float(acc) == float(sc_.sum_logprob[r]), r


@pytest.mark.parametrize("mode,kw", [("id", dict(termination_id=9)), ("eol", dict(stop_on_eol=True)), ("double_eol", dict(stop_on_double_eol=True))])
@pytest.mark.parametrize("early", [True, False])
def test_loop_scores_exactly_the_generated_positions_up_to_the_termination(mode, kw, early):
    """ragged prompts on scripted logits: the tokens of return_scores=False bit for bit; the scored positions are those in
    [prompt_len, first termination], count is their number, everything else stays 0 -- with the loop stopping early and running on"""
    import test_sampling_cpu as ts
    from youku_mplug_amd import generation
    script = [[5, 9, 198, 7, 198, 198, 628, 3], [9, 9, 198, 198, 198, 198, 628, 3], [4, 4, 4, 9, 198, 628, 3, 3]]
    if mode == "double_eol":
        script = [[5, 198, 7, 198, 198, 3, 3, 3], [4, 4, 198, 198, 3, 3, 3, 3], [198, 198, 198, 198, 3, 3, 3, 3]]
    cfg = types.SimpleNamespace(tokens_to_generate=8, eod_id=7 if mode == "id" else 639, max_position_embeddings=40, top_k=1, top_p=0.0, vocab_size=640)
    tokens, lengths = torch.tensor([[1, 2, 0, 0], [3, 4, 5, 0], [6, 198, 8, 9]]), torch.tensor([2, 3, 4])
    make = lambda b, m: ts._ScriptState(script, 640)
    kw = dict(kw, use_eod_token_for_early_termination=early)
    plain = generation.sample_batched_loop(cfg, make, tokens.clone(), prompt_length=lengths.clone(), advance_fn=ss.sample_advance, **kw)
    toks, sc_, mask, lp64 = _scored_run(make, cfg, tokens, lengths, **kw)
    assert isinstance(plain, torch.Tensor) and torch.equal(toks, plain)
    m = {"id": 0, "eol": 1, "double_eol": 2}[mode]
    _check_scores(toks, sc_, mask, lp64, lengths, m, 9)
    assert (sc_.count > 0).all()
    if not early:
        assert toks.shape[1] == 12 and (sc_.live == 0).all()                 # every script terminates: nothing is live at the end


@pytest.mark.parametrize("Q", [0, 2])
def test_loop_scores_on_the_stub_model_with_samples_and_constraints(Q):
    """the stub of the sampling tests (ragged prompts, top-p, three samples per clip, with and without a query prefix): same tokens as
    the plain call; with constraints the score is that of the EDITED logits -- the tensor advance_fn read"""
    import test_sampling_cpu as ts
    from youku_mplug_amd import generation
    stub, cfgd, tokens, lengths = ts._sample_case(Q)
    cfg = types.SimpleNamespace(**cfgd, top_k=0, top_p=0.9, vocab_size=stub.vocab)
    N = 3
    qe = torch.zeros(tokens.shape[0], Q, 4) if Q else None
    make = lambda b, m: ts._FanStubState(stub, b, m, pad_to=32)
    for constraints in (None, generation.LogitsConstraints(no_repeat_ngram_size=1, min_new_tokens=2, repetition_penalty=1.3)):
        common = dict(query_embeds=qe, temperature=1.1, seed=2024, num_samples=N)
        plain = generation.sample_batched_loop(cfg, make, tokens.clone(), prompt_length=lengths.clone(), advance_fn=ss.sample_advance,
                                               constraints=constraints, constrain_fn=sk.logits_constrain, **common)
        rec = []
        toks, sc_, mask, lp64 = _scored_run(make, cfg, tokens, lengths, record=rec, constraints=constraints, **common)
        assert torch.equal(toks, plain)
        _check_scores(toks, sc_, mask, lp64, lengths.repeat_interleave(N), 0, cfgd["eod_id"])
        assert torch.isfinite(sc_.sum_logprob).all() and (sc_.sum_logprob < 0).all()
        names = [r[0] for r in rec]
        per = ["constrain", "advance", "score"] if constraints is not None else ["advance", "score"]
        assert names == per * (len(names) // len(per))
        for i in range(0, len(rec), len(per)):
            assert all(r[1] is rec[i][1] for r in rec[i:i + len(per)])          # one logits tensor per step: edited, sampled, scored


def test_without_return_scores_nothing_is_called_allocated_or_launched(monkeypatch):
    import test_logits_constrain_cpu as tc
    import test_sampling_cpu as ts
    from youku_mplug_amd import generation

    def boom(*a, **k):
        raise AssertionError("score_fn / SampleScores must not be touched without return_scores")
    stub, cfgd, tokens, lengths = ts._sample_case(0)
    cfg = types.SimpleNamespace(**cfgd, top_k=0, top_p=0.9, vocab_size=stub.vocab)
    make = lambda b, m: ts._FanStubState(stub, b, m, pad_to=32)
    c = generation.LogitsConstraints(no_repeat_ngram_size=2)
    rec = []
    base, _, _ = tc._sample_run(c, rec, num_samples=2)                       # today's call sequence, as the constraint tests count it
    today = [r[0] for r in rec]
    assert today == ["constrain", "advance"] * (len(today) // 2)
    monkeypatch.setattr(generation, "SampleScores", boom)
    rec2 = []

    def constrain(logits, toks, **k):
        rec2.append("constrain")
        return sk.logits_constrain(logits, toks, **k)

    def advance(logits, st, **k):
        rec2.append("advance")
        return ss.sample_advance(logits, st, **k)
    for kw in (dict(), dict(return_scores=False), dict(score_fn=boom), dict(return_scores=False, score_fn=boom)):
        rec2.clear()
        out = generation.sample_batched_loop(cfg, make, tokens.clone(), prompt_length=lengths.clone(), advance_fn=advance, constraints=c,
                                             constrain_fn=constrain, temperature=1.1, seed=3, num_samples=2, **kw)
        assert isinstance(out, torch.Tensor) and torch.equal(out, base) and rec2 == today, kw
    with pytest.raises(ValueError, match="score_fn"):
        generation.sample_batched_loop(cfg, make, tokens.clone(), prompt_length=lengths.clone(), advance_fn=ss.sample_advance, return_scores=True)


def test_the_other_loops_and_entry_points_refuse_the_keyword():
    from youku_mplug_amd import generation
    for fn in (generation.sample_loop, generation.beam_search_loop, generation.beam_search_batched_loop):
        with pytest.raises(ValueError, match="return_scores"):
            fn(None, None, torch.tensor([[1, 2]]), return_scores=True)
    calls = []

    class G:
        training = False
        config = None
        def eval(self): pass
        def train(self, was): pass
        def sample(self, tokens, **kw): calls.append(("sample", kw)); return "s"
        def sample_batched(self, tokens, **kw): calls.append(("sample_batched", kw)); return "d"
        def beam_search(self, tokens, **kw): calls.append(("beam", kw)); return "b"
    real = types.SimpleNamespace()
    generation.install(real)
    assert real.generate(G(), None, termination_id=3, sampler="device", return_scores=True) == "d"
    assert calls == [("sample_batched", dict(termination_id=3, return_scores=True))]
    for kw in (dict(), dict(sampler="torch"), dict(do_sample=False), dict(do_sample=False, sampler="device")):
        with pytest.raises(ValueError, match="return_scores"):
            real.generate(G(), None, return_scores=True, **kw)
    assert len(calls) == 1
    assert real.generate(G(), None, termination_id=3, return_scores=False) == "s" and calls[-1] == ("sample", dict(termination_id=3))
    for name in ("sample", "beam_search", "beam_search_batched"):
        with pytest.raises(ValueError, match="return_scores"):
            getattr(real, name)(G(), torch.tensor([[1, 2]]), return_scores=True)


# ------------------------------------------------------------------------------ the model and the entry point on the stand-ins
def _on_cpu(monkeypatch):
    import standin_beam
    import test_pipeline_cpu as tp
    from youku_mplug_amd import ops
    dev = tp._on_cpu(monkeypatch)
    monkeypatch.setattr(ops, "sample_advance", ss.sample_advance)
    monkeypatch.setattr(ops, "beam_advance", standin_beam.beam_advance)
    monkeypatch.setattr(ops, "logits_constrain", sk.logits_constrain)
    monkeypatch.setattr(ops, "sample_score", sq.sample_score)
    return dev


def test_best_sample_rule():
    from youku_mplug_amd.downstream import best_sample
    s, c = torch.tensor([-6.0, -4.0, -9.0, -4.5]), torch.tensor([2, 1, 4, 3], dtype=torch.int32)
    assert best_sample(s, c, 0.0) == 1                                       # the plain sum: -4
    assert best_sample(s, c, 1.0) == 3                                       # per token: -3, -4, -2.25, -1.5
    assert best_sample(s, c, 2.0) == 3                                       # -1.5, -4, -0.5625, -0.5
    assert best_sample(torch.tensor([-9.0, -8.0, -8.0]), torch.tensor([3, 4, 4], dtype=torch.int32), 2.0) == 1      # -1, -0.5, -0.5: a tie, the lower index
    assert best_sample(torch.tensor([-2.0, -2.0]), torch.tensor([1, 1], dtype=torch.int32)) == 0
    for lp in (0.0, 1.0, 2.0):                                               # count 0 (sum 0, the largest number here) is never chosen
        assert best_sample(torch.tensor([0.0, -50.0, 0.0]), torch.tensor([0, 5, 0], dtype=torch.int32), lp) == 1
    assert best_sample(torch.tensor([0.0, 0.0]), torch.tensor([0, 0], dtype=torch.int32)) == 0
    assert best_sample(torch.tensor([-math.inf, -3.0]), torch.tensor([2, 2], dtype=torch.int32)) == 1


def test_caption_generate_scores_and_best_of_on_standins(monkeypatch):
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict
    from youku_mplug_amd import generation
    from youku_mplug_amd.downstream import best_sample, synthetic_gencls_model
    dev = _on_cpu(monkeypatch)
    m = torch.load(os.path.join(GOLD, "caption_tiny.pt"))["meta"]
    model = synthetic_gencls_model(CONFIG_TINY, "caption", device=dev)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in make_state_dict(CONFIG_TINY, m["weight_seed"]).items()}, strict=True)
    model.text_decoder.config.extra.update(tokens_to_generate=m["tokens_to_generate"], eod_id=m["eod_id"])
    video, ids, mask = make_inputs(CONFIG_TINY, m["batch"], m["text_len"], seed=m["input_seed"], ragged=False)
    mask[1, 4:] = 0
    video = video.to(torch.bfloat16)
    sel = [0, 1, 0]
    text = types.SimpleNamespace(input_ids=ids[sel], attention_mask=mask[sel])
    N, Lt = 4, ids.shape[1] + m["tokens_to_generate"]
    kw = dict(termination_id=m["eod_id"], do_sample=True, num_samples=N, seed=5, temperature=1.2, top_p=0.9)
    for bad in (dict(return_scores=True), dict(best_of=True), dict(return_scores=True, batched=True), dict(best_of=True, batched=True)):
        with pytest.raises(ValueError, match="do_sample=True"):
            model.generate(video[sel], text, termination_id=m["eod_id"], **bad)
    seen = []
    orig = generation.sample_batched_loop

    def spy(cfg, make_state, tokens, **k):
        seen.append((k.get("return_scores", False), k.get("score_fn")))
        return orig(cfg, make_state, tokens, **k)
    monkeypatch.setattr(generation, "sample_batched_loop", spy)
    base = model.generate(video[sel], text, **kw)
    assert seen and all(s == (False, None) for s in seen)                    # keywords absent: today's call
    seen.clear()
    res, scores = model.generate(video[sel], text, return_scores=True, **kw)
    assert seen and all(s == (True, sq.sample_score) for s in seen)
    assert len(res) == len(scores) == 3 and all(torch.equal(a, b) for a, b in zip(res, base))
    for i, (r, s) in enumerate(zip(res, scores)):
        assert set(s) == {"sum_logprob", "count", "token_logprob"} and all(not v.is_cuda for v in s.values())
        assert s["sum_logprob"].shape == (N,) and s["sum_logprob"].dtype == torch.float32 and s["count"].shape == (N,) and s["count"].dtype == torch.int32
        assert s["token_logprob"].shape == (N, Lt) and s["token_logprob"].dtype == torch.float32 and r.shape == (N, Lt)
        n_prompt = int(mask[sel[i]].sum()) - 1
        for q in range(N):                                                   # scored: the generated tokens up to and including the termination
            gen = r[q, n_prompt:].tolist()
            end = gen.index(m["eod_id"]) + 1 if m["eod_id"] in gen else len(gen)
            assert int(s["count"][q]) == end and (s["token_logprob"][q, :n_prompt] == 0).all() and (s["token_logprob"][q, n_prompt + end:] == 0).all()
            assert (s["token_logprob"][q, n_prompt:n_prompt + end] < 0).all()
            assert abs(float(s["token_logprob"][q].double().sum()) - float(s["sum_logprob"][q])) < 1e-4
    assert not torch.equal(scores[0]["sum_logprob"], scores[2]["sum_logprob"])                      # other streams, other samples
    for lp in (0.0, 1.0, 2.0):
        best, bsc = model.generate(video[sel], text, return_scores=True, best_of=True, length_penalty=lp, **kw)
        only = model.generate(video[sel], text, best_of=True, length_penalty=lp, **kw)
        for i in range(3):
            b = best_sample(scores[i]["sum_logprob"], scores[i]["count"], lp)
            ref = [float(scores[i]["sum_logprob"][q]) / float(scores[i]["count"][q]) ** lp for q in range(N)]
            assert b == max(range(N), key=lambda q: (ref[q], -q)) and bsc[i]["index"] == b
            assert best[i].shape == (1, Lt) and torch.equal(best[i], res[i][b:b + 1]) and torch.equal(only[i], best[i])
            assert torch.equal(bsc[i]["token_logprob"], scores[i]["token_logprob"][b:b + 1]) and bsc[i]["sum_logprob"].shape == (1,)
            assert float(bsc[i]["sum_logprob"]) == float(scores[i]["sum_logprob"][b]) and int(bsc[i]["count"]) == int(scores[i]["count"][b])
    # the chunking does not move the tokens (and on the stand-ins, whose logits do not depend on the row count, not the scores either)
    res1, scores1 = model.generate(video[sel], text, return_scores=True, clips_per_search=1, **kw)
    assert all(torch.equal(a, b) for a, b in zip(res1, res)) and all(torch.equal(a["sum_logprob"], b["sum_logprob"]) for a, b in zip(scores1, scores))
    # constraints and the shared-prefix keyword go through together with the scores
    con, csc = model.generate(video[sel], text, return_scores=True, no_repeat_ngram_size=1, min_new_tokens=2, **kw)
    assert all(torch.isfinite(s["sum_logprob"]).all() and (s["count"] >= 2).all() for s in csc)


def test_caption_entrypoint_best_of_flag_on_standins(tmp_path, monkeypatch):
    """--eval_sample_best_of 3: default 0; reaches model.generate as do_sample / num_samples / best_of (with the constraint flags and
    --eval_shared_kv), replaces the beam search, and the result file carries one caption per clip in the beam evaluation's format"""
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
        out = gen(self, image, text, *a, **kw)
        seen.append((kw, out))
        return out
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    try:
        out = str(tmp_path / "best_of")
        base = ["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only"]
        assert entry.get_args(base)[0].eval_sample_best_of == 0
        with pytest.raises(ValueError, match="eval_sample_best_of"):
            entry.get_args(base + ["--eval_sample_best_of", "-1"])
        args, config = entry.get_args(base + ["--eval_sample_best_of", "3", "--eval_no_repeat_ngram", "2"])
        assert args.eval_sample_best_of == 3
        stats = entry.main(args, config)
        assert seen and all(kw.get("do_sample") and kw.get("best_of") and kw.get("num_samples") == 3 and kw.get("no_repeat_ngram_size") == 2
                            for kw, _ in seen), [kw for kw, _ in seen]
        assert all(isinstance(o, list) and all(r.shape[0] == 1 for r in o) for _, o in seen)
        merged = json.load(open(os.path.join(out, "result", "val_caption_result.json")))
        assert any(k.startswith("val_") for k in stats)
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert len(merged) == 5
    for rec in merged:
        assert set(rec) == {"video_id", "pred_caption", "gold_caption"} and isinstance(rec["pred_caption"], str)


# ------------------------------------------------------------------------------ the library on the host
def _desc(**over):
    from youku_mplug_amd import _lib
    d = _lib.SampleScoreDesc()
    ok = dict(logits=0x10000, tokens=0x20000, prompt_len=0x30000, done=0x40000, live=0x50000, token_logprob=0x60000, sum_logprob=0x70000, count=0x80000,
              ld=72, rows=2, vocab=64, row_len=16, pos=5)
    for k, v in {**ok, **over}.items():
        setattr(d, k, v)
    return d


REFUSALS = [dict(logits=None), dict(tokens=None), dict(prompt_len=None), dict(done=None), dict(live=None), dict(token_logprob=None), dict(sum_logprob=None),
            dict(count=None), dict(vocab=60), dict(vocab=0), dict(vocab=65544, ld=65544), dict(ld=56), dict(ld=68), dict(logits=0x10008), dict(rows=0),
            dict(rows=-3), dict(row_len=0), dict(row_len=2049), dict(pos=-1), dict(pos=16)]


def test_library_exports_the_symbol_and_refuses_on_the_host():
    """every refusal of include/mpv.h comes back negative before anything is launched (the pointers are not memory: a launch would fault)"""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    assert "mpv_sample_score" in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "mpv_sample_score")
    fn = _lib.lib().mpv_sample_score
    for over in REFUSALS:
        assert fn(ctypes.byref(_desc(**over)), None) < 0, over
        assert b"mpv_sample_score" in _lib.lib().mpv_last_error()
    assert fn(None, None) < 0


def test_ctypes_descriptor_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    cname, ct = "mpv_sample_score_desc", _lib.SampleScoreDesc
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, re.S).group(1)
    names = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in ct._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpv.h"', 'int main(void) {', f'  printf("%zu", sizeof({cname}));']
    prog += [f'  printf(" %zu", offsetof({cname}, {n}));' for n in names] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    tok = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert tok[0] == ctypes.sizeof(ct) and tok[1:] == [getattr(ct, f[0]).offset for f in ct._fields_]


def test_score_kernel_has_no_scratch_and_fits_four_waves_per_simd():
    """sample_score_kernel in the gfx950 code object: 1024 threads = 4 waves per SIMD, so at most 128 registers; no
    scratch; static LDS = the two 16-word reduction buffers.  Register, LDS and scratch figures only, read the way tests/test_isa_cpu.py
    reads them."""
    import tempfile
    import test_isa_cpu as isa
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for i, blob in enumerate(isa._code_objects()):
            f = os.path.join(d, f"co_{i}.elf")
            open(f, "wb").write(blob)
            txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
            for blk in txt.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                if "sample_score_kernel" in name:
                    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                    found[name] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), scratch=g("private_segment_fixed_size"),
                                       lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    assert len(found) == 1, sorted(found)
    k = next(iter(found.values()))
    print(f"    sample_score_kernel: {k}")
    assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= 128 and k["lds"] <= 1024 and k["threads"] == 1024, k
