"""Sampled generation with the sampler on the device, checked without a GPU: the committed cases (tests/sampling_cases.py) all satisfy
the separation condition that makes the GPU comparison exact; the restatement tests/standin_sampling.py against the filters of
generation.py, an independent inverse CDF and a second transcription of the hash; generation.sample_batched_loop driven by
oracle/gen_golden.py's StubLogits against tests/golden/search_stub.pt (written by the reference's own sample()) and against a plain
per-row loop; DistributedGPT3_Caption.generate(do_sample=True) and --eval_sample on the stand-ins; the register / LDS / scratch budget
of the kernel in the built code object."""
import json
import os
import re
import subprocess
import types

import pytest
import torch

import sampling_cases as sc
import standin_sampling as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LLVM = "/opt/rocm/lib/llvm/bin"


# ------------------------------------------------------------------------------ the cases and the restatement
def test_every_listed_case_satisfies_the_separation_condition():
    """The guard that the GPU test leaves nothing out: every row of every committed case is unambiguous in fp64, and the committed
    skip sets are exactly what discover() finds (a candidate is left out only because it fails the condition)."""
    assert len(sc.CASES) == len(sc.PLAN)
    n_rows = 0
    for case, plan in zip(sc.CASES, sc.PLAN):
        V, rows, ld, seed, T, filt, skip = case
        assert (V, rows, ld, seed, T, tuple(filt)) == plan
        logits, taken = sc.case_rows(case)
        assert logits.shape == (rows, ld) and len(taken) == rows and (logits[:, V:] == sc.POISON).all()
        for r in range(rows):
            ok, res = sc.candidate_ok(logits[r, :V], T, filt, ss.uniform(seed, sc.POS, r))
            assert ok, (case[:6], r, res["margin_p"], res["margin_u"])
        n_rows += rows
    for plan in (sc.PLAN[1], sc.PLAN[8], sc.PLAN[20]):                      # three short cases with a non-empty skip set, recomputed
        assert sc.discover([plan])[0] == sc.CASES[sc.PLAN.index(plan)]
    assert {c[0] for c in sc.CASES} == {8, 64, 8000, 51200, 65536} and {c[1] for c in sc.CASES} >= {1, 3, 160}
    assert {c[4] for c in sc.CASES} >= {0.7, 1.0, 1.5} and {c[5][0] for c in sc.CASES} == {"plain", "greedy", "top_k", "top_p"}
    assert any(c[2] == c[0] for c in sc.CASES) and any(c[2] == c[0] + 64 for c in sc.CASES)
    print(f"    {len(sc.CASES)} cases, {n_rows} rows")


def test_variants_are_what_they_claim():
    for V in (8, 64, 8000):
        assert (sc.make_row(V, 5, "all_neg_inf") == float("-inf")).all()
        assert int((sc.make_row(V, 5, "half_neg_inf") == float("-inf")).sum()) >= V // 2
        eq = sc.make_row(V, 5, "all_equal")
        assert (eq == eq[0]).all()
        hot = sc.make_row(V, 5, "one_hot").float()
        assert ss.sample_row(hot, 1.0, 0, 0.9, 0.5)["kept"] == 1                       # a nucleus of one
        ties = sc.make_row(V, 5, "cutoff_ties").float()
        for top_k, top_p in ((0, 0.5), (0, 0.9), (2, 0.0)):                            # >= 4 entries share the cutoff value
            kept = ss.sample_row(ties, 1.0, top_k, top_p, 0.5)["kept_mask"]
            cutoff = ties[kept].min()
            assert int((ties == cutoff).sum()) >= 4, (V, top_k, top_p)
        # under top-p the tie rule cuts INSIDE the group of equal logits; under top-k the whole group stays
        assert int(ss.sample_row(ties, 1.0, 0, 0.5, 0.5)["kept"]) < int((ties == ties.max()).sum()) == ss.sample_row(ties, 1.0, 2, 0.0, 0.5)["kept"]


@pytest.mark.parametrize("V", [64, 1000])
def test_standin_filters_equal_the_torch_filters_without_ties_at_the_cutoff(V):
    """generation._filter_top_k / _filter_top_p (the reference's filters, fp32) keep exactly the stand-in's set on rows whose cutoff is
    not tied and not within DELTA of top_p"""
    from youku_mplug_amd import generation
    checked = 0
    for seed in range(12):
        row = sc.make_row(V, 900 + seed, "normal").float()
        for T in (0.7, 1.0, 1.5):
            for top_k, top_p in ((2, 0.0), (50, 0.0), (0, 0.5), (0, 0.9)):
                res = ss.sample_row(row, T, top_k, top_p, 0.5)
                cutoff = row[res["kept_mask"]].min()
                if int((row == cutoff).sum()) > 1 or res["margin_p"] < sc.DELTA:
                    continue
                lg = (row / T)[None].clone()
                if top_k:
                    generation._filter_top_k(lg, top_k)
                else:
                    generation._filter_top_p(lg, top_p)
                assert torch.equal(lg[0] > float("-inf"), res["kept_mask"]), (V, seed, T, top_k, top_p)
                checked += 1
    assert checked > 100, checked


def test_standin_draw_equals_an_independent_inverse_cdf():
    g = torch.Generator().manual_seed(3)
    for V, variant in ((8, "normal"), (64, "half_neg_inf"), (1000, "normal"), (1000, "cutoff_ties")):
        row = sc.make_row(V, 77, variant).float()
        for top_k, top_p in ((0, 0.0), (5, 0.0), (0, 0.9)):
            for u in [0.0, 1.0 - 2.0 ** -24] + torch.rand(20, generator=g, dtype=torch.float64).tolist():
                res = ss.sample_row(row, 1.3, top_k, top_p, u)
                pk = torch.where(res["kept_mask"], torch.softmax(row.double() / 1.3, dim=-1), torch.zeros(V, dtype=torch.float64))
                cdf = torch.cumsum(pk, dim=0)
                want = int(torch.searchsorted(cdf, torch.tensor(u, dtype=torch.float64) * cdf[-1], right=True))
                want = min(want, int(res["kept_mask"].nonzero()[-1]))
                assert res["token"] == want and res["kept_mask"][want], (V, variant, top_k, top_p, u)


def test_uniform_restates_the_hash():
    def literal(seed, pos, stream):                                         # csrc/mpv_common.h: mpv_mix32 / mpv_rand_pair, line by line
        def mix(x):
            x ^= x >> 16
            x = x * 0x7feb352d % 2 ** 32
            x ^= x >> 15
            x = x * 0x846ca68b % 2 ** 32
            x ^= x >> 16
            return x
        ctr = (pos << 32) | (stream % 2 ** 32)
        ka, kb = mix(seed % 2 ** 32), mix((seed >> 32) % 2 ** 32 ^ 0x85ebca6b)
        return (mix(((ctr % 2 ** 32 + ka) % 2 ** 32) ^ (((ctr >> 32) + kb) % 2 ** 32)) >> 8) / 2 ** 24
    seen = set()
    for seed in (0, 1, 7, 2 ** 40 + 12345, 2 ** 64 - 1):
        for pos in (0, 1, 5, 299, 2047):
            for stream in (0, 1, 159, 8191, 2 ** 31 + 5):
                u = ss.uniform(seed, pos, stream)
                assert 0.0 <= u < 1.0 and u == literal(seed, pos, stream) and u * 2 ** 24 == int(u * 2 ** 24)
                seen.add(u)
    # (seed, pos, stream) all matter.  Not all 125 are distinct: the hash meets pos and stream through an XOR of two sums, so for small
    # values u(pos = a, stream = b) == u(pos = b, stream = a) whenever neither sum carries (DESIGN.md section 16 notes it)
    assert len(seen) > 100
    us = [ss.uniform(11, 3, s) for s in range(4096)]
    assert abs(sum(us) / len(us) - 0.5) < 5 * (1 / 12 / 4096) ** 0.5        # mean of 4096 uniforms, five standard errors


# ------------------------------------------------------------------------------ the loop on the stub
class _FanStubState:
    """The decode state of sample_batched_loop as token prefixes: every sequence gets the stub's logits for its own prefix."""

    def __init__(self, stub, batch, max_len, pad_to=None):
        self.stub, self.batch, self.prefix, self.pad_to, self.prefills, self.steps = stub, batch, None, pad_to, 0, 0

    def _logits(self):
        lg = torch.stack([self.stub.row(self.prefix[:, j].tolist()) for j in range(self.batch)])
        if self.pad_to:                                                     # the kernel's vocab % 8 == 0: -inf columns, never drawn
            lg = torch.cat([lg, torch.full((self.batch, self.pad_to - lg.shape[1]), float("-inf"))], dim=1)
        return lg

    def prefill_fan_out(self, tokens, query_embeds, fan):
        assert self.prefix is None and tokens.shape[0] * fan == self.batch
        assert query_embeds is None or query_embeds.shape[0] == tokens.shape[0]          # the prefill runs once per clip
        self.prefix = tokens.t().contiguous().repeat_interleave(fan, dim=1)
        self.prefills += 1
        return self._logits()

    def step(self, tokens, query_embeds=None):
        assert query_embeds is None and tuple(tokens.shape) == (self.batch, 1)
        self.prefix = torch.cat([self.prefix, tokens.t().contiguous()], dim=0)
        self.steps += 1
        return self._logits()

    def reorder(self, *a, **k):
        raise AssertionError("samples never swap caches")


def _sample_case(Q):
    from oracle.gen_golden import SAMPLE_CASES, StubLogits
    vocab, stub_seed, cfgd, tokens, lengths, _ = SAMPLE_CASES[Q]
    return StubLogits(vocab=vocab, stop=7, seed=stub_seed), cfgd, torch.tensor(tokens), torch.tensor(lengths)


def _loop(stub, cfg, tokens, lengths, Q, **kw):
    from youku_mplug_amd import generation
    states = []

    def make_state(b, m):
        states.append(_FanStubState(stub, b, m, pad_to=32))
        return states[-1]
    qe = torch.zeros(tokens.shape[0], Q, 4) if Q else None
    out = generation.sample_batched_loop(cfg, make_state, tokens.clone(), query_embeds=qe, prompt_length=lengths.clone(),
                                         advance_fn=ss.sample_advance, **kw)
    return out, states[0]


@pytest.mark.parametrize("Q", [0, 2])
def test_greedy_batched_loop_matches_the_reference_golden(Q):
    """top_k = 1: token for token the ragged-prompt goldens of the reference's own sample() (teacher forcing behind the shortest prompt,
    termination bookkeeping, the prefix-inclusive slice); one prefill, one host read per step"""
    stub, cfgd, tokens, lengths = _sample_case(Q)
    cfg = types.SimpleNamespace(**cfgd, top_k=1, top_p=0.0, vocab_size=stub.vocab)
    ref = torch.load(os.path.join(GOLD, "search_stub.pt"))["sample"][Q]
    out, state = _loop(stub, cfg, tokens, lengths, Q)
    assert torch.equal(out, ref), (out.tolist(), ref.tolist())
    assert state.prefills == 1 and state.prefix.shape[0] == int(lengths.min()) + state.steps


def _per_row_reference(stub, cfgd, prompt, length, T, top_p, seed, stream, n_cols):
    """one sequence, a plain loop: its own prompt, then one draw per position from the stub's logits for its prefix"""
    seq = prompt[:length].tolist()
    for pos in range(length, n_cols):
        lg = torch.cat([stub.row(seq), torch.full((32 - stub.vocab,), float("-inf"))])
        seq.append(min(ss.sample_row(lg, T, 0, top_p, ss.uniform(seed, pos, stream))["token"], stub.vocab - 1))
    return seq


@pytest.mark.parametrize("Q", [0, 2])
def test_top_p_batched_loop_equals_a_per_row_loop_and_does_not_depend_on_the_batch(Q):
    stub, cfgd, tokens, lengths = _sample_case(Q)
    cfg = types.SimpleNamespace(**cfgd, top_k=0, top_p=0.9, vocab_size=stub.vocab)
    T, seed, N = 1.1, 2024, 3
    B = tokens.shape[0]
    one, _ = _loop(stub, cfg, tokens, lengths, Q, temperature=T, seed=seed, use_eod_token_for_early_termination=False)
    n_cols = tokens.shape[1] + cfgd["tokens_to_generate"]
    assert one.shape == (B, n_cols)                                         # no early stop: the slice is capped by the table
    for b in range(B):
        assert one[b].tolist() == _per_row_reference(stub, cfgd, tokens[b], int(lengths[b]), T, 0.9, seed, b, n_cols), b
    # num_samples = 3: row b * 3 + s draws from stream b * 3 + s and equals a one-sample run with that stream
    fan, state = _loop(stub, cfg, tokens, lengths, Q, temperature=T, seed=seed, num_samples=N, use_eod_token_for_early_termination=False)
    assert fan.shape == (B * N, n_cols) and state.prefills == 1
    for s in range(N):
        single, _ = _loop(stub, cfg, tokens, lengths, Q, temperature=T, seed=seed, streams=torch.arange(B) * N + s,
                          use_eod_token_for_early_termination=False)
        assert torch.equal(single, fan[s::N]), s
    assert len({tuple(r) for r in fan.tolist()}) > B                        # the samples of a clip differ
    # chunking: clips one at a time with their streams
    for b in range(B):
        part, _ = _loop(stub, cfg, tokens[b:b + 1], lengths[b:b + 1], Q, temperature=T, seed=seed, num_samples=N,
                        streams=torch.arange(N) + b * N, use_eod_token_for_early_termination=False)
        assert torch.equal(part[:, :n_cols], fan[b * N:(b + 1) * N]), b
    # early termination: the same tokens, cut at the step after which every row was done
    early, state = _loop(stub, cfg, tokens, lengths, Q, temperature=T, seed=seed, num_samples=N)
    filled = int(lengths.min()) + state.steps + 1                           # the slice is prefix-inclusive (sic): the columns behind the last
    assert early.shape[1] == min(filled + Q, n_cols)
    assert torch.equal(early[:, :filled], fan[:, :filled]) and (early[:, filled:] == cfgd["eod_id"]).all()       # sampled one are still padding
    min_p = int(lengths.min())
    done_at = [next((c for c in range(int(lengths[r // N]), n_cols) if fan[r, c] == cfgd["eod_id"]), None) for r in range(B * N)]
    if all(d is not None for d in done_at):
        assert state.steps + 1 == max(done_at) - min_p + 1 and early.shape[1] == min(max(done_at) + Q + 1, n_cols)


class _ScriptState:
    """forces a token sequence: the logits at step n are one-hot at script[row][n]"""

    def __init__(self, script, vocab):
        self.script, self.vocab, self.n = script, vocab, 0

    def _logits(self):
        lg = torch.full((len(self.script), self.vocab), -30.0)
        for r, s in enumerate(self.script):
            lg[r, s[min(self.n, len(s) - 1)]] = 5.0
        self.n += 1
        return lg

    def prefill_fan_out(self, tokens, query_embeds, fan):
        assert fan == 1
        return self._logits()

    def step(self, tokens, query_embeds=None):
        return self._logits()


@pytest.mark.parametrize("mode,kw,steps", [("id", dict(termination_id=9), 2), ("eol", dict(stop_on_eol=True), 3), ("double_eol", dict(stop_on_double_eol=True), 5)])
def test_termination_modes_of_the_batched_loop_equal_sample_loop(mode, kw, steps, monkeypatch):
    """termination_id / stop_on_eol (628 or 198) / stop_on_double_eol (628, or 198 after 198): the batched loop stops after the same
    step and returns the same tokens as sample_loop fed the same logits (greedy)"""
    from youku_mplug_amd import generation
    script = [[5, 9, 198, 7, 198, 198, 628, 3], [9, 9, 198, 198, 198, 198, 628, 3]]
    if mode == "double_eol":
        script = [[5, 198, 7, 198, 198, 3, 3, 3], [4, 4, 198, 198, 3, 3, 3, 3]]
    cfg = types.SimpleNamespace(tokens_to_generate=8, eod_id=7 if mode == "id" else 639, max_position_embeddings=40, top_k=1, top_p=0.0, vocab_size=640)
    tokens = torch.tensor([[1, 2], [3, 4]])
    got = generation.sample_batched_loop(cfg, lambda b, m: _ScriptState(script, 640), tokens.clone(), advance_fn=ss.sample_advance, **kw)
    kw["prompt_length"] = torch.tensor([2, 2])
    monkeypatch.setattr(generation, "sample_token", lambda logits, **k: torch.argmax(logits, dim=-1))
    want = generation.sample_loop(cfg, lambda b, m: _ScriptState(script, 640), tokens.clone(), **kw)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert got.shape[1] == 2 + steps, got.shape


def test_pad_after_termination():
    from youku_mplug_amd import generation
    t = torch.tensor([[7, 5, 3, 7, 4, 4], [7, 5, 3, 2, 4, 7], [7, 5, 1, 1, 1, 1]])
    out = generation.pad_after_termination(t, 2, 7, 8, 9)
    assert out.tolist() == [[7, 5, 3, 7, 9, 9, 9, 9], [7, 5, 3, 2, 4, 7, 9, 9], [7, 5, 1, 1, 1, 1, 9, 9]]
    assert generation.pad_after_termination(t, 2, 7, 4, 9).tolist() == [[7, 5, 3, 7], [7, 5, 3, 2], [7, 5, 1, 1]]


def test_standin_refuses_what_the_kernel_refuses():
    from youku_mplug_amd.generation import SampleState
    st = SampleState(torch.zeros(2, 4, dtype=torch.long), torch.zeros(2, dtype=torch.long))
    ok = dict(pos=1, temperature=1.0, top_k=0, top_p=0.9)
    ss.sample_advance(torch.zeros(2, 16), st, **ok)
    for logits, bad in ((torch.zeros(2, 12), {}), (torch.zeros(2, 4), {}), (torch.zeros(2, 16), dict(vocab=8, ld=4)), (torch.zeros(2, 16), dict(temperature=0.0)),
                        (torch.zeros(2, 16), dict(temperature=float("inf"))), (torch.zeros(2, 16), dict(top_k=2)), (torch.zeros(2, 16), dict(top_k=1)),
                        (torch.zeros(2, 16), dict(top_k=17, top_p=0.0)), (torch.zeros(2, 16), dict(top_p=1.5)), (torch.zeros(2, 16), dict(pos=4))):
        with pytest.raises(AssertionError):
            ss.sample_advance(logits, st, **{**ok, **bad})


# ------------------------------------------------------------------------------ the model and the entry point on the stand-ins
def _on_cpu(monkeypatch):
    import test_pipeline_cpu as tp
    from youku_mplug_amd import ops
    dev = tp._on_cpu(monkeypatch)
    monkeypatch.setattr(ops, "sample_advance", ss.sample_advance)
    return dev


def test_generate_sampler_keyword_routes_to_the_device_sampler(monkeypatch):
    """DistributedGPT3.generate: sampler="torch" (the default) is sample(), sampler="device" is sample_batched(); beam search ignores it"""
    from youku_mplug_amd import generation
    calls = []

    class G:
        training = False
        def eval(self): pass
        def train(self, was): pass
        def sample(self, tokens, **kw): calls.append(("sample", kw)); return "s"
        def sample_batched(self, tokens, **kw): calls.append(("sample_batched", kw)); return "d"
        def beam_search(self, tokens, **kw): calls.append(("beam", kw)); return "b"
    real = types.SimpleNamespace()
    generation.install(real)
    g = G()
    assert real.generate(g, None, termination_id=3) == "s" and real.generate(g, None, termination_id=3, sampler="torch") == "s"
    assert real.generate(g, None, termination_id=3, sampler="device", num_samples=2) == "d"
    assert real.generate(g, None, do_sample=False, sampler="device") == "b"
    assert calls == [("sample", dict(termination_id=3)), ("sample", dict(termination_id=3)), ("sample_batched", dict(termination_id=3, num_samples=2)),
                     ("beam", dict(stop_token=None))]
    with pytest.raises(ValueError):
        real.generate(g, None, sampler="host")


def test_caption_generate_do_sample_on_standins(monkeypatch):
    """DistributedGPT3_Caption.generate(do_sample=True, num_samples=3) in the setup of test_caption_generate_batched_on_standins: per clip
    an [N, Lt] tensor in input order that continues the clip's prompt; the same result with clips_per_search 1, 2 and 32; the same
    samples for a clip whatever its neighbours; another seed gives other samples; without do_sample nothing changes."""
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
    video = video.to(torch.bfloat16)
    sel = [0, 1, 0]
    text = types.SimpleNamespace(input_ids=ids[sel], attention_mask=mask[sel])
    calls = []
    orig = generation.sample_batched_loop

    def spy(cfg, make_state, tokens, **kw):
        calls.append((tokens.shape[0], kw["num_samples"], kw["streams"].tolist()))
        return orig(cfg, make_state, tokens, **kw)
    monkeypatch.setattr(generation, "sample_batched_loop", spy)
    kw = dict(termination_id=m["eod_id"], do_sample=True, num_samples=3, seed=5, temperature=1.2, top_p=0.9)
    Lt = ids.shape[1] + m["tokens_to_generate"]
    base = model.generate(video[sel], text, **kw)
    assert calls == [(1, 3, [3, 4, 5]), (2, 3, [0, 1, 2, 6, 7, 8])], calls      # grouped by prompt length; stream = clip * N + sample
    assert len(base) == 3 and all(r.shape == (3, Lt) and r.dtype == torch.int64 for r in base)
    for i, r in enumerate(base):
        n_prompt = int(mask[sel[i]].sum()) - 1
        assert (r[:, :n_prompt] == ids[sel[i], :n_prompt]).all(), i          # every sampled row continues its own prompt
    assert not torch.equal(base[0], base[2])                                 # the same clip at another place: other streams
    for cps in (1, 2):
        calls.clear()
        res = model.generate(video[sel], text, clips_per_search=cps, **kw)
        assert [c[0] for c in calls] == ([1, 1, 1] if cps == 1 else [1, 2])
        assert all(torch.equal(a, b) for a, b in zip(res, base)), cps
    # the neighbours do not matter: clip 0 alone at place 0 draws what it drew at place 0 of the call above
    alone = model.generate(video[[0]], types.SimpleNamespace(input_ids=ids[[0]], attention_mask=mask[[0]]), **kw)
    assert torch.equal(alone[0], base[0])
    other = model.generate(video[sel], text, **{**kw, "seed": 6})
    assert not all(torch.equal(a, b) for a, b in zip(other, base))
    # top_k / top_p of the call override the configuration: top_k = 1 gives three identical greedy rows
    greedy = model.generate(video[[0]], types.SimpleNamespace(input_ids=ids[[0]], attention_mask=mask[[0]]), **{**kw, "top_k": 1, "top_p": None})
    assert torch.equal(greedy[0][0], greedy[0][1]) and torch.equal(greedy[0][0], greedy[0][2])
    with pytest.raises(ValueError):
        model.generate(video[sel], text, **{**kw, "num_samples": 0})


def test_caption_entrypoint_eval_sample_flag_on_standins(tmp_path, monkeypatch):
    """downstream/run_caption_distributed_gpt3.py --evaluate_only --eval_sample 2: the flag defaults off, reaches model.generate as
    do_sample / num_samples, and the result file carries two sampled captions per clip next to the beam caption."""
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
    monkeypatch.setenv("MASTER_PORT", str(40000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    seen = []
    gen = downstream.DistributedGPT3_Caption.generate

    def spy(self, image, text, *a, **kw):
        seen.append((kw.get("do_sample", False), kw.get("num_samples")))
        return gen(self, image, text, *a, **kw)
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    try:
        out = str(tmp_path / "sampled")
        base = ["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only"]
        assert entry.get_args(base)[0].eval_sample == 0
        args, config = entry.get_args(base + ["--eval_sample", "2"])
        assert args.eval_sample == 2
        entry.main(args, config)
        assert (False, None) in seen and (True, 2) in seen, seen
        merged = json.load(open(os.path.join(out, "result", "val_caption_result.json")))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert len(merged) == 5
    for rec in merged:
        assert set(rec) == {"video_id", "pred_caption", "gold_caption", "sampled_captions"}
        assert len(rec["sampled_captions"]) == 2 and all(isinstance(c, str) for c in rec["sampled_captions"])


# ------------------------------------------------------------------------------ the kernel's budget
def test_sampling_kernel_fits_its_budget():
    """sample_advance_kernel in the gfx950 code object: 1024 threads = 4 waves per SIMD, so at most 128 registers;
    no scratch; static LDS = the 128 KiB key image plus under 4 KiB of reduction and scan slots, one workgroup per CU.  Register, LDS and
    scratch figures only, read the way tests/test_isa_cpu.py reads them."""
    import test_isa_cpu as isa
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    import tempfile
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for i, blob in enumerate(isa._code_objects()):
            f = os.path.join(d, f"co_{i}.elf")
            open(f, "wb").write(blob)
            txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
            for blk in txt.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                if "sample_advance_kernel" in name:
                    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                    found[name] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), scratch=g("private_segment_fixed_size"),
                                       lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    assert len(found) == 1, sorted(found)
    k = next(iter(found.values()))
    assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= 128 and k["threads"] == 1024, k
    assert 128 * 1024 <= k["lds"] <= 132 * 1024, k
