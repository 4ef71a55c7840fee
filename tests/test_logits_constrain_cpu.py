"""Generation constraints on the device, checked without a GPU: the restatement tests/standin_constrain.py against
a definition in sets and slices and against the logits processors of `transformers`; the committed cases of tests/constrain_cases.py;
both lockstep loops with the restatement as constrain_fn (never called without active constraints, call order and arguments, no n-gram
twice, no early termination token); LogitsConstraints, DistributedGPT3_Caption.generate and the caption entry point's flags; the
library's refusals on the host, the ctypes mirror of the descriptor, and the kernel's LDS / scratch figures in the built code object."""
import ctypes
import json
import math
import os
import random
import re
import shutil
import subprocess
import types

import pytest
import torch

import constrain_cases as cc
import sampling_cases as sc
import standin_constrain as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LLVM = "/opt/rocm/lib/llvm/bin"


def _C(**kw):
    from youku_mplug_amd.generation import LogitsConstraints
    return LogitsConstraints(**kw)


def _bf16(x):
    return torch.tensor(x, dtype=torch.float32).to(torch.bfloat16)


# ------------------------------------------------------------------------------ the restatement
def _definition(row, hist, prompt_len, pos, c, eos_ids, ban_value):
    """include/mpv.h, row semantics, word for word: row a list of bf16 scalars (edited copy returned), hist = tokens[:pos] as a list"""
    vocab = len(row)
    if prompt_len > pos:
        return list(row)
    h = hist[(0 if c.include_prompt else prompt_len):pos]
    m, n, g = len(h), c.no_repeat_ngram_size, pos - prompt_len
    banned = set()
    if n == 1:
        banned |= set(h)
    elif n >= 2 and m >= n:
        s = h[m - n + 1:m]
        for i in range(0, m - n + 1):
            if h[i:i + n - 1] == s:
                banned.add(h[i + n - 1])
    if g < c.min_new_tokens:
        banned |= set(eos_ids)
    banned |= set(c.banned_token_ids)
    out = list(row)
    if c.repetition_penalty != 1.0:
        p = torch.tensor(c.repetition_penalty, dtype=torch.float32)
        for v in set(h):
            if 0 <= v < vocab:
                x = row[v].float()
                out[v] = (x * p if x < 0 else x / p).to(torch.bfloat16)
    for v in banned:
        if 0 <= v < vocab:
            out[v] = _bf16(ban_value)
    return out


def _random_case(rng, oor=True):
    V = rng.choice([8, 16, 24, 64])
    m = rng.randint(0, 40)
    prompt = rng.randint(0, 3)
    pos = prompt + m
    alphabet = rng.sample(range(V), min(5, V))[:rng.randint(1, 5)]
    if oor and rng.random() < 0.3:
        alphabet += rng.sample([-1, V, 2 ** 40], rng.randint(1, 3))
    toks = [rng.choice(alphabet) for _ in range(pos)] + [rng.randrange(V) for _ in range(2)]
    c = _C(repetition_penalty=rng.choice([0.8, 1.0, 1.2, 1.3, 2.0]), no_repeat_ngram_size=rng.choice([0, 1, 2, 3, 4, 8]),
           min_new_tokens=rng.choice([0, 3, 50]), banned_token_ids=tuple(rng.sample(range(-1, V + 1), rng.choice([0, 0, 2]))),
           include_prompt=rng.random() < 0.5)
    variant = rng.choice(["normal", "half_neg_inf", "one_hot", "cutoff_ties", "all_equal"])
    row = sc.make_row(V, rng.randrange(10 ** 6), variant)
    eos = rng.sample(range(V), rng.choice([1, 2]))
    ban = rng.choice([cc.BAN_INF, cc.BAN_FINITE])
    return V, prompt, pos, toks, c, row, eos, ban


def test_standin_equals_the_definition_in_sets_and_slices():
    rng = random.Random(7)
    edited = 0
    for _ in range(480):
        V, prompt, pos, toks, c, row, eos, ban = _random_case(rng)
        want = torch.stack(_definition(list(row), toks, prompt, pos, c, eos, ban))
        got = torch.full((1, V + 8), sc.POISON, dtype=torch.bfloat16)
        got[0, :V] = row
        tokens = torch.tensor([toks])
        assert sk.logits_constrain(got, tokens, pos=pos, constraints=c, prompt_len=torch.tensor([prompt]), eos_ids=eos, ban_value=ban, vocab=V) is got
        assert torch.equal(got[0, :V].view(torch.int16), want.view(torch.int16)), (V, prompt, pos, toks, c, eos, ban)
        assert (got[0, V:] == sc.POISON).all()
        edited += int((want.view(torch.int16) != row.view(torch.int16)).any())
        also = row[None].clone()                                            # the scalar prompt length is the same thing
        sk.logits_constrain(also, tokens, pos=pos, constraints=c, prompt_len_all=prompt, eos_ids=eos, ban_value=ban)
        assert torch.equal(also[0].view(torch.int16), want.view(torch.int16))
    assert edited > 300, edited


def test_standin_equals_the_transformers_processors():
    """include_prompt=True and ban_value=-inf: bit-equal, after bf16 rounding, to RepetitionPenaltyLogitsProcessor ->
    NoRepeatNGramLogitsProcessor -> MinNewTokensLengthLogitsProcessor on the fp32 scores"""
    try:
        tf = pytest.importorskip("transformers")
    except pytest.skip.Exception as e:
        print(f"    skipped: {e}")
        raise
    rng = random.Random(11)
    n_cases = 0
    for _ in range(400):
        V, prompt, pos, toks, c, row, eos, _ = _random_case(rng, oor=False)
        c = _C(repetition_penalty=c.repetition_penalty, no_repeat_ngram_size=min(c.no_repeat_ngram_size, 4), min_new_tokens=c.min_new_tokens,
               include_prompt=True)
        ids = torch.tensor([toks[:pos]], dtype=torch.long)
        scores = row[None].float()
        if c.repetition_penalty != 1.0:
            scores = tf.RepetitionPenaltyLogitsProcessor(c.repetition_penalty)(ids, scores)
        if c.no_repeat_ngram_size:
            scores = tf.NoRepeatNGramLogitsProcessor(c.no_repeat_ngram_size)(ids, scores)
        if c.min_new_tokens:
            scores = tf.MinNewTokensLengthLogitsProcessor(prompt, c.min_new_tokens, eos)(ids, scores)
        got = row[None].clone()
        sk.logits_constrain(got, torch.tensor([toks]), pos=pos, constraints=c, prompt_len=torch.tensor([prompt]), eos_ids=eos)
        assert torch.equal(got.view(torch.int16), scores.to(torch.bfloat16).view(torch.int16)), (V, prompt, pos, toks, c, eos)
        n_cases += 1
    assert n_cases == 400


def test_standin_internals():
    h = torch.tensor([4, 9, 4, 2 ** 40, 9, -1, 2 ** 40, 4])
    assert sk.first_occurrence(h).tolist() == [True, True, False, True, False, True, False, False]
    assert sk.first_occurrence(torch.zeros(0, dtype=torch.int64)).tolist() == []
    # a b a b a: suffix of n = 3 is (b, a); the grams (b, a, b) at 1 ends at position 3 -- and the overlapping (a, b, a) do not match
    assert sk.repeat_ends(torch.tensor([1, 2, 1, 2, 1]), 3).tolist() == [False, False, False, True, False]
    assert sk.repeat_ends(torch.tensor([1, 2, 1, 2, 1]), 2).tolist() == [False, True, False, True, False]      # suffix (a): b follows twice
    assert sk.repeat_ends(torch.tensor([3, 3, 3]), 2).tolist() == [False, True, True]                            # the last gram overlaps the suffix
    assert sk.repeat_ends(torch.tensor([3, 3]), 3).tolist() == [False, False] and sk.repeat_ends(torch.tensor([3, 3]), 1).tolist() == [True, True]
    # a token that occurs five times is penalised ONCE; out-of-range tokens form no address but take part in the comparison
    row = _bf16([[-1.0, 2.0, -3.0, 4.0, 0.5, -0.25, 1.5, 3.0]])
    toks = torch.tensor([[1, 1, 1, 1, 1, 2, 8, -1, 2 ** 40, 0, 0]])
    out = sk.logits_constrain(row.clone(), toks, pos=9, constraints=_C(repetition_penalty=2.0), prompt_len_all=0)
    assert out[0].tolist() == [-1.0, 1.0, -6.0, 4.0, 0.5, -0.25, 1.5, 3.0]
    toks = torch.tensor([[2 ** 40, 3, 5, 2 ** 40, 0]])                       # (2**40, 3) then 2**40 again: 3 is banned through an out-of-range gram
    out = sk.logits_constrain(row.clone(), toks, pos=4, constraints=_C(no_repeat_ngram_size=2), prompt_len_all=0)
    assert out[0, 3] == float("-inf") and torch.equal(out[0, :3], row[0, :3]) and torch.equal(out[0, 4:], row[0, 4:])
    toks = torch.tensor([[3, 8, 5, 3, 0]])                                   # (3, 8): the banned token is out of range, nothing happens
    out = sk.logits_constrain(row.clone(), toks, pos=4, constraints=_C(no_repeat_ngram_size=2), prompt_len_all=0)
    assert torch.equal(out, row)
    # the ban wins over the penalty, and the finite ban value is the lowest finite bf16
    out = sk.logits_constrain(row.clone(), torch.tensor([[3, 3, 0]]), pos=2, constraints=_C(repetition_penalty=2.0, no_repeat_ngram_size=1),
                              prompt_len_all=0, ban_value=cc.BAN_FINITE)
    assert out[0, 3].view(torch.int16).item() == torch.tensor(0xFF7F - 0x10000, dtype=torch.int16).item() and math.isfinite(float(out[0, 3]))
    # teacher-forced rows stay, bit for bit; the prompt is history only with include_prompt
    rows = row.repeat(3, 1)
    toks = torch.tensor([[1, 1, 6, 0], [1, 1, 6, 0], [1, 1, 6, 0]])
    c = _C(repetition_penalty=2.0, min_new_tokens=1, banned_token_ids=(7,))
    out = sk.logits_constrain(rows.clone(), toks, pos=3, constraints=c, prompt_len=torch.tensor([4, 2, 3]), eos_ids=[0])
    assert torch.equal(out[0], row[0])
    assert out[1].tolist() == [-1.0, 2.0, -3.0, 4.0, 0.5, -0.25, 0.75, float("-inf")]                             # g = 1: eos is free again
    assert out[2].tolist() == [float("-inf"), 2.0, -3.0, 4.0, 0.5, -0.25, 1.5, float("-inf")]                      # g = 0, empty history
    out = sk.logits_constrain(rows.clone(), toks, pos=3, constraints=_C(repetition_penalty=2.0, include_prompt=True), prompt_len=torch.tensor([4, 2, 3]))
    assert torch.equal(out[0], row[0]) and out[1].tolist() == out[2].tolist() == [-1.0, 1.0, -3.0, 4.0, 0.5, -0.25, 0.75, 3.0]
    for bad in (dict(pos=4), dict(pos=-1), dict(ban_value=0.0), dict(ban_value=float("nan")), dict(ban_value=float("inf")), dict(vocab=12), dict(eos_ids=list(range(9)))):
        with pytest.raises(AssertionError):
            sk.logits_constrain(rows.clone(), toks, **{**dict(pos=3, constraints=c, prompt_len_all=0), **bad})


def test_the_committed_cases_cover_what_they_claim():
    C = cc.CASES
    assert len({cc.case_id(c) for c in C}) == len(C)
    assert {c["V"] for c in C} == {8, 64, 51200, 65536} and {c["rows"] for c in C} >= {1, 3, 160}
    assert {c["m"] for c in C} >= set(cc.HIST) and {c["ngram"] for c in C} == {0, 1, 2, 3, 4, 8}
    assert {c["kind"] for c in C} == {"few", "same", "overlap", "pair", "oor", "eos", "wide"} and {c["ban"] for c in C} == {"inf", "finite"}
    assert any(c["ngram"] >= 2 and c["m"] < c["ngram"] - 1 for c in C) and any(c.get("mixed") for c in C) and any(c.get("scalar_prompt") for c in C)
    assert any(c.get("pos") == 0 for c in C) and any(c.get("row_len") == 2048 and c.get("pos") == 2047 for c in C)
    alone = [c for c in C if sum([c["penalty"] != 1.0, c["ngram"] > 0, c["min_new"] > 0, c["n_banned"] > 0]) == 1]
    assert {("p" if c["penalty"] != 1.0 else "n" if c["ngram"] else "m" if c["min_new"] else "b") for c in alone} == {"p", "n", "m", "b"}
    changed = 0
    for c in C:
        if c["V"] > 64 or c["rows"] > 4 or c["m"] > 300:
            continue                                                        # the small ones are enough here
        logits, tokens, kw, ckw = cc.build(c)
        assert logits.shape == (c["rows"], c["V"] + 8) and (logits[:, c["V"]:] == sc.POISON).all() and tokens.shape[1] > kw["pos"] >= 0
        out = sk.logits_constrain(logits.clone(), tokens, constraints=_C(**ckw), vocab=c["V"], **kw)
        changed += int(not torch.equal(out.view(torch.int16), logits.view(torch.int16)))
        if c["kind"] == "pair":                                             # only even columns are edited
            assert torch.equal(out[:, 1:c["V"]:2].view(torch.int16), logits[:, 1:c["V"]:2].view(torch.int16))
        if ckw["banned_token_ids"]:
            assert (logits[:, ckw["banned_token_ids"][0]] > 0).all()         # a banned id with a positive logit
        if c.get("mixed"):
            assert torch.equal(out[1::2].view(torch.int16), logits[1::2].view(torch.int16))
    assert changed > 30, changed


# ------------------------------------------------------------------------------ LogitsConstraints
def test_logits_constraints_validate_and_know_when_they_are_off():
    assert not _C().active and not _C(include_prompt=True).active
    for kw in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=1), dict(banned_token_ids=[3])):
        assert _C(**kw).active, kw
    assert _C(banned_token_ids=[3, 4]).banned_token_ids == (3, 4) and _C(repetition_penalty=2).repetition_penalty == 2.0
    for kw, shown in ((dict(repetition_penalty=0.0), "0.0"), (dict(repetition_penalty=-1.5), "-1.5"), (dict(repetition_penalty=float("inf")), "inf"),
                      (dict(repetition_penalty=float("nan")), "nan"), (dict(repetition_penalty="2"), "'2'"), (dict(no_repeat_ngram_size=9), "9"),
                      (dict(no_repeat_ngram_size=-1), "-1"), (dict(no_repeat_ngram_size=1.5), "1.5"), (dict(min_new_tokens=-2), "-2"),
                      (dict(banned_token_ids=[1.5]), "1.5"), (dict(banned_token_ids=list(range(1025))), "1025")):
        with pytest.raises(ValueError, match=re.escape(shown)):
            _C(**kw)


# ------------------------------------------------------------------------------ the loops
def _ngrams_repeat(seq, n):
    grams = [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
    return len(grams) != len(set(grams))


def _sample_run(constraints, record=None, **kw):
    import standin_sampling as ss
    import test_sampling_cpu as ts
    from youku_mplug_amd import generation
    stub, cfgd, tokens, lengths = ts._sample_case(0)
    cfg = types.SimpleNamespace(**cfgd, top_k=0, top_p=0.9, vocab_size=stub.vocab)
    states = []

    def make_state(b, m):
        states.append(ts._FanStubState(stub, b, m, pad_to=32))
        return states[-1]

    def constrain(logits, toks, **k):
        if record is not None:
            record.append(("constrain", logits, toks, k))
        return sk.logits_constrain(logits, toks, **k)

    def advance(logits, st, **k):
        if record is not None:
            record.append(("advance", logits, st, k))
        return ss.sample_advance(logits, st, **k)
    out = generation.sample_batched_loop(cfg, make_state, tokens.clone(), prompt_length=lengths.clone(), advance_fn=advance, constraints=constraints,
                                         constrain_fn=constrain, temperature=1.1, seed=3, **kw)
    return out, lengths, cfgd


def test_sample_loop_calls_the_constraints_between_step_and_sampler():
    from youku_mplug_amd import generation
    rec = []
    base, lengths, cfgd = _sample_run(None, rec, num_samples=2, use_eod_token_for_early_termination=False)
    assert rec and all(r[0] == "advance" for r in rec)                       # no constraints: constrain_fn is never called
    n_steps = len(rec)
    rec.clear()
    off, _, _ = _sample_run(_C(include_prompt=True), rec, num_samples=2, use_eod_token_for_early_termination=False)
    assert len(rec) == n_steps and all(r[0] == "advance" for r in rec) and torch.equal(off, base)      # inactive: the same
    rec.clear()
    c = _C(no_repeat_ngram_size=2, min_new_tokens=3, repetition_penalty=1.2)
    out, _, _ = _sample_run(c, rec, num_samples=2, use_eod_token_for_early_termination=False)
    assert [r[0] for r in rec] == ["constrain", "advance"] * n_steps         # every step, the prefill's included
    for (_, lg_c, toks, kc), (_, lg_a, st, ka) in zip(rec[0::2], rec[1::2]):
        assert lg_c is lg_a and toks is st.tokens and kc["prompt_len"] is st.prompt_len and kc["pos"] == ka["pos"]
        assert kc["constraints"] is c and kc["eos_ids"] == [cfgd["eod_id"]] and kc["ban_value"] == float("-inf") and set(kc) == {"pos", "constraints", "prompt_len", "eos_ids", "ban_value"}
    assert [r[3]["pos"] for r in rec[0::2]] == list(range(int(lengths.min()), int(lengths.min()) + n_steps))
    assert not torch.equal(out, base)
    for r, row in enumerate(out.tolist()):                                   # every column is filled (no early stop, Q = 0)
        pl = int(lengths[r // 2])
        assert row[:pl] == base[r, :pl].tolist()
        assert not _ngrams_repeat(row[pl:], 2), (r, row[pl:])
        assert cfgd["eod_id"] not in row[pl:pl + 3], (r, row[pl:])
    uni, _, _ = _sample_run(_C(no_repeat_ngram_size=1), num_samples=2, use_eod_token_for_early_termination=False)
    assert not any(_ngrams_repeat(row[int(lengths[r // 2]):], 1) for r, row in enumerate(uni.tolist()))
    gen = [row[int(lengths[r // 2]):] for r, row in enumerate(base.tolist())]      # the unconstrained run has both defects to remove
    assert any(_ngrams_repeat(g, 1) for g in gen) and any(cfgd["eod_id"] in g[:3] for g in gen), gen
    # the termination ids under stop_on_eol; double_eol with a minimum length is refused; active constraints need their function
    rec.clear()
    _sample_run(_C(min_new_tokens=2), rec, stop_on_eol=True)
    assert rec[0][0] == "constrain" and rec[0][3]["eos_ids"] == [628, 198]
    with pytest.raises(ValueError, match="stop_on_double_eol"):
        _sample_run(_C(min_new_tokens=2), stop_on_double_eol=True)
    _sample_run(_C(no_repeat_ngram_size=2), stop_on_double_eol=True)
    with pytest.raises(ValueError, match="constrain_fn"):
        generation.sample_batched_loop(types.SimpleNamespace(**cfgd, top_k=0, top_p=0.9, vocab_size=29), None, torch.tensor([[1, 2]]), constraints=c)


def _beam_run(constraints, record=None, seeds=(1, 2, 3), Q=0):
    import standin_beam
    import test_beam_batched_cpu as tb
    from oracle.gen_golden import StubLogits
    from youku_mplug_amd import generation
    vocab, cfg, tokens = tb._case(Q)
    stubs = [StubLogits(vocab=vocab, stop=7, seed=s) for s in seeds]

    class Padded(tb._BatchedStubState):                                     # the kernel's vocab % 8 == 0: -inf columns, never a candidate
        def _logits(self):
            lg = super()._logits()
            return torch.cat([lg, torch.full((lg.shape[0], 40 - lg.shape[1]), float("-inf"))], dim=1)

    def constrain(logits, toks, **k):
        record.append(("constrain", logits, toks.clone(), k))
        return sk.logits_constrain(logits, toks, **k)

    def topk(logits, k, add):
        record.append(("topk", logits))
        return tb._torch_topk(logits, k, add)

    def advance(vals, idxs, bs, **k):
        record.append(("advance", k))
        return standin_beam.beam_advance(vals, idxs, bs, **k)
    record = [] if record is None else record
    qe = torch.zeros(len(seeds), Q, 4) if Q else None
    out = generation.beam_search_batched_loop(cfg, lambda b, m: Padded(stubs, b, m), tokens.repeat(len(seeds), 1), query_embeds=qe, beam_size=tb.K,
                                              num_return_gen=tb.N_RET, prompt_length=tb.PROMPT, topk_fn=topk, advance_fn=advance,
                                              constraints=constraints, constrain_fn=constrain)
    return out, cfg


@pytest.mark.parametrize("Q", [0, 3])
def test_beam_loop_calls_the_constraints_before_the_candidates(Q):
    import test_beam_batched_cpu as tb
    from youku_mplug_amd import generation
    rec = []
    base, cfg = _beam_run(None, rec, Q=Q)
    assert {r[0] for r in rec} == {"topk", "advance"}
    rec.clear()
    off, _ = _beam_run(_C(), rec, Q=Q)
    assert {r[0] for r in rec} == {"topk", "advance"} and all(torch.equal(a.sequences, b.sequences) for a, b in zip(off, base))
    rec.clear()
    c = _C(no_repeat_ngram_size=2, min_new_tokens=4, repetition_penalty=1.3)
    out, _ = _beam_run(c, rec, Q=Q)
    assert [r[0] for r in rec] == ["constrain", "topk", "advance"] * (len(rec) // 3)
    for n, ((_, lg, toks, k), (_, lg_t), (_, ka)) in enumerate(zip(rec[0::3], rec[1::3], rec[2::3])):
        assert lg is lg_t and lg.shape[0] == toks.shape[0] == 3 * tb.K and toks.dim() == 2     # all K rows of every clip, the first step too
        assert k == dict(pos=tb.PROMPT + n, constraints=c, prompt_len_all=tb.PROMPT, eos_ids=[cfg.eod_id], ban_value=generation.BAN_BEAM)
        assert ka["pos"] == tb.PROMPT + n and ka["first"] == (n == 0)
    assert generation.BAN_BEAM == cc.BAN_FINITE and float(_bf16(generation.BAN_BEAM)) == generation.BAN_BEAM
    for o in out:
        assert torch.isfinite(o.scores).all()
        for seq in o.sequences.tolist():
            gen = seq[tb.PROMPT:]
            end = gen.index(cfg.eod_id) + 1 if cfg.eod_id in gen else len(gen)
            assert end > 4 or cfg.eod_id not in gen, seq                    # no stop token among the first min_new_tokens
            assert not _ngrams_repeat(gen[:end], 2), seq
    assert any(_ngrams_repeat(s[tb.PROMPT:(s[tb.PROMPT:].index(cfg.eod_id) + tb.PROMPT + 1 if cfg.eod_id in s[tb.PROMPT:] else None)], 2) or
               cfg.eod_id in s[tb.PROMPT:tb.PROMPT + 4] for o in base for s in o.sequences.tolist())      # the plain search has a defect to remove


# ------------------------------------------------------------------------------ the model and the entry point on the stand-ins
def _on_cpu(monkeypatch):
    import standin_beam
    import standin_sampling as ss
    import test_pipeline_cpu as tp
    from youku_mplug_amd import ops
    dev = tp._on_cpu(monkeypatch)
    monkeypatch.setattr(ops, "sample_advance", ss.sample_advance)
    monkeypatch.setattr(ops, "beam_advance", standin_beam.beam_advance)
    monkeypatch.setattr(ops, "logits_constrain", sk.logits_constrain, raising=False)
    return dev


def test_generate_forwards_constraints_to_the_lockstep_loops_only():
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
    c = _C(no_repeat_ngram_size=2)
    assert real.generate(G(), None, termination_id=3, sampler="device", constraints=c) == "d"
    assert calls == [("sample_batched", dict(termination_id=3, constraints=c))]
    for kw in (dict(), dict(do_sample=False), dict(do_sample=False, sampler="device")):
        with pytest.raises(ValueError, match="constraints"):
            real.generate(G(), None, constraints=c, **kw)


def test_caption_generate_constraints_on_standins(monkeypatch):
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict
    from youku_mplug_amd import generation
    from youku_mplug_amd.downstream import synthetic_gencls_model
    dev = _on_cpu(monkeypatch)
    m = torch.load(os.path.join(GOLD, "caption_tiny.pt"))["meta"]
    model = synthetic_gencls_model(CONFIG_TINY, "caption", device=dev)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in make_state_dict(CONFIG_TINY, m["weight_seed"]).items()}, strict=True)
    model.text_decoder.config.extra.update(tokens_to_generate=m["tokens_to_generate"], eod_id=m["eod_id"])
    video, ids, mask = make_inputs(CONFIG_TINY, m["batch"], m["text_len"], seed=m["input_seed"], ragged=False)
    text = types.SimpleNamespace(input_ids=ids, attention_mask=mask)
    video = video.to(torch.bfloat16)
    for kw in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=1), dict(banned_token_ids=[3]), dict(constrain_prompt=True)):
        with pytest.raises(ValueError, match="batched=True or do_sample=True"):
            model.generate(video, text, termination_id=m["eod_id"], **kw)
    with pytest.raises(ValueError, match="0.0"):
        model.generate(video, text, termination_id=m["eod_id"], batched=True, repetition_penalty=0.0)
    seen = []
    for name in ("beam_search_batched_loop", "sample_batched_loop"):
        def spy(cfg, make_state, tokens, _orig=getattr(generation, name), _name=name, **kw):
            seen.append((_name, kw.get("constraints"), kw.get("constrain_fn")))
            return _orig(cfg, make_state, tokens, **kw)
        monkeypatch.setattr(generation, name, spy)
    n_prompt = int(mask[0].sum()) - 1
    kw = dict(termination_id=m["eod_id"], no_repeat_ngram_size=2, min_new_tokens=2)
    res = model.generate(video, text, batched=True, **kw)
    smp = model.generate(video, text, do_sample=True, num_samples=3, seed=5, temperature=1.3, **kw)
    want = generation.LogitsConstraints(no_repeat_ngram_size=2, min_new_tokens=2)
    assert [s[0] for s in seen] == ["beam_search_batched_loop", "sample_batched_loop"] and all(s[1] == want and s[2] is sk.logits_constrain for s in seen)
    for rows in list(res) + list(smp):
        for row in rows.tolist():
            gen = row[n_prompt:]
            end = gen.index(m["eod_id"]) + 1 if m["eod_id"] in gen else len(gen)
            assert end > 2 or m["eod_id"] not in gen, row
            assert not _ngrams_repeat(gen[:end], 2), row
    seen.clear()
    model.generate(video, text, termination_id=m["eod_id"], batched=True)
    assert seen[0][1] is None                                                # keywords absent: today's call


def test_caption_entrypoint_constraint_flags_on_standins(tmp_path, monkeypatch):
    """--eval_repetition_penalty / --eval_no_repeat_ngram / --eval_min_new_tokens default off, are refused without a lockstep flag, and
    reach model.generate in the --eval_batched_beam and --eval_sample calls"""
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
    monkeypatch.setenv("MASTER_PORT", str(42000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    seen = []
    gen = downstream.DistributedGPT3_Caption.generate

    def spy(self, image, text, *a, **kw):
        seen.append(kw)
        return gen(self, image, text, *a, **kw)
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    try:
        out = str(tmp_path / "constrained")
        base = ["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only"]
        a = entry.get_args(base)[0]
        assert a.eval_repetition_penalty is None and a.eval_no_repeat_ngram == 0 and a.eval_min_new_tokens == 0 and entry.constraint_keywords(a) == {}
        for flags in (["--eval_repetition_penalty", "1.2"], ["--eval_no_repeat_ngram", "2"], ["--eval_min_new_tokens", "1"]):
            with pytest.raises(ValueError, match="--eval_batched_beam or --eval_sample"):
                entry.get_args(base + flags)
        flags = ["--eval_repetition_penalty", "1.2", "--eval_no_repeat_ngram", "2", "--eval_min_new_tokens", "1"]
        assert entry.get_args(base + flags + ["--eval_sample", "2"])[0].eval_no_repeat_ngram == 2
        args, config = entry.get_args(base + flags + ["--eval_batched_beam", "--eval_sample", "2"])
        entry.main(args, config)
        want = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=1)
        assert seen and all({k: kw.get(k) for k in want} == want for kw in seen), seen
        assert any(kw.get("batched") for kw in seen) and any(kw.get("do_sample") for kw in seen)
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


# ------------------------------------------------------------------------------ the library on the host
def _desc(**over):
    from youku_mplug_amd import _lib
    d = _lib.LogitsConstrainDesc()
    ok = dict(logits=0x10000, tokens=0x20000, prompt_len=0x30000, eos_ids=0x40000, banned_ids=0x50000, ld=72, prompt_len_all=0, rows=2, vocab=64, row_len=16,
              pos=5, n_eos=1, n_banned=2, ngram=2, min_new_tokens=3, include_prompt=0, penalty=1.2, ban_value=float("-inf"))
    for k, v in {**ok, **over}.items():
        setattr(d, k, v)
    return d


REFUSALS = [dict(logits=None), dict(tokens=None), dict(vocab=60), dict(vocab=0), dict(vocab=65544, ld=65544), dict(ld=56), dict(ld=68), dict(logits=0x10008),
            dict(row_len=0), dict(row_len=2049), dict(pos=-1), dict(pos=16), dict(penalty=0.0), dict(penalty=-1.0), dict(penalty=float("inf")),
            dict(penalty=float("nan")), dict(ngram=-1), dict(ngram=9), dict(min_new_tokens=-1), dict(n_eos=-1), dict(n_eos=9), dict(n_eos=1, eos_ids=None),
            dict(n_banned=-1), dict(n_banned=1025), dict(n_banned=1, banned_ids=None), dict(ban_value=float("nan")), dict(ban_value=float("inf")),
            dict(ban_value=0.0), dict(ban_value=1.0)]


def test_library_exports_the_symbol_and_refuses_on_the_host():
    """every refusal of include/mpv.h comes back negative before anything is launched (the pointers are not memory: a launch would fault);
    a descriptor with everything off returns 0 without a launch"""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    assert "mpv_logits_constrain" in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "mpv_logits_constrain")
    fn = _lib.lib().mpv_logits_constrain
    for over in REFUSALS:
        assert fn(ctypes.byref(_desc(**over)), None) < 0, over
        assert b"mpv_logits_constrain" in _lib.lib().mpv_last_error()
    assert fn(None, None) < 0
    for off in (dict(penalty=1.0, ngram=0, n_banned=0, min_new_tokens=0), dict(penalty=1.0, ngram=0, n_banned=0, n_eos=0, eos_ids=None, banned_ids=None)):
        assert fn(ctypes.byref(_desc(**off)), None) == 0, off


def test_ctypes_descriptor_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    cname, ct = "mpv_logits_constrain_desc", _lib.LogitsConstrainDesc
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


def test_constrain_kernel_has_no_scratch_and_a_small_lds_image():
    """logits_constrain_kernel in the gfx950 code object: no scratch, static LDS (history, id lists, repeat flags) at most 32 KiB, 1024
    threads.  Register, LDS and scratch figures only, read the way tests/test_isa_cpu.py reads them."""
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
                if "logits_constrain_kernel" in name:
                    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                    found[name] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), scratch=g("private_segment_fixed_size"),
                                       lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    assert len(found) == 1, sorted(found)
    k = next(iter(found.values()))
    assert k["scratch"] == 0 and 0 < k["lds"] <= 32 * 1024 and k["vgpr"] + k["agpr"] <= 128 and k["threads"] == 1024, k
