"""What the generation host code calls, recorded once and compared for equality (tests/golden/generation_trace.json):
(a) the C entries behind the decode states -- entry name, every integer argument, null / ptr for the pointers and the name handed to
ops.check -- for a prefill and two steps of every state on bf16 and on FP8 weights, against a library that only records;
(b) the calls of the lockstep loops on the stand-ins (tests/standin_inflight.py and what it builds on) -- every ops function a loop is
handed, the row gathers and the public state methods, with their scalar arguments and tensor shapes -- and what the loops return.
The stand-ins replace _shared_step, _ragged_prefill and _steps_step, so (b) alone never sees an entry's arguments; (a) does.
`python tests/test_generation_trace_cpu.py --record` rewrites the fixture; the comparison has no tolerance (the same arithmetic in the
same order).  A recording with a case missing fails: the case lists below are the fixture's required keys."""
import ctypes as C
import functools
import inspect
import itertools
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "generation_trace.json")
BF = torch.bfloat16
LENGTHS, SAMPLES, NEW_TOKENS, BEAMS, WIDTH, Q = [2, 4, 3], 2, 5, 2, 4, 2
INFLIGHT_LENGTHS, INFLIGHT_BUDGETS, SLOTS = [2, 4, 3, 4, 2], [2, 4, 1, 3, 2], 2

ENTRY_CASES = [f"{state}/{w}" for state in ("decode", "prefill_ragged", "shared_uniform", "shared_ragged", "inflight") for w in ("bf16", "fp8")]


def _loop_cases():
    """name -> (family, keywords of the case)"""
    cases = {}
    for mode, kv, scores, con in itertools.product(("uniform", "mixed"), ("per_sequence", "shared_prefix"), (False, True), (False, True)):
        if mode == "mixed" and kv != "shared_prefix":
            continue
        cases[f"sample/{mode}/{kv}/scores={int(scores)}/constraints={int(con)}/bf16"] = ("sample", dict(mode=mode, kv=kv, scores=scores, con=con, w="bf16"))
    cases["sample/mixed/shared_prefix/scores=1/constraints=1/fp8"] = ("sample", dict(mode="mixed", kv="shared_prefix", scores=True, con=True, w="fp8"))
    for groups, (mode, kv), con in itertools.product((1, 2), (("uniform", "per_sequence"), ("uniform", "shared_prefix"), ("mixed", "shared_prefix")),
                                                     (False, True)):
        cases[f"beam/groups={groups}/{mode}/{kv}/constraints={int(con)}/bf16"] = ("beam", dict(groups=groups, mode=mode, kv=kv, con=con, w="bf16"))
    cases["beam/groups=2/mixed/shared_prefix/constraints=1/fp8"] = ("beam", dict(groups=2, mode="mixed", kv="shared_prefix", con=True, w="fp8"))
    for refill_min, scores, con in itertools.product((1, 2), (False, True), (False, True)):
        cases[f"inflight/refill_min={refill_min}/scores={int(scores)}/constraints={int(con)}/bf16"] = \
            ("inflight", dict(refill_min=refill_min, scores=scores, con=con, w="bf16"))
    cases["inflight/refill_min=1/scores=1/constraints=1/fp8"] = ("inflight", dict(refill_min=1, scores=True, con=True, w="fp8"))
    return cases


LOOP_CASES = _loop_cases()


@functools.lru_cache(maxsize=None)
def _tiny_decoder():
    from oracle.weights import CONFIG_TINY, make_state_dict
    from youku_mplug_amd.pretrain import synthetic_model
    model = synthetic_model(CONFIG_TINY, device=torch.device("cpu"))
    model.load_state_dict({k: v.to(BF) for k, v in make_state_dict(CONFIG_TINY, 6).items()}, strict=True)
    model.eval()
    gpt = model.text_decoder
    gpt.config.extra.update(tokens_to_generate=NEW_TOKENS)
    return CONFIG_TINY, gpt


def _inputs(cfg, n, seed=31):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(8, cfg.vocab, (n, WIDTH), generator=g), (torch.randn(n, Q, cfg.hidden, generator=g) * 0.5).to(BF)


# ------------------------------------------------------------------------------------------------ (a) the entries behind the states
class RecordingLib:
    """stands where _lib.lib() does: every entry of _lib._SIGS is a recorder that checks the argument count, notes the integers and
    null / ptr for the pointers, and returns 0 (a *_workspace_size: 256 bytes)"""

    def __init__(self, sigs, calls):
        self._sigs, self._calls = sigs, calls

    def __getattr__(self, name):
        if name.startswith("_") or name not in self._sigs:
            raise AttributeError(name)
        argtypes = self._sigs[name][1]

        def record(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for the {len(argtypes)} of its signature"
            row = []
            for a, t in zip(args, argtypes):
                if t in (C.c_int, C.c_int64, C.c_size_t, C.c_uint64):
                    assert isinstance(a, int) and not isinstance(a, bool), (name, a)
                    row.append(a)
                elif t is C.c_float:
                    row.append(float(a).hex())
                else:                                                    # c_void_p or a POINTER(...)
                    null = a is None or (isinstance(a, int) and a == 0)
                    if not null and hasattr(t, "_type_") and not isinstance(t._type_, str) and hasattr(a, "_obj"):
                        assert isinstance(a._obj, t._type_), f"{name}: a {type(a._obj).__name__} where a {t._type_.__name__} goes"
                    row.append("null" if null else "ptr")
            self._calls.append({"entry": name, "args": row})
            return 256 if name.endswith("_workspace_size") else 0
        return record


def _entry_trace(monkeypatch):
    import standin_w8 as sw
    from youku_mplug_amd import _lib, generation, ops
    calls = []
    fake = RecordingLib(_lib._SIGS, calls)
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "workspace", lambda nbytes, device: torch.empty(max(int(nbytes), 1), dtype=torch.uint8))
    monkeypatch.setattr(ops, "check", lambda rc, what="": calls[-1].update(checked=what))
    monkeypatch.setattr(ops, "quantize_rows_e4m3", sw.quantize_rows_e4m3)
    monkeypatch.setattr(ops, "scatter_rows", lambda *a, **k: None)
    cfg, gpt = _tiny_decoder()
    ids, qe = _inputs(cfg, 3)
    tok = lambda rows: torch.zeros((rows, 1), dtype=torch.long)
    out = {}
    for w in ("bf16", "fp8"):
        def section(name):
            del calls[:]
            out[f"{name}/{w}"] = sec = []
            return lambda: sec.extend(dict(c) for c in calls)
        done = section("decode")
        st = generation.DecodeState(gpt, 2, Q + WIDTH + 2, w)
        st.step(ids[:2, :3], qe[:2])
        st.step(tok(2))
        st.step(tok(2))
        done()
        done = section("prefill_ragged")                                  # no query slots: a null pointer in the tail
        st = generation.SharedPrefixDecodeState(gpt, 3, WIDTH + 2, w)
        st.prefill_fan_out(ids, None, 1, prompt_len=LENGTHS)
        done()
        for name, lens in (("shared_uniform", None), ("shared_ragged", [4, 2])):
            done = section(name)
            st = generation.SharedPrefixDecodeState(gpt, 2 * 3, Q + WIDTH + 2, w)
            st.prefill_fan_out(ids[:2], qe[:2], 3, **({} if lens is None else dict(prompt_len=lens)))
            st.step(tok(6))
            st.step(tok(6))
            done()
        done = section("inflight")                                        # slot 1 stays idle
        st = generation.InflightDecodeState(gpt, 3, 2, Q + WIDTH, 3, w)
        st.install([0, 2], ids[:2], qe[:2], [3, 4])
        st.step(tok(6), torch.tensor([0, -1, 0], dtype=torch.int32), 0)
        st.step(tok(6), torch.tensor([1, -1, 1], dtype=torch.int32), 1)
        done()
    return out


# ------------------------------------------------------------------------------------------------ (b) the loops on the stand-ins
LISTS = ("row_step", "group_t", "slot_ids")
OPS = ("sample_advance", "sample_advance_ragged", "sample_advance_steps", "logits_constrain", "logits_constrain_ragged", "logits_constrain_steps",
       "sample_score", "sample_score_ragged", "sample_score_steps", "beam_advance", "beam_advance_groups", "logprob_topk", "gather_rows_ld",
       "scatter_rows")
STATE_METHODS = (("DecodeState", ("step", "prefill_fan_out", "reorder")), ("SharedPrefixDecodeState", ("step", "prefill_fan_out", "reorder")),
                 ("InflightDecodeState", ("install", "step")))


def _value(name, v):
    if torch.is_tensor(v):
        return [int(x) for x in v.reshape(-1).tolist()] if name in LISTS else {"shape": list(v.shape)}
    if isinstance(v, bool) or v is None or isinstance(v, (int, str)):
        return v
    if isinstance(v, float):
        return v.hex()
    if isinstance(v, (list, tuple)) and all(isinstance(x, int) for x in v):
        return [int(x) for x in v]
    return type(v).__name__                                               # a state, a constraints object


def _traced(trace, name, fn, method=False):
    sig = inspect.signature(fn)

    @functools.wraps(fn)                                                  # the loops look for prefill_fan_out's prompt_len keyword
    def call(*args, **kw):
        line = {"call": name}
        for k, v in sig.bind(*args, **kw).arguments.items():
            if method and k == "self":
                continue
            if sig.parameters[k].kind is inspect.Parameter.VAR_KEYWORD:
                line.update({kk: _value(kk, vv) for kk, vv in v.items()})
            else:
                line[k] = _value(k, v)
        trace.append(line)
        return fn(*args, **kw)
    return call


def _scores(sc):
    if sc is None:
        return None
    return {k: [float(x).hex() if getattr(sc, k).is_floating_point() else int(x) for x in getattr(sc, k).reshape(-1).tolist()]
            for k in ("live", "token_logprob", "sum_logprob", "count")}


def _loop_setup(monkeypatch):
    """the stand-ins, the trace wrappers over them, the tiny decoder -> (trace, cfg, gpt)"""
    import test_inflight_cpu as ti
    from youku_mplug_amd import generation, ops
    ti._on_cpu(monkeypatch)
    trace = []
    for name in OPS:
        monkeypatch.setattr(ops, name, _traced(trace, "ops." + name, getattr(ops, name)))
    for cls, methods in STATE_METHODS:
        for m in methods:
            monkeypatch.setattr(getattr(generation, cls), m, _traced(trace, f"{cls}.{m}", getattr(getattr(generation, cls), m), method=True))
    cfg, gpt = _tiny_decoder()
    return trace, cfg, gpt


def _run_loop_case(trace, cfg, gpt, family, kw):
    from youku_mplug_amd.generation import LogitsConstraints
    del trace[:]
    con = LogitsConstraints(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=2) if kw["con"] else None
    common = dict(constraints=con, decode_weights=kw["w"])
    if family == "sample":
        ids, qe = _inputs(cfg, len(LENGTHS))
        mixed = kw["mode"] == "mixed"
        out = gpt.sample_batched(ids, query_embeds=qe, prompt_length=LENGTHS if mixed else torch.tensor(LENGTHS), num_samples=SAMPLES, seed=11,
                                 temperature=1.1, top_p=0.9, kv=kw["kv"], return_scores=kw["scores"], mixed_prompts=mixed, **common)
        toks, sc = out if kw["scores"] else (out, None)
        res = {"tokens": toks.tolist(), "scores": _scores(sc)}
    elif family == "beam":
        ids, qe = _inputs(cfg, len(LENGTHS))
        more = {} if kw["groups"] == 1 else dict(beam_groups=kw["groups"], diversity_penalty=1.5)
        outs = gpt.beam_search_batched(ids, query_embeds=qe, beam_size=BEAMS, num_return_gen=2, kv=kw["kv"],
                                       prompt_length=LENGTHS if kw["mode"] == "mixed" else 3, **more, **common)
        res = [{"sequences": o.sequences.tolist(), "scores": [float(x).hex() for x in o.scores.tolist()],
                "group": o.group.tolist() if hasattr(o, "group") else None} for o in outs]
    else:
        ids, qe = _inputs(cfg, len(INFLIGHT_LENGTHS))
        out = gpt.sample_inflight(ids, query_embeds=qe, prompt_length=INFLIGHT_LENGTHS, num_samples=SAMPLES, slots=SLOTS, seed=11, temperature=1.1,
                                  top_p=0.9, max_new_tokens=INFLIGHT_BUDGETS, refill_min=kw["refill_min"], return_scores=kw["scores"], **common)
        res = {"tokens": out.tokens.tolist(), "written": list(out.written), "steps": out.steps, "prefills": out.prefills,
               "scores": _scores(out.scores)}
    return {"trace": [dict(line) for line in trace], "result": res}


# ------------------------------------------------------------------------------------------------ the fixture and the tests
@pytest.fixture(scope="module")
def golden():
    with open(GOLD) as f:
        return json.load(f)


def test_fixture_holds_every_case(golden):
    assert sorted(golden["entries"]) == sorted(ENTRY_CASES)
    assert sorted(golden["loops"]) == sorted(LOOP_CASES)
    for name in ENTRY_CASES:
        calls = golden["entries"][name]
        assert len(calls) >= 2 and all(c["checked"] == c["entry"] for c in calls if not c["entry"].endswith("_workspace_size")), name
        assert any(c["entry"].endswith("_q8") for c in calls) == name.endswith("/fp8"), name
    for name in LOOP_CASES:
        assert len(golden["loops"][name]["trace"]) >= 4, name


def test_entries_and_arguments_are_the_recorded_ones(monkeypatch, golden):
    got = json.loads(json.dumps(_entry_trace(monkeypatch)))
    assert sorted(got) == sorted(ENTRY_CASES)
    for name in ENTRY_CASES:
        assert got[name] == golden["entries"][name], name


@pytest.fixture
def loops(monkeypatch):
    return _loop_setup(monkeypatch)


@pytest.mark.parametrize("name", sorted(LOOP_CASES))
def test_loop_calls_and_results_are_the_recorded_ones(loops, golden, name):
    trace, cfg, gpt = loops
    got = json.loads(json.dumps(_run_loop_case(trace, cfg, gpt, *LOOP_CASES[name])))
    want = golden["loops"][name]
    for i, (a, b) in enumerate(zip(got["trace"], want["trace"])):
        assert a == b, (name, i)
    assert len(got["trace"]) == len(want["trace"]), name
    assert got["result"] == want["result"], name


def _record():
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        out["entries"] = _entry_trace(mp)
    with pytest.MonkeyPatch.context() as mp:
        trace, cfg, gpt = _loop_setup(mp)
        out["loops"] = {name: _run_loop_case(trace, cfg, gpt, *LOOP_CASES[name]) for name in sorted(LOOP_CASES)}
    with open(GOLD, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"recorded {len(out['entries'])} entry cases and {len(out['loops'])} loop cases into {GOLD}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_generation_trace_cpu.py --record")
    for p in (HERE, os.path.dirname(HERE)):
        if p not in sys.path:
            sys.path.insert(0, p)
    _record()
