"""DistributedGPT3_Caption.generate as a router, on CPU: which decoder calls a keyword combination turns into, and which refusal wins
when a call breaks two rules.  The decoder's five entry points are replaced by recorders that return canned results of the right
shapes, so every row of TABLE below is the whole observable behaviour of the method for its keywords: the sequence of decoder calls
(method, keyword names, clips, the values that route), the shape of what comes back, or the exception and its full message.  The
query features are passed in and _query_features fails the test when reached: a refused call never needs the ViT.

5 clips with prompts of 3 / 5 / 3 / 4 / 5 tokens and clips_per_search=2: grouped by prompt length the chunks are [0, 2], [3], [1, 4];
in input order [0, 1], [2, 3], [4]."""
import types

import pytest
import torch

import caption_score_cases as cs
import standin_overlap as so

LENGTHS = [3, 5, 3, 4, 5]
L, N, GEN = 6, 3, 4                     # input row width, samples per clip, tokens_to_generate
W = L + GEN                             # the full width of a result row
FIRST = 100                             # input_ids[i, 0] = FIRST + i: a recorder reads the clips of a call from its token rows
JUNK = 5                                # what a canned sampled row holds behind its termination: must be cut
GENS = [[20, 21], [20, 22, 21], [20, 21]]                  # the generated part of sample s
VALUE_KEYS = ("prompt_length", "slots", "kv", "mixed_prompts", "return_scores", "streams")
BASE = {"generate": {"query_embeds", "termination_id", "do_sample", "prompt_length"},
        "sample_batched": {"query_embeds", "temperature", "num_samples", "seed", "streams", "top_k", "top_p", "termination_id", "prompt_length"},
        "sample_inflight": {"query_embeds", "temperature", "num_samples", "slots", "seed", "top_k", "top_p", "termination_id", "prompt_length",
                            "max_new_tokens", "refill_min"},
        "beam_search_batched": {"query_embeds", "stop_token", "prompt_length"},
        "beam_search_inflight": {"query_embeds", "stop_token", "prompt_length", "slots", "max_new_tokens", "refill_min"}}


def _plain(v):
    return v.tolist() if torch.is_tensor(v) else v


class _Recorders:
    """the decoder's entry points: record (method, clips, keyword names, routing values), return a canned result"""

    def __init__(self, term):
        self.term, self.calls = term, []

    def _record(self, name, tokens, kw):
        clips = [int(r[0]) - FIRST for r in tokens.tolist()]
        self.calls.append((name, clips, tuple(sorted(kw)), {k: _plain(kw[k]) for k in VALUE_KEYS if k in kw}))

    def _sampled(self, tokens, lens, width, scored):
        from youku_mplug_amd import generation
        rows = []
        sc = generation.SampleScores(len(lens) * N, width, tokens.device)
        for j, pl in enumerate(lens):
            for s in range(N):
                gen = GENS[s] + [self.term]
                rows.append(tokens[j, :pl].tolist() + gen + [JUNK] * (width - pl - len(gen)))
                r = j * N + s
                sc.token_logprob[r, pl:pl + len(gen)] = -0.5 * (s + 1)
                sc.sum_logprob[r], sc.count[r] = -0.5 * (s + 1) * len(gen), len(gen)
        return torch.tensor(rows, dtype=torch.int64), (sc if scored else None)

    def _beams(self, tokens, lens, kw):
        trie = getattr(kw.get("constraints"), "allowed_phrases", None)
        out = []
        for j, pl in enumerate(lens):
            rows = [tokens[j, :pl].tolist() + gen + [self.term] * (W - pl - len(gen)) for gen in ([20, 21], [20, 22])]
            res = types.SimpleNamespace(sequences=torch.tensor(rows, dtype=torch.int64), scores=torch.tensor([-1.0, -2.0]))
            if "beam_groups" in kw:
                res.group = torch.tensor([0, 1], dtype=torch.int64)
            if trie is not None:
                res.phrase_index = torch.tensor([0, 1], dtype=torch.int64)
            out.append(res)
        return out

    def generate(self, tokens, **kw):
        self._record("generate", tokens, kw)
        assert kw["do_sample"] is False and tokens.shape[0] == 1
        return types.SimpleNamespace(sequences=self._beams(tokens, [kw["prompt_length"]], kw)[0].sequences[:1])

    def sample_batched(self, tokens, **kw):
        self._record("sample_batched", tokens, kw)
        toks, sc = self._sampled(tokens, _plain(kw["prompt_length"]), L + 3, kw.get("return_scores", False))
        return (toks, sc) if sc is not None else toks

    def sample_inflight(self, tokens, **kw):
        self._record("sample_inflight", tokens, kw)
        toks, sc = self._sampled(tokens, kw["prompt_length"], W, kw.get("return_scores", False))
        return types.SimpleNamespace(tokens=toks, written=[pl + 4 for pl in kw["prompt_length"]], scores=sc)

    def beam_search_batched(self, tokens, **kw):
        self._record("beam_search_batched", tokens, kw)
        pl = kw["prompt_length"]
        return self._beams(tokens, pl if isinstance(pl, list) else [pl] * tokens.shape[0], kw)

    def beam_search_inflight(self, tokens, **kw):
        self._record("beam_search_inflight", tokens, kw)
        return types.SimpleNamespace(results=self._beams(tokens, kw["prompt_length"], kw))


@pytest.fixture(scope="module")
def tiny():
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(torch.device("cpu"))
    term = g["meta"]["eod_id"]
    model.text_decoder.config.extra.update(tokens_to_generate=GEN)
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(30, 90, (len(LENGTHS), L), generator=gen)
    ids[:, 0] = FIRST + torch.arange(len(LENGTHS))
    mask = torch.zeros_like(ids)
    for i, pl in enumerate(LENGTHS):
        mask[i, :pl + 1] = 1
    text = types.SimpleNamespace(input_ids=ids, attention_mask=mask)
    qf = torch.zeros(len(LENGTHS) * model.num_learnable_token, model.text_width, dtype=torch.bfloat16)
    return model, term, text, qf


def _run(tiny, monkeypatch, keywords):
    model, term, text, qf = tiny
    rec = _Recorders(term)
    for name in BASE:
        monkeypatch.setattr(model.text_decoder, name, getattr(rec, name))
    monkeypatch.setattr(model, "_query_features", lambda *a, **k: pytest.fail("_query_features reached"))
    so.install(monkeypatch)
    del so.calls[:]
    was = model.training
    try:
        return rec, model.generate(None, text, termination_id=term, clips_per_search=2, query_features=qf, **keywords)
    finally:
        assert model.training == was


def _shape(out):
    """the return value -> ("list", shape of every clip's tensor) or ("pair", shape, sorted keys of every clip's dict)"""
    res, info = out if isinstance(out, tuple) else (out, None)
    assert isinstance(res, list) and len(res) == len(LENGTHS) and all(r.dtype == torch.int64 for r in res)
    shapes = {tuple(r.shape) for r in res}
    assert len(shapes) == 1, shapes
    if info is None:
        return ("list", shapes.pop())
    assert isinstance(info, list) and len(info) == len(LENGTHS)
    keys = {tuple(sorted(d)) for d in info}
    assert len(keys) == 1, keys
    return ("pair", shapes.pop(), keys.pop())


# ------------------------------------------------------------------------------------------------ the table
PER_CLIP = [(3, [0]), (5, [1]), (3, [2]), (4, [3]), (5, [4])]
GROUPED = [(3, [0, 2]), (4, [3]), (5, [1, 4])]                                # the beam search: one length per chunk
GROUPED_ROWS = [([3, 3], [0, 2]), ([4], [3]), ([5, 5], [1, 4])]                 # the sampler: one length per clip of the chunk
INPUT_ORDER = [([3, 5], [0, 1]), ([3, 4], [2, 3]), ([5], [4])]
ALL = [(LENGTHS, [0, 1, 2, 3, 4])]


def calls(method, chunks, extra=(), **values):
    """one expected call per chunk: the method's own keywords plus `extra`; prompt_length and (the sampler's rule: stream = clip * N +
    sample) streams from the chunk, the other routing values from `values`"""
    names = tuple(sorted(BASE[method] | set(extra)))
    out = []
    for pl, clips in chunks:
        vals = dict(values, prompt_length=pl)
        if method == "sample_batched":
            vals["streams"] = [i * N + s for i in clips for s in range(N)]
        out.append((method, clips, names, vals))
    return out


def ok(expected_calls, shape, overlap=0):
    return ("ok", expected_calls, shape, overlap)


def refused(message):
    return ("refused", message)


SP = dict(kv_cache="shared_prefix")
MODES = {"per_clip": {}, "batched": dict(batched=True), "do_sample": dict(do_sample=True, num_samples=N),
         "mixed_prompts": dict(batched=True, mixed_prompts=True, **SP), "sample_mixed_prompts": dict(do_sample=True, num_samples=N, sample_mixed_prompts=True, **SP),
         "inflight": dict(do_sample=True, num_samples=N, inflight=True, **SP), "beam_inflight": dict(batched=True, beam_inflight=True, **SP)}
FP8, NGRAM, PHRASES, GROUPS = dict(decode_weights="fp8"), dict(no_repeat_ngram_size=2), dict(allowed_phrases=[[20, 21], [20, 22]]), dict(beam_groups=2)
KV = "shared_prefix"
ONE, TWO, ALL_N = ("list", (1, W)), ("list", (2, W)), ("list", (N, W))
SCORE_KEYS = ("count", "sum_logprob", "token_logprob")
PICK_KEYS = ("count", "index", "sum_logprob", "token_logprob")
CONS_KEYS = ("consensus", "count", "index", "sum_logprob", "token_logprob")
NO_GROUPS = "beam_groups=2 needs batched=True without do_sample: the per-clip search and the samplers have no groups"
NO_CONSTRAINTS = ("repetition_penalty / no_repeat_ngram_size / min_new_tokens / banned_token_ids / constrain_prompt need batched=True or "
                  "do_sample=True (got repetition_penalty=None, no_repeat_ngram_size=2, min_new_tokens=0, banned_token_ids=None, "
                  "constrain_prompt=False): the per-clip search has no constraints")

TABLE = {
    # every mode alone
    "per_clip": ({}, ok(calls("generate", PER_CLIP), ONE)),
    "batched": (MODES["batched"], ok(calls("beam_search_batched", GROUPED), TWO)),
    "do_sample": (MODES["do_sample"], ok(calls("sample_batched", GROUPED_ROWS), ALL_N)),
    "mixed_prompts": (MODES["mixed_prompts"], ok(calls("beam_search_batched", INPUT_ORDER, ["kv"], kv=KV), TWO)),
    "sample_mixed_prompts": (MODES["sample_mixed_prompts"],
                             ok(calls("sample_batched", INPUT_ORDER, ["kv", "mixed_prompts"], kv=KV, mixed_prompts=True), ALL_N)),
    "inflight": (MODES["inflight"], ok(calls("sample_inflight", ALL, slots=2), ALL_N)),                      # kv is not forwarded in flight
    "beam_inflight": (MODES["beam_inflight"], ok(calls("beam_search_inflight", ALL, slots=2), TWO)),
    # x decode_weights="fp8"
    "per_clip+fp8": (FP8, ok(calls("generate", PER_CLIP, ["decode_weights"]), ONE)),
    "batched+fp8": (dict(MODES["batched"], **FP8), ok(calls("beam_search_batched", GROUPED, ["decode_weights"]), TWO)),
    "do_sample+fp8": (dict(MODES["do_sample"], **FP8), ok(calls("sample_batched", GROUPED_ROWS, ["decode_weights"]), ALL_N)),
    "mixed_prompts+fp8": (dict(MODES["mixed_prompts"], **FP8), ok(calls("beam_search_batched", INPUT_ORDER, ["decode_weights", "kv"], kv=KV), TWO)),
    "sample_mixed_prompts+fp8": (dict(MODES["sample_mixed_prompts"], **FP8),
                                 ok(calls("sample_batched", INPUT_ORDER, ["decode_weights", "kv", "mixed_prompts"], kv=KV, mixed_prompts=True), ALL_N)),
    "inflight+fp8": (dict(MODES["inflight"], **FP8), ok(calls("sample_inflight", ALL, ["decode_weights"], slots=2), ALL_N)),
    "beam_inflight+fp8": (dict(MODES["beam_inflight"], **FP8), ok(calls("beam_search_inflight", ALL, ["decode_weights"], slots=2), TWO)),
    # x kv_cache="shared_prefix" (the four modes that need it carry it above)
    "per_clip+kv": (SP, refused('kv_cache="shared_prefix" needs batched=True or do_sample=True (the per-clip search keeps a cache per beam)')),
    "batched+kv": (dict(MODES["batched"], **SP), ok(calls("beam_search_batched", GROUPED, ["kv"], kv=KV), TWO)),
    "do_sample+kv": (dict(MODES["do_sample"], **SP), ok(calls("sample_batched", GROUPED_ROWS, ["kv"], kv=KV), ALL_N)),
    # x one constraint
    "per_clip+ngram": (NGRAM, refused(NO_CONSTRAINTS)),
    "batched+ngram": (dict(MODES["batched"], **NGRAM), ok(calls("beam_search_batched", GROUPED, ["constraints"]), TWO)),
    "do_sample+ngram": (dict(MODES["do_sample"], **NGRAM), ok(calls("sample_batched", GROUPED_ROWS, ["constraints"]), ALL_N)),
    "mixed_prompts+ngram": (dict(MODES["mixed_prompts"], **NGRAM), ok(calls("beam_search_batched", INPUT_ORDER, ["constraints", "kv"], kv=KV), TWO)),
    "sample_mixed_prompts+ngram": (dict(MODES["sample_mixed_prompts"], **NGRAM),
                                   ok(calls("sample_batched", INPUT_ORDER, ["constraints", "kv", "mixed_prompts"], kv=KV, mixed_prompts=True), ALL_N)),
    "inflight+ngram": (dict(MODES["inflight"], **NGRAM), ok(calls("sample_inflight", ALL, ["constraints"], slots=2), ALL_N)),
    "beam_inflight+ngram": (dict(MODES["beam_inflight"], **NGRAM), ok(calls("beam_search_inflight", ALL, ["constraints"], slots=2), TWO)),
    # x allowed_phrases: the beam modes return (res, info); the sampled ones only add phrase_index to the scores
    "per_clip+phrases": (PHRASES, refused("allowed_phrases need batched=True or do_sample=True: the per-clip search has no constraints")),
    "batched+phrases": (dict(MODES["batched"], **PHRASES),
                        ok(calls("beam_search_batched", GROUPED, ["constraints"]), ("pair", (2, W), ("phrase_index", "scores")))),
    "do_sample+phrases": (dict(MODES["do_sample"], **PHRASES), ok(calls("sample_batched", GROUPED_ROWS, ["constraints"]), ALL_N)),
    "do_sample+phrases+return_scores": (dict(MODES["do_sample"], return_scores=True, **PHRASES),
                                        ok(calls("sample_batched", GROUPED_ROWS, ["constraints", "return_scores"], return_scores=True),
                                           ("pair", (N, W), ("count", "phrase_index", "sum_logprob", "token_logprob")))),
    "mixed_prompts+phrases": (dict(MODES["mixed_prompts"], **PHRASES),
                              ok(calls("beam_search_batched", INPUT_ORDER, ["constraints", "kv"], kv=KV), ("pair", (2, W), ("phrase_index", "scores")))),
    "sample_mixed_prompts+phrases": (dict(MODES["sample_mixed_prompts"], **PHRASES),
                                     ok(calls("sample_batched", INPUT_ORDER, ["constraints", "kv", "mixed_prompts"], kv=KV, mixed_prompts=True), ALL_N)),
    "inflight+phrases": (dict(MODES["inflight"], **PHRASES), ok(calls("sample_inflight", ALL, ["constraints"], slots=2), ALL_N)),
    "beam_inflight+phrases": (dict(MODES["beam_inflight"], **PHRASES),
                              ok(calls("beam_search_inflight", ALL, ["constraints"], slots=2), ("pair", (2, W), ("phrase_index", "scores")))),
    # x beam_groups=2
    "per_clip+groups": (GROUPS, refused(NO_GROUPS)),
    "batched+groups": (dict(MODES["batched"], **GROUPS), ok(calls("beam_search_batched", GROUPED, ["beam_groups", "diversity_penalty"]), TWO)),
    "do_sample+groups": (dict(MODES["do_sample"], **GROUPS), refused(NO_GROUPS)),
    "mixed_prompts+groups": (dict(MODES["mixed_prompts"], **GROUPS),
                             ok(calls("beam_search_batched", INPUT_ORDER, ["beam_groups", "diversity_penalty", "kv"], kv=KV), TWO)),
    "sample_mixed_prompts+groups": (dict(MODES["sample_mixed_prompts"], **GROUPS), refused(NO_GROUPS)),
    "inflight+groups": (dict(MODES["inflight"], **GROUPS), refused(NO_GROUPS)),
    "beam_inflight+groups": (dict(MODES["beam_inflight"], **GROUPS),
                             ok(calls("beam_search_inflight", ALL, ["beam_groups", "diversity_penalty"], slots=2), TWO)),
    # the sampled modes x return_scores / best_of / consensus / both: return_scores=True is forwarded whenever scores are needed
    "do_sample+return_scores": (dict(MODES["do_sample"], return_scores=True),
                                ok(calls("sample_batched", GROUPED_ROWS, ["return_scores"], return_scores=True), ("pair", (N, W), SCORE_KEYS))),
    "do_sample+best_of": (dict(MODES["do_sample"], best_of=True), ok(calls("sample_batched", GROUPED_ROWS, ["return_scores"], return_scores=True), ONE)),
    "do_sample+best_of+return_scores": (dict(MODES["do_sample"], best_of=True, return_scores=True),
                                        ok(calls("sample_batched", GROUPED_ROWS, ["return_scores"], return_scores=True), ("pair", (1, W), PICK_KEYS))),
    "do_sample+consensus": (dict(MODES["do_sample"], consensus="rouge_l"), ok(calls("sample_batched", GROUPED_ROWS), ONE, overlap=3)),
    "do_sample+consensus+return_scores": (dict(MODES["do_sample"], consensus="rouge_l", return_scores=True),
                                          ok(calls("sample_batched", GROUPED_ROWS, ["return_scores"], return_scores=True),
                                             ("pair", (1, W), CONS_KEYS), overlap=3)),
    "sample_mixed_prompts+return_scores": (dict(MODES["sample_mixed_prompts"], return_scores=True),
                                           ok(calls("sample_batched", INPUT_ORDER, ["kv", "mixed_prompts", "return_scores"], kv=KV, mixed_prompts=True,
                                                    return_scores=True), ("pair", (N, W), SCORE_KEYS))),
    "sample_mixed_prompts+best_of": (dict(MODES["sample_mixed_prompts"], best_of=True),
                                     ok(calls("sample_batched", INPUT_ORDER, ["kv", "mixed_prompts", "return_scores"], kv=KV, mixed_prompts=True,
                                              return_scores=True), ONE)),
    "sample_mixed_prompts+consensus": (dict(MODES["sample_mixed_prompts"], consensus="rouge_l"),
                                       ok(calls("sample_batched", INPUT_ORDER, ["kv", "mixed_prompts"], kv=KV, mixed_prompts=True), ONE, overlap=3)),
    "sample_mixed_prompts+consensus+return_scores": (dict(MODES["sample_mixed_prompts"], consensus="ngram_f", return_scores=True),
                                                     ok(calls("sample_batched", INPUT_ORDER, ["kv", "mixed_prompts", "return_scores"], kv=KV,
                                                              mixed_prompts=True, return_scores=True), ("pair", (1, W), CONS_KEYS), overlap=3)),
    "inflight+return_scores": (dict(MODES["inflight"], return_scores=True),
                               ok(calls("sample_inflight", ALL, ["return_scores"], slots=2, return_scores=True), ("pair", (N, W), SCORE_KEYS))),
    "inflight+best_of": (dict(MODES["inflight"], best_of=True), ok(calls("sample_inflight", ALL, ["return_scores"], slots=2, return_scores=True), ONE)),
    "inflight+consensus": (dict(MODES["inflight"], consensus="rouge_l"), ok(calls("sample_inflight", ALL, slots=2), ONE, overlap=1)),
    "inflight+consensus+return_scores": (dict(MODES["inflight"], consensus="rouge_l", return_scores=True),
                                         ok(calls("sample_inflight", ALL, ["return_scores"], slots=2, return_scores=True),
                                            ("pair", (1, W), CONS_KEYS), overlap=1)),
    # the batched modes x rerank_by_consensus: one overlap call over all the clips' rows
    "batched+rerank_by_consensus": (dict(MODES["batched"], rerank_by_consensus="rouge_l"),
                                    ok(calls("beam_search_batched", GROUPED), ("pair", (2, W), ("consensus", "group")), overlap=1)),
    "mixed_prompts+rerank_by_consensus": (dict(MODES["mixed_prompts"], rerank_by_consensus="ngram_f"),
                                          ok(calls("beam_search_batched", INPUT_ORDER, ["kv"], kv=KV), ("pair", (2, W), ("consensus", "group")), overlap=1)),
    "beam_inflight+rerank_by_consensus": (dict(MODES["beam_inflight"], rerank_by_consensus="rouge_l"),
                                          ok(calls("beam_search_inflight", ALL, slots=2), ("pair", (2, W), ("consensus", "group")), overlap=1)),
    # two rules broken at once: the first refusal
    "consensus+best_of-do_sample": (dict(consensus="rouge_l", best_of=True),
                                    refused("consensus needs do_sample=True (beam hypotheses: batched=True with rerank_by_consensus=)")),
    "beam_inflight+mixed_prompts+do_sample": (dict(MODES["beam_inflight"], mixed_prompts=True, do_sample=True),
                                              refused("mixed_prompts does not combine with do_sample: a sampled token is a function of its table column, "
                                                      "which the left padding would make depend on the longest prompt of the chunk (sampled captions over "
                                                      "prompts of different lengths: sample_mixed_prompts=True)")),
    "inflight-do_sample-kv": (dict(inflight=True),
                              refused("inflight needs do_sample=True (beam search in flight: batched=True with beam_inflight=True; greedy captions: "
                                      "do_sample=True with top_k=1)")),
    "max_new_tokens-inflight+return_scores-do_sample": (dict(max_new_tokens=3, return_scores=True),
                                                        refused("max_new_tokens / refill_min belong to inflight=True (sampled captions) or "
                                                                "beam_inflight=True (beam search)")),
    "phrases+rerank_by_logprob-lockstep": (dict(PHRASES, rerank_by_logprob=True),
                                           refused("rerank_by_logprob needs batched=True without do_sample (sampled captions: best_of=True)")),
    "kv_paged+return_scores-do_sample": (dict(kv_cache="paged", return_scores=True),
                                         refused("return_scores / best_of need do_sample=True (got return_scores=True, best_of=False): beam hypotheses "
                                                 "carry their own scores")),
}


def test_the_chunks_are_the_ones_the_table_assumes():
    from youku_mplug_amd.downstream import _prompt_length_chunks
    assert [(pl, c) for pl, c in _prompt_length_chunks(LENGTHS, 2)] == GROUPED
    assert [c for _, c in INPUT_ORDER] == [[0, 1], [2, 3], [4]] and [pl for pl, _ in INPUT_ORDER] == [[3, 5], [3, 4], [5]]


@pytest.mark.parametrize("row", list(TABLE))
def test_generate_routes_and_refuses_as_tabled(tiny, monkeypatch, row):
    keywords, expect = TABLE[row]
    if expect[0] == "refused":
        with pytest.raises(ValueError) as e:
            _run(tiny, monkeypatch, keywords)
        assert type(e.value) is ValueError and str(e.value) == expect[1]
        return
    rec, out = _run(tiny, monkeypatch, keywords)
    _, want_calls, want_shape, overlap = expect
    assert rec.calls == want_calls
    assert _shape(out) == want_shape
    assert len(so.calls) == overlap
    res = out[0] if isinstance(out, tuple) else out
    _, term, text, _ = tiny
    for i, r in enumerate(res):                                        # every row continues its own clip's prompt; nothing canned leaks
        assert (r[:, :LENGTHS[i]] == text.input_ids[i, :LENGTHS[i]]).all() and not (r == JUNK).any(), i
