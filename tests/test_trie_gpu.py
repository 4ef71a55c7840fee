"""mpv_logits_trie_mask on the GPU: the kernel, bit for bit on the whole [rows, ld] matrix, against the
independent reference tests/ref_trie.py on every case of tests/trie_cases.py -- poison in the columns behind the vocabulary, a canary
behind the matrix, node_out --; the ragged and steps entries against the uniform entry on the row alone; determinism, independence of
the launch and the refusals; then the four loops on the tiny model with a 12-phrase trie against the same call whose trie_fn masks on
the host (tests/standin_trie.py), DistributedGPT3_Caption.generate(allowed_phrases=) and the caption entry point's flag."""
import ctypes as C
import random
import types

import pytest
import torch

import ref_trie
import standin_trie as stt
import trie_cases as tc

pytestmark = pytest.mark.gpu
CANARY = 64
MARK = -7.5
EOS_IDS = [tc.EOS]


def _trie(phrases, vocab):
    from youku_mplug_amd.generation import PhraseTrie
    return PhraseTrie(phrases, vocab)


_TRIES = {}


def _case_trie(c):
    key = (c["trie"], c["V"])
    if key not in _TRIES:
        ph = tc.phrases_of(*key)
        _TRIES[key] = (_trie(ph, c["V"]), ref_trie.build(ph))
    return _TRIES[key]


def _guarded(logits, dev):
    buf = torch.full((logits.numel() + CANARY,), MARK, dtype=torch.bfloat16, device=dev)
    view = buf[:logits.numel()].view(logits.shape)
    view.copy_(logits)
    return view, buf


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _uniform(dev, trie, logits, tokens, prompt_len, pos, ban, V, eos=EOS_IDS):
    """the uniform entry -> (logits, node_out), both on the CPU"""
    from youku_mplug_amd import ops
    view, buf = _guarded(logits, dev)
    node = torch.full((logits.shape[0],), -9, dtype=torch.int32, device=dev)
    out = ops.logits_trie_mask(view, tokens.to(dev), pos=pos, trie=trie, prompt_len=prompt_len.to(dev), eos_ids=eos, ban_value=ban, node_out=node,
                               vocab=V)
    torch.cuda.synchronize()
    assert out is view and bool((buf[logits.numel():] == MARK).all()), "the canary behind the logits was overwritten"
    return view.cpu(), node.cpu()


@pytest.mark.parametrize("case", tc.KERNEL_CASES, ids=tc.case_id)
def test_kernel_equals_the_reference_bitwise(dev, case):
    b = tc.build(case)
    V, rows = case["V"], case["rows"]
    trie, root = _case_trie(case)
    got, node = _uniform(dev, trie, b["logits"], b["tokens"], b["prompt_len"], b["pos"], b["ban"], V)
    want, want_node = ref_trie.trie_mask(b["logits"], b["tokens"], root, columns=[b["pos"]] * rows, prompt_len=b["prompt_len"].tolist(),
                                         eos_ids=EOS_IDS, ban_value=b["ban"], vocab=V)
    assert (got[:, V:] == tc.POISON).all(), "a column behind the vocabulary was written"
    diff = (_bits(got) != _bits(want)).nonzero()
    assert diff.numel() == 0, (tc.case_id(case), diff[:8].tolist(), [(b["kinds"][r], float(got[r, c]), float(want[r, c])) for r, c in diff[:8].tolist()])
    assert node.tolist() == want_node, [(r, b["kinds"][r], n, w) for r, (n, w) in enumerate(zip(node.tolist(), want_node)) if n != w][:8]
    forced = [r for r, k in enumerate(b["kinds"]) if k == "forced"]
    assert torch.equal(_bits(got[forced]), _bits(b["logits"][forced])) and all(node[r] == -2 for r in forced)
    if rows >= 7:                                              # the launch holds live, dead and untouched rows
        assert {-2, -1} <= set(want_node) and max(want_node) >= 0
    # the same launch again: identical bits
    again, node2 = _uniform(dev, trie, b["logits"], b["tokens"], b["prompt_len"], b["pos"], b["ban"], V)
    assert torch.equal(_bits(again), _bits(got)) and torch.equal(node2, node)


def test_both_ban_values_and_several_termination_ids(dev):
    """the finite ban value is the lowest finite bf16; termination ids out of range are ignored, the in-range ones are all allowed at a
    terminal node and on a dead row"""
    c = dict(V=1000, rows=160, trie="prefix", ban="inf")
    b = tc.build(c, seed=3)
    trie, root = _case_trie(c)
    eos = [7, 999, 1000, -1, 2 ** 40, 0, 7, 500]
    for ban in (tc.BAN_INF, tc.BAN_FINITE):
        got, node = _uniform(dev, trie, b["logits"], b["tokens"], b["prompt_len"], b["pos"], ban, 1000, eos=eos)
        want, want_node = ref_trie.trie_mask(b["logits"], b["tokens"], root, columns=[b["pos"]] * 160, prompt_len=b["prompt_len"].tolist(),
                                             eos_ids=eos, ban_value=ban, vocab=1000)
        assert torch.equal(_bits(got), _bits(want)) and node.tolist() == want_node
        dead = want_node.index(-1)
        kept = (_bits(got[dead, :1000]) == _bits(b["logits"][dead, :1000])).nonzero().view(-1).tolist()
        assert {0, 7, 500, 999} <= set(kept)
    assert float(torch.tensor(tc.BAN_FINITE).to(torch.bfloat16)) == tc.BAN_FINITE


def test_a_row_alone_equals_the_row_inside_a_batch(dev):
    c = dict(V=1000, rows=160, trie="random", ban="finite")
    b = tc.build(c, seed=5)
    trie, _ = _case_trie(c)
    full, node = _uniform(dev, trie, b["logits"], b["tokens"], b["prompt_len"], b["pos"], b["ban"], 1000)
    for r in (0, 1, 2, 3, 4, 5, 6, 80, 159):
        one, n1 = _uniform(dev, trie, b["logits"][r:r + 1].clone(), b["tokens"][r:r + 1].clone(), b["prompt_len"][r:r + 1], b["pos"], b["ban"], 1000)
        assert torch.equal(_bits(one[0]), _bits(full[r])) and int(n1[0]) == int(node[r]), r
    order = torch.randperm(160, generator=torch.Generator().manual_seed(1))
    perm, nperm = _uniform(dev, trie, b["logits"][order].clone(), b["tokens"][order].clone(), b["prompt_len"][order], b["pos"], b["ban"], 1000)
    assert torch.equal(_bits(perm), _bits(full[order])) and torch.equal(nperm, node[order])


def _left_aligned(c, seed, steps_of):
    """a left-aligned table for the ragged / steps entries: row r holds a prompt of r % 4 tokens and behind it a history of the case
    table's kinds -> (logits, tokens, prompt_len, row_step per row)"""
    V, rows = c["V"], c["rows"]
    phrases = tc.phrases_of(c["trie"], V)
    rng = random.Random(seed)
    row_len = 14
    tokens = torch.tensor([[rng.randrange(V) for _ in range(row_len)] for _ in range(rows)], dtype=torch.int64)
    prompt_len = torch.tensor([r % 4 for r in range(rows)], dtype=torch.int64)
    steps = []
    for r in range(rows):
        h, _ = tc.history(tc.HISTORIES[r % 6], phrases, V, rng, tc._PREFIXES[(c["trie"], V)])
        h = h[:8]
        tokens[r, r % 4:r % 4 + len(h)] = torch.tensor(h, dtype=torch.int64)
        steps.append(steps_of(r, len(h)))
    g = torch.Generator().manual_seed(seed)
    logits = torch.full((rows, V + 8), tc.POISON, dtype=torch.bfloat16)
    logits[:, :V] = (torch.randn(rows, V, generator=g) * 3.0).to(torch.bfloat16)
    return logits, tokens, prompt_len, steps


@pytest.mark.parametrize("entry", ["ragged", "steps"])
def test_ragged_and_steps_rows_equal_the_uniform_entry_on_the_row_alone(dev, entry):
    from youku_mplug_amd import ops
    c = dict(V=1000, rows=41, trie="prefix", ban="inf")
    trie, root = _case_trie(c)
    if entry == "ragged":                                      # one step for all: rows 3, 7, ... (prompt 3) run out of columns at step 11
        logits, tokens, prompt_len, steps = _left_aligned(c, 21, lambda r, n: 2)
        steps = [11 if r >= 20 else 2 for r in range(41)]
        runs = [(2, list(range(20))), (11, list(range(20, 41)))]
    else:                                                      # a step per row: its history's length, -1 (frozen), or behind the table
        logits, tokens, prompt_len, steps = _left_aligned(c, 22, lambda r, n: -1 if r % 9 == 4 else 13 if r % 9 == 8 else n)
        runs = [(None, list(range(41)))]
    for ban in (tc.BAN_INF, tc.BAN_FINITE):
        for step, rows in runs:
            sel = torch.tensor(rows)
            view, buf = _guarded(logits[sel], dev)
            node = torch.full((len(rows),), -9, dtype=torch.int32, device=dev)
            kw = dict(trie=trie, prompt_len=prompt_len[sel].to(dev), eos_ids=EOS_IDS, ban_value=ban, node_out=node, vocab=1000)
            if entry == "ragged":
                ops.logits_trie_mask_ragged(view, tokens[sel].to(dev), step=step, **kw)
            else:
                ops.logits_trie_mask_steps(view, tokens[sel].to(dev), row_step=torch.tensor([steps[r] for r in rows], dtype=torch.int32, device=dev), **kw)
            torch.cuda.synchronize()
            assert bool((buf[view.numel():] == MARK).all())
            got, node = view.cpu(), node.cpu()
            cols = [stt._column(prompt_len, r, tokens.shape[1], steps[r]) for r in rows]
            want, want_node = ref_trie.trie_mask(logits[sel], tokens[sel], root, columns=cols, prompt_len=prompt_len[sel].tolist(), eos_ids=EOS_IDS,
                                                 ban_value=ban, vocab=1000)
            assert torch.equal(_bits(got), _bits(want)) and node.tolist() == want_node
            frozen = [i for i, col in enumerate(cols) if col is None]
            assert (frozen or step == 2) and torch.equal(_bits(got[frozen]), _bits(logits[sel][frozen])) and all(node[i] == -2 for i in frozen)
            for i, r in enumerate(rows):                       # the uniform entry on the row alone at pos = c_r
                if cols[i] is None or i % 3:
                    continue
                one, n1 = _uniform(dev, trie, logits[r:r + 1].clone(), tokens[r:r + 1].clone(), prompt_len[r:r + 1], cols[i], ban, 1000)
                assert torch.equal(_bits(one[0]), _bits(got[i])) and int(n1[0]) == int(node[i]), (entry, r)


def test_refusals_leave_the_logits_untouched(dev):
    import test_trie_cpu as tcpu
    from youku_mplug_amd import _lib, ops
    c = dict(V=64, rows=2, trie="prefix", ban="inf")
    trie = _trie(tc.phrases_of("prefix", 64), 64)
    logits = torch.full((2, 72), tc.POISON, dtype=torch.bfloat16)
    logits[:, :64] = torch.randn(2, 64, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    view, buf = _guarded(logits, dev)
    before = buf.clone()
    tokens = torch.randint(0, 64, (2, 16), device=dev)
    arrays = trie.arrays(dev)
    real = dict(logits=view, tokens=tokens, prompt_len=torch.zeros(2, dtype=torch.int64, device=dev), eos_ids=torch.tensor([7], device=dev),
                child_begin=arrays[0], child_tok=arrays[1], child_node=arrays[2], terminal=arrays[3],
                node_out=torch.zeros(2, dtype=torch.int32, device=dev))
    ptr = {k: v.data_ptr() for k, v in real.items()}
    ptr.update(n_nodes=trie.n_nodes, n_edges=trie.n_edges)
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib()
    for over in tcpu.REFUSALS:
        fields = dict(ptr)
        fields.update({k: (None if v is None else ptr[k] + (v & 15)) if k in real else v for k, v in over.items()})
        for fn, more in ((lib.mpv_logits_trie_mask, ()), (lib.mpv_logits_trie_mask_ragged, ()),
                         (lib.mpv_logits_trie_mask_steps, (torch.zeros(2, dtype=torch.int32, device=dev).data_ptr(),))):
            if more and set(over) == {"pos"}:
                continue                                       # the steps entry ignores pos
            rc = fn(C.byref(tcpu._desc(**fields)), *more, stream)
            torch.cuda.synchronize()
            assert rc < 0 and torch.equal(_bits(buf), _bits(before)), over
    assert lib.mpv_logits_trie_mask(C.byref(tcpu._desc(**ptr)), stream) == 0       # the accepted descriptor does edit
    torch.cuda.synchronize()
    assert not torch.equal(_bits(buf), _bits(before))
    for bad_logits, bad_tokens in ((view.float(), tokens), (view, tokens.int()), (view, tokens[:1]), (view.cpu(), tokens.cpu())):
        with pytest.raises(_lib.MpvError):
            ops.logits_trie_mask(bad_logits, bad_tokens, pos=3, trie=trie, eos_ids=[7])


# ------------------------------------------------------------------------------ on the tiny model
_MODEL = {}


def _caption_model(dev):
    if not _MODEL:
        import test_sampling_gpu as tg
        _MODEL["m"] = tg._caption_model(dev)
    return _MODEL["m"]


def _host_mask(name):
    """a trie_fn that masks on the host with the stand-in, from the downloaded logits and table"""
    fn = getattr(stt, name)

    def masked(logits, tokens, **kw):
        host = logits.cpu()
        fn(host, tokens.cpu(), **{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in kw.items()})
        logits.copy_(host)
        return logits
    return masked


def _inputs(dev, B=3, Q=6, seed=8):
    from oracle.weights import CONFIG_TINY
    g = torch.Generator().manual_seed(seed)
    qe = (torch.randn(B, Q, CONFIG_TINY.hidden, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    return qe, torch.randint(0, CONFIG_TINY.vocab, (B, 5), generator=g).to(dev)


def _twelve(eod):
    """12 phrases of 1..4 tokens over the tiny vocabulary with shared prefixes, one the prefix of another, one given twice"""
    from oracle.weights import CONFIG_TINY
    rng = random.Random(12)
    free = [t for t in range(CONFIG_TINY.vocab) if t != eod]
    a = rng.sample(free, 6)
    ph = [[a[0]], [a[0], a[1]], [a[0], a[1], a[2]], [a[0], a[3]], [a[1], a[0]], [a[1], a[1], a[4], a[5]], [a[2]], [a[3], a[3]], [a[4], a[0], a[1]],
          [a[5], a[2]], [a[5], a[4]], [a[0], a[1]]]
    return ph, _trie(ph, CONFIG_TINY.vocab)


def _check_rows_are_phrases(rows, pl, eod, trie, index=None):
    from youku_mplug_amd.generation import generated_part
    for i, row in enumerate(rows.tolist()):
        idx = trie.lookup(generated_part(row, pl, eod))
        assert idx >= 0 and eod in row[pl:], (i, row)
        assert index is None or int(index[i]) == idx


@pytest.mark.parametrize("kv,weights", [("per_sequence", "bf16"), ("shared_prefix", "bf16"), ("shared_prefix", "fp8")])
def test_beam_search_batched_along_the_trie_equals_the_loop_with_the_host_mask(dev, kv, weights):
    from youku_mplug_amd import generation, ops
    m, model, video, ids, mask = _caption_model(dev)
    td, eod = model.text_decoder, m["eod_id"]
    qe, tokens = _inputs(dev, seed=12)
    ph, trie = _twelve(eod)
    c = generation.LogitsConstraints(allowed_phrases=trie)
    P, K = 4, 4
    kw = dict(query_embeds=qe, beam_size=K, num_return_gen=4, stop_token=eod, prompt_length=P)
    model.eval()
    with torch.no_grad():
        got = td.beam_search_batched(tokens.clone(), kv=kv, constraints=c, decode_weights=weights, **kw)
        want = generation.beam_search_batched_loop(generation._gen_config(td), generation.make_state_fn(td, kv, weights), tokens.clone(),
                                                   topk_fn=lambda lg, k, add: ops.logprob_topk(lg, k, add=add), advance_fn=ops.beam_advance,
                                                   constraints=c, trie_fn=_host_mask("logits_trie_mask"), **kw)
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert torch.equal(a.sequences, b.sequences) and torch.equal(a.scores, b.scores) and torch.equal(a.phrase_index, b.phrase_index)
        assert a.sequences.shape[0] == 4 and torch.isfinite(a.scores).all() and len(set(a.phrase_index.tolist())) == 4
        _check_rows_are_phrases(a.sequences, P, eod, trie, a.phrase_index)


def test_fewer_phrases_than_beams_return_only_phrases_and_no_nan(dev):
    from youku_mplug_amd import generation
    m, model, video, ids, mask = _caption_model(dev)
    td, eod = model.text_decoder, m["eod_id"]
    qe, tokens = _inputs(dev, seed=12)
    ph, _ = _twelve(eod)
    trie = _trie(ph[:2], 1024)
    with torch.no_grad():
        for groups in ({}, dict(beam_groups=2, diversity_penalty=0.5)):
            got = td.beam_search_batched(tokens.clone(), query_embeds=qe, beam_size=4, num_return_gen=4, stop_token=eod, prompt_length=4,
                                         kv="shared_prefix", constraints=generation.LogitsConstraints(allowed_phrases=trie), **groups)
            for o in got:
                assert 1 <= o.sequences.shape[0] <= 4 and not torch.isnan(o.scores).any() and torch.isfinite(o.scores).all()
                _check_rows_are_phrases(o.sequences, 4, eod, trie, o.phrase_index)
                if not groups:
                    assert sorted(o.phrase_index.tolist()) == [0, 1]


@pytest.mark.parametrize("kv", ["per_sequence", "shared_prefix"])
def test_sample_batched_along_the_trie_equals_the_loop_with_the_host_mask(dev, kv):
    from youku_mplug_amd import generation, ops
    m, model, video, ids, mask = _caption_model(dev)
    td, eod = model.text_decoder, m["eod_id"]
    qe, tokens = _inputs(dev)
    ph, trie = _twelve(eod)
    c = generation.LogitsConstraints(allowed_phrases=trie)
    lengths = torch.tensor([5, 2, 3], device=dev)
    kw = dict(query_embeds=qe, prompt_length=lengths.clone(), termination_id=eod, temperature=1.2, num_samples=4, seed=9)
    with torch.no_grad():
        got, gsc = td.sample_batched(tokens.clone(), top_p=0.95, kv=kv, constraints=c, return_scores=True, **kw)
        cfg = generation._gen_config(td)
        cfg.top_k, cfg.top_p = 0, 0.95
        want, wsc = generation.sample_batched_loop(cfg, generation.make_state_fn(td, kv), tokens.clone(), advance_fn=ops.sample_advance, constraints=c,
                                                   trie_fn=_host_mask("logits_trie_mask"), return_scores=True, score_fn=ops.sample_score, **kw)
    assert torch.equal(got, want) and torch.equal(gsc.token_logprob, wsc.token_logprob) and torch.equal(gsc.sum_logprob, wsc.sum_logprob)
    assert torch.isfinite(gsc.sum_logprob).all() and (gsc.sum_logprob <= 0).all()
    for r in range(got.shape[0]):
        _check_rows_are_phrases(got[r:r + 1], int(lengths[r // 4]), eod, trie)
        assert int(gsc.count[r]) == len(generation.generated_part(got[r], int(lengths[r // 4]), eod)) + 1


def test_inflight_loops_along_the_trie_equal_the_loops_with_the_host_mask(dev):
    from youku_mplug_amd import generation, ops
    m, model, video, ids, mask = _caption_model(dev)
    td, eod = model.text_decoder, m["eod_id"]
    qe, tokens = _inputs(dev, B=5, seed=31)
    ph, trie = _twelve(eod)
    c = generation.LogitsConstraints(allowed_phrases=trie)
    lens = [5, 2, 3, 1, 4]
    topk = lambda lg, k, add: ops.logprob_topk(lg, k, add=add)
    with torch.no_grad():
        got = td.beam_search_inflight(tokens.clone(), query_embeds=qe, beam_size=4, num_return_gen=3, stop_token=eod, prompt_length=lens, slots=2,
                                      refill_min=1, constraints=c)
        want = generation.beam_inflight_loop(generation._gen_config(td), generation.make_inflight_state_fn(td), tokens.clone(), query_embeds=qe,
                                             beam_size=4, num_return_gen=3, stop_token=eod, prompt_length=lens, slots=2, refill_min=1, constraints=c,
                                             topk_fn=topk, advance_fn=ops.beam_advance_steps, trie_fn=_host_mask("logits_trie_mask_steps"))
        assert max(got.advances) <= trie.max_len + 1 and got.steps == want.steps
        for i, (a, b) in enumerate(zip(got.results, want.results)):
            assert torch.equal(a.sequences, b.sequences) and torch.equal(a.scores, b.scores) and torch.equal(a.phrase_index, b.phrase_index)
            assert a.sequences.shape[0] == 3 and torch.isfinite(a.scores).all()
            _check_rows_are_phrases(a.sequences, lens[i], eod, trie, a.phrase_index)
        kw = dict(query_embeds=qe, prompt_length=lens, termination_id=eod, temperature=1.1, num_samples=3, seed=4, slots=2, refill_min=1)
        sg = td.sample_inflight(tokens.clone(), top_p=0.9, constraints=c, return_scores=True, **kw)
        cfg = generation._gen_config(td)
        cfg.top_k, cfg.top_p = 0, 0.9
        sw = generation.sample_inflight_loop(cfg, generation.make_inflight_state_fn(td), tokens.clone(), advance_fn=ops.sample_advance_steps,
                                             constraints=c, trie_fn=_host_mask("logits_trie_mask_steps"), return_scores=True,
                                             score_fn=ops.sample_score_steps, **kw)
    assert torch.equal(sg.tokens, sw.tokens) and sg.written == sw.written and torch.equal(sg.scores.sum_logprob, sw.scores.sum_logprob)
    assert all(w - pl <= trie.max_len + 1 for w, pl in zip(sg.written, lens))
    for r in range(sg.tokens.shape[0]):
        _check_rows_are_phrases(sg.tokens[r:r + 1], lens[r // 3], eod, trie)


def test_caption_generate_with_allowed_phrases_on_the_tiny_model(dev):
    from youku_mplug_amd.generation import generated_part
    m, model, video, ids, mask = _caption_model(dev)
    eod = m["eod_id"]
    ph, trie = _twelve(eod)
    sel = [0, 1, 0]
    text = types.SimpleNamespace(input_ids=ids[sel].to(dev), attention_mask=mask[sel].to(dev))
    n_prompt = int(mask[0].sum()) - 1
    res, info = model.generate(video[sel], text, termination_id=eod, batched=True, kv_cache="shared_prefix", allowed_phrases=ph, num_return_gen=3,
                               beam_size=4)
    assert len(res) == len(info) == 3
    for rows, inf in zip(res, info):
        assert rows.shape[0] == 3 and inf["phrase_index"].shape == (3,) and torch.isfinite(inf["scores"]).all()
        for row, idx in zip(rows.tolist(), inf["phrase_index"].tolist()):
            assert trie.lookup(generated_part(row, n_prompt, eod)) == idx >= 0
    assert torch.equal(res[0], res[2]) and torch.equal(info[0]["phrase_index"], info[2]["phrase_index"])
    smp, sc = model.generate(video[sel], text, termination_id=eod, do_sample=True, num_samples=3, seed=31, allowed_phrases=trie, return_scores=True)
    for rows, s in zip(smp, sc):
        assert s["phrase_index"].shape == (3,)
        for row, idx in zip(rows.tolist(), s["phrase_index"].tolist()):
            assert trie.lookup(generated_part(row, n_prompt, eod)) == idx >= 0
    with pytest.raises(ValueError, match="batched=True or do_sample=True"):
        model.generate(video[sel], text, termination_id=eod, allowed_phrases=ph)


def test_caption_entrypoint_allowed_phrases_flag_and_strings(tmp_path, dev, monkeypatch):
    """--eval_allowed_phrases on the synthetic loader: pred_caption is a phrase of the file, pred_candidates the best with their scores;
    model.generate(allowed_phrases=[strings]), tokenised with the model's tokenizer, equals the call with the entry point's trie"""
    import json
    import math
    import os
    from test_entrypoint_gpu import _finetune_entry, _write_finetune_config
    from youku_mplug_amd import downstream
    entry = _finetune_entry("run_caption_distributed_gpt3")
    cfg = _write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    ch = lambda *ks: "".join(chr(0x4E00 + k) for k in ks)
    phrases = [ch(3), ch(3, 4), ch(3, 4, 5), ch(9, 3), ch(20), ch(21, 22), ch(3, 4)]
    listing = tmp_path / "phrases.txt"
    listing.write_text("\n".join(phrases) + "\n", encoding="utf-8")
    gen = downstream.DistributedGPT3_Caption.generate
    seen = []

    def spy(self, image, text, *a, **kw):
        out = gen(self, image, text, *a, **kw)
        if getattr(self, "tokenizer", None) is not None and "allowed_phrases" in kw:
            seen.append((out, gen(self, image, text, *a, **dict(kw, allowed_phrases=phrases))))
        return out
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    out = str(tmp_path / "closed")
    args, config = entry.get_args(["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7",
                                   "--evaluate_only", "--eval_allowed_phrases", str(listing), "--eval_batched_beam", "--eval_shared_kv"])
    entry.main(args, config)
    result = json.load(open(os.path.join(out, "result", "val_caption_result.json")))
    assert result
    for rec in result:
        cands = rec["pred_candidates"]
        assert 1 <= len(cands) <= 5 and rec["pred_caption"] == cands[0]["caption"] and rec["pred_caption"] in phrases
        assert all(phrases[c["phrase_index"]] == c["caption"] and c["phrase_index"] != 6 and math.isfinite(c["score"]) for c in cands)
        assert [c["score"] for c in cands] == sorted((c["score"] for c in cands), reverse=True)
    assert seen, "the model of the entry point carries no tokenizer"
    for (res, info), (res2, info2) in seen:
        for a, b, ia, ib in zip(res, res2, info, info2):
            assert torch.equal(a, b) and torch.equal(ia["phrase_index"], ib["phrase_index"]) and torch.equal(ia["scores"], ib["scores"])
