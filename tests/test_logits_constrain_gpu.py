"""mpv_logits_constrain on the GPU: the kernel against tests/standin_constrain.py on every committed case of
tests/constrain_cases.py -- bitwise on the whole [rows, ld] matrix, poison in the columns behind the vocabulary and a canary behind the
matrix -- its independence of the launch, its determinism and its refusals; the finite ban value through mpv_logprob_topk; and both
lockstep loops, the shared-prefix cache and DistributedGPT3_Caption.generate with constraints on the tiny model.  The stand-in runs on
the CPU (its divide is the IEEE one there) and its result is copied back."""
import ctypes as C
import os
import types

import pytest
import torch

import constrain_cases as cc
import sampling_cases as sc
import standin_constrain as sk

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY = 64
MARK = -7.5


def _Cn(**kw):
    from youku_mplug_amd.generation import LogitsConstraints
    return LogitsConstraints(**kw)


def _guarded(logits, dev):
    """-> (the device copy of logits, the buffer it lives in: CANARY marked elements follow the matrix)"""
    buf = torch.full((logits.numel() + CANARY,), MARK, dtype=torch.bfloat16, device=dev)
    view = buf[:logits.numel()].view(logits.shape)
    view.copy_(logits)
    return view, buf


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _launch(dev, logits, tokens, kw, ckw, V):
    """-> (what the kernel leaves, what the stand-in leaves), both on the CPU"""
    from youku_mplug_amd import ops
    view, buf = _guarded(logits, dev)
    tok_dev = tokens.to(dev)
    dkw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
    out = ops.logits_constrain(view, tok_dev, constraints=_Cn(**ckw), vocab=V, **dkw)
    torch.cuda.synchronize()
    assert out is view and bool((buf[logits.numel():] == MARK).all()), "the canary behind the logits was overwritten"
    assert torch.equal(tok_dev.cpu(), tokens)
    want = sk.logits_constrain(logits.clone(), tokens, constraints=_Cn(**ckw), vocab=V, **kw)
    return view.cpu(), want


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_kernel_equals_the_standin_bitwise(dev, case):
    logits, tokens, kw, ckw = cc.build(case)
    V = case["V"]
    got, want = _launch(dev, logits, tokens, kw, ckw, V)
    assert (got[:, V:] == sc.POISON).all(), "a column behind the vocabulary was written"
    diff = (_bits(got) != _bits(want)).nonzero()
    assert diff.numel() == 0, (cc.case_id(case), diff[:8].tolist(), [(float(got[r, c]), float(want[r, c]), float(logits[r, c])) for r, c in diff[:8].tolist()])


def test_a_rows_result_does_not_depend_on_its_place_or_on_the_launch(dev):
    case = next(c for c in cc.CASES if c["V"] == 64 and c["rows"] == 3 and c["m"] == 256)
    logits, tokens, kw, ckw = cc.build(case)
    alone = {}
    for r in range(3):
        k1 = dict(kw, prompt_len=kw["prompt_len"][r:r + 1])
        alone[r], want = _launch(dev, logits[r:r + 1].clone(), tokens[r:r + 1].clone(), k1, ckw, 64)
        assert torch.equal(_bits(alone[r]), _bits(want))
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        ko = dict(kw, prompt_len=kw["prompt_len"][order])
        got, _ = _launch(dev, logits[order].clone(), tokens[order].clone(), ko, ckw, 64)
        for place, r in enumerate(order):
            assert torch.equal(_bits(got[place]), _bits(alone[r][0])), (order, place)


def test_the_same_launch_twice_gives_the_same_bits(dev):
    for case in (c for c in cc.CASES if c["seed"] in (133, 136, 137)):
        logits, tokens, kw, ckw = cc.build(case)
        a, _ = _launch(dev, logits, tokens, kw, ckw, case["V"])
        b, _ = _launch(dev, logits, tokens, kw, ckw, case["V"])
        assert torch.equal(_bits(a), _bits(b)), cc.case_id(case)


def test_refusals_leave_the_logits_untouched(dev):
    import test_logits_constrain_cpu as tc
    from youku_mplug_amd import _lib, ops
    logits = torch.full((2, 72), sc.POISON, dtype=torch.bfloat16)
    logits[:, :64] = torch.stack([sc.make_row(64, 5 + r, "normal") for r in range(2)])
    view, buf = _guarded(logits, dev)
    before = buf.clone()
    tokens = torch.randint(0, 64, (2, 16), device=dev)
    real = dict(logits=view.data_ptr(), tokens=tokens.data_ptr(), prompt_len=torch.zeros(2, dtype=torch.int64, device=dev),
                eos_ids=torch.tensor([5], device=dev), banned_ids=torch.tensor([9, 11], device=dev))
    ptr = {k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in real.items()}
    stream = torch.cuda.current_stream().cuda_stream
    for over in tc.REFUSALS:
        fields = dict(ptr)
        fields.update({k: (None if v is None else ptr[k] + (v & 15)) if k in ptr else v for k, v in over.items()})
        rc = _lib.lib().mpv_logits_constrain(C.byref(tc._desc(**fields)), stream)
        torch.cuda.synchronize()
        assert rc < 0 and torch.equal(_bits(buf), _bits(before)), over
    # the accepted descriptor does edit, and everything off does not
    assert _lib.lib().mpv_logits_constrain(C.byref(tc._desc(**ptr, penalty=1.0, ngram=0, n_banned=0, min_new_tokens=0)), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(before))
    assert _lib.lib().mpv_logits_constrain(C.byref(tc._desc(**ptr)), stream) == 0
    torch.cuda.synchronize()
    assert not torch.equal(_bits(buf), _bits(before))
    # the wrapper's own checks
    for bad_logits, bad_tokens in ((view.float(), tokens), (view, tokens.int()), (view, tokens[:1]), (view.cpu(), tokens.cpu())):
        with pytest.raises(_lib.MpvError):
            ops.logits_constrain(bad_logits, bad_tokens, pos=3, constraints=_Cn(no_repeat_ngram_size=1))


def test_a_slice_banned_with_the_finite_value_goes_through_logprob_topk(dev):
    """vocab 64: a slice of mpv_logprob_topk's first kernel is two columns.  Columns 10 and 11 (and the whole history) banned with the
    lowest finite bf16: every candidate value is finite and equals logprob_topk of the stand-in's matrix; the banned columns are not
    among the candidates."""
    from youku_mplug_amd import ops
    rows, V, K2 = 3, 64, 8
    logits = torch.stack([sc.make_row(V, 700 + r, "normal") for r in range(rows)])
    tokens = torch.tensor([[3, 20, 21, 20, 0, 0], [3, 30, 31, 32, 0, 0], [3, 12, 13, 12, 0, 0]])
    c = _Cn(banned_token_ids=(10, 11), no_repeat_ngram_size=1, min_new_tokens=9)
    kw = dict(pos=4, prompt_len_all=1, eos_ids=[40], ban_value=cc.BAN_FINITE)
    got = ops.logits_constrain(logits.to(dev), tokens.to(dev), constraints=c, **kw)
    want = sk.logits_constrain(logits.clone(), tokens, constraints=c, **kw)
    assert torch.equal(_bits(got), _bits(want)) and (want[:, [10, 11, 40]] == cc.BAN_FINITE).all() and torch.isfinite(want).all()
    add = torch.tensor([0.0, -1.5, -3.0], device=dev)
    val, idx = ops.logprob_topk(got, K2, add=add)
    ref_val, ref_idx = ops.logprob_topk(want.to(dev), K2, add=add)
    assert torch.isfinite(val).all() and torch.equal(val, ref_val) and torch.equal(idx, ref_idx)
    banned = [{10, 11, 40} | set(tokens[r, 1:4].tolist()) for r in range(rows)]
    assert all(not (set(idx[r].tolist()) & banned[r]) for r in range(rows))
    lp = torch.log_softmax(torch.where(want == cc.BAN_FINITE, torch.tensor(float("-inf")), want.float()), dim=-1) + add.cpu()[:, None]
    # the banned entries count as probability zero: fp32 log-sum-exp of 64 terms with the hardware exp / log (a few ulp of values below
    # 32 in magnitude, i.e. a few 1e-6) against torch's
    assert torch.allclose(val.cpu(), lp.gather(1, idx.cpu()), atol=1e-4, rtol=0)


# ------------------------------------------------------------------------------ on the tiny model
_MODEL = {}


def _caption_model(dev):
    if not _MODEL:
        import test_sampling_gpu as tg
        _MODEL["m"] = tg._caption_model(dev)
    return _MODEL["m"]


def _standin_fn(logits, tokens, **kw):
    host = logits.cpu()
    sk.logits_constrain(host, tokens.cpu(), **{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in kw.items()})
    logits.copy_(host)
    return logits


def _repeats(seq, n):
    grams = [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
    return len(grams) != len(set(grams))


def _inputs(dev, B=3, Q=6, seed=8):
    from oracle.weights import CONFIG_TINY
    g = torch.Generator().manual_seed(seed)
    qe = (torch.randn(B, Q, CONFIG_TINY.hidden, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    return qe, torch.randint(0, CONFIG_TINY.vocab, (B, 5), generator=g).to(dev)


@pytest.mark.parametrize("kv", ["per_sequence", "shared_prefix"])
def test_sample_batched_with_constraints_equals_the_loop_on_the_standin(dev, kv):
    from youku_mplug_amd import generation, ops
    m, model, video, ids, mask = _caption_model(dev)
    td = model.text_decoder
    qe, tokens = _inputs(dev)
    lengths = torch.tensor([5, 2, 3], device=dev)
    c = _Cn(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3, banned_token_ids=(17, 400))
    kw = dict(query_embeds=qe, prompt_length=lengths.clone(), termination_id=m["eod_id"], temperature=1.2, num_samples=2, seed=9,
              use_eod_token_for_early_termination=False)
    model.eval()
    with torch.no_grad():
        got = td.sample_batched(tokens.clone(), top_p=0.95, kv=kv, constraints=c, **kw)
        cfg = generation._gen_config(td)
        cfg.top_k, cfg.top_p = 0, 0.95
        want = generation.sample_batched_loop(cfg, generation.make_state_fn(td, kv), tokens.clone(), advance_fn=ops.sample_advance, constraints=c,
                                              constrain_fn=_standin_fn, **kw)
        plain = td.sample_batched(tokens.clone(), top_p=0.95, kv=kv, **kw)
        if kv == "per_sequence":                                            # clip 1 alone, with its streams
            alone = td.sample_batched(tokens[1:2].clone(), top_p=0.95, kv=kv, constraints=c, **dict(kw, query_embeds=qe[1:2], streams=torch.tensor([2, 3]),
                                                                                                 prompt_length=lengths[1:2].clone()))
        else:                                                               # the shared-prefix step is bit-stable at an equal row count only (as
            qo, to = _inputs(dev, seed=77)                                  # tests/test_decode_shared_gpu.py states it): clip 1 between other clips
            qo[1], to[1] = qe[1], tokens[1]
            alone = td.sample_batched(to, top_p=0.95, kv=kv, constraints=c, **dict(kw, query_embeds=qo))[2:4]
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert not torch.equal(got, plain)
    Q = qe.shape[1]
    n_cols = got.shape[1] - Q                                               # the slice is prefix-inclusive (sic): the last Q columns are padding
    for r, row in enumerate(got.tolist()):
        pl = int(lengths[r // 2])
        gen = row[pl:n_cols]
        assert not _repeats(gen, 2), (r, gen)
        assert m["eod_id"] not in gen[:3] and 17 not in gen and 400 not in gen, (r, gen)
    assert torch.equal(alone[:, :n_cols], got[2:4, :n_cols])                 # the same rows whatever the other clips are


@pytest.mark.parametrize("kv", ["per_sequence", "shared_prefix"])
def test_beam_search_batched_with_constraints_equals_the_loop_on_the_standin(dev, kv):
    from youku_mplug_amd import generation, ops
    m, model, video, ids, mask = _caption_model(dev)
    td = model.text_decoder
    qe, tokens = _inputs(dev, seed=12)
    P, K = 4, 4
    c = _Cn(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=3)
    kw = dict(query_embeds=qe, beam_size=K, num_return_gen=3, stop_token=m["eod_id"], prompt_length=P)
    model.eval()
    with torch.no_grad():
        got = td.beam_search_batched(tokens.clone(), kv=kv, constraints=c, **kw)
        want = generation.beam_search_batched_loop(generation._gen_config(td), generation.make_state_fn(td, kv), tokens.clone(),
                                                   topk_fn=lambda lg, k, add: ops.logprob_topk(lg, k, add=add), advance_fn=ops.beam_advance,
                                                   constraints=c, constrain_fn=_standin_fn, **kw)
        plain = td.beam_search_batched(tokens.clone(), kv=kv, **kw)
        # clip 2 next to other clips, at the same row count: a search of one clip runs the decoder's GEMMs at another row count, through
        # another dispatch, and its fp32 scores differ in the fourth digit with or without constraints (tests/test_beam_batched_gpu.py
        # compares at an equal row count for the same reason)
        qo, to = _inputs(dev, seed=78)
        qo[2], to[2] = qe[2], tokens[2]
        alone = td.beam_search_batched(to, kv=kv, constraints=c, **dict(kw, query_embeds=qo))[2]
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert torch.equal(a.sequences, b.sequences) and torch.equal(a.scores, b.scores) and torch.isfinite(a.scores).all()
    assert any(not torch.equal(a.sequences, b.sequences) for a, b in zip(got, plain))
    for o in got:
        for seq in o.sequences.tolist():
            gen = seq[P:]
            end = gen.index(m["eod_id"]) + 1 if m["eod_id"] in gen else len(gen)
            assert end > 3 or m["eod_id"] not in gen, seq
            assert not _repeats(gen[:end], 2), seq
    assert torch.equal(alone.sequences, got[2].sequences) and torch.equal(alone.scores, got[2].scores)


def test_caption_generate_with_constraints_on_the_tiny_model(dev):
    m, model, video, ids, mask = _caption_model(dev)
    sel = [0, 1, 0]
    text = types.SimpleNamespace(input_ids=ids[sel].to(dev), attention_mask=mask[sel].to(dev))
    n_prompt = int(mask[0].sum()) - 1
    kw = dict(termination_id=m["eod_id"], no_repeat_ngram_size=2, min_new_tokens=2)
    smp = model.generate(video[sel], text, do_sample=True, num_samples=3, seed=31, temperature=1.0, top_p=0.9, **kw)
    beam = model.generate(video[sel], text, batched=True, kv_cache="shared_prefix", **kw)
    assert len(smp) == len(beam) == 3 and all(r.shape[0] == 3 for r in smp)
    for rows in list(smp) + list(beam):
        for row in rows.tolist():
            gen = row[n_prompt:]
            end = gen.index(m["eod_id"]) + 1 if m["eod_id"] in gen else len(gen)
            assert end > 2 or m["eod_id"] not in gen, row                   # not empty: no termination token in the first two columns
            assert not _repeats(gen[:end], 2), row                          # no bigram twice
    with pytest.raises(ValueError):
        model.generate(video[sel], text, termination_id=m["eod_id"], no_repeat_ngram_size=2)
