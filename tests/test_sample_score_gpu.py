"""mpv_sample_score on the GPU: the kernel on every committed launch of tests/sample_score_cases.py -- the
log-probability within 2e-5 of the fp64 definition computed from the same bf16 logits; count, live, the running sum and every word it
must not touch bit for bit against tests/standin_sample_score.py, NaN canaries in the skipped cells and behind the table -- six chained
steps, its independence of the launch, its determinism and its refusals; then sample_batched with return_scores and
DistributedGPT3_Caption.generate(best_of=True) on the tiny model, in both KV modes and with constraints.

The gate 2e-5 is derived (|x| <= 64: log S <= 11.1; the fixed summation tree over at most 65536 terms and the hardware exp move log S by
about 1e-6; m + log S and x_t - lse round once each, half an ulp at a magnitude below 128 = 3.8e-6 each; under 1e-5 in all, times two);
the measured maximum is printed by every case and recorded in DESIGN.md section 19."""
import ctypes as C
import math
import os
import types

import pytest
import torch

import sample_score_cases as cases
import standin_sample_score as sq

pytestmark = pytest.mark.gpu
GATE = cases.GATE
WORST = {"lp": 0.0}


def _lp64(logits, V, tokens_at_pos):
    """the fp64 definition for every row at once, on the logits' device: log_softmax in float64; -inf where x_t is -inf"""
    x = logits[:, :V].double()
    t = tokens_at_pos.view(-1, 1)
    xt = x.gather(1, t)
    lp = torch.log_softmax(x, dim=1).gather(1, t)
    return torch.where(xt == float("-inf"), xt, lp).view(-1).cpu()


def _launch(dev, b, c):
    """one ops.sample_score launch of a built case -> (st, sc, table) on the device; checks that the inputs are left alone"""
    from youku_mplug_amd import ops
    st, sc_, table = cases.states(b, dev)
    logits = b.logits.to(dev)
    assert ops.sample_score(logits, st, sc_, pos=c["pos"], vocab=c["V"]) is sc_
    torch.cuda.synchronize()
    assert torch.equal(logits.cpu().view(torch.int16), b.logits.view(torch.int16)) and torch.equal(st.tokens.cpu(), b.tokens)
    assert torch.equal(st.done.cpu(), b.done) and torch.equal(st.prompt_len.cpu(), b.prompt_len)
    return st, sc_, table


@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_kernel_on_the_committed_launches(dev, c):
    b = cases.build(c)
    _, sc_, table = _launch(dev, b, c)
    ref_st, ref_sc, ref_table = cases.states(b)
    sq.sample_score(b.logits, ref_st, ref_sc, pos=c["pos"], vocab=c["V"])
    rows, L, pos = c["rows"], c["row_len"], c["pos"]
    scored = torch.tensor([cases.role_of(c, r) in ("live", "ends") for r in range(rows)])
    assert torch.equal(sc_.count.cpu(), ref_sc.count) and torch.equal(sc_.live.cpu(), ref_sc.live)
    cell = torch.zeros(rows * L + cases.TAIL, dtype=torch.bool)
    cell[torch.arange(rows)[scored] * L + pos] = True
    got_table = table.cpu()
    assert cases.same_bits(got_table[~cell], b.table[~cell]), "a cell of a skipped row, another column or the tail was written"
    lp = sc_.token_logprob.cpu()[:, pos]
    want = _lp64(b.logits.to(dev), c["V"], b.tokens[:, pos].to(dev))
    assert not torch.isnan(lp[scored]).any()
    inf = want == float("-inf")
    assert torch.equal(lp[scored & inf], want[scored & inf].float())         # -inf exactly where the chosen logit is -inf
    fin = scored & ~inf
    err = float((lp[fin].double() - want[fin]).abs().max()) if bool(fin.any()) else 0.0
    WORST["lp"] = max(WORST["lp"], err)
    print(f"    {cases.case_id(c)}: max |lp - lp64| = {err:.3e} over {int(fin.sum())} rows (so far {WORST['lp']:.3e}; gate {GATE:.0e})")
    assert err <= GATE, (cases.case_id(c), err)
    # the running sum: one fp32 add of the kernel's own entry; untouched where the row was skipped
    got_sum = sc_.sum_logprob.cpu()
    assert cases.same_bits(got_sum[~scored], b.sum_logprob[~scored]) and cases.same_bits(got_sum[scored], (b.sum_logprob + lp)[scored])


def test_six_chained_steps_sum_in_position_order(dev):
    """five rows with ragged prompts over columns 10 .. 15, fresh logits every step, two rows ending on the way: count, live and the
    untouched cells equal the stand-in's; sum_logprob is the sequential fp32 sum of the kernel's own entries in position order"""
    from youku_mplug_amd import ops
    V, ld, L, rows = 520, 528, 37, 5
    prompt = torch.tensor([10, 12, 11, 10, 14])
    ends_at = {0: 12, 3: 10}                                                 # row -> the column whose token terminates it
    g = torch.Generator().manual_seed(4)
    tokens = torch.randint(0, V, (rows, L), generator=g)
    mk = lambda device: (types.SimpleNamespace(rows=rows, row_len=L, tokens=tokens.clone().to(device), prompt_len=prompt.clone().to(device),
                                               done=torch.zeros(rows, dtype=torch.int32, device=device)),
                         types.SimpleNamespace(rows=rows, row_len=L, live=torch.ones(rows, dtype=torch.int32, device=device),
                                               token_logprob=torch.full((rows, L), float("nan"), device=device),
                                               sum_logprob=torch.zeros(rows, device=device), count=torch.zeros(rows, dtype=torch.int32, device=device)))
    (st, sc_), (rst, rsc) = mk(dev), mk("cpu")
    for pos in range(10, 16):
        logits = torch.full((rows, ld), float("nan"), dtype=torch.bfloat16)
        for r in range(rows):
            logits[r, :V] = cases.make_row(V, 1000 * pos + r, ("normal", "wide", "flat")[(pos + r) % 3])[0]
        for r, col in ends_at.items():
            if col == pos:
                st.done[r], rst.done[r] = 1, 1                               # what the sampler leaves when this column's token terminates
        ops.sample_score(logits.to(dev), st, sc_, pos=pos, vocab=V)
        sq.sample_score(logits, rst, rsc, pos=pos, vocab=V)
    torch.cuda.synchronize()
    tl = sc_.token_logprob.cpu()
    assert torch.equal(sc_.count.cpu(), rsc.count) and torch.equal(sc_.live.cpu(), rsc.live)
    assert sc_.count.tolist() == [3, 4, 5, 1, 2] and sc_.live.tolist() == [0, 1, 1, 0, 1]
    assert torch.equal(torch.isnan(tl), torch.isnan(rsc.token_logprob))       # the same cells written, all others still the canary
    assert ((tl - rsc.token_logprob)[~torch.isnan(tl)].abs() <= 2 * GATE).all()
    for r in range(rows):
        acc = torch.zeros((), dtype=torch.float32)
        for col in range(L):
            if not math.isnan(float(tl[r, col])):
                acc = acc + tl[r, col]
        assert float(acc) == float(sc_.sum_logprob[r]), (r, float(acc), float(sc_.sum_logprob[r]))


def test_a_rows_result_does_not_depend_on_its_place_or_on_the_launch(dev):
    c = next(c for c in cases.CASES if c["rows"] == 160 and c["V"] == 51200)
    b = cases.build(c)
    _, full, _ = _launch(dev, b, c)
    order = list(reversed(range(160)))
    flipped = types.SimpleNamespace(**{k: (getattr(b, k)[order].clone() if k != "table" else b.table.clone()) for k in vars(b)})
    _, back, _ = _launch(dev, flipped, c)
    lp_full, lp_back = full.token_logprob.cpu()[:, c["pos"]], back.token_logprob.cpu()[:, c["pos"]]
    assert cases.same_bits(lp_full, lp_back[order]) and torch.equal(full.count.cpu(), back.count.cpu()[order]) and torch.equal(full.live.cpu(), back.live.cpu()[order])
    assert cases.same_bits(full.sum_logprob.cpu(), back.sum_logprob.cpu()[order])
    checked = 0
    for r in range(160):
        if cases.role_of(c, r) not in ("live", "ends") or checked >= 7:
            continue
        one = types.SimpleNamespace(**{k: (getattr(b, k)[r:r + 1].clone() if k != "table" else b.table[:c["row_len"] + cases.TAIL].clone()) for k in vars(b)})
        _, alone, _ = _launch(dev, one, dict(c, rows=1))
        assert cases.same_bits(alone.token_logprob.cpu()[0, c["pos"]], lp_full[r]), r
        assert cases.same_bits(alone.sum_logprob.cpu(), full.sum_logprob.cpu()[r:r + 1]) and int(alone.live[0]) == int(full.live[r])
        checked += 1
    assert checked == 7


def test_the_same_launch_twice_gives_the_same_bits(dev):
    for c in (c for c in cases.CASES if c["seed"] in (51, 53)):
        b = cases.build(c)
        (_, a, ta), (_, a2, ta2) = _launch(dev, b, c), _launch(dev, b, c)
        assert cases.same_bits(ta, ta2) and cases.same_bits(a.sum_logprob, a2.sum_logprob) and torch.equal(a.count, a2.count) and torch.equal(a.live, a2.live)


def test_refusals_leave_every_output_untouched(dev):
    import test_sample_score_cpu as tc
    from youku_mplug_amd import _lib, generation, ops
    c = dict(V=64, ldx=8, rows=2, row_len=16, pos=5, seed=2)                 # the shapes of the descriptor of tests/test_sample_score_cpu.py
    b = cases.build(c)
    st, sc_, table = cases.states(b, dev)
    logits = b.logits.to(dev)
    ptr = dict(logits=logits.data_ptr(), tokens=st.tokens.data_ptr(), prompt_len=st.prompt_len.data_ptr(), done=st.done.data_ptr(), live=sc_.live.data_ptr(),
               token_logprob=sc_.token_logprob.data_ptr(), sum_logprob=sc_.sum_logprob.data_ptr(), count=sc_.count.data_ptr())
    outs = lambda: [t.clone() for t in (table, sc_.sum_logprob, sc_.count, sc_.live)]
    same = lambda a, b_: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b_))
    before = outs()
    stream = torch.cuda.current_stream().cuda_stream
    for over in tc.REFUSALS:
        fields = dict(ptr)
        fields.update({k: (None if v is None else ptr[k] + (v & 15)) if k in ptr else v for k, v in over.items()})
        rc = _lib.lib().mpv_sample_score(C.byref(tc._desc(**fields)), stream)
        torch.cuda.synchronize()
        assert rc < 0 and same(outs(), before), over
    assert _lib.lib().mpv_sample_score(C.byref(tc._desc(**ptr)), stream) == 0    # the accepted descriptor does write
    torch.cuda.synchronize()
    assert not same(outs(), before)
    # the wrapper's own checks
    good_st = generation.SampleState(b.tokens.to(dev), b.prompt_len.to(dev))
    for bad_logits, bad_sc in ((logits.float(), generation.SampleScores(2, 16, dev)), (logits, generation.SampleScores(3, 16, dev)),
                               (logits, generation.SampleScores(2, 8, dev)), (logits[:1], generation.SampleScores(2, 16, dev)),
                               (logits.cpu(), generation.SampleScores(2, 16, dev))):
        with pytest.raises(_lib.MpvError):
            ops.sample_score(bad_logits, good_st, bad_sc, pos=3)


# ------------------------------------------------------------------------------ on the tiny model
_MODEL = {}


def _caption_model(dev):
    if not _MODEL:
        import test_sampling_gpu as tg
        _MODEL["m"] = tg._caption_model(dev)
    return _MODEL["m"]


def _inputs(dev, B=3, Q=6, seed=8):
    from oracle.weights import CONFIG_TINY
    g = torch.Generator().manual_seed(seed)
    qe = (torch.randn(B, Q, CONFIG_TINY.hidden, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    return qe, torch.randint(0, CONFIG_TINY.vocab, (B, 5), generator=g).to(dev)


@pytest.mark.parametrize("constrained", [False, True], ids=["plain", "constrained"])
@pytest.mark.parametrize("kv", ["per_sequence", "shared_prefix"])
def test_sample_batched_scores_on_the_tiny_model(dev, kv, constrained):
    """the tokens of the plain call bit for bit; every scored entry within the gate of an fp64 recomputation from the logits cloned at
    every step of that same run -- behind the constraints' edit when they are on; scored are the columns in [prompt_len, termination]"""
    from youku_mplug_amd import generation, ops
    m, model, video, ids, mask = _caption_model(dev)
    td = model.text_decoder
    qe, tokens = _inputs(dev)
    lengths = torch.tensor([5, 2, 3], device=dev)
    N = 2
    c = generation.LogitsConstraints(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3, banned_token_ids=(17, 400)) if constrained else None
    for early in (True, False):
        kw = dict(query_embeds=qe, prompt_length=lengths.clone(), termination_id=m["eod_id"], temperature=1.2, num_samples=N, seed=9,
                  use_eod_token_for_early_termination=early)
        model.eval()
        captured = {}

        def advance(logits, st, **k):
            captured[k["pos"]] = logits.clone()                              # what the sampler reads: the constraints have edited it
            return ops.sample_advance(logits, st, **k)
        with torch.no_grad():
            plain = td.sample_batched(tokens.clone(), top_p=0.95, kv=kv, constraints=c, **kw)
            got, sc_ = td.sample_batched(tokens.clone(), top_p=0.95, kv=kv, constraints=c, return_scores=True, **kw)
            cfg = generation._gen_config(td)
            cfg.top_k, cfg.top_p = 0, 0.95
            again, sc2 = generation.sample_batched_loop(cfg, generation.make_state_fn(td, kv), tokens.clone(), advance_fn=advance, constraints=c,
                                                        constrain_fn=ops.logits_constrain, return_scores=True, score_fn=ops.sample_score, **kw)
        assert isinstance(plain, torch.Tensor) and torch.equal(got, plain) and torch.equal(again, plain)
        tl = sc_.token_logprob.cpu()
        assert tl.shape == got.shape and cases.same_bits(tl, sc2.token_logprob) and cases.same_bits(sc_.sum_logprob, sc2.sum_logprob)
        toks, R, Q = got.cpu(), got.shape[0], qe.shape[1]
        want_mask, lp64 = torch.zeros(tl.shape, dtype=torch.bool), torch.zeros(tl.shape, dtype=torch.float64)
        for r in range(R):
            for col in range(int(lengths[r // N]), toks.shape[1]):
                if col not in captured:
                    break                                                    # the columns the loop never reached (the slice is prefix-inclusive)
                want_mask[r, col] = True
                lp64[r, col] = sq.logprob_row_fp64(captured[col][r].cpu(), int(toks[r, col]))
                if int(toks[r, col]) == m["eod_id"]:
                    break
        assert torch.equal(sc_.count.cpu(), want_mask.sum(dim=1).to(torch.int32)) and (tl[~want_mask] == 0).all()
        err = float((tl.double() - lp64)[want_mask].abs().max())
        WORST["lp"] = max(WORST["lp"], err)
        print(f"    {kv} constrained={constrained} early={early}: max |lp - lp64| = {err:.3e} over {int(want_mask.sum())} entries (gate {GATE:.0e})")
        assert err <= GATE and torch.isfinite(tl).all() and (tl[want_mask] < 0).all()
        for r in range(R):
            acc = torch.zeros((), dtype=torch.float32)
            for col in want_mask[r].nonzero().view(-1).tolist():
                acc = acc + tl[r, col]
            assert float(acc) == float(sc_.sum_logprob[r]), r
        if constrained:                                                      # the captured logits are the edited ones: the banned ids are -inf
            pos0 = int(lengths.max())
            assert (captured[pos0][:, [17, 400]] == float("-inf")).all()


@pytest.mark.parametrize("kv", ["per_sequence", "shared_prefix"])
def test_caption_generate_best_of_returns_a_row_of_the_sampled_result(dev, kv):
    from youku_mplug_amd.downstream import best_sample
    m, model, video, ids, mask = _caption_model(dev)
    sel = [0, 1, 0]
    text = types.SimpleNamespace(input_ids=ids[sel].to(dev), attention_mask=mask[sel].to(dev))
    N, Lt = 4, ids.shape[1] + m["tokens_to_generate"]
    kw = dict(termination_id=m["eod_id"], do_sample=True, num_samples=N, seed=31, temperature=1.1, top_p=0.9, kv_cache=kv, no_repeat_ngram_size=2)
    plain = model.generate(video[sel], text, **kw)
    res, scores = model.generate(video[sel], text, return_scores=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(res, plain))
    for lp in (1.0, 0.0):
        best, bsc = model.generate(video[sel], text, best_of=True, return_scores=True, length_penalty=lp, **kw)
        for i in range(3):
            s = scores[i]
            assert s["token_logprob"].shape == (N, Lt) and s["sum_logprob"].shape == (N,) and s["count"].dtype == torch.int32 and not s["sum_logprob"].is_cuda
            b = best_sample(s["sum_logprob"], s["count"], lp)
            assert best[i].shape == (1, Lt) and torch.equal(best[i], res[i][b:b + 1]) and bsc[i]["index"] == b
            assert cases.same_bits(bsc[i]["sum_logprob"], s["sum_logprob"][b:b + 1]) and cases.same_bits(bsc[i]["token_logprob"], s["token_logprob"][b:b + 1])
    with pytest.raises(ValueError):
        model.generate(video[sel], text, termination_id=m["eod_id"], best_of=True)
