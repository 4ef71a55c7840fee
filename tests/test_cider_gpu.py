"""CIDEr on the GPU: ops.caption_cider (include/mpv.h: mpv_caption_cider) against tests/ref_cider.py on every case of
tests/cider_cases.py, element-wise on `pair` and `score`; a pair's bits alone and among others; the refusals; self-critical training
(DistributedGPT3_Caption.forward_scst) on the tiny synthetic caption model against fp32 autograd through the restated loss; the caption
entry point's corpus CIDEr against the recorded corpus mean of the reference project's scorer.  The model tests take the device as an
argument: tests/test_cider_cpu.py runs them on the stand-ins."""
import json
import math
import os
import types

import pytest
import torch

import cider_cases as cc
import ref_cider as rc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF = torch.bfloat16


def close(x, ref):
    """the kernel gate: |x - ref| <= 1e-12 |ref| + 1e-15.  Reordering an fp64 sum of at most 255 non-negative terms costs at most
    255 * 2^-53 = 3e-14 relative, the sqrt, divide and exp a few ulp: the gate sits 30x above that and 1e4 below any real defect."""
    return math.isfinite(x) and abs(x - ref) <= 1e-12 * abs(ref) + 1e-15


def stats_of(case):
    from youku_mplug_amd import generation
    return generation.CiderStats(case["corpus"], case["vocab"], capacity=case["capacity"])


def call(fn, case, dev, stats=None, **over):
    c = dict(case, **over)
    return fn(c["tok_a"].to(dev)[:, :c["width_a"]], c["start_a"], c["begin_a"], c["tok_b"].to(dev)[:, :c["width_b"]], c["start_b"], c["begin_b"],
              term=c["term"], stats=stats if stats is not None else stats_of(case))


def check_case(fn, case, dev):
    """fn (ops.caption_cider or its stand-in) on a case against the reference, element-wise, twice -> (pair, score) on the CPU"""
    want_pair, want_score = rc.case_values(case)
    first, second = call(fn, case, dev), call(fn, case, dev)
    for pair, score in (first, second):
        assert pair.dtype == score.dtype == torch.float64 and pair.shape == (len(want_pair), 4) and score.shape == (len(want_score),)
        bad = [(p, n, g, w) for p, (gs, ws) in enumerate(zip(pair.tolist(), want_pair)) for n, (g, w) in enumerate(zip(gs, ws)) if not close(g, w)]
        assert not bad, bad[:5]
        bad = [(r, g, w) for r, (g, w) in enumerate(zip(score.tolist(), want_score)) if not close(g, w)]
        assert not bad, bad[:5]
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    return first[0].cpu(), first[1].cpu()


@pytest.mark.parametrize("case", cc.CASES, ids=cc.NAMES)
def test_kernel_equals_the_reference_on_every_value_twice(dev, case):
    from youku_mplug_amd import ops
    pair, score = check_case(ops.caption_cider, case, dev)
    torch.cuda.synchronize()
    if case["name"] == "one_clip":
        assert (pair == 0).all() and (score == 0).all()
    if case["name"] == "long":                                     # 255 tokens against 3: exp(-252^2 / 72) underflows to 0
        assert (pair[1] == 0).all() and pair[0].max() > 0


def alone_and_among_others(fn, dev):
    """every group of the `edges` and `long` cases run ALONE gives the bits its pairs and scores have in the whole call"""
    for case in (cc.CASES[0], cc.CASES[2]):
        stats = stats_of(case)
        pair, score = call(fn, case, dev, stats)
        pair, score, at = pair.cpu(), score.cpu(), 0
        for g in range(len(case["begin_a"]) - 1):
            a0, a1, b0, b1 = case["begin_a"][g], case["begin_a"][g + 1], case["begin_b"][g], case["begin_b"][g + 1]
            one = dict(tok_a=case["tok_a"][a0:a1], start_a=case["start_a"][a0:a1], begin_a=[0, a1 - a0], tok_b=case["tok_b"][b0:b1],
                       start_b=case["start_b"][b0:b1], begin_b=[0, b1 - b0])
            p1, s1 = call(fn, case, dev, stats, **one)
            n = (a1 - a0) * (b1 - b0)
            assert torch.equal(p1.cpu(), pair[at:at + n]) and torch.equal(s1.cpu(), score[a0:a1]), (case["name"], g)
            at += n
        assert at == pair.shape[0]


def test_a_pair_is_bit_identical_alone_and_among_others(dev):
    from youku_mplug_amd import ops
    alone_and_among_others(ops.caption_cider, dev)


def test_wrapper_and_library_refuse_without_launching(dev):
    """256 tokens: ValueError from the wrapper before any launch; the library's negative codes leave the outputs' bits"""
    import ctypes
    from youku_mplug_amd import _lib, ops
    case = cc.CASES[0]
    stats = stats_of(case)
    ta, sa, ba, tb, sb, bb = cc.refused_table()
    with pytest.raises(ValueError, match="256"):
        ops.caption_cider(ta.to(dev), sa, ba, tb.to(dev), sb, bb, term=cc.TERM, stats=stats)
    with pytest.raises(_lib.MpvError, match="uint64"):
        ops.caption_cider(ta[:, :8].to(dev), [0] * 3, ba, tb.to(dev), sb, bb, term=cc.TERM, stats=(stats.idf.to(dev), stats.idf.to(dev), 0.0))
    keys, idf, log_ref_len = stats.arrays(dev)
    tok_a, tok_b = case["tok_a"].to(dev), case["tok_b"].to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    na, nb = torch.tensor(case["begin_a"]).diff(), torch.tensor(case["begin_b"]).diff()
    host = dict(start_a=i32(case["start_a"]), start_b=i32(case["start_b"]), begin_a=i32(case["begin_a"]), begin_b=i32(case["begin_b"]),
                pair_begin=torch.cat([torch.zeros(1, dtype=torch.int64), (na * nb).cumsum(0)]))
    devs = {k: v.to(dev) for k, v in host.items()}
    pairs = int(host["pair_begin"][-1])
    pair = torch.full((pairs, 4), -7.0, dtype=torch.float64, device=dev)
    score = torch.full((tok_a.shape[0],), -7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=dev)

    def run(ws_bytes=None, **over):
        h = dict(host, **{k: v for k, v in over.items() if k in host})
        d = _lib.CaptionCiderDesc()
        d.tok_a, d.tok_b, d.pair, d.score, d.table_keys, d.table_idf = (t.data_ptr() for t in (tok_a, tok_b, pair, score, keys, idf))
        for k in host:
            setattr(d, k, devs[k].data_ptr())
            setattr(d, "host_" + k, h[k].data_ptr())
        d.ld_a, d.ld_b, d.term, d.table_capacity, d.log_ref_len, d.sigma = tok_a.stride(0), tok_b.stride(0), case["term"], keys.numel(), log_ref_len, 6.0
        d.rows_a, d.rows_b, d.width_a, d.width_b, d.groups = tok_a.shape[0], tok_b.shape[0], case["width_a"], case["width_b"], len(case["begin_a"]) - 1
        for k, v in over.items():
            if k not in host:
                setattr(d, k, v)
        need = _lib.lib().mpv_caption_cider_workspace_size(ctypes.byref(d))
        assert 0 < need <= ws.numel()
        rc_ = _lib.lib().mpv_caption_cider(ctypes.byref(d), ws.data_ptr(), need if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc_
    bad_begin = list(case["begin_a"])
    bad_begin[2] = bad_begin[1] - 1
    for over in (dict(begin_a=i32(bad_begin)), dict(start_a=i32([case["width_a"] + 1] + case["start_a"][1:])), dict(start_b=i32([-1] + case["start_b"][1:])),
                 dict(pair_begin=host["pair_begin"] + 1), dict(pair=None), dict(score=None), dict(table_keys=None), dict(table_idf=None),
                 dict(table_capacity=keys.numel() - 1), dict(table_capacity=0), dict(log_ref_len=float("nan")), dict(log_ref_len=-1.0),
                 dict(sigma=0.0), dict(sigma=float("inf")), dict(groups=0), dict(ld_b=case["width_b"] - 1), dict(ws_bytes=64)):
        assert run(**over) < 0, over
        assert b"mpv_caption_cider" in _lib.lib().mpv_last_error()
        assert (pair == -7).all() and (score == -7).all(), over
    assert run() == 0
    want_pair, want_score = rc.case_values(case)
    assert all(close(g, w) for gs, ws_ in zip(pair.tolist(), want_pair) for g, w in zip(gs, ws_))
    assert all(close(g, w) for g, w in zip(score.tolist(), want_score))


# ------------------------------------------------------------------------------------------------ self-critical training on the tiny model
B, N, PL, GEN = 2, 3, 3, 6


def scst_setup(dev):
    """the tiny caption model of the model tests with dropout off, 2 clips with prompts of 3 tokens, rows of 3 + 6 columns; rollouts
    [B * N, 9] whose samples end after 6 (no terminator), 1, 2, 4, 0 and 3 tokens; references that share n-grams with some of them"""
    import test_decode_ragged_cpu as tdr
    from youku_mplug_amd import generation
    model, cfg, term, video, text = tdr._setup(dev, lengths=[PL] * B, width=PL + 2, tokens_to_generate=GEN)
    model.text_decoder.config.hidden_dropout = model.text_decoder.config.attention_dropout = 0.0
    g = torch.Generator().manual_seed(4242)
    lens = [6, 1, 2, 4, 0, 3]
    table = torch.full((B * N, PL + GEN), term, dtype=torch.int64)
    table[:, :PL] = text.input_ids.cpu().repeat_interleave(N, dim=0)[:, :PL]
    for r, n in enumerate(lens):
        t = torch.randint(8, cfg.vocab, (n,), generator=g)
        t[t == term] = term + 1
        table[r, PL:PL + n] = t
    gen = [table[r, PL:PL + n].tolist() for r, n in enumerate(lens)]
    refs = [[gen[0][:4] + [9, 10], gen[0][2:] + [11]], [gen[3] + [12], [13, 14] + gen[5][:2]]]
    stats = generation.CiderStats(refs, cfg.vocab)
    return model, cfg, term, video.to(dev), text, table, gen, refs, stats


def restated(dev, model, cfg, video, table, gen, refs, term, baseline="mean_others", greedy=None):
    """the rewards by tests/ref_cider.py, the weights on the host in fp64, the loss by fp32 autograd on oracle.restate with the model's
    (bf16-rounded) weights -> (loss, d visual_fc.weight, d visual_fc.bias, d query_features [B, Q, H], rewards)"""
    df, log_ref_len = rc.doc_freq(refs)
    rewards = [[rc.score_of([rc.pair_values(gen[b * N + s], r, df, log_ref_len) for r in refs[b]]) for s in range(N)] for b in range(B)]
    w, T = rc.scst_weights(table.tolist(), rewards, PL, term, baseline, greedy)
    sd = {k: v.detach().float().to(dev) for k, v in model.state_dict().items()}
    for k in ("visual_fc.weight", "visual_fc.bias"):
        sd[k].requires_grad_(True)
    loss, qf = rc.scst_loss(video.float(), None, table.to(dev), torch.tensor(w, dtype=torch.float32, device=dev), sd, cfg)
    loss.backward()
    return loss.item(), sd["visual_fc.weight"].grad, sd["visual_fc.bias"].grad, qf.grad, rewards


def scst_loss_and_gradients(dev):
    """forward_scst with GIVEN rollouts: loss, d visual_fc and d query_features against fp32 autograd through the restatement, under the
    ITM model's gates of tests/test_model_gpu.py (PLAIN["itm_tiny"]: loss, norm, wide: the pipeline and the fold are the same)"""
    import test_model_gpu as tm
    model, cfg, term, video, text, table, gen, refs, stats = scst_setup(dev)
    seen = []
    plain = model.text_decoder.backward_lm

    def spy(*a, **k):
        out = plain(*a, **k)
        seen.append(out)
        return out
    model.text_decoder.backward_lm = spy
    try:
        model.zero_grad(set_to_none=True)
        loss, stats_out = model.forward_scst(video, text, refs, cider=stats, num_samples=N, rollouts=table.to(dev), termination_id=term)
        loss.backward()
    finally:
        del model.text_decoder.backward_lm
    want, gw, gb, gq, rewards = restated(dev, model, cfg, video, table, gen, refs, term)
    flat = [x for row in rewards for x in row]
    assert abs(stats_out["reward"] - sum(flat) / len(flat)) <= 1e-6 and abs(stats_out["baseline"] - sum(flat) / len(flat)) <= 1e-6
    assert abs(stats_out["length"] - 16 / 6) <= 1e-6 and abs(stats_out["terminated"] - 5 / 6) <= 1e-6
    assert max(flat) > 0.5 and min(flat) == 0.0, flat                              # the rewards do differ
    tm.plain_gate("itm_tiny", "loss", abs(loss.item() - want) / abs(want), where=f"scst loss {loss.item():.6f} vs {want:.6f}")
    Q, H = model.num_learnable_token, model.text_width
    dq = seen[0].float().view(N, B, Q, H).sum(dim=0)                               # sequence s * B + b, folded onto clip b
    for name, mine, ref in (("visual_fc.weight", model.visual_fc.weight.grad, gw), ("visual_fc.bias", model.visual_fc.bias.grad, gb),
                            ("query_features", dq, gq)):
        mine, ref = mine.float().reshape(-1), ref.float().reshape(-1)
        tm.plain_gate("itm_tiny", "norm", abs(mine.norm().item() - ref.norm().item()) / ref.norm().item(), where=name)
        tm.plain_gate("itm_tiny", "wide", ((mine - ref).norm() / ref.norm()).item(), where=name)
    # the greedy baseline: the same samples against the reward of one top_k = 1 caption per clip
    loss_g, st_g = model.forward_scst(video, text, refs, cider=stats, num_samples=N, baseline="greedy", rollouts=table.to(dev), termination_id=term)
    assert math.isfinite(loss_g.item()) and abs(st_g["reward"] - stats_out["reward"]) <= 1e-6 and st_g["baseline"] >= 0.0


def scst_identical_samples_give_zero(dev):
    """top_k = 1: every clip's samples are identical, so every advantage, the loss and every gradient are EXACTLY zero"""
    model, cfg, term, video, text, table, gen, refs, stats = scst_setup(dev)
    model.zero_grad(set_to_none=True)
    loss, st = model.forward_scst(video, text, refs, cider=stats, num_samples=4, top_k=1, seed=3, termination_id=term)
    loss.backward()
    assert loss.item() == 0.0 and abs(st["reward"] - st["baseline"]) == 0.0
    grads = [p.grad for p in model.parameters() if p.requires_grad and p.grad is not None]
    assert grads and all((g == 0).all() for g in grads)


def scst_same_seed_same_bits(dev):
    """two calls with one seed: bit-identical rollouts and loss; another seed: other rollouts.  The default seed follows step_seed"""
    model, cfg, term, video, text, table, gen, refs, stats = scst_setup(dev)
    seen = []
    plain = model.text_decoder.sample_batched

    def spy(*a, **k):
        out = plain(*a, **k)
        seen.append((k.get("seed"), out.clone()))
        return out
    model.text_decoder.sample_batched = spy
    try:
        kw = dict(cider=stats, num_samples=N, top_k=8, termination_id=term)
        with torch.no_grad():
            l1, s1 = model.forward_scst(video, text, refs, seed=11, **kw)
            l2, s2 = model.forward_scst(video, text, refs, seed=11, **kw)
            l3, s3 = model.forward_scst(video, text, refs, seed=12, **kw)
            model.text_decoder.step_seed = 5
            model.forward_scst(video, text, refs, **kw)
            model.forward_scst(video, text, refs, **kw)
            model.text_decoder.step_seed = 6
            model.forward_scst(video, text, refs, **kw)
    finally:
        del model.text_decoder.sample_batched
        model.text_decoder.step_seed = 0
    assert torch.equal(seen[0][1], seen[1][1]) and torch.equal(l1, l2) and s1 == s2
    assert not torch.equal(seen[0][1], seen[2][1])
    assert seen[3][0] == seen[4][0] != seen[5][0] and torch.equal(seen[3][1], seen[4][1])


def test_scst_loss_and_gradients_against_fp32_autograd(dev):
    scst_loss_and_gradients(dev)


def test_scst_identical_samples_give_exactly_zero(dev):
    scst_identical_samples_give_zero(dev)


def test_scst_same_seed_gives_the_same_rollouts_and_loss(dev):
    scst_same_seed_same_bits(dev)


# ------------------------------------------------------------------------------------------------ the evaluation metric
def corpus_cider_equals_the_golden(dev):
    import test_entrypoint_gpu as t
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    gold = json.load(open(os.path.join(GOLD, "cider_reference.json")))["eval"]
    units = lambda cap: [chr(0x4e00 + t) for t in cap]                              # any hashable units: CJK characters here
    got = entry.corpus_cider([(units(h), [units(r) for r in refs]) for h, refs in zip(gold["hypotheses"], gold["references"])], dev)
    print(f"    corpus CIDEr {got!r} (recorded {gold['mean']!r})")
    assert close(got, gold["mean"])


def test_entry_point_corpus_cider_equals_the_recorded_mean(dev):
    corpus_cider_equals_the_golden(dev)
