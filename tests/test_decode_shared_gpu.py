"""Decode against a per-clip shared prefix KV cache, on the GPU: mpv_attn_decode_shared_fwd (csrc/decode_shared_attention.hip)
against the fp32 torch softmax over the concatenated keys (tests/standin_decode_shared.py, proven against fp64 in
tests/test_decode_shared_cpu.py), that it never reads the suffix rows beyond own_len, that a group's output depends on that group
alone, its refusals; generation.SharedPrefixDecodeState against DecodeState on the tiny model; DistributedGPT3_Caption.generate(
kv_cache="shared_prefix") for the lockstep beam search and for sampling."""
import types

import pytest
import torch

import standin_decode_shared as sd
from test_kernels_gpu import close, rel_err

pytestmark = pytest.mark.gpu


def _run(c):
    from youku_mplug_amd import ops
    lay = ops.AttnLayout(c["lay"].q, c["lay"].k, c["lay"].v, c["lay"].o)
    sd.run_case(ops.attn_decode_shared_fwd, {**c, "lay": lay})
    return c["o"]


def _ref(c):
    return sd.attn_decode_shared_ref(*[c[n] for n in ("q", "k", "v", "pk", "pv", "lay", "prefix_lay", "n_seq", "group_size", "heads",
                                                      "prefix_len", "own_len", "hd", "scale")])


@pytest.mark.parametrize("case", sd.SWEEP, ids=lambda c: "-".join(map(str, c)))
def test_kernel_matches_the_fp32_softmax_over_the_concatenated_keys(dev, case):
    """1e-2 in max-abs error over max-abs reference: the gate of test_attention_decode_step (bf16 output, bf16 probabilities)"""
    c = sd.make_case(*case, seed=3, device=dev)
    want = _ref(c)
    got = _run(c).view(c["n_seq"], c["heads"], c["hd"])
    print(f"    {case}: max-abs error / max-abs ref = {rel_err(got, want):.3e}")
    close(got, want, 1e-2, str(case))


@pytest.mark.parametrize("case", [(64, 3, 3, 5, 264, 12, 0), (80, 1, 3, 8, 65, 33, 3), (64, 1, 1, 33, 33, 1, 0)], ids=str)
def test_padding_rows_of_the_suffix_cache_are_never_read(dev, case):
    """suffix rows at and beyond own_len hold NaN: the output is bit-identical to the run with zeros there"""
    zero = _run(sd.make_case(*case, seed=5, device=dev, suffix_max=case[5] + 3, pad=0.0))
    nan = _run(sd.make_case(*case, seed=5, device=dev, suffix_max=case[5] + 3, pad=float("nan")))
    assert torch.isfinite(nan.float()).all() and torch.equal(zero, nan)


@pytest.mark.parametrize("case", [(64, 3, 3, 5, 264, 12), (80, 1, 3, 8, 65, 33), (64, 1, 3, 33, 31, 2)], ids=str)
def test_a_group_depends_on_its_own_inputs_only(dev, case):
    """group g alone equals group g inside a batch of 3, bit for bit; permuting the sequences of a group permutes its output rows"""
    hd, heads, groups, gs, P, own = case
    H = heads * hd
    c = sd.make_case(*case, seed=7, device=dev)
    full = _run(c).clone()
    S = c["S"]
    for g in range(groups):
        one = dict(c, n_seq=gs, o=torch.zeros(gs, H, dtype=torch.bfloat16, device=dev), q=c["q"][g * gs * S * 3 * H:],
                   k=c["k"][g * gs * S * 3 * H:], v=c["v"][g * gs * S * 3 * H:], pk=c["pk"][g * P * 3 * H:], pv=c["pv"][g * P * 3 * H:])
        assert torch.equal(_run(one), full[g * gs:(g + 1) * gs]), g
    perm = torch.randperm(gs, generator=torch.Generator().manual_seed(1)).to(dev)
    g = 1
    rows = c["suffix"].view(groups * gs, S, 3 * H)[g * gs:(g + 1) * gs][perm].contiguous().view(-1)
    moved = dict(c, n_seq=gs, o=torch.zeros(gs, H, dtype=torch.bfloat16, device=dev), q=rows[(own - 1) * 3 * H:], k=rows[hd:], v=rows[2 * hd:],
                 pk=c["pk"][g * P * 3 * H:], pv=c["pv"][g * P * 3 * H:])
    assert torch.equal(_run(moved), full[g * gs:(g + 1) * gs][perm])


def test_refusals_leave_the_output_untouched(dev):
    from youku_mplug_amd import _lib
    c = sd.make_case(64, 3, 3, 5, 33, 4, device=dev)
    c["o"].fill_(7.0)
    H = 3 * 64
    bad = [dict(hd=96), dict(group_size=0), dict(own_len=0), dict(own_len=2049), dict(prefix_len=0),
           dict(prefix_lay=((33 * 3 * H + 4, 3 * 64, 3 * H), c["prefix_lay"][1])), dict(q=c["q"][4:])]
    for over in bad:
        with pytest.raises(_lib.MpvError):
            _run({**c, **over})
    torch.cuda.synchronize()
    assert (c["o"] == 7.0).all()


def test_shared_state_matches_decode_state_on_the_tiny_model(dev):
    """the case of tests/test_decode_shared_cpu.py on the real kernels: prefill, two steps, three steps after in-group re-orders; the
    logits agree with DecodeState's within 1e-2 (the project's KV-cache gate) and two shared states are bit-identical"""
    from test_decode_shared_cpu import run_state_case
    from youku_mplug_amd.generation import DecodeState, SharedPrefixDecodeState
    out, ref, sh, (cfg, B, K, Q, P) = run_state_case(dev, DecodeState, SharedPrefixDecodeState)
    for i, (a, b, b2) in enumerate(out):
        e = rel_err(b, a)
        print(f"    call {i}: shared vs per-sequence logits {e:.3e}")
        assert e <= 1e-2, (i, e)
        assert torch.equal(b, b2), i
    assert sh.kv_bytes() == cfg.layers * (B * (Q + P) + 2 * B * K * 6) * 3 * cfg.hidden * 2 < ref.kv_bytes()


def test_caption_generate_shared_prefix_on_the_tiny_model(dev):
    """generate(batched=True, kv_cache="shared_prefix") under the gate of test_caption_generate_batched_on_the_tiny_model: the best
    hypothesis' score deviates from the golden's fp32 score by at most 1.5 x the larger of the reference's own bf16 deviation and
    the deviation of the unchanged per-clip generate in this run (the three numbers are printed).  Then the same clip three times
    in one search: bit-identical results, equal to that clip's result next to a different neighbour."""
    from test_beam_batched_gpu import _caption_model
    g, model, video, ids, mask = _caption_model(dev)
    m, f32, b16 = g["meta"], g["fp32"], g["bf16"]
    text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    td = model.text_decoder
    plain_scores, batched = [], []
    orig, orig_b = td.beam_search, td.beam_search_batched

    def spy(*a, **k):
        out = orig(*a, **k)
        plain_scores.append(out.scores[0].item())
        return out

    def spy_b(tokens, **k):
        assert k["kv"] == "shared_prefix"
        outs = orig_b(tokens, **k)
        batched.append((tokens.shape[0], k["prompt_length"], [o.scores[0].item() for o in outs], outs))
        return outs
    td.beam_search, td.beam_search_batched = spy, spy_b
    try:
        plain = model.generate(video, text, termination_id=m["eod_id"])
        res = model.generate(video, text, termination_id=m["eod_id"], batched=True, kv_cache="shared_prefix")
        assert [(c[0], c[1]) for c in batched] == [(1, 3), (1, 5)]                 # two prompt lengths: two groups
        scores = {0: batched[1][2][0], 1: batched[0][2][0]}
        assert len(res) == len(plain) == m["batch"]
        for i, (r, p) in enumerate(zip(res, plain)):
            ref, refb = f32["scores"][i][0].item(), b16["scores"][i][0].item()
            assert r.shape == p.shape == f32["sequences"][i].shape and r.dtype == p.dtype
            n_prompt = int(mask[i].sum()) - 1
            assert torch.equal(r[0, :n_prompt], ids[i, :n_prompt])                    # the prompt is kept, in input order
            dev_ref, dev_plain, dev_shared = abs(refb - ref) / abs(ref), abs(plain_scores[i] - ref) / abs(ref), abs(scores[i] - ref) / abs(ref)
            print(f"    clip {i}: shared prefix {dev_shared:.3e} <= 1.5 * max(reference bf16 {dev_ref:.3e}, per-clip generate {dev_plain:.3e})")
            assert dev_shared <= 1.5 * max(dev_ref, dev_plain), (i, dev_shared, dev_ref, dev_plain)
        ids0, mask0 = ids[[0, 0, 0]].to(dev), mask[[0, 0, 0]].to(dev)
        text0 = types.SimpleNamespace(input_ids=ids0, attention_mask=mask0)
        batched.clear()
        same = model.generate(video[[0, 0, 0]], text0, termination_id=m["eod_id"], batched=True, kv_cache="shared_prefix")
        other = model.generate(video[[0, 1, 0]], text0, termination_id=m["eod_id"], batched=True, kv_cache="shared_prefix")
        assert [(c[0], c[1]) for c in batched] == [(3, 5), (3, 5)]
        (_, _, s_same, o_same), (_, _, s_other, o_other) = batched
        assert torch.equal(same[0], same[1]) and torch.equal(same[0], same[2]) and s_same[0] == s_same[1] == s_same[2]
        assert torch.equal(o_same[0].scores, o_same[1].scores) and torch.equal(o_same[0].scores, o_same[2].scores)
        assert torch.equal(other[0], same[0]) and torch.equal(other[2], same[0]) and s_other[0] == s_other[2] == s_same[0]
    finally:
        td.beam_search, td.beam_search_batched = orig, orig_b


def test_caption_sampling_shared_prefix_on_the_tiny_model(dev):
    """generate(do_sample=True, num_samples=4, seed=3, kv_cache="shared_prefix"): per clip a [4, Lt] tensor that continues the clip's
    prompt; a clip's samples are bit-identical next to a different neighbour at the same row count"""
    from test_beam_batched_gpu import _caption_model
    g, model, video, ids, mask = _caption_model(dev)
    m = g["meta"]
    kw = dict(termination_id=m["eod_id"], do_sample=True, num_samples=4, seed=3, kv_cache="shared_prefix")
    Lt = ids.shape[1] + m["tokens_to_generate"]
    text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    res = model.generate(video, text, **kw)
    assert len(res) == m["batch"]
    for i, r in enumerate(res):
        n_prompt = int(mask[i].sum()) - 1
        assert r.shape == (4, Lt) and r.dtype == torch.int64 and (r[:, :n_prompt] == ids[i, :n_prompt]).all(), i
    text0 = types.SimpleNamespace(input_ids=ids[[0, 0, 0]].to(dev), attention_mask=mask[[0, 0, 0]].to(dev))
    same = model.generate(video[[0, 0, 0]], text0, **kw)
    other = model.generate(video[[0, 1, 0]], text0, **kw)
    assert torch.equal(same[0], other[0]) and torch.equal(same[2], other[2])
