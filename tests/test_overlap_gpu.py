"""Consensus caption choice on the GPU: ops.caption_overlap (include/mpv.h: mpv_caption_overlap) against tests/ref_overlap.py on every
case of tests/overlap_cases.py -- every integer, twice --, the library's refusals with the outputs untouched, and
generate(consensus=) / generate(rerank_by_consensus=) on the tiny synthetic caption model against the reference's choice from the
tokens of the same call made without the keyword."""
import ctypes

import pytest
import torch

import overlap_cases as oc
import ref_overlap as ro

pytestmark = pytest.mark.gpu
METRICS = ("rouge_l", "ngram_f")


def _call(case, dev):
    from youku_mplug_amd import ops
    tok_a = case["tok_a"].to(dev)
    if case["same"]:
        return ops.caption_overlap(tok_a, case["start_a"], case["begin_a"], term=case["term"], width_a=case["width_a"])
    return ops.caption_overlap(tok_a, case["start_a"], case["begin_a"], case["tok_b"].to(dev), case["start_b"], case["begin_b"],
                               term=case["term"], width_a=case["width_a"], width_b=case["width_b"])


@pytest.mark.parametrize("case", oc.CASES, ids=oc.NAMES)
def test_kernel_equals_the_reference_on_every_integer_twice(dev, case):
    la, lb, counts = ro.case_counts(case)
    first = _call(case, dev)
    second = _call(case, dev)
    torch.cuda.synchronize()
    for len_a, len_b, got in (first, second):
        assert len_a.dtype == len_b.dtype == got.dtype == torch.int32 and got.shape == (len(counts), 5)
        assert len_a.tolist() == la and len_b.tolist() == lb
        bad = [(p, g, w) for p, (g, w) in enumerate(zip(got.tolist(), counts)) if g != w]
        assert not bad, bad[:5]
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    if case["same"]:
        assert first[0] is first[1]                                             # one table: its lengths once


def test_a_view_with_a_row_stride_and_tensor_arguments(dev):
    """the table as a column slice of a wider one (row stride above the width, no copy), start / begin as tensors"""
    from youku_mplug_amd import ops
    case = next(c for c in oc.CASES if c["name"] == "two_tables")
    la, lb, counts = ro.case_counts(case)
    wide_a, wide_b = case["tok_a"].to(dev), torch.cat([case["tok_b"], case["tok_b"][:, :5]], dim=1).to(dev)
    len_a, len_b, got = ops.caption_overlap(wide_a[:, :case["width_a"]], torch.tensor(case["start_a"]), torch.tensor(case["begin_a"]),
                                            wide_b[:, :case["width_b"]], torch.tensor(case["start_b"]), torch.tensor(case["begin_b"]), term=case["term"])
    assert len_a.tolist() == la and len_b.tolist() == lb and got.tolist() == counts


def test_wrapper_and_library_refuse_without_launching(dev):
    """the wrapper raises ValueError for a table whose width - start is 256; the library returns a negative code for a non-monotone
    begin, a start above the width, a pair_begin that is no running sum and a null pointer -- and the outputs keep their bits"""
    from youku_mplug_amd import _lib, ops
    tok, start, begin = oc.refused_table()
    with pytest.raises(ValueError, match="256"):
        ops.caption_overlap(tok.to(dev), start, begin, term=oc.TERM)
    case = oc.CASES[2]
    tok = case["tok_a"].to(dev)
    rows, groups = tok.shape[0], len(case["begin_a"]) - 1
    pair = [0, rows * rows]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    host = dict(start=i32(case["start_a"]), begin=i32(case["begin_a"]), pair=torch.tensor(pair, dtype=torch.int64))
    devs = {k: v.to(dev) for k, v in host.items()}
    len_out = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((rows * rows, 5), -7, dtype=torch.int32, device=dev)

    def run(**over):
        h = dict(host, **{k: v for k, v in over.items() if k in host})
        d = _lib.CaptionOverlapDesc()
        d.tok_a = d.tok_b = tok.data_ptr()
        d.start_a = d.start_b = devs["start"].data_ptr()
        d.begin_a = d.begin_b = devs["begin"].data_ptr()
        d.pair_begin, d.len_a, d.len_b, d.counts = devs["pair"].data_ptr(), len_out.data_ptr(), len_out.data_ptr(), counts.data_ptr()
        d.host_start_a = d.host_start_b = h["start"].data_ptr()
        d.host_begin_a = d.host_begin_b = h["begin"].data_ptr()
        d.host_pair_begin = h["pair"].data_ptr()
        d.ld_a = d.ld_b = tok.stride(0)
        d.term, d.rows_a, d.rows_b, d.width_a, d.width_b, d.groups = case["term"], rows, rows, case["width_a"], case["width_a"], groups
        for k, v in over.items():
            if k not in host:
                setattr(d, k, v)
        rc = _lib.lib().mpv_caption_overlap(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc
    for over in (dict(begin=i32([0, rows + 1])), dict(begin=i32([1, rows])), dict(start=i32([case["width_a"] + 1] + case["start_a"][1:])),
                 dict(start=i32([-1] + case["start_a"][1:])), dict(pair=torch.tensor([0, rows * rows - 1])), dict(counts=None), dict(tok_b=None),
                 dict(host_begin_b=None), dict(groups=0), dict(ld_a=case["width_a"] - 1)):
        assert run(**over) < 0, over
        assert b"mpv_caption_overlap" in _lib.lib().mpv_last_error()
        assert (len_out == -7).all() and (counts == -7).all(), over
    # two groups with a begin that steps back
    assert run(groups=2, begin=i32([0, rows + 1, rows]), pair=torch.tensor([0, (rows + 1) ** 2, rows * rows])) < 0
    assert (len_out == -7).all() and (counts == -7).all()
    assert run() == 0 and counts.tolist() == ro.case_counts(case)[2]


# ------------------------------------------------------------------------------------------------ on the tiny caption model
N = 8


@pytest.fixture(scope="module")
def tiny(dev):
    import caption_score_cases as cs
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    sel = [0, 1, 0]
    text = cs.text_of(ids, mask, sel, dev)
    return model, g["meta"]["eod_id"], video[sel].to(dev).to(torch.bfloat16), text, (text.attention_mask.sum(-1) - 1).tolist()


def _reference(rows, start, term, metric):
    rows = rows.tolist()
    n, width = len(rows), len(rows[0])
    la, lb, counts = ro.table_counts(rows, [start] * n, [0, n], width, rows, [start] * n, [0, n], width, term)
    return ro.choice(ro.group_utilities(counts, la, lb, metric))[0]


@pytest.mark.parametrize("mode", ["grouped", "mixed", "inflight"])
def test_generate_consensus_is_the_references_choice(tiny, mode):
    """generate(do_sample=True, num_samples=8, consensus=, return_scores=True) returns exactly the sample the reference chooses from
    the tokens of the same call made without the keyword (generation itself is unchanged: the tokens are identical), with its scores,
    its index and U of every sample"""
    model, term, vid, text, lengths = tiny
    more = {"grouped": {}, "mixed": dict(kv_cache="shared_prefix", sample_mixed_prompts=True),
            "inflight": dict(kv_cache="shared_prefix", inflight=True, refill_min=1)}[mode]
    kw = dict(termination_id=term, do_sample=True, num_samples=N, seed=17, top_k=3, clips_per_search=2, **more)
    res, sc = model.generate(vid, text, return_scores=True, **kw)
    for metric in METRICS:
        got, gsc = model.generate(vid, text, return_scores=True, consensus=metric, **kw)
        only = model.generate(vid, text, consensus=metric, **kw)
        for i in range(len(res)):
            U = _reference(res[i], lengths[i], term, metric)
            assert ro.clear_choice(U), [float(x) for x in U]
            best = max(range(N), key=lambda s: (U[s], -s))
            print(f"    {mode} {metric} clip {i}: index {best}, U {[round(float(x), 4) for x in U]}")
            assert gsc[i]["index"] == best and torch.equal(got[i], res[i][best:best + 1]) and torch.equal(only[i], got[i])
            assert gsc[i]["consensus"].dtype == torch.float64 and gsc[i]["consensus"].shape == (N,)
            assert all(abs(float(a) - float(b)) <= 1e-12 for a, b in zip(gsc[i]["consensus"].tolist(), U))
            for k in ("sum_logprob", "count", "token_logprob"):
                assert torch.equal(gsc[i][k], sc[i][k][best:best + 1]), k


@pytest.mark.parametrize("beams", [dict(beam_size=2, num_return_gen=4, diversity_penalty=0.5), dict(beam_size=3, num_return_gen=6, diversity_penalty=2.0)],
                         ids=["2x2", "2x3"])
def test_generate_rerank_by_consensus_with_beam_groups(tiny, beams):
    """generate(batched=True, beam_groups=2, rerank_by_consensus=): the rows of the call without the keyword, by the reference's U
    descending with ties in search order"""
    model, term, vid, text, lengths = tiny
    kw = dict(termination_id=term, batched=True, beam_groups=2, clips_per_search=2, **beams)
    res = model.generate(vid, text, **kw)
    for metric in METRICS:
        got, info = model.generate(vid, text, rerank_by_consensus=metric, **kw)
        for i in range(len(res)):
            U = _reference(res[i], lengths[i], term, metric)
            srt = sorted(set(U), reverse=True)
            assert all(a - b > ro.Fraction(1, 10 ** 9) for a, b in zip(srt, srt[1:]))           # distinct U are far apart
            order = sorted(range(len(U)), key=lambda s: -U[s])
            print(f"    {metric} clip {i}: order {order}, U {[round(float(x), 4) for x in U]}")
            assert torch.equal(got[i], res[i][order])
            assert all(abs(float(a) - float(U[s])) <= 1e-12 for a, s in zip(info[i]["consensus"].tolist(), order))
            assert info[i]["group"].shape == (len(U),) and info[i]["group"].dtype == torch.int64
