"""Consensus caption choice on the host: the reference (tests/ref_overlap.py) against the caption entry point's own ROUGE-L and clipped
n-gram counts, the stand-in (tests/standin_overlap.py) against the reference on every case of tests/overlap_cases.py,
generation.consensus_utility / consensus_choice against the exact fractions, the refusals, the new symbol's declaration and
descriptor, what the library refuses on the host, generate(consensus=) in the grouped, mixed-prompt and in-flight modes and
generate(rerank_by_consensus=) with beam groups on the stand-ins, and the entry point's flags."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest
import torch

import overlap_cases as oc
import ref_overlap as ro
import standin_overlap as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("rouge_l", "ngram_f")
BF = torch.bfloat16


def _entry():
    import test_entrypoint_gpu as t
    return t._finetune_entry("run_caption_distributed_gpt3")


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("case", oc.CASES, ids=oc.NAMES)
def test_reference_is_the_entry_points_rouge_l_and_clipped_counts(case):
    """on every pair of every case: the reference's ROUGE-L utility is rouge_l([(h, [r])]) of the caption entry point within 1e-12, and
    its clipped matches are those of the entry point's _ngrams counters.  Two empty candidates are the one place where the two
    differ by definition: the entry point's guard gives 0, the consensus utility 1 (identical candidates agree)."""
    entry = _entry()
    la, lb, counts = ro.case_counts(case)
    ca = [ro.candidate(r, s, case["term"], case["width_a"]) for r, s in zip(case["tok_a"].tolist(), case["start_a"])]
    cb = [ro.candidate(r, s, case["term"], case["width_b"]) for r, s in zip(case["tok_b"].tolist(), case["start_b"])]
    assert [len(c) for c in ca] == la and ca == case["cands_a"] and cb == case["cands_b"]
    seen, at = set(), 0
    for g in range(len(case["begin_a"]) - 1):
        for i in range(case["begin_a"][g], case["begin_a"][g + 1]):
            for j in range(case["begin_b"][g], case["begin_b"][g + 1]):
                c, h, r = counts[at], ca[i], cb[j]
                at += 1
                key = (tuple(h), tuple(r))
                if key in seen:
                    continue
                seen.add(key)
                want = entry.rouge_l([(h, [r])])
                got = float(ro.utility(c, len(h), len(r), "rouge_l"))
                if not h and not r:
                    assert want == 0.0 and got == 1.0
                else:
                    assert abs(got - want) <= 1e-12, (h, r, got, want)
                for n in (1, 2, 3, 4):
                    gh, gr = entry._ngrams(h, n), entry._ngrams(r, n)
                    assert c[n] == sum(min(x, gr[k]) for k, x in gh.items()), (h, r, n)
                assert c == ro.pair_counts(r, h)                                            # all five are symmetric
    assert at == len(counts)


def test_cases_hold_the_edges_they_promise():
    lens = {len(c) for case in oc.CASES for c in case["cands_a"] + case["cands_b"]}
    assert set(oc.LENGTH_EDGES) <= lens
    sizes = {b - a for case in oc.CASES for side in ("begin_a", "begin_b") for a, b in zip(case[side], case[side][1:])}
    assert set(oc.GROUP_EDGES) <= sizes
    assert max(t for case in oc.CASES for c in case["cands_a"] for t in c) == 51199
    assert any(case["tok_a"].shape[1] > case["width_a"] for case in oc.CASES)
    assert any(not case["same"] and case["width_a"] != case["width_b"] for case in oc.CASES)
    for case in oc.CASES:                                                                   # no term, term at start, term in the prompt
        rows = case["tok_a"].tolist()
        kinds = {("none" if oc.TERM not in r[s:case["width_a"]] else "at_start" if r[s] == oc.TERM else "behind")
                 for r, s in zip(rows, case["start_a"])}
        case["kinds"] = kinds
    assert {"none", "at_start", "behind"} <= set().union(*(case["kinds"] for case in oc.CASES))
    assert any(oc.TERM in r[:s] for case in oc.CASES for r, s in zip(case["tok_a"].tolist(), case["start_a"]))
    assert any(len(set(case["start_a"])) > 1 for case in oc.CASES)


# ------------------------------------------------------------------------------------------------ the stand-in
def _standin(case):
    if case["same"]:
        return so.caption_overlap(case["tok_a"][:, :], case["start_a"], case["begin_a"], term=case["term"], width_a=case["width_a"])
    return so.caption_overlap(case["tok_a"], case["start_a"], case["begin_a"], case["tok_b"], case["start_b"], case["begin_b"],
                              term=case["term"], width_a=case["width_a"], width_b=case["width_b"])


@pytest.mark.parametrize("case", oc.CASES, ids=oc.NAMES)
def test_standin_equals_the_reference_exactly(case):
    la, lb, counts = ro.case_counts(case)
    len_a, len_b, got = _standin(case)
    assert len_a.dtype == len_b.dtype == got.dtype == torch.int32
    assert len_a.tolist() == la and len_b.tolist() == lb
    assert got.tolist() == counts


def test_standin_refuses_a_candidate_of_256_tokens():
    tok, start, begin = oc.refused_table()
    with pytest.raises(ValueError, match="256"):
        so.caption_overlap(tok, start, begin, term=oc.TERM)


# ------------------------------------------------------------------------------------------------ utilities and the choice
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", oc.CASES, ids=oc.NAMES)
def test_consensus_utility_and_choice_against_exact_fractions(case, metric):
    """consensus_utility within 1e-12 of the exact fractions on every pair, U within 1e-12, and the choice is the reference's index
    in every group -- where the reference's best two U are exactly tied or more than 1e-9 apart, which is asserted: no case hides
    behind rounding"""
    from youku_mplug_amd import generation
    groups = ro.case_groups(case)
    assert any(len(lh) > 1 and len(lr) for _, lh, lr in groups)
    for counts, lh, lr in groups:
        u_ref = ro.group_utilities(counts, lh, lr, metric)
        U_ref, best = ro.choice(u_ref)
        assert ro.clear_choice(U_ref), [float(x) for x in U_ref]
        u = generation.consensus_utility(torch.tensor(counts, dtype=torch.int32).reshape(-1, 5), torch.tensor(lh, dtype=torch.int32),
                                         torch.tensor(lr, dtype=torch.int32), metric)
        assert u.dtype == torch.float64 and tuple(u.shape) == (len(lh), len(lr))
        for h in range(len(lh)):
            for r in range(len(lr)):
                assert abs(float(u[h, r]) - float(u_ref[h][r])) <= 1e-12, (h, r)
        U, index = generation.consensus_choice(u)
        assert U.dtype == torch.float64 and index == best
        assert all(abs(float(a) - float(b)) <= 1e-12 for a, b in zip(U.tolist(), U_ref))
    # weights: the reference's weighted mean, and uniform weights are the default bit for bit
    counts, lh, lr = max(groups, key=lambda g: len(g[1]) * len(g[2]))
    u = generation.consensus_utility(torch.tensor(counts).reshape(len(lh), len(lr), 5), lh, lr, metric)
    w = [1 + (3 * r) % 5 for r in range(len(lr))]
    U_ref, best = ro.choice(ro.group_utilities(counts, lh, lr, metric), w)
    U, index = generation.consensus_choice(u, torch.tensor(w))
    assert ro.clear_choice(U_ref) and index == best and all(abs(float(a) - float(b)) <= 1e-12 for a, b in zip(U.tolist(), U_ref))
    assert torch.equal(generation.consensus_choice(u, [1.0] * len(lr))[0], generation.consensus_choice(u)[0])


def test_identical_candidates_get_bit_identical_consensus():
    from youku_mplug_amd import generation
    case = next(c for c in oc.CASES if c["name"] == "clipping_identical_disjoint")
    la, lb, counts = ro.case_counts(case)
    for metric in METRICS:
        u = generation.consensus_utility(torch.tensor(counts).reshape(8, 8, 5), la, lb, metric)
        U, index = generation.consensus_choice(u)
        assert float(U[0]) == float(U[2]) and float(U[3]) == float(U[5])
        assert case["cands_a"][0] == case["cands_a"][2] and case["cands_a"][3] == case["cands_a"][5]


def test_empty_candidates_and_host_refusals():
    from youku_mplug_amd import generation
    zero = torch.zeros((1, 5), dtype=torch.int32)
    for metric in METRICS:
        assert float(generation.consensus_utility(zero, [0], [0], metric)) == 1.0
        assert float(generation.consensus_utility(zero, [0], [4], metric)) == 0.0
        assert float(generation.consensus_utility(zero, [4], [0], metric)) == 0.0
    # rouge_l is asymmetric: h is the candidate being judged
    c = torch.tensor([[2, 2, 1, 0, 0]], dtype=torch.int32)
    assert float(generation.consensus_utility(c, [2], [6], "rouge_l")) != float(generation.consensus_utility(c, [6], [2], "rouge_l"))
    with pytest.raises(ValueError, match="metric"):
        generation.consensus_utility(zero, [0], [0], "cider")
    with pytest.raises(ValueError, match="weights"):
        generation.consensus_choice(torch.zeros((2, 3), dtype=torch.float64), [1.0, 2.0])
    assert generation.consensus_choice(torch.zeros((0, 0), dtype=torch.float64))[1] is None
    # a tie goes to the lowest index
    assert generation.consensus_choice(torch.tensor([[0.5, 0.25], [0.25, 0.5], [0.1, 0.1]], dtype=torch.float64))[1] == 0
    # ... also where fp64 sums of exactly equal totals differ in their last bit: (0.1 + 0.2) + 0.3 > (0.3 + 0.2) + 0.1 > 0.6
    u = torch.tensor([[0.3, 0.2, 0.1], [0.1, 0.2, 0.3], [0.2, 0.2, 0.2]], dtype=torch.float64)
    U, index = generation.consensus_choice(u)
    assert float(U[1]) > float(U[0]) and index == 0 and generation.consensus_order(U) == [0, 1, 2]
    assert generation.consensus_order([0.25, 0.5, 0.25, 0.5]) == [1, 3, 0, 2]


def test_ops_wrapper_refuses_on_the_host_before_any_launch():
    """ops.caption_overlap: a table whose width - start is 256 raises ValueError; a CPU table is no GPU table (no fallback)"""
    from youku_mplug_amd import _lib, ops
    tok, start, begin = oc.refused_table()
    with pytest.raises(_lib.MpvError, match="GPU only"):
        ops.caption_overlap(tok, start, begin, term=oc.TERM)


# ------------------------------------------------------------------------------------------------ the library on the host
def _arr(ct, values):
    return (ct * len(values))(*values)


def _desc(**over):
    """a descriptor over 4 rows in 2 groups with REAL host arrays and device pointers that are not memory (a launch would fault)"""
    from youku_mplug_amd import _lib
    host = dict(host_start_a=[2, 3, 0, 1], host_start_b=[2, 3, 0, 1], host_begin_a=[0, 3, 4], host_begin_b=[0, 3, 4], host_pair_begin=[0, 9, 10])
    host.update({k: v for k, v in over.items() if k in host})
    keep = {k: (None if v is None else _arr(ctypes.c_int64 if k == "host_pair_begin" else ctypes.c_int32, v)) for k, v in host.items()}
    ok = dict(tok_a=0x10000, tok_b=0x10000, start_a=0x20000, start_b=0x20000, begin_a=0x30000, begin_b=0x30000, pair_begin=0x40000,
              len_a=0x50000, len_b=0x50000, counts=0x60000, ld_a=16, ld_b=16, term=2, rows_a=4, rows_b=4, width_a=12, width_b=12, groups=2)
    ok.update({k: v for k, v in over.items() if k not in host})
    d = _lib.CaptionOverlapDesc()
    for k, v in ok.items():
        setattr(d, k, v)
    for k, v in keep.items():
        setattr(d, k, None if v is None else ctypes.cast(v, ctypes.c_void_p).value)
    return d, keep


REFUSALS = [dict(tok_a=None), dict(tok_b=None), dict(start_a=None), dict(start_b=None), dict(begin_a=None), dict(begin_b=None),
            dict(pair_begin=None), dict(len_a=None), dict(len_b=None), dict(counts=None), dict(host_start_a=None), dict(host_begin_b=None),
            dict(host_pair_begin=None), dict(groups=0), dict(rows_a=-1), dict(width_b=-1), dict(ld_a=11),
            dict(host_begin_a=[0, 3, 2]), dict(host_begin_a=[0, 5, 4]), dict(host_begin_b=[1, 3, 4]), dict(host_begin_a=[0, 3, 5]),
            dict(host_start_a=[2, 13, 0, 1]), dict(host_start_b=[2, -1, 0, 1]), dict(host_pair_begin=[0, 9, 11]), dict(host_pair_begin=[1, 10, 11]),
            dict(width_a=258, ld_a=258, host_start_a=[3, 3, 2, 3])]


def test_library_exports_the_symbol_and_refuses_on_the_host():
    """every refusal of include/mpv.h comes back negative before anything is launched (the device pointers are not memory: a launch
    would fault): null pointers, a non-monotone begin, a start above the width, a pair_begin that is no running sum, a candidate of
    256 tokens"""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    assert "mpv_caption_overlap" in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "mpv_caption_overlap")
    fn = _lib.lib().mpv_caption_overlap
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 2
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    assert re.search(r"int mpv_caption_overlap\(const mpv_caption_overlap_desc\* d, mpv_stream_t stream\);", hdr)
    assert _lib.CAPTION_OVERLAP_MAX_LEN == int(re.search(r"#define MPV_CAPTION_OVERLAP_MAX_LEN (\d+)", hdr).group(1)) == 255
    for over in REFUSALS:
        d, keep = _desc(**over)
        rc = fn(ctypes.byref(d), None)
        assert rc < 0, over
        assert b"mpv_caption_overlap" in _lib.lib().mpv_last_error(), over
    assert fn(None, None) < 0
    d, keep = _desc(width_a=258, ld_a=258, host_start_a=[3, 3, 2, 3])
    assert fn(ctypes.byref(d), None) == -1 and b"256 tokens" in _lib.lib().mpv_last_error()


def test_ctypes_descriptor_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    cname, ct = "mpv_caption_overlap_desc", _lib.CaptionOverlapDesc
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


def test_overlap_kernels_have_no_scratch_and_one_rolling_row_of_lds():
    """co_pairs in the gfx950 code object: one wave per workgroup, 255 x 64 uint8 cells of static LDS, no scratch; co_lengths: no LDS,
    no scratch.  Register, LDS and scratch figures only, read the way tests/test_isa_cpu.py reads them."""
    import tempfile
    import test_isa_cpu as isa
    if not os.path.isfile(os.path.join(isa.LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for i, blob in enumerate(isa._code_objects()):
            f = os.path.join(d, f"co_{i}.elf")
            open(f, "wb").write(blob)
            txt = subprocess.run([os.path.join(isa.LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
            for blk in txt.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                for key in ("co_pairs", "co_lengths"):
                    if key in name:
                        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
                        found[key] = dict(vgpr=g("vgpr_count"), scratch=g("private_segment_fixed_size"), lds=g("group_segment_fixed_size"),
                                          threads=g("max_flat_workgroup_size"))
    print(f"    {found}")
    assert set(found) == {"co_pairs", "co_lengths"}
    assert found["co_pairs"] == dict(found["co_pairs"], scratch=0, lds=255 * 64, threads=64)
    assert found["co_lengths"] == dict(found["co_lengths"], scratch=0, lds=0)


# ------------------------------------------------------------------------------------------------ generate on the stand-ins
N = 6
MODES = {"grouped": {}, "grouped_shared_kv": dict(kv_cache="shared_prefix"), "mixed": dict(kv_cache="shared_prefix", sample_mixed_prompts=True),
         "inflight": dict(kv_cache="shared_prefix", inflight=True, refill_min=1)}


def _on_cpu(monkeypatch):
    import test_beam_inflight_cpu as tbi
    dev = tbi._on_cpu(monkeypatch)
    so.install(monkeypatch)
    return dev


def _reference_pick(rows, start, term, metric):
    """rows [n, Lt] of ONE clip -> (U fractions, index) by the reference, from the tokens alone"""
    rows = rows.tolist()
    n, width = len(rows), len(rows[0]) if rows else 0
    la, lb, counts = ro.table_counts(rows, [start] * n, [0, n], width, rows, [start] * n, [0, n], width, term)
    U, best = ro.choice(ro.group_utilities(counts, la, lb, metric))
    assert ro.clear_choice(U), [float(x) for x in U]
    return U, best


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("mode", list(MODES))
def test_generate_consensus_is_the_references_choice_on_standins(monkeypatch, mode, metric):
    """generate(consensus=) returns, clip by clip, the sample the reference chooses from the tokens of the SAME call made without the
    keyword (generation is unchanged: the tokens are identical); with return_scores the chosen sample's entries, index and U of every
    sample; without the keyword the stand-in is never reached"""
    import test_inflight_cpu as ti
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = ti._setup(dev)
    lengths = (text.attention_mask.sum(-1) - 1).tolist()
    kw = dict(termination_id=term, do_sample=True, num_samples=N, seed=5, top_k=2, clips_per_search=2, **MODES[mode])
    del so.calls[:]
    res, sc = model.generate(vid, text, return_scores=True, **kw)
    plain = model.generate(vid, text, **kw)
    assert not so.calls
    got, gsc = model.generate(vid, text, return_scores=True, consensus=metric, **kw)
    only = model.generate(vid, text, consensus=metric, **kw)
    assert so.calls and all(a == b for a, b, g in so.calls)
    picked = set()
    for i in range(len(res)):
        assert torch.equal(plain[i], res[i])
        U, best = _reference_pick(res[i], lengths[i], term, metric)
        picked.add(best)
        assert got[i].shape == (1, res[i].shape[1]) and torch.equal(got[i], res[i][best:best + 1]) and torch.equal(only[i], got[i])
        assert gsc[i]["index"] == best and gsc[i]["consensus"].dtype == torch.float64 and gsc[i]["consensus"].shape == (N,)
        assert all(abs(float(a) - float(b)) <= 1e-12 for a, b in zip(gsc[i]["consensus"].tolist(), U))
        for k in ("sum_logprob", "count", "token_logprob"):
            assert torch.equal(gsc[i][k], sc[i][k][best:best + 1]), k
    assert len(picked) > 1, picked                                             # (the cases do not all fall to index 0)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("mode", ["grouped", "mixed", "inflight"])
def test_generate_rerank_by_consensus_with_beam_groups_on_standins(monkeypatch, mode, metric):
    """generate(batched=True, beam_groups=2, rerank_by_consensus=): every clip's rows are the rows of the same call without the
    keyword, reordered by the reference's U descending with ties in search order; info carries U and the groups in the new order"""
    import test_inflight_cpu as ti
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = ti._setup(dev)
    lengths = (text.attention_mask.sum(-1) - 1).tolist()
    more = {"grouped": {}, "mixed": dict(kv_cache="shared_prefix", mixed_prompts=True), "inflight": dict(kv_cache="shared_prefix", beam_inflight=True)}[mode]
    kw = dict(termination_id=term, batched=True, beam_groups=2, diversity_penalty=0.5, beam_size=2, num_return_gen=4, clips_per_search=2, **more)
    del so.calls[:]
    res = model.generate(vid, text, **kw)
    assert not so.calls
    got, info = model.generate(vid, text, rerank_by_consensus=metric, **kw)
    assert len(so.calls) == 1 and so.calls[0][2] == len(res)
    moved = []
    for i in range(len(res)):
        rows = res[i].tolist()
        n, width = len(rows), res[i].shape[1]
        la, lb, counts = ro.table_counts(rows, [lengths[i]] * n, [0, n], width, rows, [lengths[i]] * n, [0, n], width, term)
        U, _ = ro.choice(ro.group_utilities(counts, la, lb, metric))
        srt = sorted(set(U), reverse=True)
        assert all(a - b > ro.Fraction(1, 10 ** 9) for a, b in zip(srt, srt[1:]))               # distinct U are far apart
        order = sorted(range(n), key=lambda s: -U[s])
        moved.append(order != list(range(n)))
        assert torch.equal(got[i], res[i][order]), (i, order)
        assert info[i]["consensus"].dtype == torch.float64 and all(abs(float(a) - float(U[s])) <= 1e-12 for a, s in zip(info[i]["consensus"].tolist(), order))
        assert info[i]["group"].dtype == torch.int64 and info[i]["group"].shape == (n,)
        assert sorted(info[i]["group"].tolist()) == sorted(g for g in range(2) for _ in range(n // 2))
    assert any(moved)                                                              # (the keyword does reorder something here)


def test_generate_refusals_name_the_keywords(monkeypatch):
    import test_inflight_cpu as ti
    dev = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = ti._setup(dev)
    del so.calls[:]
    s = dict(termination_id=term, do_sample=True, num_samples=2)
    b = dict(termination_id=term, batched=True)
    for kw, words in ((dict(s, consensus="rouge_l", best_of=True), ("consensus", "best_of")),
                      (dict(s, consensus="cider"), ("consensus",)),
                      (dict(b, consensus="rouge_l"), ("consensus", "do_sample")),
                      (dict(termination_id=term, consensus="ngram_f"), ("consensus", "do_sample")),
                      (dict(b, rerank_by_consensus="rouge_l", rerank_by_logprob=True), ("rerank_by_consensus", "rerank_by_logprob")),
                      (dict(b, rerank_by_consensus="rouge_l", allowed_phrases=[[9, 10]]), ("rerank_by_consensus", "allowed_phrases")),
                      (dict(b, rerank_by_consensus="bleu"), ("rerank_by_consensus",)),
                      (dict(s, rerank_by_consensus="rouge_l"), ("rerank_by_consensus", "batched")),
                      (dict(termination_id=term, rerank_by_consensus="rouge_l"), ("rerank_by_consensus", "batched"))):
        with pytest.raises(ValueError) as e:
            model.generate(vid, text, **kw)
        assert all(w in str(e.value) for w in words), (kw, str(e.value))
    # a table that could hold a candidate of more than 255 tokens is refused before anything runs
    model.text_decoder.config.extra.update(tokens_to_generate=300)
    monkeypatch.setattr(model.text_decoder.config, "max_position_embeddings", 10 ** 4)
    ran = []
    monkeypatch.setattr(model.text_decoder, "sample_batched", lambda *a, **k: ran.append(1))
    with pytest.raises(ValueError, match="255"):
        model.generate(vid, text, consensus="rouge_l", **s)
    assert not ran and not so.calls


def test_caption_entrypoint_consensus_flags_on_standins(tmp_path, monkeypatch):
    """--eval_sample_consensus 3 [--eval_consensus_metric ngram_f]: default 0; reaches model.generate as do_sample / num_samples /
    consensus, replaces the beam search, is refused with --eval_sample_best_of and --eval_beam_groups, and the result file carries one
    caption per clip in the beam evaluation's format"""
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
    monkeypatch.setenv("MASTER_PORT", str(50000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    seen = []
    gen = downstream.DistributedGPT3_Caption.generate

    def spy(self, image, text, *a, **kw):
        out = gen(self, image, text, *a, **kw)
        seen.append((kw, out))
        return out
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    try:
        out = str(tmp_path / "consensus")
        base = ["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only"]
        args0 = entry.get_args(base)[0]
        assert args0.eval_sample_consensus == 0 and args0.eval_consensus_metric is None
        for bad in (["--eval_sample_consensus", "-1"], ["--eval_consensus_metric", "rouge_l"],
                    ["--eval_sample_consensus", "3", "--eval_sample_best_of", "3"],
                    ["--eval_sample_consensus", "3", "--eval_batched_beam", "--eval_beam_groups", "2"]):
            with pytest.raises(ValueError, match="eval_sample_consensus"):
                entry.get_args(base + bad)
        with pytest.raises(SystemExit):
            entry.get_args(base + ["--eval_sample_consensus", "3", "--eval_consensus_metric", "cider"])
        args, config = entry.get_args(base + ["--eval_sample_consensus", "3", "--eval_consensus_metric", "ngram_f", "--eval_no_repeat_ngram", "2",
                                              "--eval_shared_kv", "--eval_sample_inflight"])
        stats = entry.main(args, config)
        assert seen and all(kw.get("do_sample") and kw.get("consensus") == "ngram_f" and kw.get("num_samples") == 3 and kw.get("inflight") and
                            kw.get("no_repeat_ngram_size") == 2 and not kw.get("best_of") for kw, _ in seen), [kw for kw, _ in seen]
        assert all(isinstance(o, list) and all(r.shape[0] == 1 for r in o) for _, o in seen)
        merged = json.load(open(os.path.join(out, "result", "val_caption_result.json")))
        assert any(k.startswith("val_") for k in stats)
        del seen[:]
        args, config = entry.get_args(base + ["--eval_sample_consensus", "2"])
        entry.main(args, config)
        assert seen and all(kw.get("consensus") == "rouge_l" for kw, _ in seen)
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert len(merged) == 5
    for rec in merged:
        assert set(rec) == {"video_id", "pred_caption", "gold_caption"} and isinstance(rec["pred_caption"], str)
