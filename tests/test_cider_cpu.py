"""CIDEr on the host: the reference (tests/ref_cider.py) against the recorded scores of the reference project's own scorer
(tests/golden/cider_reference.json), generation.CiderStats (document frequencies, the table, its slot rule, persistence), the stand-in
(tests/standin_cider.py) under the kernel's gates, the new symbols' declarations and host refusals, self-critical training
(DistributedGPT3_Caption.forward_scst) on the stand-in pipelines -- the same checks the GPU suite runs -- and the entry point's flags."""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

import cider_cases as cc
import ref_cider as rc
import standin_cider as sc
import test_cider_gpu as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "cider_reference.json")))


def _on_cpu(monkeypatch):
    import test_overlap_cpu as to
    dev = to._on_cpu(monkeypatch)
    sc.install(monkeypatch)
    return dev


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("case", cc.CASES, ids=cc.NAMES)
def test_reference_equals_the_recorded_scorer(case):
    """every candidate's score within 1e-12 relative of what the reference project's scorer gave; the record holds this case's inputs"""
    rec = GOLD["cases"][case["name"]]
    assert rec["candidates"] == case["groups_a"] and rec["references"] == case["groups_b"]
    pair, score = rc.case_values(case)
    gold = [s for g in rec["score"] for s in g]
    assert len(gold) == len(score) and len(pair) == sum(len(a) * len(b) for a, b in zip(case["groups_a"], case["groups_b"]))
    for got, want in zip(score, gold):
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    assert any(s > 0 for s in score) or case["name"] == "one_clip"
    mean, per_clip = rc.corpus_cider(cc.EVAL_HYPS, cc.EVAL_REFS)
    assert abs(mean - GOLD["eval"]["mean"]) <= 1e-12 * GOLD["eval"]["mean"]
    assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(per_clip, GOLD["eval"]["score"]))


def test_cases_hold_the_edges_they_promise():
    lens = {len(c) for case in cc.CASES for side in ("groups_a", "groups_b") for g in case[side] for c in g}
    assert set(cc.LENGTH_EDGES) <= lens
    edges = cc.CASES[0]
    assert any(not g for g in edges["groups_a"]) and any(not g for g in edges["groups_b"])
    assert edges["tok_a"][0, 0].item() == cc.TERM and edges["start_a"][0] == 0            # `term` in the first column
    assert len(set(edges["start_a"])) > 1 and max(edges["start_b"]) > 0
    assert edges["tok_a"].shape[1] > edges["width_a"] and (edges["tok_a"][:, edges["width_a"]:] == cc.GUARD).all()
    toks = {t for g in edges["groups_a"] for c in g for t in c}
    assert {0, 65534} <= toks
    df, _ = rc.doc_freq(edges["corpus"])
    assert any((t,) not in df for t in toks)                                            # n-grams the corpus does not hold
    assert any(c in edges["groups_b"][g] for g, cands in enumerate(edges["groups_a"]) for c in cands)     # a candidate equal to its reference
    assert any(max(rc.counts(c).values(), default=0) > 1 for g in edges["groups_a"] for c in g)
    assert len(cc.CASES[1]["corpus"]) == 1
    long = cc.CASES[2]
    assert len(long["groups_a"][0][0]) == 255 and len(long["groups_b"][0][1]) == 3


# ------------------------------------------------------------------------------------------------ CiderStats
def test_cider_stats_document_frequency_and_idf():
    from youku_mplug_amd import generation
    refs = [[[5, 6, 5, 6], [5, 6]], [[5, 7]], [[8], [8, 8, 8]]]
    st = generation.CiderStats(refs, 100)
    assert st.clips == 3 and st.log_ref_len == math.log(3.0)
    assert st.df([5]) == 2 and st.df([5, 6]) == 1 and st.df([8]) == 1 and st.df([8, 8]) == 1 and st.df([6, 5, 6]) == 1      # once per clip
    assert st.df([9]) == 0 and st.df([6, 5, 6, 5]) == 0
    assert st.lookup([5]) == math.log(3.0) - math.log(2.0) and st.lookup([8, 8, 8]) == math.log(3.0) - math.log(1.0)
    assert st.lookup([9]) == st.log_ref_len and st.lookup([5, 5]) == st.log_ref_len and st.slot([9]) == -1
    assert st.capacity >= 2 * st.entries and st.capacity & (st.capacity - 1) == 0
    assert generation.CiderStats.key([0]) == 1 and generation.CiderStats.key([65534, 0, 2]) == 65535 | 1 << 16 | 3 << 32
    for case in cc.CASES:
        st = tg.stats_of(case)
        df, log_ref_len = rc.doc_freq(case["corpus"])
        assert st.entries == len(df) and st.log_ref_len == log_ref_len
        for g, d in df.items():
            assert st.df(g) == d and st.lookup(g) == log_ref_len - math.log(max(1.0, float(d))), g


def test_cider_stats_refusals_and_persistence(tmp_path):
    from youku_mplug_amd import generation
    with pytest.raises(ValueError, match="vocab"):
        generation.CiderStats([[[1, 2]]], 65536)
    with pytest.raises(ValueError, match="outside"):
        generation.CiderStats([[[1, 200]]], 100)
    with pytest.raises(ValueError, match="capacity"):
        generation.CiderStats([[[1, 2, 3]]], 100, capacity=4)                              # 6 entries
    with pytest.raises(ValueError, match="capacity"):
        generation.CiderStats([[[1, 2, 3]]], 100, capacity=12)
    with pytest.raises(ValueError, match="no clips"):
        generation.CiderStats([], 100)
    case = cc.CASES[3]
    st = tg.stats_of(case)
    path = str(tmp_path / "stats.pt")
    st.save(path)
    sd = torch.load(path)
    assert all(torch.is_tensor(v) for v in sd.values())                                      # plain tensors
    back = generation.CiderStats.load(path)
    assert (back.vocab, back.clips, back.entries, back.capacity, back.log_ref_len) == (st.vocab, st.clips, st.entries, st.capacity, st.log_ref_len)
    assert torch.equal(back.keys.view(torch.int64), st.keys.view(torch.int64)) and torch.equal(back.idf, st.idf)
    flat = [r for g in case["groups_b"] for r in g]
    begin = [0]
    for g in case["groups_b"]:
        begin.append(begin[-1] + len(g))
    again = generation.CiderStats.from_token_table(case["tok_b"][:, :case["width_b"]], case["start_b"], begin, cc.TERM, cc.VOCAB, capacity=st.capacity)
    assert torch.equal(again.keys.view(torch.int64), st.keys.view(torch.int64)) and torch.equal(again.idf, st.idf) and len(flat) == begin[-1]
    keys, idf, lrl = st.arrays("cpu")
    assert st.arrays("cpu")[0] is keys and keys.dtype == torch.uint64 and idf.dtype == torch.float64 and lrl == st.log_ref_len


def test_forced_capacity_gives_long_chains_that_wrap_and_the_slot_rule_is_splitmix64():
    """the `chains` case: a table at the smallest capacity above its entries; every key sits on the probe path from its splitmix64 home
    slot (restated in tests/ref_cider.py) with no empty slot on the way; some chains are long, some wrap past the last slot; absent
    keys are not found, also where their probe crosses a long chain and the table's end"""
    case = cc.CASES[3]
    st = tg.stats_of(case)
    assert st.capacity == case["capacity"] and st.entries < st.capacity < 2 * st.entries
    keys = [k & rc.MASK64 for k in st.keys.view(torch.int64).tolist()]
    longest = wrapped = 0
    for slot, k in enumerate(keys):
        if k == 0:
            continue
        home = rc.mix(k) & (st.capacity - 1)
        dist = (slot - home) % st.capacity
        assert all(keys[(home + d) % st.capacity] != 0 for d in range(dist))
        longest, wrapped = max(longest, dist), wrapped + (slot < home)
    print(f"    {st.entries} entries in {st.capacity} slots: longest probe {longest}, {wrapped} keys wrapped")
    assert longest >= 16 and wrapped >= 1
    df, log_ref_len = rc.doc_freq(case["corpus"])
    for g in df:
        assert keys[st.slot(g)] == rc.key_of(g)
    rng = torch.Generator().manual_seed(1)
    absent = [tuple(torch.randint(100, 160, (n,), generator=rng).tolist()) for n in (1, 2, 3, 4) for _ in range(200)]
    absent = [g for g in absent if g not in df]
    assert len(absent) > 300 and all(st.slot(g) == -1 and st.lookup(g) == log_ref_len for g in absent)


# ------------------------------------------------------------------------------------------------ the stand-in
@pytest.mark.parametrize("case", cc.CASES, ids=cc.NAMES)
def test_standin_passes_the_kernels_gates(case):
    pair, score = tg.check_case(sc.caption_cider, case, torch.device("cpu"))
    if case["name"] == "one_clip":
        assert (pair == 0).all() and (score == 0).all()


def test_standin_alone_and_among_others_and_refusal():
    tg.alone_and_among_others(sc.caption_cider, torch.device("cpu"))
    ta, sa, ba, tb, sb, bb = cc.refused_table()
    with pytest.raises(ValueError, match="256"):
        sc.caption_cider(ta, sa, ba, tb, sb, bb, term=cc.TERM, stats=tg.stats_of(cc.CASES[0]))


def test_ops_wrapper_has_no_cpu_fallback():
    from youku_mplug_amd import _lib, ops
    ta, sa, ba, tb, sb, bb = cc.refused_table()
    with pytest.raises(_lib.MpvError, match="GPU only"):
        ops.caption_cider(ta, sa, ba, tb, sb, bb, term=cc.TERM, stats=tg.stats_of(cc.CASES[0]))


# ------------------------------------------------------------------------------------------------ the library on the host
def _arr(ct, values):
    return (ct * len(values))(*values)


def _desc(**over):
    """a descriptor over 4 candidate and 3 reference rows in 2 groups with REAL host arrays and device pointers that are not memory (a
    launch would fault)"""
    from youku_mplug_amd import _lib
    host = dict(host_start_a=[2, 3, 0, 1], host_start_b=[2, 0, 1], host_begin_a=[0, 3, 4], host_begin_b=[0, 2, 3], host_pair_begin=[0, 6, 7])
    host.update({k: v for k, v in over.items() if k in host})
    keep = {k: (None if v is None else _arr(ctypes.c_int64 if k == "host_pair_begin" else ctypes.c_int32, v)) for k, v in host.items()}
    ok = dict(tok_a=0x10000, tok_b=0x11000, start_a=0x20000, start_b=0x21000, begin_a=0x30000, begin_b=0x31000, pair_begin=0x40000,
              table_keys=0x50000, table_idf=0x51000, pair=0x60000, score=0x61000, ld_a=16, ld_b=16, term=2, table_capacity=64,
              log_ref_len=1.0, sigma=6.0, rows_a=4, rows_b=3, width_a=12, width_b=12, groups=2)
    ok.update({k: v for k, v in over.items() if k not in host})
    d = _lib.CaptionCiderDesc()
    for k, v in ok.items():
        setattr(d, k, v)
    for k, v in keep.items():
        setattr(d, k, None if v is None else ctypes.cast(v, ctypes.c_void_p).value)
    return d, keep


REFUSALS = [dict(tok_a=None), dict(tok_b=None), dict(start_a=None), dict(begin_b=None), dict(pair_begin=None), dict(table_keys=None),
            dict(table_idf=None), dict(pair=None), dict(score=None), dict(host_start_a=None), dict(host_begin_b=None),
            dict(host_pair_begin=None), dict(groups=0), dict(rows_a=-1), dict(width_b=-1), dict(ld_a=11), dict(table_capacity=0),
            dict(table_capacity=1), dict(table_capacity=48), dict(log_ref_len=-0.5), dict(log_ref_len=float("inf")), dict(sigma=0.0),
            dict(sigma=float("nan")), dict(host_begin_a=[0, 3, 2]), dict(host_begin_b=[1, 2, 3]), dict(host_begin_a=[0, 3, 5]),
            dict(host_start_a=[2, 13, 0, 1]), dict(host_start_b=[2, -1, 1]), dict(host_pair_begin=[0, 6, 8]), dict(host_pair_begin=[1, 7, 8]),
            dict(width_a=258, ld_a=258, host_start_a=[3, 3, 2, 3])]


def test_library_exports_the_symbols_and_refuses_on_the_host():
    """every refusal of include/mpv.h comes back negative before anything is launched (the device pointers are not memory: a launch
    would fault); the workspace size follows the longest caption the host copies allow; a missing or small workspace is refused"""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ("mpv_caption_cider", "mpv_caption_cider_workspace_size", "mpv_cider_table_fill", "mpv_cider_table_lookup"):
        assert sym in _lib.EXPORTS and hasattr(raw, sym)
    fn, size = _lib.lib().mpv_caption_cider, _lib.lib().mpv_caption_cider_workspace_size
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    assert re.search(r"int mpv_caption_cider\(const mpv_caption_cider_desc\* d, void\* workspace, size_t workspace_bytes, mpv_stream_t stream\);", hdr)
    assert re.search(r"size_t mpv_caption_cider_workspace_size\(const mpv_caption_cider_desc\* d\);", hdr)
    assert _lib.CAPTION_CIDER_ORDERS == int(re.search(r"#define MPV_CAPTION_CIDER_ORDERS (\d+)", hdr).group(1)) == 4
    d, keep = _desc()
    need = size(ctypes.byref(d))
    assert need == (7 * (4 * 12 * 16 + 4 * 8 + 4) + 7) // 8 * 8                             # 7 rows, P = 12 - 0 positions
    buf = ctypes.create_string_buffer(need + 8)
    ws = (ctypes.addressof(buf) + 7) // 8 * 8
    for over in REFUSALS:
        d, keep = _desc(**over)
        assert fn(ctypes.byref(d), ws, need + 4096, None) < 0, over
        assert b"mpv_caption_cider" in _lib.lib().mpv_last_error(), over
    assert fn(None, ws, need, None) < 0
    d, keep = _desc()
    for bad in ((None, need), (ws, need - 8), (ws + 4, need + 8)):
        assert fn(ctypes.byref(d), bad[0], bad[1], None) < 0 and b"workspace" in _lib.lib().mpv_last_error()
    d, keep = _desc(width_a=258, ld_a=258, host_start_a=[3, 3, 2, 3])
    assert fn(ctypes.byref(d), ws, need + 4096, None) == -1 and b"256 tokens" in _lib.lib().mpv_last_error()
    # the host table: fill refuses a zero key, a key twice and a capacity that is no power of two above the entries
    fill = _lib.lib().mpv_cider_table_fill
    tk, ti = torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.float64)
    k, v = torch.tensor([5, 9, 5]), torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    assert fill(k.data_ptr(), v.data_ptr(), 3, tk.data_ptr(), ti.data_ptr(), 8) < 0 and b"twice" in _lib.lib().mpv_last_error()
    assert fill(k.data_ptr(), v.data_ptr(), 2, tk.data_ptr(), ti.data_ptr(), 6) < 0
    assert fill(k.data_ptr(), v.data_ptr(), 2, tk.data_ptr(), ti.data_ptr(), 2) < 0
    assert fill(torch.tensor([0]).data_ptr(), v.data_ptr(), 1, tk.data_ptr(), ti.data_ptr(), 8) < 0
    assert fill(k.data_ptr(), v.data_ptr(), 2, tk.data_ptr(), ti.data_ptr(), 8) == 0
    look = _lib.lib().mpv_cider_table_lookup
    assert ti[look(tk.data_ptr(), 8, 5)] == 1.0 and ti[look(tk.data_ptr(), 8, 9)] == 2.0 and look(tk.data_ptr(), 8, 7) == -1 and look(tk.data_ptr(), 8, 0) == -1
    assert look(tk.data_ptr(), 8, 5) == rc.mix(5) & 7 and look(tk.data_ptr(), 8, 9) in (rc.mix(9) & 7, (rc.mix(9) + 1) & 7)     # splitmix64's finaliser


def test_ctypes_descriptor_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    cname, ct = "mpv_caption_cider_desc", _lib.CaptionCiderDesc
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


def test_cider_kernels_have_no_scratch_and_the_lds_they_state():
    """cc_rows / cc_pairs / cc_scores in the gfx950 code object: one wave per workgroup for the first two, no scratch anywhere;
    cc_pairs holds the reference's keys and weights (4 x 255 x 16 bytes) in LDS.  Register, LDS and scratch figures only, read the
    way tests/test_isa_cpu.py reads them."""
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
                for key in ("cc_rows", "cc_pairs", "cc_scores"):
                    if key in name:
                        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
                        found[key] = dict(vgpr=g("vgpr_count"), scratch=g("private_segment_fixed_size"), lds=g("group_segment_fixed_size"),
                                          threads=g("max_flat_workgroup_size"))
    print(f"    {found}")
    assert set(found) == {"cc_rows", "cc_pairs", "cc_scores"}
    assert found["cc_pairs"] == dict(found["cc_pairs"], scratch=0, lds=4 * 255 * 16, threads=64)
    assert found["cc_rows"] == dict(found["cc_rows"], scratch=0, lds=260 * 2 + 256 * 8, threads=64)
    assert found["cc_scores"] == dict(found["cc_scores"], scratch=0, lds=0)


# ------------------------------------------------------------------------------------------------ self-critical training on the stand-ins
def test_scst_loss_and_gradients_on_standins(monkeypatch):
    tg.scst_loss_and_gradients(_on_cpu(monkeypatch))
    assert sc.calls


def test_scst_identical_samples_give_exactly_zero_on_standins(monkeypatch):
    tg.scst_identical_samples_give_zero(_on_cpu(monkeypatch))


def test_scst_same_seed_on_standins(monkeypatch):
    tg.scst_same_seed_same_bits(_on_cpu(monkeypatch))


def test_scst_refusals_come_before_any_launch(monkeypatch):
    """N = 1 with "mean_others", mixed prompt lengths, a clip without references, a bad baseline, no CiderStats, a rollout table of the
    wrong shape: ValueError, and neither the encoder, the sampler nor the reward was reached"""
    import types
    dev = _on_cpu(monkeypatch)
    model, cfg, term, video, text, table, gen, refs, stats = tg.scst_setup(dev)
    ran = []
    monkeypatch.setattr(model, "_query_features", lambda *a, **k: ran.append("encode"))
    monkeypatch.setattr(model.text_decoder, "sample_batched", lambda *a, **k: ran.append("sample"))
    del sc.calls[:]
    mixed = types.SimpleNamespace(input_ids=text.input_ids, attention_mask=text.attention_mask.clone())
    mixed.attention_mask[1, :] = 1
    ok = dict(cider=stats, num_samples=tg.N, termination_id=term)
    for t, r, kw, word in ((text, refs, dict(ok, num_samples=1), "mean_others"), (mixed, refs, ok, "prompt length"),
                           (text, [refs[0], []], ok, "no references"), (text, refs[:1], ok, "reference lists"),
                           (text, refs, dict(ok, baseline="median"), "baseline"), (text, refs, dict(ok, cider=None), "CiderStats"),
                           (text, refs, dict(ok, rollouts=table[:, :tg.PL]), "rollouts"), (text, refs, dict(ok, rollouts=table[:-1]), "rollouts"),
                           (text, [refs[0], [list(range(8, 264))]], ok, "255"), (text, refs, dict(ok, max_new_tokens=0), "no room"), (text, refs, dict(ok, num_samples=0), "at least 1")):
        with pytest.raises(ValueError, match=word):
            model.forward_scst(video, t, r, **kw)
    assert not ran and not sc.calls


def test_scst_refuses_a_foreign_vocabulary_and_a_pass_beyond_the_gemm_operand_limit(monkeypatch):
    """statistics built for fewer ids than the decoder draws from (the kernel's 16-bit key fields would alias), and a call whose one
    training pass needs a GEMM operand of 2 GiB or more: ValueError before any launch.  The operand rule at the 1.3B dims: 32 clips x
    16 samples at 30 tokens (the MLP's activation) and 16 clips at 100 tokens (the window's logits) are refused, 16 / 8 clips pass"""
    from youku_mplug_amd import generation
    dev = _on_cpu(monkeypatch)
    model, cfg, term, video, text, table, gen, refs, stats = tg.scst_setup(dev)
    ran, n0 = [], len(sc.calls)
    monkeypatch.setattr(model, "_query_features", lambda *a, **k: ran.append("encode"))
    small = generation.CiderStats(refs, cfg.vocab - 1)
    with pytest.raises(ValueError, match="vocabulary"):
        model.forward_scst(video, text, refs, cider=small, num_samples=tg.N, termination_id=term)
    monkeypatch.setattr(model, "SCST_MAX_OPERAND_BYTES", 1 << 16)
    with pytest.raises(ValueError, match="larger than 2 GiB"):
        model.forward_scst(video, text, refs, cider=stats, num_samples=tg.N, termination_id=term)
    assert not ran and len(sc.calls) == n0
    limit = type(model).SCST_MAX_OPERAND_BYTES
    worst = lambda clips, tokens: max(clips * 16 * (256 + 8 + tokens) * 8192, clips * 16 * tokens * 51200) * 2
    assert worst(32, 30) >= limit > worst(16, 30) and worst(16, 100) >= limit > worst(8, 100)


def test_scst_step_refuses_a_batch_whose_prompts_differ_in_length(monkeypatch):
    """the entry point's --scst step is ONE forward_scst call: with a non-empty prompt the tokenizer shortens the prompt of an over-long
    pair, the batch then holds two prompt lengths, and the step is refused before anything runs (the backward kernels overwrite .grad:
    a step cannot be the sum of several calls); the same captions at one prompt length go through to the encoder"""
    import argparse
    import types
    import test_entrypoint_gpu as t
    dev = _on_cpu(monkeypatch)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    model, cfg, term, video, text, table, gen, refs, stats = tg.scst_setup(dev)
    tok = entry.ft.SyntheticTextTokenizer(cfg.vocab)
    caps = ["\u4e00\u4e01", "\u4e02\u4e03\u4e04\u4e05\u4e06\u4e07"]                        # 2 and 6 characters
    s = types.SimpleNamespace(model=model, tokenizer=tok, device=dev)
    loader = types.SimpleNamespace(dataset=types.SimpleNamespace(fields=lambda i: (caps[i],), n=len(caps)))
    args = argparse.Namespace(max_length=10, scst=True)
    enc = tok([["\u4e10\u4e11\u4e12\u4e13", c] for c in caps], padding="max_length", truncation=True, max_length=10)
    assert enc["prompt_lengths"].tolist() == [4, 2]                                          # the over-long pair lost half its prompt
    reached = []
    monkeypatch.setattr(model, "_query_features", lambda *a, **k: reached.append("encode") or (_ for _ in ()).throw(KeyboardInterrupt))
    step = entry.scst_step_fn(args, {"prompt": "\u4e10\u4e11\u4e12\u4e13"}, s, loader)
    with pytest.raises(ValueError, match="one prompt length per call"):
        step((video[:2].float(), caps))
    assert not reached
    with pytest.raises(KeyboardInterrupt):                                                   # one length: the call gets as far as the encoder
        step((video[:2].float(), [caps[0], caps[0][::-1]]))
    assert reached == ["encode"]


# ------------------------------------------------------------------------------------------------ the entry point
def test_corpus_cider_on_the_standin(monkeypatch):
    tg.corpus_cider_equals_the_golden(_on_cpu(monkeypatch))


def test_entry_point_flags_parse_and_are_absent_by_default(tmp_path):
    import test_entrypoint_gpu as t
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    base = ["--config", cfg, "--output_dir", str(tmp_path / "out"), "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7"]
    names = ("scst", "scst_samples", "scst_baseline", "scst_temperature", "scst_stats")
    args0 = entry.get_args(base)[0]
    assert not any(hasattr(args0, n) for n in names)                     # without the flags the namespace is the one before them
    args = entry.get_args(base + ["--scst", "--scst_samples", "4", "--scst_baseline", "greedy", "--scst_temperature", "0.7", "--scst_stats", "x.pt"])[0]
    assert (args.scst, args.scst_samples, args.scst_baseline, args.scst_temperature, args.scst_stats) == (True, 4, "greedy", 0.7, "x.pt")
    assert {k: v for k, v in vars(args).items() if k not in names} == vars(args0)
    assert vars(entry.get_args(base + ["--scst"])[0]) == dict(vars(args0), scst=True)
    for bad in (["--scst_samples", "4"], ["--scst", "--scst_samples", "1"], ["--scst", "--scst_temperature", "0"]):
        with pytest.raises(ValueError, match="scst"):
            entry.get_args(base + bad)
    with pytest.raises(SystemExit):
        entry.get_args(base + ["--scst", "--scst_baseline", "median"])
    assert entry.get_args(base + ["--scst", "--scst_samples", "1", "--scst_baseline", "greedy"])[0].scst_samples == 1


def test_entry_point_scst_training_loop_on_standins(tmp_path, monkeypatch):
    """--scst --synthetic_steps 2: the loop runs forward_scst (statistics from the synthetic training captions), logs loss_scst, and
    an evaluation on a CPU run leaves CIDEr out and says so"""
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
    monkeypatch.setenv("MASTER_PORT", str(52000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    seen = []
    plain = downstream.DistributedGPT3_Caption.forward_scst

    def spy(self, *a, **kw):
        out = plain(self, *a, **kw)
        seen.append((kw, out[1]))
        return out
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "forward_scst", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    base = ["--config", cfg, "--output_dir", str(tmp_path / "scst"), "--bf16", "--enable_deepspeed", "--synthetic_steps", "2", "--seed", "7"]
    try:
        del sc.calls[:]
        stats = entry.main(*entry.get_args(base + ["--scst", "--scst_samples", "3", "--scst_temperature", "1.5"]))
        assert len(seen) >= 2 and sc.calls and all(kw["num_samples"] == 3 and kw["baseline"] == "mean_others" and kw["temperature"] == 1.5 for kw, _ in seen)
        assert all(0.0 <= st["terminated"] <= 1.0 and st["reward"] >= 0.0 for _, st in seen)
        assert math.isfinite(stats["train_loss_scst"])
        del seen[:]
        res = entry.main(*entry.get_args(base + ["--evaluate_only"]))
        assert not seen and "val_CIDEr" not in res and "a CPU run" in res["val_scorer"]
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
