"""Scoring of given captions, checked without a GPU: mpv_attn_prefix_packed_layout through the C ABI against a
Python restatement, the refusals of the two new entry points on the host, the ctypes mirror of the descriptor, the compiler's resource
figures of the new attention kernel; DistributedGPT3_Caption.score_captions on the stand-ins (tests/standin_prefix_packed.py) against the
fp32 restatement's teacher-forced log-probabilities and against the padded forward_continuation, its shapes, order, chunking, `best`,
score_termination and errors; the anchor to the reference module's golden; the entry point's flag."""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import caption_score_cases as cs
import standin_prefix_packed

ROOT = cs.ROOT


# ------------------------------------------------------------------------------ the layout function through the ABI
def _layout(cont_len, per_group):
    from youku_mplug_amd import _lib
    I = ctypes.c_int32
    seg, grp = (I * max(sum(max(x, 0) for x in cont_len), 1))(), (I * (len(per_group) + 1))()
    rows, mgr = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.lib().mpv_attn_prefix_packed_layout((I * max(len(cont_len), 1))(*cont_len), len(cont_len), (I * max(len(per_group), 1))(*per_group),
                                                  len(per_group), seg, grp, ctypes.byref(rows), ctypes.byref(mgr))
    return rc, list(seg[:max(rows.value, 0)]), list(grp), rows.value, mgr.value


@pytest.mark.parametrize("lay", cs.LAYOUTS, ids=cs.layout_id)
def test_layout_function_equals_its_restatement(lay):
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import ops
    rc, seg, grp, rows, mgr = _layout(*lay)
    assert rc == 0 and (seg, grp, rows, mgr) == cs.layout_restated(*lay)
    assert all(s <= r for r, s in enumerate(seg)) and grp[0] == 0 and grp[-1] == rows == sum(lay[0])
    pl = ops.PackedLayout(*lay)                                              # no device: host lists only
    assert (pl.seg_start_host, pl.group_row_host, pl.rows, pl.max_group_rows) == (seg, grp, rows, mgr) and pl.seg_start is None
    assert pl.pos_in_cont == [p for n in lay[0] for p in range(n)]
    dv = ops.PackedLayout(*lay, device="cpu")
    assert dv.seg_start.dtype == torch.int32 and dv.seg_start.tolist() == seg and dv.group_row.tolist() == grp


@pytest.mark.parametrize("bad", [([3, 0, 2], [3]), ([3, -1], [2]), ([3, 2], [1]), ([3, 2], [2, 1]), ([3, 2], [2, 0]), ([3, 2], [0, 2]), ([], [])],
                         ids=["zero-length", "negative-length", "counts-short", "counts-long", "empty-last-group", "empty-first-group", "nothing"])
def test_layout_function_refuses(bad):
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib, ops
    rc, _, _, rows, mgr = _layout(*bad)
    assert rc < 0 and (rows, mgr) == (-1, -1) and b"mpv_attn_prefix_packed_layout" in _lib.lib().mpv_last_error()
    with pytest.raises(_lib.MpvError, match="mpv_attn_prefix_packed_layout"):
        ops.PackedLayout(*bad)


def test_layout_function_refuses_too_many_rows():
    """refused before anything is written: one-element output buffers are enough"""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib, ops
    I = ctypes.c_int32
    seg, grp, rows, mgr = (I * 1)(-5), (I * 2)(-5, -5), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.lib().mpv_attn_prefix_packed_layout((I * 2)(1 << 29, 1 << 29), 2, (I * 1)(2), 1, seg, grp, ctypes.byref(rows), ctypes.byref(mgr))
    assert rc < 0 and (rows.value, mgr.value, seg[0], list(grp)) == (-1, -1, -5, [-5, -5])
    with pytest.raises(_lib.MpvError, match="2\\^30"):
        ops.PackedLayout([1 << 29, 1 << 29], [2])


# ------------------------------------------------------------------------------ the library on the host
def _desc(**over):
    from youku_mplug_amd import _lib
    d = _lib.AttnPrefixPackedDesc()
    ok = dict(q=0x10000, k=0x20000, v=0x30000, pk=0x40000, pv=0x50000, o=0x60000, seg_start=0x70000, group_row=0x80000,
              q_rs=192, q_hs=64, k_rs=192, k_hs=64, v_rs=192, v_hs=64, o_rs=64, o_hs=64, pk_gs=1920, pk_hs=64, pk_rs=192, pv_gs=1920, pv_hs=64,
              pv_rs=192, rows=40, n_groups=2, heads=1, prefix_len=10, head_dim=64, max_group_rows=30, scale=0.125)
    for k, v in {**ok, **over}.items():
        setattr(d, k, v)
    return d


REFUSALS = [dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(pk=None), dict(pv=None), dict(seg_start=None), dict(group_row=None),
            dict(head_dim=96), dict(head_dim=128), dict(head_dim=0), dict(rows=0), dict(rows=-2), dict(n_groups=0), dict(heads=0), dict(prefix_len=-1),
            dict(max_group_rows=0), dict(max_group_rows=41), dict(q_rs=196), dict(k_hs=68), dict(v_rs=100), dict(pk_rs=4), dict(pv_gs=1921),
            dict(o_rs=66), dict(o_hs=2), dict(q=0x10008), dict(pk=0x40002), dict(o=0x60004), dict(scale=0.0), dict(scale=-1.0)]


def test_library_exports_the_symbols_and_refuses_on_the_host():
    """every refusal of include/mpv.h comes back negative before anything is launched (the pointers are not memory: a launch would fault)"""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mpv_attn_prefix_packed_fwd", "mpv_attn_prefix_packed_layout", "mpv_gpt_embed_rows_fwd"):
        assert name in _lib.EXPORTS and hasattr(raw, name)
    fn = _lib.lib().mpv_attn_prefix_packed_fwd
    for over in REFUSALS:
        assert fn(ctypes.byref(_desc(**over)), None) < 0, over
        assert b"mpv_attn_prefix_packed_fwd" in _lib.lib().mpv_last_error()
    assert fn(None, None) < 0
    emb = _lib.lib().mpv_gpt_embed_rows_fwd
    ok = dict(ids=0x1000, pos=0x2000, wte=0x3000, wpe=0x4000, out=0x5000, rows=4, H=160, max_positions=64)
    for over in (dict(ids=None), dict(pos=None), dict(wte=None), dict(wpe=None), dict(out=None), dict(rows=0), dict(rows=-1), dict(H=164), dict(H=0),
                 dict(max_positions=0)):
        a = {**ok, **over}
        assert emb(a["ids"], a["pos"], a["wte"], a["wpe"], a["out"], a["rows"], a["H"], a["max_positions"], None) < 0, over
        assert b"mpv_gpt_embed_rows_fwd" in _lib.lib().mpv_last_error()


def test_embed_rows_checks_the_positions_on_the_host():
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib, ops
    wte, wpe = torch.zeros(8, 16, dtype=torch.bfloat16), torch.zeros(12, 16, dtype=torch.bfloat16)
    ids, pos = torch.zeros(3, dtype=torch.long), torch.tensor([0, 11, 12], dtype=torch.int32)
    with pytest.raises(_lib.MpvError, match="max_position_embeddings = 12"):
        ops.gpt_embed_rows_fwd(ids, pos, [0, 11, 12], wte, wpe, 3, 16)
    with pytest.raises(_lib.MpvError, match="host positions"):
        ops.gpt_embed_rows_fwd(ids, pos, [0, 11], wte, wpe, 3, 16)


def test_ctypes_descriptor_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    cname, ct = "mpv_attn_prefix_packed_desc", _lib.AttnPrefixPackedDesc
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in ct._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpv.h"', 'int main(void) {', f'  printf("%zu", sizeof({cname}));']
    prog += [f'  printf(" %zu", offsetof({cname}, {n}));' for n in names] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    tok = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert tok[0] == ctypes.sizeof(ct) and tok[1:] == [getattr(ct, f[0]).offset for f in ct._fields_]


def test_packed_attention_kernel_has_no_scratch_and_fits_two_workgroups_per_cu():
    """attn_prefix_fwd_kernel<64 / 80, uniform / packed> in the gfx950 code object ("Merged"): the one kernel body behind
    mpv_attn_prefix_fwd and mpv_attn_prefix_packed_fwd, four instances and no second prefix kernel.  No scratch; 52 KiB of LDS (two buffers
    of 64-row K and V chunks at a 208-byte pitch), of which two fit the CU's 160 KiB; each instance inside the register tier it had before
    the two kernels became one: at most 168 registers (three waves per SIMD) for both hd-64 instances and packed hd-80, at most 256 (two
    waves, launch_bounds(256, 2)) for uniform hd-80.  Register, LDS and scratch figures only, read the way tests/test_isa_cpu.py reads
    them."""
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
                if "attn_prefix" in name:
                    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                    found[name] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), scratch=g("private_segment_fixed_size"),
                                       lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    # template arguments as the Itanium mangling spells them: Li<head_dim>E, Lb<packed>E
    tier = {"attn_prefix_fwd_kernelILi64ELb0EE": 168, "attn_prefix_fwd_kernelILi64ELb1EE": 168, "attn_prefix_fwd_kernelILi80ELb1EE": 168,
            "attn_prefix_fwd_kernelILi80ELb0EE": 256}
    assert len(found) == 4 and all(sum(t in n for n in found) == 1 for t in tier), sorted(found)   # every prefix kernel is one of the four
    for n, k in found.items():
        print(f"    {n}: {k}")
        regs = next(v for t, v in tier.items() if t in n)
        assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= regs and k["lds"] == 4 * 64 * 208 and 2 * k["lds"] <= 160 * 1024 and k["threads"] == 256, (n, k)


# ------------------------------------------------------------------------------ the host pipeline on the stand-ins
def _on_cpu(monkeypatch):
    import test_pipeline_cpu as tp
    dev = tp._on_cpu(monkeypatch)
    standin_prefix_packed.install(monkeypatch)
    return dev


SEL = [0, 1, 0, 1, 0]                     # two prompt lengths (5 and 3 tokens) in one call
COUNTS = [3, 1, 0, 3, 1]                  # 0 / 1 / 3 candidates per clip


def _setup(monkeypatch):
    dev = _on_cpu(monkeypatch)
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    term = g["meta"]["eod_id"]
    cands = cs.ragged_candidates(cfg, COUNTS, seed=21, avoid=term)
    cands[0][1] = torch.zeros(0, dtype=torch.long)                           # an empty caption: only the terminator is scored
    cands[3][2] = cands[3][2].tolist()                                       # a list instead of a tensor
    return dev, model, cfg, g, sd, video, ids, mask, term, cands


def _restated(video, ids, mask, cands, term, sd, cfg):
    out = []
    for i, (s, cl) in enumerate(zip(SEL, cands)):
        pl = int(mask[s].sum()) - 1
        out.append(cs.restated_logprobs(("pipeline", i), video[s], ids[s, :pl].tolist(), [list(map(int, c)) for c in cl], term, sd, cfg) if cl else [])
    return out


def test_score_captions_on_standins_against_the_restatement_and_the_padded_path(monkeypatch):
    """score_captions against the fp32 restatement's teacher-forced log_softmax (same weights).  Two gates, neither from the code under test
    alone: (a) the deviation from the restatement may be at most 1.5 x the padded forward_continuation's own deviation from it + 1e-6, on
    the same candidates, per token; (b) packed against padded, both on the stand-ins: relative L2 <= 1e-4 over the per-candidate sums, which
    is the gate tests/test_shared_prefix_cpu.py applies and the quantity it applies it to (per-sequence generation scores of a pass whose
    prefix rows come from a pass of their own; the per-token figure is printed: single entries carry the bf16 rounding flips that another
    matmul shape causes on the host BLAS, 1.1e-4 here, which a sum averages).  Both over EVERY clip that has candidates -- one and three per clip,
    both prompt lengths, the first and the last clip of a mixed pass: the padded path takes them one clip at a time."""
    from youku_mplug_amd.downstream import best_sample
    dev, model, cfg, g, sd, video, ids, mask, term, cands = _setup(monkeypatch)
    text = cs.text_of(ids, mask, SEL, dev)
    vid = video[SEL].to(torch.bfloat16)
    res = model.score_captions(vid, text, cands, termination_id=term)
    ref = _restated(video, ids, mask, cands, term, sd, cfg)
    assert len(res) == len(SEL)
    e_packed = 0.0
    for i, (r, cl) in enumerate(zip(res, cands)):                            # input order, shapes, counts, zero padding, sums
        C = len(cl)
        assert set(r) == {"sum_logprob", "count", "token_logprob", "best"} and all(not v.is_cuda for k, v in r.items() if k != "best")
        assert r["sum_logprob"].shape == (C,) and r["sum_logprob"].dtype == torch.float32 and r["count"].shape == (C,) and r["count"].dtype == torch.int32
        if C == 0:
            assert r["best"] is None and r["token_logprob"].shape == (0, 0)
            continue
        lens = [len(c) + 1 for c in cl]
        assert r["count"].tolist() == lens and r["token_logprob"].shape == (C, max(lens)) and r["token_logprob"].dtype == torch.float32
        assert r["best"] == best_sample(r["sum_logprob"], r["count"], 1.0)
        for j, n in enumerate(lens):
            row = r["token_logprob"][j]
            assert (row[:n] < 0).all() and (row[n:] == 0).all()
            acc = 0.0
            for x in row[:n].tolist():
                acc += x
            assert r["sum_logprob"][j].item() == torch.tensor(acc, dtype=torch.float64).to(torch.float32).item()
            e_packed = max(e_packed, (row[:n].double() - ref[i][j]).abs().max().item())
    # (a) + (b): the padded path, one clip at a time, on every clip that has candidates
    e_pk3, e_pad, num, den, s_mine, s_pad = 0.0, 0.0, 0.0, 0.0, [], []
    scored = [i for i, cl in enumerate(cands) if cl]
    assert scored == [0, 1, 3, 4] and sorted(len(cands[i]) for i in scored) == [1, 1, 3, 3]
    for i in scored:
        s, pl = SEL[i], int(mask[SEL[i]].sum()) - 1
        qf = model.encode_video(vid[i:i + 1])
        pad = cs.padded_logprobs(model, qf, text.input_ids[i:i + 1], pl, [cands[i]], term)[0]
        assert len(pad) == len(cands[i])
        for j, lp in enumerate(pad):
            assert len(lp) == int(res[i]["count"][j])
            mine = res[i]["token_logprob"][j, :len(lp)]
            e_pad = max(e_pad, (lp.double() - ref[i][j]).abs().max().item())
            e_pk3 = max(e_pk3, (mine.double() - ref[i][j]).abs().max().item())
            num += ((mine - lp).double() ** 2).sum().item()
            den += (lp.double() ** 2).sum().item()
            s_mine.append(float(res[i]["sum_logprob"][j]))
            s_pad.append(lp.double().sum().item())
    rel_tok = math.sqrt(num / den)
    rel = ((torch.tensor(s_mine) - torch.tensor(s_pad)).norm() / torch.tensor(s_pad).norm()).item()
    print(f"    (per-token relative L2, packed vs padded, not gated: {rel_tok:.3e})")
    print(f"    stand-ins, every clip with candidates: e_packed {e_packed:.3e}, e_padded {e_pad:.3e}, packed vs padded rel L2 {rel:.3e}")
    assert e_pk3 == e_packed                                                 # both loops saw the same entries: nothing is only reported
    assert e_packed <= 1.5 * e_pad + 1e-6 and rel <= 1e-4, (e_packed, e_pad, rel)
    # length_penalty reaches best_sample
    for lp in (0.0, 2.0):
        r2 = model.score_captions(vid, text, cands, termination_id=term, length_penalty=lp)
        assert [r["best"] for r in r2] == [None if r["best"] is None else best_sample(r["sum_logprob"], r["count"], lp) for r in res]


def test_score_captions_chunking_features_and_termination(monkeypatch):
    dev, model, cfg, g, sd, video, ids, mask, term, cands = _setup(monkeypatch)
    from youku_mplug_amd import ops
    text = cs.text_of(ids, mask, SEL, dev)
    vid = video[SEL].to(torch.bfloat16)
    seen = []
    orig_attn, orig_gemm = ops.attn_prefix_packed_fwd, ops.gemm

    def attn(*a, **k):
        seen.append(("attn", a[8].rows, a[8].conts_per_group, a[10]))        # layout, prefix_len
        return orig_attn(*a, **k)

    def gemm(a, b, M, N, K, **k):
        if b is wte:                                                         # the tied LM head
            seen.append(("lm_head", M))
        return orig_gemm(a, b, M, N, K, **k)
    wte = model.text_decoder.dist_model.language_model.embedding.word_embeddings.weight
    monkeypatch.setattr(ops, "attn_prefix_packed_fwd", attn)
    monkeypatch.setattr(ops, "gemm", gemm)
    res = model.score_captions(vid, text, cands, termination_id=term)
    Q = model.num_learnable_token
    rows = {3: sum(len(c) + 1 for i in (1, 3) for c in cands[i]), 5: sum(len(c) + 1 for i in (0, 4) for c in cands[i])}
    # one packed pass per prompt length: no padding row in the attention or in the LM head, clips without candidates left out
    assert [s for s in seen if s[0] == "attn"][::cfg.layers] == [("attn", rows[3], [1, 3], Q + 2), ("attn", rows[5], [3, 1], Q + 4)]
    assert [s[1] for s in seen if s[0] == "lm_head"] == [rows[3], rows[5]]
    monkeypatch.setattr(ops, "attn_prefix_packed_fwd", orig_attn)
    monkeypatch.setattr(ops, "gemm", orig_gemm)
    one = model.score_captions(vid, text, cands, termination_id=term, clips_per_pass=1)
    qf = model.encode_video(vid)
    feat = model.score_captions(None, text, cands, query_features=qf, termination_id=term)
    for a, b, c in zip(res, one, feat):
        for k in ("sum_logprob", "count", "token_logprob"):
            assert torch.equal(a[k], c[k]), k                                    # the same passes on given features: the same bits
        assert a["best"] == c["best"] and torch.equal(a["count"], b["count"])
    # another chunking: other matmul shapes (fp32 summation order of the host BLAS, which flips bf16 roundings).  Two bf16 evaluations of one
    # function differ by at most the sum of their distances from it: the distance of the all-in-one pass from the fp32 restatement, twice
    ref = _restated(video, ids, mask, cands, term, sd, cfg)
    e_all = max((a["token_logprob"][j, :len(r)].double() - r).abs().max().item() for a, rl in zip(res, ref) for j, r in enumerate(rl))
    d_one = max((a["token_logprob"] - b["token_logprob"]).abs().max().item() for a, b in zip(res, one) if a["count"].numel())
    print(f"    clips_per_pass 1 against all: max |difference| {d_one:.3e} <= 2 x {e_all:.3e}")
    assert d_one <= 2 * e_all, (d_one, e_all)
    # score_termination=False drops exactly the last entry of every candidate
    full = [[c for c in cl if len(c)] for cl in cands]
    base = model.score_captions(vid, text, full, termination_id=term)
    cut = model.score_captions(vid, text, full, termination_id=term, score_termination=False)
    for a, b, cl in zip(base, cut, full):
        assert b["count"].tolist() == [len(c) for c in cl]
        for j, c in enumerate(cl):
            assert torch.equal(b["token_logprob"][j, :len(c)], a["token_logprob"][j, :len(c)]) and (b["token_logprob"][j, len(c):] == 0).all()
    # the default terminator is the decoder's eod_id (no tokenizer on this model)
    dflt = model.score_captions(vid, text, cands)
    assert all(torch.equal(a["token_logprob"], b["token_logprob"]) for a, b in zip(res, dflt))


def test_score_captions_errors(monkeypatch):
    from youku_mplug_amd import _lib
    dev, model, cfg, g, sd, video, ids, mask, term, cands = _setup(monkeypatch)
    text = cs.text_of(ids, mask, SEL, dev)
    vid = video[SEL].to(torch.bfloat16)
    qf = model.encode_video(vid)
    with pytest.raises(ValueError, match="exactly one"):
        model.score_captions(vid, text, cands, query_features=qf)
    with pytest.raises(ValueError, match="exactly one"):
        model.score_captions(None, text, cands)
    with pytest.raises(ValueError, match="score_termination=False"):
        model.score_captions(vid, text, cands, score_termination=False)      # cands[0][1] is empty
    with pytest.raises(ValueError, match="clips_per_pass"):
        model.score_captions(vid, text, cands, clips_per_pass=0)
    with pytest.raises(ValueError, match="candidate lists"):
        model.score_captions(vid, text, cands[:-1])
    m0 = mask[SEL].clone()
    m0[2, 1:] = 0                                                            # a prompt of zero tokens
    with pytest.raises(ValueError, match="at least one token"):
        model.score_captions(vid, types.SimpleNamespace(input_ids=ids[SEL], attention_mask=m0), cands)
    with pytest.raises(ValueError, match="query features"):
        model.score_captions(None, text, cands, query_features=qf[:-model.num_learnable_token])
    long = [[torch.ones(cfg.max_pos, dtype=torch.long)]] + [[] for _ in SEL[1:]]
    with pytest.raises(_lib.MpvError, match="max_position_embeddings"):
        model.score_captions(vid, text, long)


# ------------------------------------------------------------------------------ the anchor to the reference module's golden
def golden_anchor(model, cfg, g, sd, video, ids, mask, dev, gate):
    """tests/golden/caption_tiny.pt's fp32 best sequence of each clip, scored teacher-forced.  The beam score is the summed
    log-probability over the ROW length, and the span of that sum is, established with the fp32 restatement below:
    every position from the prompt's end through the ROW'S END (the goldens' best rows hold no termination token: the search ran out of
    positions).  So sum_logprob of the row's generated tokens, scored with score_termination=False, must reproduce golden score x row
    length: to 1e-4 relative for the fp32 restatement, and at `gate` for the model under test.  -> the worst relative deviation."""
    f32 = g["fp32"]
    worst = 0.0
    for i in range(g["meta"]["batch"]):
        seq = f32["sequences"][i][0].tolist()
        pl = int(mask[i].sum()) - 1
        gen = seq[pl:]
        assert g["meta"]["eod_id"] not in gen
        want = f32["scores"][i][0].item() * len(seq)
        lp = cs.restated_logprobs(("anchor", i), video[i], seq[:pl], [gen[:-1]], gen[-1], sd, cfg, weights="fp32")[0]
        e_ref = abs(lp.sum().item() - want) / abs(want)
        res = model.score_captions(video[i:i + 1].to(dev).to(torch.bfloat16), cs.text_of(ids, mask, [i], dev), [[gen]], score_termination=False)[0]
        assert res["count"].tolist() == [len(gen)]
        e = abs(res["sum_logprob"][0].item() - want) / abs(want)
        print(f"    clip {i}: golden score x row length {want:.5f}; fp32 restatement {lp.sum().item():.5f} (rel {e_ref:.2e}); score_captions "
              f"{res['sum_logprob'][0].item():.5f} (rel {e:.2e} <= {gate:.1e})")
        assert e_ref <= 1e-4, (i, e_ref)
        assert e <= gate, (i, e, gate)
        worst = max(worst, e)
    return worst


def test_golden_anchor_on_standins(monkeypatch):
    from test_model_gpu import PLAIN
    dev = _on_cpu(monkeypatch)
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    golden_anchor(model, cfg, g, sd, video, ids, mask, dev, PLAIN["caption_tiny"]["score"])


# ------------------------------------------------------------------------------ the entry point's flag
def test_caption_entrypoint_score_gold_flag_on_standins(tmp_path, monkeypatch):
    """the GPU entry-point test of tests/test_caption_score_gpu.py on CPU / gloo through the stand-ins"""
    import test_caption_score_gpu as e
    import test_entrypoint_gpu as t
    from test_engine_cpu import _stub_optimizer_kernels
    import test_sample_score_cpu as tsc
    orig = t._write_configs

    def write(d, update_freq=1):
        path = orig(d, update_freq)
        cfg = json.load(open(os.path.join(d, "txt.json")))
        cfg.update(hidden_dropout=0.0, attention_dropout=0.0)               # the stand-ins do not model the hash dropout
        json.dump(cfg, open(os.path.join(d, "txt.json"), "w"))
        return path
    monkeypatch.setattr(t, "_write_configs", write)
    _stub_optimizer_kernels(monkeypatch)
    monkeypatch.setenv("MASTER_PORT", str(46000 + os.getpid() % 2000))
    tsc._on_cpu(monkeypatch)
    standin_prefix_packed.install(monkeypatch)
    try:
        base = e.run_entrypoint_with_and_without_the_flag(tmp_path / "a")
        # the flag combines with the other evaluation flags: the same gold scores beside every kind of prediction
        for k, more in enumerate((["--eval_batched_beam", "--eval_sample", "2"], ["--eval_sample_best_of", "3", "--eval_no_repeat_ngram", "2"])):
            got = e.run_entrypoint_with_and_without_the_flag(tmp_path / f"b{k}", more=more)
            assert [(r["gold_logprob"], r["gold_tokens"]) for r in got] == [(r["gold_logprob"], r["gold_tokens"]) for r in base]
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
