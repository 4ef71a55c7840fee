"""Query-max search without a GPU: the torch stand-in against a loop-written fp64 definition, the C ABI of the built library (symbols,
struct layout, host-side refusals), MaxSimIndex on the stand-in, the zero-shot tool end to end on stand-ins, and the seed choice of
the GPU test's random-unit-row case."""
import ctypes
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maxsim_cases as mc                      # noqa: E402
import standin_maxsim_search as sm             # noqa: E402

import youku_mplug_amd  # noqa: E402,F401


def _loop_scores(q, g):
    """s(i, j) by the definition, in Python floats (fp64): max over the row pairs, NaN products skipped, NaN when all are NaN"""
    q3 = q if q.dim() == 3 else q[:, None]
    g3 = g if g.dim() == 3 else g[:, None]
    out = [[float("nan")] * g3.shape[0] for _ in range(q3.shape[0])]
    for i in range(q3.shape[0]):
        for j in range(g3.shape[0]):
            best = None
            for a in q3[i].double():
                for b in g3[j].double():
                    p = float((a * b).sum())
                    if p == p and (best is None or p > best):
                        best = p
            if best is not None:
                out[i][j] = best
    return out


def _loop_topk(s, k, scale):
    vals, idx = [], []
    for row in s:
        cand = sorted((j for j, v in enumerate(row) if v == v), key=lambda j: (-row[j] * scale, j))[:k]
        vals.append([row[j] * scale for j in cand] + [float("-inf")] * (k - len(cand)))
        idx.append(cand + [-1] * (k - len(cand)))
    return vals, idx


def _loop_rank(s, target):
    out = []
    for row, ts in zip(s, target.tolist()):
        best = len(row)
        for t in ts:
            if 0 <= t < len(row) and row[t] == row[t]:
                best = min(best, sum(1 for g, v in enumerate(row) if v > row[t] or (v == row[t] and g < t)))
        out.append(best)
    return out


@pytest.mark.parametrize("side", ["g", "q", "none"])
def test_standin_equals_the_loop_definition(side):
    group = None if side == "none" else 3
    q = mc.exact_features(5, group if side == "q" else None, 32, 1).clone()
    g = mc.exact_features(7, group if side == "g" else None, 32, 2).clone()
    if side == "g":                            # one NaN row in item 0, item 1 all NaN
        g[0, 1] = float("nan")
        g[1] = float("nan")
    if side == "q":
        q[0, 1] = float("nan")
        g[1] = float("nan")
    s = _loop_scores(q, g)
    for k, scale in ((3, 1.0), (7, 0.5), (9, 2.0)):                 # 9 > ng: the tail is (-inf, -1)
        vals, idx = sm.maxsim_topk(q, g, k, scale=scale)
        wv, wi = _loop_topk(s, k, scale)
        assert idx.tolist() == wi and vals.double().tolist() == wv
    t = torch.tensor([[1, -1], [0, 3], [7, -1], [2, 2], [6, 1]])
    assert sm.maxsim_rank(q, g, t).tolist() == _loop_rank(s, t)
    assert sm.maxsim_rank(q, g, t)[2] == 7                         # no valid target
    assert side == "none" or sm.maxsim_rank(q, g, t)[0] == 7       # a NaN target counts as no target
    flat = [v for row in s for v in row if v == v]
    assert len(set(flat)) < len(flat)                               # the exact data does tie


def test_standin_tie_rule_and_refusals():
    from youku_mplug_amd._lib import MpvError
    z = torch.zeros(32)
    e = z.clone()
    e[0] = 1
    g = torch.stack([torch.stack([z, .5 * e]), torch.stack([.5 * e, z]), torch.stack([.25 * e, z])]).to(torch.bfloat16)
    q = e[None].to(torch.bfloat16)
    vals, idx = sm.maxsim_topk(q, g, 2)
    assert idx.tolist() == [[0, 1]] and vals.tolist() == [[.5, .5]]
    assert sm.maxsim_rank(q, g, torch.tensor([[1]])).tolist() == [1]
    for bad in (lambda: sm.maxsim_topk(q, g, 0), lambda: sm.maxsim_topk(q, g, 33), lambda: sm.maxsim_topk(q.float(), g, 1),
                lambda: sm.maxsim_topk(q[None].expand(1, 2, 32), g, 1),                       # both sides grouped
                lambda: sm.maxsim_topk(q[:, :16], g[:, :, :16], 1),                           # dim 16
                lambda: sm.maxsim_topk(q, g[:0], 1), lambda: sm.maxsim_rank(q, g, torch.tensor([[1]], dtype=torch.int32)),
                lambda: sm.maxsim_rank(q, g, torch.zeros((1, 33), dtype=torch.long)),
                lambda: sm.maxsim_topk(q, torch.zeros((1, 1025, 32), dtype=torch.bfloat16), 1)):
        with pytest.raises(MpvError):
            bad()


def test_unit_row_seed_can_be_chosen_on_the_cpu():
    seed = mc.pick_seed()
    assert seed is not None and seed in mc.SEEDS


# ------------------------------------------------------------------------------------------------ C ABI
SYMBOLS = ("mpv_maxsim_topk", "mpv_maxsim_rank", "mpv_maxsim_topk_workspace_size", "mpv_maxsim_rank_workspace_size")


def test_maxsim_search_desc_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    body = re.search(r"typedef struct mpv_maxsim_search_desc \{(.*?)\} mpv_maxsim_search_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    ct = _lib.MaxSimSearchDesc
    assert names == [f[0] for f in ct._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpv.h"', 'int main(void) {',
            '  printf("%zu", sizeof(mpv_maxsim_search_desc));'] + \
           [f'  printf(" %zu", offsetof(mpv_maxsim_search_desc, {n}));' for n in names] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    tok = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert tok[0] == ctypes.sizeof(ct)
    assert tok[1:] == [getattr(ct, f[0]).offset for f in ct._fields_]
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s


def test_maxsim_symbols_are_exported_and_refuse_bad_descriptors():
    """descriptor checks run on the host before any launch, so they can be exercised without a GPU"""
    from youku_mplug_amd import _lib
    lib = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.EXPORTS and getattr(lib, s) is not None
    d = _lib.MaxSimSearchDesc()
    d.queries = d.gallery = 4096
    d.q_rs = d.g_rs = d.dim = 256
    d.nq, d.ng, d.k, d.scale, d.q_group, d.g_group = 3, 1000, 10, 1.0, 1, 256
    assert lib.mpv_maxsim_topk_workspace_size(ctypes.byref(d)) > 0
    d.slices = 3
    assert lib.mpv_maxsim_topk_workspace_size(ctypes.byref(d)) >= 2 * 3 * 3 * 10 * 4
    assert lib.mpv_maxsim_rank_workspace_size(ctypes.byref(d), 4) >= 2 * 3 * 4 * 4
    assert lib.mpv_maxsim_rank_workspace_size(ctypes.byref(d), 33) == 0
    d.q_group, d.g_group = 40, 1
    assert lib.mpv_maxsim_topk_workspace_size(ctypes.byref(d)) > 0
    out = ctypes.create_string_buffer(1024)
    addr = ctypes.addressof(out)
    for field, bad in (("dim", 48), ("dim", 2048), ("k", 0), ("k", 33), ("g_rs", 252), ("q_rs", 128), ("ng", 0), ("nq", 0),
                       ("g_group", 2),                  # both groups above 1
                       ("q_group", 0), ("q_group", 1025), ("g_group", 0), ("nq", (1 << 31) // 40 + 1), ("ng", 1 << 31),
                       ("slices", -1), ("slices", 4097), ("queries", 4104)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        assert lib.mpv_maxsim_topk(ctypes.byref(d), addr, addr, addr, 1 << 30, None) < 0, (field, bad)
        assert lib.mpv_maxsim_topk_workspace_size(ctypes.byref(d)) == 0, (field, bad)
        if field != "k":
            assert lib.mpv_maxsim_rank(ctypes.byref(d), addr, 1, addr, addr, 1 << 30, None) < 0, (field, bad)
            assert lib.mpv_maxsim_rank_workspace_size(ctypes.byref(d), 1) == 0, (field, bad)
        assert lib.mpv_last_error()
        setattr(d, field, keep)
    assert lib.mpv_maxsim_topk(ctypes.byref(d), addr, addr, addr, 8, None) == -5            # workspace too small: MPV_E_ARG
    assert lib.mpv_maxsim_rank(ctypes.byref(d), addr, 1, addr, addr, 8, None) == -5
    assert lib.mpv_maxsim_rank(ctypes.byref(d), addr, 0, addr, addr, 1 << 30, None) == -5   # n_targets out of range


# ------------------------------------------------------------------------------------------------ index and tool on stand-ins
def test_maxsim_index_growth_and_refusals(monkeypatch):
    sm.install(monkeypatch)
    from youku_mplug_amd._lib import MpvError
    from youku_mplug_amd.retrieval import MaxSimIndex
    clips = mc.unit_rows(11, 5, 32, 1)
    titles = mc.unit_rows(7, None, 32, 2)
    vi = MaxSimIndex(32, 5, device="cpu", capacity=2)
    assert vi.add(clips[:3]) == 0 and vi.capacity >= 3 and vi.add(clips[3:4]) == 3
    cap = vi.capacity
    assert vi.add(clips[4:]) == 4 and len(vi) == 11 and vi.capacity >= 11 and vi.capacity != cap
    assert torch.equal(vi.features, clips)
    ti = MaxSimIndex(32, device="cpu", capacity=1)
    ti.add(titles[:4])
    ti.add(titles[4:, None, :])                                      # [n, 1, dim] is accepted by a group == 1 index
    assert torch.equal(ti.features[:, 0], titles)
    v, i = vi.search(titles, 3, scale=2.0)
    wv, wi = sm.maxsim_topk(titles, clips, 3, scale=2.0)
    assert torch.equal(i, wi) and torch.equal(v, wv)
    v, i = ti.search(clips, 9)                                       # grouped queries against single rows; k > size
    assert (i[:, 7:] == -1).all() and torch.equal(i, sm.maxsim_topk(clips, titles, 9)[1])
    assert torch.equal(vi.rank(titles, [0, 1, 2, 3, 4, 5, -1]), sm.maxsim_rank(titles, clips, torch.tensor([0, 1, 2, 3, 4, 5, -1])))
    assert torch.equal(ti.rank(clips, torch.arange(11) % 7), sm.maxsim_rank(clips, titles, torch.arange(11) % 7))
    for bad in (lambda: MaxSimIndex(48), lambda: MaxSimIndex(32, 0), lambda: MaxSimIndex(32, 1025),
                lambda: vi.add(clips.float()), lambda: vi.add(clips[:, :4]), lambda: vi.add(titles), lambda: vi.add(clips[:, :, :16]),
                lambda: vi.search(clips, 3),                         # grouped queries against a grouped index
                lambda: vi.search(titles, 0), lambda: vi.search(titles, 33), lambda: vi.rank(titles, [11] * 7),
                lambda: MaxSimIndex(32, 5, device="cpu").search(titles, 1)):
        with pytest.raises(MpvError):
            bad()


def _tool():
    spec = importlib.util.spec_from_file_location("zero_shot_retrieval", os.path.join(ROOT, "tools", "zero_shot_retrieval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_zero_shot_tool_synthetic_end_to_end_on_standins(monkeypatch, capsys):
    import standin_contrastive
    sm.install(monkeypatch)
    if hasattr(standin_contrastive, "install"):
        standin_contrastive.install(monkeypatch)
        sm.install(monkeypatch)
    tool = _tool()
    result = tool.main(["--synthetic", "6", "--batch_size", "4", "--device", "cpu", "--seed", "5"])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    assert json.loads(line) == result
    # the same features through the entry point's itm_eval on the stand-in's score matrices
    entry = tool._entry()
    model, split, tok, max_length = tool.synthetic_setup(6, 4, torch.device("cpu"), 5)
    vi, ti = tool.build_indexes(model, split, tok, torch.device("cpu"), max_length)
    assert vi.features.shape[:2] == (6, model.num_learnable_token) and ti.features.shape[:2] == (6, 1)
    norms = vi.features.float().norm(dim=-1)
    assert torch.allclose(norms, torch.ones_like(norms), atol=1e-2)
    v2t = sm.item_scores(vi.features, ti.features[:, 0]).numpy()
    t2v = sm.item_scores(ti.features[:, 0], vi.features).numpy()
    rv, rt = tool.zero_shot_ranks(model, split, tok, torch.device("cpu"), max_length)
    assert rv.tolist() == sm.rank_of(torch.from_numpy(v2t), torch.arange(6)[:, None]).tolist()
    assert result == entry.recall_from_ranks(rv, rt)
    if all(len(np.unique(r)) == len(r) for m in (v2t, t2v) for r in m):          # itm_eval's argsort is only defined without ties
        assert result == entry.itm_eval(v2t, t2v, split.txt2vid, split.vid2txt)


def test_pretrain_model_without_the_head_refuses():
    from oracle.weights import CONFIG_TINY
    from youku_mplug_amd.pretrain import synthetic_model
    model = synthetic_model(CONFIG_TINY, device="cpu")
    with pytest.raises(RuntimeError, match="use_contrastive"):
        model.extract_text_feature(None)
    with pytest.raises(RuntimeError, match="use_contrastive"):
        model.extract_vision_feature(torch.zeros(1))
