"""Retrieval search on CPU: RetrievalIndex, recall_from_ranks and the entry point's `--eval_on_device` evaluation on the torch
stand-ins of the two ops (tests/standin_search.py), on one process and on two gloo ranks; the refusals; the C ABI (header, ctypes
mirror, exported symbols) and the ISA budget of the new object (no scratch, no scalar memory writes)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest
import torch

import standin_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def _entry():
    sys.path.insert(0, os.path.join(ROOT, "downstream"))
    sys.path.insert(0, ROOT)
    import run_retrieval_distributed_gpt3 as entry
    return entry


def _feats(n, dim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=1).to(BF)


# ------------------------------------------------------------------------------------------------ RetrievalIndex
def test_index_grows_geometrically_and_keeps_row_order(monkeypatch):
    standin_search.install(monkeypatch)
    from youku_mplug_amd.retrieval import RetrievalIndex
    rows = _feats(100, 64, 0)
    index = RetrievalIndex(64, device="cpu", capacity=8)
    caps, firsts = [], []
    for lo, hi in ((0, 3), (3, 8), (8, 9), (9, 40), (40, 41), (41, 100)):
        firsts.append(index.add(rows[lo:hi]))
        caps.append(index.capacity)
    assert firsts == [0, 3, 8, 9, 40, 41] and len(index) == 100
    assert caps == [8, 8, 16, 40, 80, 160]                       # doubled (or the needed size), never one allocation per call
    assert torch.equal(index.features, rows)
    vals, idx = index.search(rows[17:19], 3)
    assert idx[:, 0].tolist() == [17, 18] and vals.dtype == torch.float32 and idx.dtype == torch.int64
    assert index.rank(rows[17:19], torch.tensor([17, 18])).tolist() == [0, 0]


def test_index_search_and_rank_follow_the_order_rule(monkeypatch):
    standin_search.install(monkeypatch)
    from youku_mplug_amd.retrieval import RetrievalIndex
    g = torch.zeros(6, 32)
    g[:, 0] = torch.tensor([1., 2., 2., 0., 2., 1.])              # rows 1, 2, 4 tie, rows 0 and 5 tie
    index = RetrievalIndex(32, device="cpu")
    index.add(g.to(BF))
    q = torch.zeros(1, 32)
    q[0, 0] = 1
    vals, idx = index.search(q.to(BF), 8)
    assert idx[0].tolist() == [1, 2, 4, 0, 5, 3, -1, -1]
    assert vals[0, :6].tolist() == [2, 2, 2, 1, 1, 0] and torch.isinf(vals[0, 6:]).all() and (vals[0, 6:] < 0).all()
    assert index.rank(q.to(BF), torch.tensor([[4, -1]])).tolist() == [2]
    assert index.rank(q.to(BF), torch.tensor([[5, 4, 3]])).tolist() == [2]      # the best of several targets
    assert index.rank(q.to(BF), torch.tensor([[-1, -1]])).tolist() == [6]       # no target: worse than every real rank


def test_refusals(monkeypatch):
    standin_search.install(monkeypatch)
    from youku_mplug_amd._lib import MpvError
    from youku_mplug_amd.retrieval import RetrievalIndex
    with pytest.raises(MpvError, match="multiple of 32"):
        RetrievalIndex(48, device="cpu")
    index = RetrievalIndex(64, device="cpu")
    with pytest.raises(MpvError, match="bfloat16"):
        index.add(torch.zeros(2, 64))
    with pytest.raises(MpvError, match=r"\[rows, 64\]"):
        index.add(torch.zeros(2, 32, dtype=BF))
    with pytest.raises(MpvError, match="empty"):
        index.search(_feats(1, 64, 0), 1)
    index.add(_feats(5, 64, 1))
    for k in (0, 33):
        with pytest.raises(MpvError, match="k "):
            index.search(_feats(1, 64, 0), k)
    with pytest.raises(MpvError, match="bfloat16"):
        index.search(_feats(1, 64, 0).float(), 1)
    with pytest.raises(MpvError, match="target rows"):
        index.rank(_feats(2, 64, 0), torch.tensor([0, 5]))
    with pytest.raises(MpvError, match="target rows"):
        index.rank(_feats(2, 64, 0), torch.tensor([0, -2]))


def test_ops_refuse_host_tensors_and_bad_operands():
    """the real wrappers (no stand-in): CUDA tensors only, bf16 only -- checked before the library is touched"""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import ops
    from youku_mplug_amd._lib import MpvError
    with pytest.raises(MpvError, match="GPU only"):
        ops.sim_topk(_feats(1, 64, 0), _feats(4, 64, 1), 1)
    with pytest.raises(MpvError, match="GPU only"):
        ops.sim_rank(_feats(1, 64, 0), _feats(4, 64, 1), torch.tensor([0]))


# ------------------------------------------------------------------------------------------------ recall_from_ranks
def _ranks_by_rule(scores, targets):
    o = standin_search.order(torch.as_tensor(scores))
    return np.array([min(int((o[i] == t).nonzero()[0, 0]) for t in ts) for i, ts in enumerate(targets)])


def test_recall_from_ranks_equals_itm_eval_without_ties():
    entry = _entry()
    rng = np.random.RandomState(0)
    V, T = 23, 40
    s = rng.permutation(V * T).reshape(V, T).astype(np.float32)            # all scores distinct
    img2txt = {v: [t for t in range(T) if t % V == v] for v in range(V)}
    txt2img = {t: t % V for t in range(T)}
    want = entry.itm_eval(s, s.T.copy(), txt2img, img2txt)
    got = entry.recall_from_ranks(_ranks_by_rule(s, [img2txt[v] for v in range(V)]), _ranks_by_rule(s.T.copy(), [[txt2img[t]] for t in range(T)]))
    assert got == want and set(got) == {"txt_r1", "txt_r5", "txt_r10", "txt_r_mean", "vid_r1", "vid_r5", "vid_r10", "vid_r_mean", "r_mean"}


def test_recall_from_ranks_tie_rule():
    """ties go to the lower gallery index: with equal scores everywhere video v's text v has rank v"""
    entry = _entry()
    s = np.zeros((12, 12), dtype=np.float32)
    ranks = _ranks_by_rule(s, [[v] for v in range(12)])
    assert ranks.tolist() == list(range(12))
    got = entry.recall_from_ranks(ranks, ranks)
    assert got["txt_r1"] == pytest.approx(100 / 12) and got["txt_r5"] == pytest.approx(500 / 12) and got["txt_r10"] == pytest.approx(1000 / 12)
    assert got["vid_r1"] == got["txt_r1"] and got["r_mean"] == pytest.approx((100 + 500 + 1000) / 36)


# ------------------------------------------------------------------------------------------------ evaluation on the stand-ins
class _Towers:
    """feature tables behind the model interface `evaluation` uses: title (i,) -> text row i, clip filled with j -> video row j"""

    def __init__(self, V, T, dim, seed):
        self.vf, self.tf = _feats(V, dim, seed), _feats(T, dim, seed + 1)
        self.vf[:, :] = (self.vf.float() + 0.5 * self.tf[torch.arange(V) % T].float()).to(BF)       # a video leans towards its text

    def eval(self):
        return self

    def extract_text_feature(self, text):
        return self.tf[text.input_ids[:, 0]]

    def extract_vision_feature(self, video):
        return self.vf[video[:, 0].long()]


class _Split:
    def __init__(self, V, T, bs):
        self.text = [(t,) for t in range(T)]
        self.txt2vid = {t: t % V for t in range(T)}
        self.vid2txt = {v: [t for t in range(T) if t % V == v] for v in range(V)}
        self.dataset, self.V, self.bs = self, V, bs

    def __iter__(self):
        for lo in range(0, self.V, self.bs):
            ids = torch.arange(lo, min(self.V, lo + self.bs))
            yield ids[:, None].float(), ids


def _both_paths(entry, V=37, T=90, dim=64):
    model, split, tok = _Towers(V, T, dim, 3), _Split(V, T, 8), entry.SyntheticTokenizer()
    cfg = {"max_length": 8}
    v2t, t2v = entry.evaluation(model, split, tok, torch.device("cpu"), cfg)
    want = entry.itm_eval(v2t, t2v, split.txt2vid, split.vid2txt)
    rv, rt = entry.evaluation_on_device(model, split, tok, torch.device("cpu"), cfg)
    return want, rv, rt, v2t


def test_eval_on_device_matches_itm_eval_on_standins(monkeypatch):
    standin_search.install(monkeypatch)
    entry = _entry()
    want, rv, rt, v2t = _both_paths(entry)
    gaps = np.diff(np.sort(v2t, axis=1), axis=1)
    assert gaps.min() > 0                                        # no ties: argsort and the order rule agree
    assert rv.dtype == np.int32 and rv.shape == (37,) and rt.shape == (90,)
    got = entry.recall_from_ranks(rv, rt)
    assert got == want
    assert 0 < got["txt_r1"] < 100                               # the split discriminates: not all hits, not all misses


def test_eval_on_device_flag_defaults_off_and_reaches_main(tmp_path):
    import test_entrypoint_gpu as t
    entry = _entry()
    cfg = t._write_retrieval_config(str(tmp_path))
    args, _ = entry.get_args(["--config", cfg, "--output_dir", str(tmp_path / "o")])
    assert args.eval_on_device is False
    args, _ = entry.get_args(["--config", cfg, "--output_dir", str(tmp_path / "o"), "--eval_on_device"])
    assert args.eval_on_device is True


def _world2_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    import torch.distributed as dist

    class MP:
        def setattr(self, obj, name, val):
            setattr(obj, name, val)
    standin_search.install(MP())
    entry = _entry()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seen = []
    from youku_mplug_amd import ops
    orig = ops.sim_rank
    ops.sim_rank = lambda qf, g, tgt, slices=0: (seen.append((qf.shape[0], g.shape[0])), orig(qf, g, tgt, slices))[1]
    want, rv, rt, _ = _both_paths(entry)
    q.put((rank, want, rv.tolist(), rt.tolist(), seen))
    dist.barrier()
    dist.destroy_process_group()


def test_eval_on_device_world2_gloo(monkeypatch):
    """two gloo ranks: each ranks its share of the queries against the FULL gallery, the int32 rank vectors are all-gathered, and
    both ranks report the single-process result"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 41000 + os.getpid() % 3000
    procs = [ctx.Process(target=_world2_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        r = q.get(timeout=240)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    standin_search.install(monkeypatch)
    entry = _entry()
    want, rv, rt, _ = _both_paths(entry)
    for rank in (0, 1):
        w, v, t, seen = res[rank]
        assert w == want and v == rv.tolist() and t == rt.tolist()
        assert entry.recall_from_ranks(np.array(v), np.array(t)) == want
    assert res[0][3] == [(19, 90), (45, 37)] and res[1][3] == [(18, 90), (45, 37)]       # (queries of this rank, whole gallery)


# ------------------------------------------------------------------------------------------------ C ABI and ISA
SYMBOLS = ("mpv_sim_topk", "mpv_sim_rank", "mpv_sim_topk_workspace_size", "mpv_sim_rank_workspace_size")


def test_sim_search_desc_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    body = re.search(r"typedef struct mpv_sim_search_desc \{(.*?)\} mpv_sim_search_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    ct = _lib.SimSearchDesc
    assert names == [f[0] for f in ct._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpv.h"', 'int main(void) {',
            '  printf("%zu", sizeof(mpv_sim_search_desc));'] + [f'  printf(" %zu", offsetof(mpv_sim_search_desc, {n}));' for n in names] + \
           ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    tok = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert tok[0] == ctypes.sizeof(ct)
    assert tok[1:] == [getattr(ct, f[0]).offset for f in ct._fields_]
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s


def test_sim_search_symbols_are_exported_and_refuse_bad_descriptors():
    """the built library exports the calls; descriptor checks run on the host before any launch, so they can be exercised here"""
    from youku_mplug_amd import _lib
    lib = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.EXPORTS and getattr(lib, s) is not None
    d = _lib.SimSearchDesc()
    d.queries = d.gallery = 4096
    d.q_rs = d.g_rs = d.dim = 256
    d.nq, d.ng, d.k, d.scale = 1, 1000000, 10, 1.0
    auto = lib.mpv_sim_topk_workspace_size(ctypes.byref(d))
    assert auto > 0 and auto % 8 == 0
    d.slices = 3
    assert lib.mpv_sim_topk_workspace_size(ctypes.byref(d)) >= 2 * 3 * 10 * 4
    assert lib.mpv_sim_rank_workspace_size(ctypes.byref(d), 4) >= 2 * 4 * 4
    assert lib.mpv_sim_rank_workspace_size(ctypes.byref(d), 33) == 0
    out = ctypes.create_string_buffer(1024)
    addr = ctypes.addressof(out)
    for field, bad, code in (("dim", 48, _lib.lib().mpv_sim_topk), ("dim", 2048, None), ("k", 0, None), ("k", 33, None), ("g_rs", 252, None),
                             ("ng", 0, None), ("ng", 1 << 31, None), ("slices", -1, None)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        assert lib.mpv_sim_topk(ctypes.byref(d), addr, addr, addr, 1 << 30, None) < 0, (field, bad)
        assert lib.mpv_sim_topk_workspace_size(ctypes.byref(d)) == 0
        assert lib.mpv_last_error()
        setattr(d, field, keep)
    assert lib.mpv_sim_topk(ctypes.byref(d), addr, addr, addr, 8, None) == -5           # workspace too small: MPV_E_ARG
    assert lib.mpv_sim_rank(ctypes.byref(d), addr, 0, addr, addr, 1 << 30, None) == -5  # n_targets out of range


def test_retrieval_search_kernel_budget():
    """every kernel of retrieval_search.hip: no scratch; at most 256 registers (vgpr_count is the unified VGPR + AGPR file: two
    workgroups of the stream per CU) except the top-k stream with 32 list slots (64 registers of list: one workgroup per CU);
    and no scalar store / scalar atomic / scalar cache write-back instruction in the library's gfx950 code"""
    import test_isa_cpu as isa
    if not os.path.isfile(os.path.join(isa.LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    ks = {}
    d = tempfile.mkdtemp()
    banned = re.compile(r"\b(s_(buffer_|scratch_)?store_\w+|s_(buffer_)?atomic_\w+|s_dcache_(wb|discard)\w*)\b")
    found = []
    for i, blob in enumerate(isa._code_objects()):
        f = os.path.join(d, f"co_{i}.elf")
        open(f, "wb").write(blob)
        txt = subprocess.run([os.path.join(isa.LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
        mine = False
        for blk in txt.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if re.search(r"sim_(stream|topk_merge|target|rank_finish)_kernel", name):
                mine = True
                g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                ks[name] = dict(vgpr=g("vgpr_count"), scratch=g("private_segment_fixed_size"))
        if mine and os.path.isfile(os.path.join(isa.LLVM, "llvm-objdump")):
            asm = subprocess.run([os.path.join(isa.LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", f], capture_output=True, text=True).stdout
            assert "v_mfma_f32_32x32x16_bf16" in asm
            found += banned.findall(asm)
    shutil.rmtree(d, ignore_errors=True)
    assert len(ks) == 7, sorted(ks)            # stream: top-k at 4 / 16 / 32 list slots + rank; merge, target scores, rank finish
    for n, k in ks.items():
        assert k["scratch"] == 0 and k["vgpr"] <= (512 if "Li0ELi32E" in n else 256), (n, k)
    assert not found, found
