"""Searches over an FP8 gallery without a GPU: the stand-ins (tests/standin_search_q8.py: the bf16 stand-ins on the dequantised
gallery), the C ABI of the built library (symbols, host-side refusals before any launch), the index classes with storage="fp8"
on the stand-ins (growth, views, refusals), the flag rules of the two entry points, and the analytic bound on what the rounding to
e4m3 does to a score."""
import ctypes
import importlib.util
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maxsim_cases as mc                      # noqa: E402
import standin_maxsim_search as sm             # noqa: E402
import standin_search as ss                    # noqa: E402
import standin_search_q8 as sq                 # noqa: E402
import standin_w8                              # noqa: E402

import youku_mplug_amd  # noqa: E402,F401

BF = torch.bfloat16
SYMBOLS = ("mpv_sim_topk_q8", "mpv_sim_rank_q8", "mpv_maxsim_topk_q8", "mpv_maxsim_rank_q8")


def _unit(n, dim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=1).to(BF)


# ------------------------------------------------------------------------------------------------ stand-ins
def test_standins_are_the_bf16_standins_on_the_dequantised_gallery():
    q, g = _unit(5, 64, 0), _unit(40, 64, 1)
    codes, scale = standin_w8.quantize_rows_e4m3(g)
    deq = sq.dequantize(codes, scale)
    assert deq.dtype == BF and torch.equal(deq.float(), codes.view(torch.float8_e4m3fn).float() * scale[:, None])     # exact
    for a, b in zip(sq.sim_topk_q8(q, codes, scale, 7, scale=0.5), ss.sim_topk(q, deq, 7, scale=0.5)):
        assert torch.equal(a, b)
    t = torch.tensor([[3, -1], [0, 39], [7, 7], [-1, -1], [12, 1]])
    assert torch.equal(sq.sim_rank_q8(q, codes, scale, t), ss.sim_rank(q, deq, t))
    c3, s3 = codes.view(8, 5, 64), scale.view(8, 5)
    for a, b in zip(sq.maxsim_topk_q8(q, c3, s3, 9), sm.maxsim_topk(q, deq.view(8, 5, 64), 9)):
        assert torch.equal(a, b)
    assert torch.equal(sq.maxsim_rank_q8(q, c3, s3, t[:, :1].clamp(max=7)), sm.maxsim_rank(q, deq.view(8, 5, 64), t[:, :1].clamp(max=7)))


def test_standin_refusals():
    from youku_mplug_amd._lib import MpvError
    q, g = _unit(2, 32, 0), _unit(6, 32, 1)
    codes, scale = standin_w8.quantize_rows_e4m3(g)
    for bad in (lambda: sq.sim_topk_q8(q, g, scale, 1),                                  # bf16 rows are not codes
                lambda: sq.sim_topk_q8(q, codes, scale[:5], 1), lambda: sq.sim_topk_q8(q, codes, scale.double(), 1),
                lambda: sq.sim_topk_q8(q, codes, None, 1), lambda: sq.sim_topk_q8(q, codes, scale, 0),
                lambda: sq.sim_rank_q8(q, codes.view(2, 3, 32), scale.view(2, 3), torch.tensor([0, 1])),
                lambda: sq.maxsim_topk_q8(q, codes.view(2, 3, 32), scale, 1),             # one scale per ROW
                lambda: sq.maxsim_topk_q8(q.view(1, 2, 32), codes, scale, 1),             # grouped queries
                lambda: sq.maxsim_rank_q8(q.view(1, 2, 32), codes, scale, torch.tensor([0]))):
        with pytest.raises(MpvError):
            bad()


def test_ops_refuse_host_tensors_and_bad_operands():
    """the real wrappers (no stand-in): checked before the library is touched"""
    from youku_mplug_amd import ops
    from youku_mplug_amd._lib import MpvError
    q, g = _unit(1, 64, 0), _unit(4, 64, 1)
    codes, scale = standin_w8.quantize_rows_e4m3(g)
    for call in (lambda: ops.sim_topk_q8(q, codes, scale, 1), lambda: ops.sim_rank_q8(q, codes, scale, torch.tensor([0])),
                 lambda: ops.maxsim_topk_q8(q, codes, scale, 1), lambda: ops.maxsim_rank_q8(q, codes, scale, torch.tensor([0]))):
        with pytest.raises(MpvError, match="GPU only"):
            call()


# ------------------------------------------------------------------------------------------------ C ABI
def test_q8_symbols_are_declared_exported_and_documented():
    from youku_mplug_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    lib = _lib.lib()
    for s in SYMBOLS:
        for name in (s, s + "_workspace_size"):
            assert name in _lib.EXPORTS and getattr(lib, name) is not None
            assert re.search(r"\b" + name + r"\(", hdr), name
    block = hdr[hdr.index("Searches over an FP8 gallery"):hdr.index("mpv_sim_topk_q8_workspace_size(")]
    for word in ("e4m3fn", "multiple of 16", "power", "subnormal", "0x7F", "q_group", "not been measured"):
        assert word in block, word


def _desc(lib_mod, kind):
    d = lib_mod.SimSearchDesc() if kind == "sim" else lib_mod.MaxSimSearchDesc()
    d.queries = d.gallery = 4096
    d.q_rs = d.g_rs = d.dim = 256
    d.nq, d.ng, d.k, d.scale = 3, 1000, 10, 1.0
    if kind != "sim":
        d.q_group, d.g_group = 1, 8
    return d


@pytest.mark.parametrize("kind", ["sim", "maxsim"])
def test_q8_entries_refuse_before_any_launch(kind):
    """descriptor checks run on the host before any launch, so they can be exercised without a GPU: negative code, workspace
    size 0, an error text, and the output buffers untouched"""
    from youku_mplug_amd import _lib
    lib = _lib.lib()
    topk, rank = getattr(lib, f"mpv_{kind}_topk_q8"), getattr(lib, f"mpv_{kind}_rank_q8")
    topk_ws, rank_ws = getattr(lib, f"mpv_{kind}_topk_q8_workspace_size"), getattr(lib, f"mpv_{kind}_rank_q8_workspace_size")
    d = _desc(_lib, kind)
    out = ctypes.create_string_buffer(b"\x5a" * 1024, 1024)
    addr, gs = ctypes.addressof(out), 8192
    assert topk_ws(ctypes.byref(d), gs) > 0 and rank_ws(ctypes.byref(d), gs, 4) >= 2 * 3 * 4 * 4
    d.slices = 3
    assert topk_ws(ctypes.byref(d), gs) >= 2 * 3 * 3 * 10 * 4
    d.g_rs = 256 + 16                                      # a row pitch in codes
    assert topk_ws(ctypes.byref(d), gs) > 0
    d.g_rs = 256

    def refused(what):
        assert topk(ctypes.byref(d), gs_now, addr, addr, addr, 1 << 30, None) < 0, what
        assert topk_ws(ctypes.byref(d), gs_now) == 0, what
        assert rank(ctypes.byref(d), gs_now, addr, 1, addr, addr, 1 << 30, None) < 0, what
        assert rank_ws(ctypes.byref(d), gs_now, 1) == 0, what
        assert lib.mpv_last_error()
        assert out.raw == b"\x5a" * 1024, what

    gs_now = None                                          # a null g_scale
    refused("g_scale")
    assert topk(ctypes.byref(d), None, addr, addr, addr, 1 << 30, None) == -5
    gs_now = gs
    bad = [("g_rs", 264), ("g_rs", 248), ("g_rs", 128), ("gallery", 4104), ("queries", 4104), ("dim", 48), ("dim", 2048), ("ng", 0),
           ("nq", 0), ("q_rs", 128), ("slices", -1), ("slices", 4097)]
    if kind == "maxsim":
        bad += [("q_group", 2), ("q_group", 256), ("g_group", 0), ("g_group", 1025)]
    for field, value in bad:
        keep = getattr(d, field)
        setattr(d, field, value)
        refused((field, value))
        setattr(d, field, keep)
    d.g_rs = 264                                           # a multiple of 8, which the bf16 entries take, is not enough
    assert topk(ctypes.byref(d), gs, addr, addr, addr, 1 << 30, None) == -2            # MPV_E_ALIGN
    d.g_rs = 256
    if kind == "maxsim":
        d.q_group, d.g_group = 8, 1
        assert topk(ctypes.byref(d), gs, addr, addr, addr, 1 << 30, None) == -1        # MPV_E_SHAPE, and the text says why
        assert b"q_group" in lib.mpv_last_error()
        assert lib.mpv_maxsim_topk_workspace_size(ctypes.byref(d)) > 0                 # the bf16 entry still takes that direction
        d.q_group, d.g_group = 1, 8
    for k in (0, 33):
        d.k = k
        assert topk(ctypes.byref(d), gs, addr, addr, addr, 1 << 30, None) == -5 and topk_ws(ctypes.byref(d), gs) == 0
    d.k = 10
    assert topk(ctypes.byref(d), gs, addr, addr, addr, 8, None) == -5                  # workspace too small: MPV_E_ARG
    assert rank(ctypes.byref(d), gs, addr, 1, addr, addr, 8, None) == -5
    assert rank(ctypes.byref(d), gs, addr, 0, addr, addr, 1 << 30, None) == -5         # n_targets out of range
    assert rank_ws(ctypes.byref(d), gs, 33) == 0
    assert out.raw == b"\x5a" * 1024


# ------------------------------------------------------------------------------------------------ index classes on the stand-ins
def test_retrieval_index_fp8_growth_views_and_refusals(monkeypatch):
    sq.install(monkeypatch)
    from youku_mplug_amd._lib import MpvError
    from youku_mplug_amd.retrieval import RetrievalIndex
    rows = _unit(21, 64, 3) * torch.logspace(-2, 1, 21, base=2.0)[:, None].to(BF)     # exponents differ from row to row
    index = RetrievalIndex(64, device="cpu", capacity=4, storage="fp8")
    assert index.storage == "fp8" and index.add(rows[:3]) == 0 and index.capacity == 4
    assert index.add(rows[3:]) == 3 and len(index) == 21 and index.capacity >= 21      # grew across the capacity in the second add
    codes, scale = standin_w8.quantize_rows_e4m3(rows)
    assert index.codes.dtype == torch.uint8 and torch.equal(index.codes, codes) and torch.equal(index.scales, scale)
    assert index.codes.data_ptr() == index._rows.data_ptr()                            # views of the storage
    assert torch.equal(index.dequantized(), sq.dequantize(codes, scale)) and index.dequantized().dtype == BF
    assert index.nbytes == 21 * 64 + 21 * 4
    with pytest.raises(MpvError, match=r"dequantized\(\)"):
        index.features
    twin = RetrievalIndex(64, device="cpu", capacity=4)                                # default storage: bf16, nothing new
    twin.add(index.dequantized())
    assert twin.storage == "bf16" and twin.nbytes == 21 * 64 * 2 and torch.equal(twin.features, index.dequantized())
    q = _unit(4, 64, 9) * 3
    for a, b in zip(index.search(q, 5, scale=2.0), twin.search(q, 5, scale=2.0)):
        assert torch.equal(a, b)
    t = torch.tensor([[0, 20], [5, -1], [-1, -1], [7, 7]])
    assert torch.equal(index.rank(q, t), twin.rank(q, t))
    for bad in (lambda: RetrievalIndex(64, device="cpu", storage="int8"), lambda: twin.codes, lambda: twin.scales, lambda: twin.dequantized(),
                lambda: index.add(rows.float()), lambda: index.search(q, 33), lambda: index.rank(q, [21] * 4),
                lambda: RetrievalIndex(64, device="cpu", storage="fp8").search(q, 1)):
        with pytest.raises(MpvError):
            bad()


def test_maxsim_index_fp8_growth_and_grouped_queries_refused(monkeypatch):
    sq.install(monkeypatch)
    from youku_mplug_amd import ops
    from youku_mplug_amd._lib import MpvError
    from youku_mplug_amd.retrieval import MaxSimIndex
    clips, titles = mc.unit_rows(11, 5, 32, 1), mc.unit_rows(7, None, 32, 2)
    vi = MaxSimIndex(32, 5, device="cpu", capacity=2, storage="fp8")
    assert vi.add(clips[:2]) == 0 and vi.capacity == 2 and vi.add(clips[2:]) == 2 and len(vi) == 11 and vi.capacity >= 11
    codes, scale = standin_w8.quantize_rows_e4m3(clips.reshape(-1, 32))
    assert torch.equal(vi.codes, codes.view(11, 5, 32)) and torch.equal(vi.scales, scale.view(11, 5)) and vi.nbytes == 55 * 32 + 55 * 4
    with pytest.raises(MpvError, match=r"dequantized\(\)"):
        vi.features
    twin = MaxSimIndex(32, 5, device="cpu")
    twin.add(vi.dequantized())
    for a, b in zip(vi.search(titles, 3, scale=0.5), twin.search(titles, 3, scale=0.5)):
        assert torch.equal(a, b)
    t = torch.tensor([0, 10, -1, 3, 4, 5, 6])
    assert torch.equal(vi.rank(titles, t), twin.rank(titles, t))
    # an index of single rows: single-row queries are served, grouped queries are refused before any op is reached
    ti = MaxSimIndex(32, device="cpu", capacity=1, storage="fp8")
    ti.add(titles[:4])
    ti.add(titles[4:, None, :])
    assert ti.codes.shape == (7, 1, 32) and ti.scales.shape == (7, 1)
    assert torch.equal(ti.search(titles[:, None, :], 2)[1][:, 0], torch.arange(7))
    called = []
    for n in sq.NAMES:
        monkeypatch.setattr(ops, n, lambda *a, **k: called.append(1))
    for bad in (lambda: ti.search(clips, 3), lambda: ti.rank(clips, torch.arange(11) % 7), lambda: vi.search(clips, 3)):
        with pytest.raises(MpvError):
            bad()
    with pytest.raises(MpvError, match="bf16"):
        ti.search(clips, 3)
    assert not called


# ------------------------------------------------------------------------------------------------ entry points
def _entry():
    sys.path.insert(0, os.path.join(ROOT, "downstream"))
    sys.path.insert(0, ROOT)
    import run_retrieval_distributed_gpt3 as entry
    return entry


def test_eval_index_fp8_flag_rules(tmp_path, capsys):
    import test_entrypoint_gpu as t
    entry = _entry()
    cfg = t._write_retrieval_config(str(tmp_path))
    base = ["--config", cfg, "--output_dir", str(tmp_path / "o")]
    assert entry.get_args(base)[0].eval_index_fp8 is False
    assert entry.get_args(base + ["--eval_on_device"])[0].eval_index_fp8 is False
    args, _ = entry.get_args(base + ["--eval_on_device", "--eval_index_fp8"])
    assert args.eval_index_fp8 is True and args.eval_on_device is True
    with pytest.raises(SystemExit):
        entry.get_args(base + ["--eval_index_fp8"])
    assert "--eval_on_device" in capsys.readouterr().err


def test_eval_on_device_with_fp8_galleries_on_standins(monkeypatch, capsys):
    """the ranks are those of bf16 galleries holding the dequantised features, and the index bytes are logged"""
    import test_retrieval_search_cpu as trs
    sq.install(monkeypatch)
    entry = _entry()
    model, split, tok = trs._Towers(37, 90, 64, 3), trs._Split(37, 90, 8), entry.SyntheticTokenizer()
    dev, cfg = torch.device("cpu"), {"max_length": 8}
    rv, rt = entry.evaluation_on_device(model, split, tok, dev, cfg, index_fp8=True)
    assert f"index bytes: video {37 * 64 + 37 * 4} (fp8), text {90 * 64 + 90 * 4} (fp8)" in capsys.readouterr().out
    deq = lambda f: sq.dequantize(*standin_w8.quantize_rows_e4m3(f))
    assert rv.tolist() == ss.sim_rank(model.vf, deq(model.tf), entry._targets(split.vid2txt, range(37), dev)).tolist()
    assert rt.tolist() == ss.sim_rank(model.tf, deq(model.vf), entry._targets(split.txt2vid, range(90), dev)).tolist()
    rv0, rt0 = entry.evaluation_on_device(model, split, tok, dev, cfg)
    assert f"index bytes: video {37 * 64 * 2} (bf16), text {90 * 64 * 2} (bf16)" in capsys.readouterr().out
    assert rv0.shape == rv.shape and rt0.shape == rt.shape


def _tool():
    spec = importlib.util.spec_from_file_location("zero_shot_retrieval", os.path.join(ROOT, "tools", "zero_shot_retrieval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_zero_shot_tool_index_fp8_on_standins(monkeypatch, capsys):
    """--index_fp8 quantises the video index only; the ranks are those of the bf16 tool run on the dequantised clips"""
    import standin_contrastive
    sq.install(monkeypatch)
    if hasattr(standin_contrastive, "install"):
        standin_contrastive.install(monkeypatch)
        sq.install(monkeypatch)
    tool = _tool()
    argv = ["--synthetic", "6", "--batch_size", "4", "--device", "cpu", "--seed", "5"]
    result = tool.main(argv + ["--index_fp8"])
    out = capsys.readouterr().out
    model, split, tok, max_length = tool.synthetic_setup(6, 4, torch.device("cpu"), 5)
    vi, ti = tool.build_indexes(model, split, tok, torch.device("cpu"), max_length, index_fp8=True)
    assert vi.storage == "fp8" and ti.storage == "bf16"
    Q, E = model.num_learnable_token, vi.dim
    assert f"index bytes: video {6 * Q * E + 6 * Q * 4} (fp8), text {6 * E * 2} (bf16)" in out
    rv, rt = tool.zero_shot_ranks(model, split, tok, torch.device("cpu"), max_length, index_fp8=True)
    deq = vi.dequantized()
    assert rv.tolist() == sm.maxsim_rank(deq, ti.features[:, 0], torch.arange(6)[:, None]).tolist()
    assert rt.tolist() == sm.maxsim_rank(ti.features[:, 0], deq, torch.arange(6)[:, None]).tolist()
    assert result == tool._entry().recall_from_ranks(rv, rt)
    tool.main(argv)                                                                    # the default: both indexes bf16
    assert f"index bytes: video {6 * Q * E * 2} (bf16), text {6 * E * 2} (bf16)" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ what the rounding costs
def test_quantisation_error_of_a_score_is_within_the_analytic_bound():
    """fp64: |<q, deq> - <q, g>| <= sum_i |q_i| (2^-4 |g_i| + 2^-10 scale_row) for quantised unit rows -- 2^-4 is e4m3's relative
    half-ulp on normals (3 mantissa bits), 2^-10 its absolute half-ulp on subnormals (spacing 2^-9), in units of the row scale"""
    for dim, seed in ((32, 0), (256, 1), (1024, 2)):
        g, q = _unit(200, dim, seed), _unit(16, dim, seed + 10)
        codes, scale = standin_w8.quantize_rows_e4m3(g)
        e = torch.log2(scale)
        assert torch.equal(e, e.round()) and e.min() >= -13 and e.max() <= -8            # powers of two, around -11 for unit rows
        deq = sq.dequantize(codes, scale).double()
        err = (q.double() @ (deq - g.double()).t()).abs()
        bound = q.double().abs() @ (2.0 ** -4 * g.double().abs() + 2.0 ** -10 * scale.double()[:, None]).t()
        assert (err <= bound).all()
        per_element = (deq - g.double()).abs() <= 2.0 ** -4 * g.double().abs() + 2.0 ** -10 * scale.double()[:, None]
        assert per_element.all()
        assert err.max() > 0                                                             # the rounding is not a no-op on this data
