"""Searches with per-row priors on the CPU: the torch stand-ins (tests/standin_search_prior.py) proven against an independent fp64
restatement written with Python loops; RetrievalIndex's priors, exclusions and normaliser and the entry point's
`--eval_inverted_softmax` on those stand-ins; the C ABI (header, ctypes mirror, exported symbols) and the refusals, which run on
the host before any launch."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import standin_search_prior as sp
import standin_w8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
NEG_INF = float("-inf")
SYMBOLS = tuple(f"mpv_sim_{n}{ws}" for n in ("topk_prior", "rank_prior", "topk_prior_q8", "rank_prior_q8", "bank_lse", "bank_lse_q8")
                for ws in ("", "_workspace_size"))


def _ints(n, d, seed):
    return torch.randint(-2, 3, (n, d), generator=torch.Generator().manual_seed(seed)).to(BF)


def _unit(n, d, seed):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=1).to(BF)


def _quarters(n, seed, share=0.15):
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(-12, 13, (n,), generator=g).float() / 4
    p[torch.rand(n, generator=g) < share] = NEG_INF
    return p


# ------------------------------------------------------------------------------------------------ the stand-ins against fp64 loops
def _by_hand(q, g, prior, scale):
    """per query the eligible (score, row) pairs, best first, computed one row at a time in Python floats (fp64)"""
    out = []
    for qi in q.double().tolist():
        rows = []
        for j, (gj, pj) in enumerate(zip(g.double().tolist(), prior.tolist())):
            s = scale * sum(a * b for a, b in zip(qi, gj)) + pj
            if s == s and s != NEG_INF:
                rows.append((s, j))
        out.append(sorted(rows, key=lambda r: (-r[0], r[1])))
    return out


def test_standins_follow_the_contract_against_fp64_loops():
    """integer features, quarter priors and scales {1, 0.5, -1}: fp32 and fp64 agree exactly, so the stand-ins must return the
    hand-sorted lists -- eligibility (-inf, NaN), ties by the lower index, the (-inf, -1) tail, ranks with the scale applied"""
    nq, ng, d = 5, 41, 32
    q, g, prior = _ints(nq, d, 1), _ints(ng, d, 2), _quarters(ng, 3)
    g[7] = g[3]
    prior[7] = prior[3] = 0.5                                    # a forced tie
    prior[11] = float("inf")
    assert torch.isinf(prior).sum() > 3
    target = torch.tensor([[3, -1, 7], [7, -1, -1], [int(torch.isinf(prior).nonzero()[1]), -1, -1], [-1, -1, -1], [11, 5, 40]])
    for scale in (1.0, 0.5, -1.0):
        hand = _by_hand(q, g, prior, scale)
        for k in (1, 8, 32):
            vals, idx = sp.sim_topk_prior(q, g, prior, k, scale=scale)
            for i in range(nq):
                want = hand[i][:k]
                assert idx[i].tolist() == [j for _, j in want] + [-1] * (k - len(want))
                assert vals[i].tolist() == [s for s, _ in want] + [NEG_INF] * (k - len(want))
        pos = [{j: p for p, (_, j) in enumerate(rows)} for rows in hand]
        want_rank = [min([pos[i][t] for t in row if t in pos[i]] or [ng]) for i, row in enumerate(target.tolist())]
        assert sp.sim_rank_prior(q, g, prior, target, scale=scale).tolist() == want_rank
        assert want_rank[3] == ng and (want_rank[2] == ng or prior[target[2, 0]] == float("inf"))
        assert hand[0][0][1] == 11                               # +inf is an ordinary score: first
    few = torch.full((ng,), NEG_INF)
    few[[4, 9]] = 0.0
    vals, idx = sp.sim_topk_prior(q, g, few, 4)
    assert (idx[:, 2:] == -1).all() and (vals[:, 2:] == NEG_INF).all() and set(idx[0, :2].tolist()) == {4, 9}
    vals, idx = sp.sim_topk_prior(q, g, torch.full((ng,), NEG_INF), 4)
    assert (idx == -1).all() and (vals == NEG_INF).all()
    g[4, 0] = float("nan")
    assert not (sp.sim_topk_prior(q, g, few, 4)[1] == 4).any()
    assert sp.sim_rank_prior(q, g, few, torch.tensor([4] * nq)).tolist() == [ng] * nq


def test_standin_scores_are_two_roundings():
    """fl(fl(scale * s) + prior): the stand-in multiplies and adds in fp32, one operation each -- checked on a case where a fused
    multiply-add would give another bit pattern"""
    q = torch.zeros(1, 32, dtype=BF)
    g = torch.zeros(1, 32, dtype=BF)
    q[0, 0], g[0, 0] = 1.0, 1.0 + 2.0 ** -7                      # s = 1 + 2^-7 exactly
    scale, prior = 1.0 + 2.0 ** -17, torch.tensor([-1.0])
    s = np.float32(1.0 + 2.0 ** -7)
    two = np.float32(np.float32(s * np.float32(scale)) + np.float32(-1.0))
    fused = np.float32(np.float64(s) * np.float64(np.float32(scale)) - 1.0)
    assert two != fused
    assert sp.scores(q, g, prior, scale)[0, 0].item() == float(two)


def test_standin_lse_against_fp64_loops():
    for d, nb, ng in ((32, 1, 3), (64, 33, 5), (256, 200, 4)):
        bank, g = _unit(nb, d, 5), _unit(ng, d, 6)
        for beta in (0.0, 1.0, 20.0, 1000.0, -20.0):
            got = sp.sim_bank_lse(bank, g, beta)
            for j, gj in enumerate(g.double().tolist()):
                x = [beta * sum(a * b for a, b in zip(bi, gj)) for bi in bank.double().tolist()]
                m = max(x)
                want = m + math.log(sum(math.exp(v - m) for v in x))
                # fp32 products (D 2^-24 each, times beta), an fp32 log-sum-exp of nb terms
                assert math.isfinite(got[j].item()) and abs(got[j].item() - want) <= abs(beta) * d * 2.0 ** -23 + (nb + 64) * 2.0 ** -23 + 1e-6 * abs(want)
            if beta == 0.0:
                assert torch.allclose(got, torch.full((ng,), math.log(nb)), atol=1e-6)
    bank[3, 0] = float("nan")
    assert torch.isnan(sp.sim_bank_lse(bank, g, 1.0)).all()
    codes, scale = standin_w8.quantize_rows_e4m3(g)
    deq = standin_w8.dequantize(codes, scale)
    assert torch.equal(sp.sim_bank_lse_q8(_unit(9, 256, 7), codes, scale, 20.0), sp.sim_bank_lse(_unit(9, 256, 7), deq, 20.0))


# ------------------------------------------------------------------------------------------------ the index on the stand-ins
@pytest.mark.parametrize("storage", ["bf16", "fp8"])
def test_index_terms_on_standins(monkeypatch, storage):
    sp.install(monkeypatch)
    from youku_mplug_amd import ops
    from youku_mplug_amd._lib import MpvError
    from youku_mplug_amd.retrieval import MaxSimIndex, RetrievalIndex
    D = 64
    rows, q, bank = _unit(137, D, 11), _unit(9, D, 12), _unit(50, D, 13)
    calls = []
    for name in ("sim_topk", "sim_rank", "sim_topk_q8", "sim_rank_q8") + tuple(sp.NAMES):
        monkeypatch.setattr(ops, name, (lambda n, f: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(name, getattr(ops, name)))
    index = RetrievalIndex(D, device="cpu", capacity=100, storage=storage)
    index.add(rows[:100])
    before = set(vars(index))
    plain = index.search(q, 10, scale=2.0)
    plain_rank = index.rank(q, torch.arange(9))
    q8 = "_q8" if storage == "fp8" else ""
    assert calls == ["sim_topk" + q8, "sim_rank" + q8] and set(vars(index)) == before          # exactly today's ops, nothing kept
    assert index.prior is None and index.normaliser is None and not index.excluded.any() and set(vars(index)) == before
    for call in (lambda: index.search(q, 10, use_prior=True), lambda: index.rank(q, torch.arange(9), normalised=True)):
        with pytest.raises(MpvError, match="never called"):
            call()
    assert set(vars(index)) == before
    # fit on 100, add 37 across a growth: the 37 new rows are the only ones the bank pass sees
    index.fit_normaliser(bank, 20.0)
    index.set_prior(torch.tensor([0.25, -0.5]), rows=[3, 50])
    index.exclude([7, 99])
    calls.clear()
    index.add(rows[100:])
    assert calls == ["sim_bank_lse" + q8] and index.capacity >= 137
    whole = RetrievalIndex(D, device="cpu", storage=storage)
    whole.add(rows)
    whole.fit_normaliser(bank, 20.0)
    assert torch.equal(index.normaliser[2], whole.normaliser[2]) and torch.equal(index.normaliser[0], bank)
    gal = index.dequantized() if storage == "fp8" else index.features
    want_prior = torch.zeros(137)
    want_prior[3], want_prior[50] = 0.25, -0.5
    assert torch.equal(index.prior, want_prior) and index.excluded.nonzero().flatten().tolist() == [7, 99]
    term = want_prior - index.normaliser[2]
    term[[7, 99]] = NEG_INF
    got = index.search(q, 10)
    want = sp.sim_topk_prior(q, gal, term, 10, scale=20.0)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not ((got[1] == 7) | (got[1] == 99)).any()
    s64 = 20.0 * (q.double() @ gal.double().t()) - torch.logsumexp(20.0 * (bank.double() @ gal.double().t()), dim=0) + want_prior.double()
    assert (got[0].double() - torch.gather(s64, 1, got[1])).abs().max() < 1e-4                 # beta s - lse[g] + prior[g]
    t = torch.arange(9) * 5
    assert torch.equal(index.rank(q, t), sp.sim_rank_prior(q, gal, term, t, scale=20.0))
    assert index.rank(q[:1], torch.tensor([[7]])).item() == 137 and index.rank(q[:1], torch.tensor([[7, 3]])).item() < 137
    # the term is cached until something changes
    first = index._terms.cache[(True, True)]
    index.search(q, 3)
    assert index._terms.cache[(True, True)] is first
    index.include([7])
    assert not index._terms.cache and index.excluded.nonzero().flatten().tolist() == [99]
    index.include([99])
    whole.set_prior(want_prior)
    a, b = index.search(q, 10), whole.search(q, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                                 # include restored the rows
    # normalised=False / use_prior=False: the plain scores
    a = whole.search(q, 10, normalised=False, use_prior=False, scale=2.0)
    b = (ops.sim_topk_q8(q, whole.codes, whole.scales, 10, scale=2.0) if storage == "fp8" else ops.sim_topk(q, gal, 10, scale=2.0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a = whole.search(q, 10, normalised=False)                                                  # the prior alone, scale 1
    b = sp.sim_topk_prior(q, gal, want_prior, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(MpvError, match="pass no scale"):
        whole.search(q, 10, scale=2.0)
    whole.clear_prior()
    whole.clear_normaliser()
    assert whole.prior is None and whole.normaliser is None
    calls.clear()
    whole.search(q, 10)
    assert calls == ["sim_topk" + q8]
    # a rank with a scale goes through the prior entry (the plain one applies none): -1 reverses the order
    r = whole.rank(q, torch.arange(9), scale=-1.0)
    assert torch.equal(r, sp.sim_rank_prior(q, gal, torch.zeros(137), torch.arange(9), scale=-1.0))
    # the untouched index of the beginning
    again = RetrievalIndex(D, device="cpu", storage=storage)
    again.add(rows[:100])
    a = again.search(q, 10, scale=2.0)
    assert torch.equal(a[0], plain[0]) and torch.equal(a[1], plain[1]) and torch.equal(again.rank(q, torch.arange(9)), plain_rank)
    for call, word in ((lambda: index.set_prior(float("nan")), "NaN"), (lambda: index.exclude([137]), "rows must be"),
                       (lambda: index.set_prior(1.0, rows=[-1]), "rows must be"), (lambda: index.set_prior(torch.zeros(5)), "shape"),
                       (lambda: index.set_prior(torch.zeros(3), rows=[1, 2]), "3 values for 2 rows"),
                       (lambda: index.fit_normaliser(bank[:, :32].contiguous(), 20.0), "features must be"),
                       (lambda: index.fit_normaliser(bank.float(), 20.0), "bfloat16"),
                       (lambda: index.fit_normaliser(bank, float("nan")), "finite beta"),
                       (lambda: index.fit_normaliser(bank[:0], 1.0), "non-empty bank")):
        with pytest.raises(MpvError, match=word):
            call()
    assert not hasattr(MaxSimIndex, "set_prior")                                               # MaxSimIndex is unchanged


# ------------------------------------------------------------------------------------------------ the entry point
def _entry():
    sys.path.insert(0, os.path.join(ROOT, "downstream"))
    sys.path.insert(0, ROOT)
    import run_retrieval_distributed_gpt3 as entry
    return entry


def test_eval_inverted_softmax_flag_rules(tmp_path, capsys):
    import test_entrypoint_gpu as t
    entry = _entry()
    cfg = t._write_retrieval_config(str(tmp_path))
    base = ["--config", cfg, "--output_dir", str(tmp_path / "o")]
    args, _ = entry.get_args(base + ["--eval_on_device"])
    assert args.eval_inverted_softmax is None and args.eval_bank is None               # default off
    args, _ = entry.get_args(base + ["--eval_on_device", "--eval_index_fp8", "--eval_inverted_softmax", "20"])
    assert args.eval_inverted_softmax == 20.0 and args.eval_index_fp8 is True
    for argv, word in ((["--eval_inverted_softmax", "20"], "--eval_on_device"),
                       (["--eval_on_device", "--eval_inverted_softmax", "inf"], "finite"),
                       (["--eval_on_device", "--eval_bank", "x.pt"], "--eval_inverted_softmax")):
        with pytest.raises(SystemExit):
            entry.get_args(base + argv)
        assert word in capsys.readouterr().err
    good = {"text": _unit(7, 64, 1), "video": _unit(5, 64, 2)}
    torch.save(good, tmp_path / "bank.pt")
    bank = entry.load_eval_bank(str(tmp_path / "bank.pt"), 64)
    assert torch.equal(bank["text"], good["text"]) and torch.equal(bank["video"], good["video"])
    for bad, word in (({"text": _unit(7, 32, 1), "video": _unit(5, 64, 2)}, r"\[n, 64\]"), ({"text": good["text"]}, "keys"),
                      ({"text": good["text"].float(), "video": good["video"]}, "bfloat16")):
        torch.save(bad, tmp_path / "bad.pt")
        with pytest.raises(ValueError, match=word):
            entry.load_eval_bank(str(tmp_path / "bad.pt"), 64)


def _rank_is(ranks, t, lists, tol=2e-4):
    """the ranks are the positions read from the fp64 matrix t: exactly, where the best target's score is further than tol from
    every other score of its row (nearly everywhere), and within the interval that tol leaves open otherwise.  tol covers the fp32
    stand-in's worst case at these shapes: beta D 2^-24 = 7.6e-5 for the products (beta 20, D 64), as much again for the lse."""
    sure = 0
    for r, row, ts in zip(ranks, t, lists):
        ts = list(ts) if isinstance(ts, (list, tuple)) else [ts]
        lo = min(int((row > row[x] + tol).sum()) for x in ts)
        hi = min(int((row > row[x] - tol).sum()) - 1 for x in ts)
        assert lo <= r <= hi, (r, lo, hi)
        sure += lo == hi
    assert sure >= 0.95 * len(lists)


@pytest.mark.parametrize("fp8", [False, True])
def test_eval_inverted_softmax_on_standins(monkeypatch, capsys, fp8):
    """dual softmax (the bank is the evaluation's own queries): the ranks equal the positions in beta S - logsumexp(beta S, axis =
    queries) computed in fp64; with a bank of training queries, in beta S - lse over that bank; without the flag nothing changes"""
    import test_retrieval_search_cpu as trs
    sp.install(monkeypatch)
    entry = _entry()
    model, split, tok = trs._Towers(37, 90, 64, 3), trs._Split(37, 90, 8), entry.SyntheticTokenizer()
    dev, cfg, beta = torch.device("cpu"), {"max_length": 8}, 20.0
    deq = (lambda f: standin_w8.dequantize(*standin_w8.quantize_rows_e4m3(f))) if fp8 else (lambda f: f)
    before = entry.evaluation_on_device(model, split, tok, dev, cfg, index_fp8=fp8)
    capsys.readouterr()
    rv, rt = entry.evaluation_on_device(model, split, tok, dev, cfg, index_fp8=fp8, inverted_softmax=beta)
    out = capsys.readouterr().out
    assert "dual softmax" in out and "all test queries are known at once" in out and "37 clips" in out and "90 titles" in out

    def transformed(queries, gallery, bank):
        s = queries.double() @ gallery.double().t()
        return beta * s - torch.logsumexp(beta * (bank.double() @ gallery.double().t()), dim=0)[None, :]

    v_lists, t_lists = [split.vid2txt[v] for v in range(37)], [split.txt2vid[t] for t in range(90)]
    _rank_is(rv.tolist(), transformed(model.vf, deq(model.tf), model.vf), v_lists)
    _rank_is(rt.tolist(), transformed(model.tf, deq(model.vf), model.tf), t_lists)
    assert rv.tolist() != before[0].tolist() or rt.tolist() != before[1].tolist()     # the correction does change ranks here
    bank = {"text": _unit(40, 64, 21), "video": _unit(30, 64, 22)}
    rv, rt = entry.evaluation_on_device(model, split, tok, dev, cfg, index_fp8=fp8, inverted_softmax=beta, bank=bank)
    out = capsys.readouterr().out
    assert "QB-Norm" in out and "30 clip and 40 title" in out
    _rank_is(rv.tolist(), transformed(model.vf, deq(model.tf), bank["video"]), v_lists)
    _rank_is(rt.tolist(), transformed(model.tf, deq(model.vf), bank["text"]), t_lists)
    again = entry.evaluation_on_device(model, split, tok, dev, cfg, index_fp8=fp8)
    assert again[0].tolist() == before[0].tolist() and again[1].tolist() == before[1].tolist()
    with pytest.raises(Exception, match="features must be"):
        entry.evaluation_on_device(model, split, tok, dev, cfg, index_fp8=fp8, inverted_softmax=beta,
                                   bank={"text": _unit(4, 32, 1), "video": _unit(4, 32, 2)})


# ------------------------------------------------------------------------------------------------ C ABI and refusals
def test_bank_desc_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    body = re.search(r"typedef struct mpv_sim_bank_desc \{(.*?)\} mpv_sim_bank_desc;", hdr, re.S).group(1)
    names = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    ct = _lib.SimBankDesc
    assert names == [f[0] for f in ct._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpv.h"', 'int main(void) {',
            '  printf("%zu", sizeof(mpv_sim_bank_desc));'] + [f'  printf(" %zu", offsetof(mpv_sim_bank_desc, {n}));' for n in names] + \
           ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    tok = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert tok[0] == ctypes.sizeof(ct) and tok[1:] == [getattr(ct, f[0]).offset for f in ct._fields_]
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s


def test_prior_symbols_are_exported_and_refuse_on_the_host():
    """descriptor checks run before any launch, so the refusal codes can be exercised without a GPU; outputs stay untouched"""
    from youku_mplug_amd import _lib
    lib = _lib.lib()
    assert len(SYMBOLS) == 12
    for s in SYMBOLS:
        assert s in _lib.EXPORTS and getattr(lib, s) is not None
    out = ctypes.create_string_buffer(b"\x5a" * 1024, 1024)
    addr = ctypes.addressof(out)
    d = _lib.SimSearchDesc()
    d.queries = d.gallery = 4096
    d.q_rs = d.g_rs = d.dim = 256
    d.nq, d.ng, d.k, d.scale = 1, 1000000, 10, 1.0
    by = ctypes.byref(d)
    E_SHAPE, E_ALIGN, E_ARG = -1, -2, -5
    assert lib.mpv_sim_topk_prior_workspace_size(by, 4096) == lib.mpv_sim_topk_workspace_size(by) > 0
    assert lib.mpv_sim_rank_prior_workspace_size(by, 4096, 4) == lib.mpv_sim_rank_workspace_size(by, 4) > 0
    assert lib.mpv_sim_topk_prior_q8_workspace_size(by, 4096, 4096) > 0 and lib.mpv_sim_rank_prior_q8_workspace_size(by, 4096, 4096, 4) > 0
    for prior, code in ((None, E_ARG), (4098, E_ALIGN)):                               # null, misaligned
        assert lib.mpv_sim_topk_prior(by, prior, addr, addr, addr, 1 << 30, None) == code
        assert lib.mpv_sim_rank_prior(by, prior, addr, 1, addr, addr, 1 << 30, None) == code
        assert lib.mpv_sim_topk_prior_q8(by, 4096, prior, addr, addr, addr, 1 << 30, None) == code
        assert lib.mpv_sim_rank_prior_q8(by, 4096, prior, addr, 1, addr, addr, 1 << 30, None) == code
        assert lib.mpv_sim_topk_prior_workspace_size(by, prior) == 0 and lib.mpv_sim_rank_prior_workspace_size(by, prior, 1) == 0
        assert lib.mpv_sim_topk_prior_q8_workspace_size(by, 4096, prior) == 0
        assert lib.mpv_sim_rank_prior_q8_workspace_size(by, 4096, prior, 1) == 0
        assert b"g_prior" in lib.mpv_last_error()
    assert lib.mpv_sim_topk_prior_q8(by, None, 4096, addr, addr, addr, 1 << 30, None) == E_ARG      # what the plain entries refuse
    for field, bad in (("dim", 48), ("dim", 2048), ("k", 0), ("k", 33), ("g_rs", 252), ("ng", 0), ("slices", -1)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        assert lib.mpv_sim_topk_prior(by, 4096, addr, addr, addr, 1 << 30, None) < 0, (field, bad)
        assert lib.mpv_sim_topk_prior_workspace_size(by, 4096) == 0
        setattr(d, field, keep)
    assert lib.mpv_sim_topk_prior(by, 4096, addr, addr, addr, 8, None) == E_ARG       # workspace too small
    assert lib.mpv_sim_rank_prior(by, 4096, addr, 0, addr, addr, 1 << 30, None) == E_ARG
    assert lib.mpv_sim_rank_prior_workspace_size(by, 4096, 33) == 0
    b = _lib.SimBankDesc()
    b.bank = b.gallery = 4096
    b.b_rs = b.g_rs = b.dim = 256
    b.nb, b.ng, b.beta = 1000, 100000, 20.0
    bb = ctypes.byref(b)
    assert lib.mpv_sim_bank_lse_workspace_size(bb) > 0 and lib.mpv_sim_bank_lse_q8_workspace_size(bb, 4096) > 0
    for field, bad, code in (("bank", None, E_ARG), ("gallery", None, E_ARG), ("beta", float("inf"), E_ARG), ("beta", float("nan"), E_ARG),
                             ("dim", 48, E_SHAPE), ("dim", 2048, E_SHAPE), ("nb", 0, E_SHAPE), ("ng", 0, E_SHAPE), ("b_rs", 252, E_ALIGN),
                             ("gallery", 4104, E_ALIGN)):
        keep = getattr(b, field)
        setattr(b, field, bad)
        assert lib.mpv_sim_bank_lse(bb, addr, None, 0, None) == code, (field, bad)
        assert lib.mpv_sim_bank_lse_q8(bb, 4096, addr, None, 0, None) == code, (field, bad)
        assert lib.mpv_sim_bank_lse_workspace_size(bb) == 0 and lib.mpv_sim_bank_lse_q8_workspace_size(bb, 4096) == 0
        assert lib.mpv_last_error()
        setattr(b, field, keep)
    assert lib.mpv_sim_bank_lse(bb, None, None, 0, None) == E_ARG                      # null output
    assert lib.mpv_sim_bank_lse_q8(bb, None, addr, None, 0, None) == E_ARG             # null g_scale
    b.g_rs = 264
    assert lib.mpv_sim_bank_lse(bb, None, None, 0, None) == E_ARG                      # fine for bf16 rows up to the null output ...
    assert lib.mpv_sim_bank_lse_q8(bb, 4096, addr, None, 0, None) == E_ALIGN           # ... not for codes: a multiple of 16
    assert out.raw == b"\x5a" * 1024


def test_ops_refuse_host_tensors():
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import ops
    from youku_mplug_amd._lib import MpvError
    q, g = _unit(1, 64, 0), _unit(4, 64, 1)
    for call in (lambda: ops.sim_topk_prior(q, g, torch.zeros(4), 1), lambda: ops.sim_rank_prior(q, g, torch.zeros(4), torch.tensor([0])),
                 lambda: ops.sim_bank_lse(q, g, 1.0)):
        with pytest.raises(MpvError, match="GPU only"):
            call()
