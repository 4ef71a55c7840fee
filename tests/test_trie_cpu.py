"""Closed-vocabulary generation, checked without a GPU: generation.PhraseTrie's CSR arrays and lookup; the
stand-in tests/standin_trie.py against the independent reference tests/ref_trie.py on every case of tests/trie_cases.py; the
library's refusals on the host and the ctypes mirror of the descriptor; every loop that takes constraints on the stand-ins with the
stand-in as trie_fn (what comes back is a phrase and the termination id; one call per step, none without a trie); and the exhaustive
check of the lockstep beam search on the stub decoder: with P <= K phrases it returns exactly the P phrases, in the order and with
the scores of an fp64 teacher-forced reference."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import ref_trie
import standin_trie as stt
import trie_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
EOS_IDS = [tc.EOS]
NEW_SYMBOLS = ("mpv_logits_trie_mask", "mpv_logits_trie_mask_ragged", "mpv_logits_trie_mask_steps")


def _gen():
    from youku_mplug_amd import generation
    return generation


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------ PhraseTrie
@pytest.mark.parametrize("kind,V", [("one", 8), ("prefix", 8), ("edges", 1000), ("chunks", 1000), ("all", 1000), ("long", 1000), ("random", 1000),
                                    ("wave", 1000), ("stage", 51200)])
def test_phrase_trie_csr_invariants_and_lookup(kind, V):
    phrases = tc.phrases_of(kind, V)
    t = _gen().PhraseTrie(phrases, V)
    root = ref_trie.build(phrases)
    cb, ct, cn, term = t.child_begin, t.child_tok, t.child_node, t.terminal
    assert len(cb) == t.n_nodes + 1 and len(ct) == len(cn) == t.n_edges == cb[-1] and len(term) == t.n_nodes and cb[0] == 0
    assert all(a <= b for a, b in zip(cb, cb[1:]))
    for u in range(t.n_nodes):
        kids = ct[cb[u]:cb[u + 1]]
        assert all(a < b for a, b in zip(kids, kids[1:])), u                 # strictly ascending: no token twice under a node
    assert sorted(cn) == list(range(1, t.n_nodes))                           # merged prefixes: every node but the root has ONE edge into it
    assert t.n_edges == len({tuple(p[:i]) for p in phrases for i in range(1, len(p) + 1)})
    assert t.n_phrases == len(phrases) and t.max_len == max(len(p) for p in phrases)
    first = {}
    for i, p in enumerate(phrases):
        first.setdefault(tuple(p), i)                                        # a phrase given twice keeps the lowest index
    assert sorted(x for x in term if x >= 0) == sorted(first.values())
    some = phrases if len(phrases) <= 300 else phrases[::37]
    for p in some:
        assert t.lookup(p) == first[tuple(p)] == ref_trie.lookup(root, p)
        assert t.lookup(torch.tensor(p)) == first[tuple(p)]
        for i in range(len(p)):                                              # every proper prefix, the empty one included
            assert t.lookup(p[:i]) == first.get(tuple(p[:i]), -1)
        assert t.lookup(list(p) + [tc.EOS]) == -1 and t.lookup([tc.EOS]) == -1 and t.lookup(list(p) + [V]) == -1 and t.lookup([-1]) == -1
        u, node = 0, root                                                    # the nodes carry the reference's numbers
        for tok in p:
            j = ct.index(tok, cb[u], cb[u + 1])
            u, node = cn[j], node.kids[tok]
            assert u == node.number and term[u] == node.phrase
    assert not t.contains(tc.EOS) and t.contains(phrases[0][0])
    arrays = t.arrays("cpu")
    assert arrays is t.arrays(torch.device("cpu")) and all(a.dtype == torch.int32 for a in arrays)
    assert [a.tolist() for a in arrays] == [cb, ct, cn, term]


def test_phrase_trie_duplicates_and_refusals(monkeypatch):
    PT = _gen().PhraseTrie
    t = PT([[4, 5], [4], [4, 5], [4, 5, 6], [4]], 8)
    assert (t.n_nodes, t.n_edges, t.n_phrases, t.max_len) == (4, 3, 5, 3)
    assert [t.lookup(p) for p in ([4, 5], [4], [4, 5, 6], [5], [])] == [0, 1, 3, -1, -1]
    for bad, shown in (([], "at least one"), ([[1], []], "phrase 1 is empty"), ([[1, 8]], "token 8"), ([[-1]], "token -1"),
                       ([[1] * 256], "256 tokens")):
        with pytest.raises(ValueError, match=shown):
            PT(bad, 8)
    PT([[1] * 255], 8)
    monkeypatch.setattr(PT, "MAX_EDGES", 3)                                   # the limit of 2^31 - 1 edges, at a size a test can reach
    PT([[1, 2, 3]], 8)
    with pytest.raises(ValueError, match="more than 3 edges"):
        PT([[1, 2, 3], [2]], 8)
    with pytest.raises(ValueError, match="PhraseTrie"):
        _gen().LogitsConstraints(allowed_phrases=[[1, 2]])
    assert _gen().LogitsConstraints(allowed_phrases=t).active and not _gen().LogitsConstraints(allowed_phrases=t).edits
    assert _gen().as_phrase_trie(t, 8) is t and _gen().as_phrase_trie([[1], [2, 3]], 8).n_phrases == 2
    assert _gen().as_phrase_trie(["ab", [3]], 8, encode=lambda s: [ord(c) - 96 for c in s]).lookup([1, 2]) == 0
    with pytest.raises(ValueError, match="tokenizer"):
        _gen().as_phrase_trie(["ab"], 8)


# ------------------------------------------------------------------------------ the stand-in against the reference
_TRIES = {}


def _case_trie(c):
    key = (c["trie"], c["V"])
    if key not in _TRIES:
        ph = tc.phrases_of(*key)
        _TRIES[key] = (_gen().PhraseTrie(ph, c["V"]), ref_trie.build(ph))
    return _TRIES[key]


@pytest.mark.parametrize("case", tc.KERNEL_CASES, ids=tc.case_id)
def test_standin_equals_the_reference(case):
    b = tc.build(case)
    V, rows = case["V"], case["rows"]
    trie, root = _case_trie(case)
    node = torch.full((rows,), -9, dtype=torch.int32)
    got = b["logits"].clone()
    assert stt.logits_trie_mask(got, b["tokens"], pos=b["pos"], trie=trie, prompt_len=b["prompt_len"], eos_ids=EOS_IDS, ban_value=b["ban"], node_out=node,
                                vocab=V) is got
    want, want_node = ref_trie.trie_mask(b["logits"], b["tokens"], root, columns=[b["pos"]] * rows, prompt_len=b["prompt_len"].tolist(),
                                         eos_ids=EOS_IDS, ban_value=b["ban"], vocab=V)
    assert torch.equal(_bits(got), _bits(want)) and node.tolist() == want_node and (got[:, V:] == tc.POISON).all()
    if rows >= 7:
        assert set(b["kinds"]) == set(tc.HISTORIES) and {-2, -1} <= set(want_node) and max(want_node) >= 0
        changed = (_bits(got) != _bits(b["logits"])).any(dim=1)
        assert all(bool(changed[r]) == (k != "forced") for r, k in enumerate(b["kinds"]) if case["trie"] != "all" or k == "forced")


def test_the_cases_cover_what_they_claim():
    C = tc.KERNEL_CASES
    assert len({tc.case_id(c) for c in C}) == len(C)
    assert {c["V"] for c in C} == {8, 1000, 51200} and {c["rows"] for c in C} == {1, 5, 160, 513} and {c["trie"] for c in C} == set(tc.TRIES)
    for V in (8, 1000, 51200):
        assert {c["rows"] for c in C if c["V"] == V} == {1, 5, 160, 513} and {c["ban"] for c in C if c["V"] == V} == {"inf", "finite"}
    assert len(tc.phrases_of("random", 51200)) == 10000 and max(len(p) for p in tc.phrases_of("long", 1000)) == 255
    t, _ = _case_trie(dict(trie="stage", V=51200))
    sizes = {t.child_begin[u + 1] - t.child_begin[u] for u in range(t.n_nodes)}
    assert {4096, 4097} <= sizes                                             # both sides of the kernel's LDS staging limit
    t, _ = _case_trie(dict(trie="wave", V=1000))
    assert {64, 65} <= {t.child_begin[u + 1] - t.child_begin[u] for u in range(t.n_nodes)}
    t, _ = _case_trie(dict(trie="random", V=51200))
    assert t.child_begin[1] > 64 * 64 // 8                                   # a root wide enough for a narrowing round of the wave's search
    t, _ = _case_trie(dict(trie="prefix", V=8))
    assert any(t.terminal[u] >= 0 and t.child_begin[u + 1] > t.child_begin[u] for u in range(t.n_nodes))   # terminal AND internal


def test_ragged_and_steps_standins_are_the_uniform_one_row_by_row():
    c = dict(V=64, rows=12, trie="prefix", ban="inf")
    trie, root = _gen().PhraseTrie(tc.phrases_of("prefix", 64), 64), ref_trie.build(tc.phrases_of("prefix", 64))
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(12, 64, generator=g).to(torch.bfloat16)
    tokens = torch.randint(0, 64, (12, 8), generator=g)
    hist = [[2, 5, 1], [2], [2, 5], [6, 6, 6], [9], [], [2, 4, 7, 2], [2, 5, 1], [2], [6], [2, 5], [2, 4]]
    prompt_len = torch.tensor([r % 3 for r in range(12)])
    for r, h in enumerate(hist):
        tokens[r, r % 3:r % 3 + len(h)] = torch.tensor(h, dtype=torch.int64)
    steps = [len(h) for h in hist]
    steps[4], steps[9] = -1, 7
    for name, kw, per_row in (("steps", dict(row_step=torch.tensor(steps, dtype=torch.int32)), steps), ("ragged", dict(step=2), [2] * 12),
                              ("ragged", dict(step=6), [6] * 12)):
        node = torch.zeros(12, dtype=torch.int32)
        got = getattr(stt, "logits_trie_mask_" + name)(logits.clone(), tokens, trie=trie, prompt_len=prompt_len, eos_ids=EOS_IDS, node_out=node, **kw)
        cols = [stt._column(prompt_len, r, 8, per_row[r]) for r in range(12)]
        want, want_node = ref_trie.trie_mask(logits, tokens, root, columns=cols, prompt_len=prompt_len.tolist(), eos_ids=EOS_IDS,
                                             ban_value=float("-inf"), vocab=64)
        assert torch.equal(_bits(got), _bits(want)) and node.tolist() == want_node
        for r in range(12):
            if cols[r] is not None:
                one = stt.logits_trie_mask(logits[r:r + 1].clone(), tokens[r:r + 1], pos=cols[r], trie=trie, prompt_len=prompt_len[r:r + 1], eos_ids=EOS_IDS)
                assert torch.equal(_bits(one[0]), _bits(got[r]))
        assert (name, kw.get("step")) != ("ragged", 6) or any(c is None for c in cols)


# ------------------------------------------------------------------------------ the library on the host
def _desc(**over):
    from youku_mplug_amd import _lib
    d = _lib.LogitsTrieDesc()
    ok = dict(logits=0x10000, tokens=0x20000, prompt_len=0x30000, eos_ids=0x40000, child_begin=0x50000, child_tok=0x60000, child_node=0x70000,
              terminal=0x80000, node_out=0x90000, ld=72, prompt_len_all=0, rows=2, vocab=64, row_len=16, pos=5, n_eos=1, n_nodes=5, n_edges=4,
              ban_value=float("-inf"))
    for k, v in {**ok, **over}.items():
        setattr(d, k, v)
    return d


REFUSALS = [dict(logits=None), dict(tokens=None), dict(vocab=60), dict(vocab=0), dict(vocab=65544, ld=65544), dict(ld=56), dict(ld=68), dict(logits=0x10008),
            dict(rows=0), dict(row_len=0), dict(row_len=2049), dict(pos=-1), dict(pos=16), dict(n_eos=0), dict(n_eos=-1), dict(n_eos=9),
            dict(n_eos=1, eos_ids=None), dict(child_begin=None), dict(child_tok=None), dict(child_node=None), dict(terminal=None), dict(n_nodes=0),
            dict(n_nodes=-3), dict(ban_value=float("nan")), dict(ban_value=float("inf")), dict(ban_value=0.0), dict(ban_value=1.0)]


def test_library_exports_the_symbols_and_refuses_on_the_host():
    """every refusal of include/mpv.h comes back negative before anything is launched (the pointers are not memory: a launch would fault)"""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(raw, sym)
    lib = _lib.lib()
    for over in REFUSALS:
        for name, more in (("mpv_logits_trie_mask", ()), ("mpv_logits_trie_mask_ragged", ()), ("mpv_logits_trie_mask_steps", (0xA0000,))):
            if more and set(over) == {"pos"}:
                continue                                                     # the steps entry ignores pos
            assert getattr(lib, name)(ctypes.byref(_desc(**over)), *more, None) < 0, (name, over)
            assert name.encode() in lib.mpv_last_error()
    assert lib.mpv_logits_trie_mask(None, None) < 0
    assert lib.mpv_logits_trie_mask_ragged(ctypes.byref(_desc(prompt_len=None)), None) < 0
    assert lib.mpv_logits_trie_mask_steps(ctypes.byref(_desc()), None, None) < 0


def test_ctypes_descriptor_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    cname, ct = "mpv_logits_trie_desc", _lib.LogitsTrieDesc
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


def test_trie_kernels_have_no_scratch_and_the_documented_lds_image():
    """the three instantiations in the gfx950 code object: no scratch, 1024 threads, static LDS (history, staged child run) of the
    32808 bytes DESIGN.md section 28 records.  Register, LDS and scratch figures only, read the way tests/test_isa_cpu.py reads them."""
    import tempfile
    import test_isa_cpu as isa
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for i, blob in enumerate(isa._code_objects()):
            f = os.path.join(d, f"co_{i}.elf")
            open(f, "wb").write(blob)
            txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
            for blk in txt.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                if "tm_rows" in name:
                    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                    found[name] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), scratch=g("private_segment_fixed_size"),
                                       lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    assert len(found) == 3 and sum("logits_trie_mask_kernel" in n for n in found) == 1, sorted(found)
    for k in found.values():
        assert k["scratch"] == 0 and k["lds"] == 32808 and k["vgpr"] + k["agpr"] <= 64 and k["threads"] == 1024, k


# ------------------------------------------------------------------------------ the loops on the stand-ins
def _on_cpu(monkeypatch):
    """the tiny model on the host with every stand-in, the trie's included -> (dev, counts of the calls of the trie / candidate / draw functions)"""
    import test_beam_inflight_cpu as tbi
    from youku_mplug_amd import ops
    dev = tbi._on_cpu(monkeypatch)
    stt.install(monkeypatch)
    counts = dict(trie=0, step=0)

    def counted(fn, key):
        def wrapper(*a, **kw):
            counts[key] += 1
            return fn(*a, **kw)
        return wrapper
    for name in ("logits_trie_mask", "logits_trie_mask_ragged", "logits_trie_mask_steps"):
        monkeypatch.setattr(ops, name, counted(getattr(ops, name), "trie"))
    for name in ("logprob_topk", "sample_advance", "sample_advance_ragged", "sample_advance_steps"):
        monkeypatch.setattr(ops, name, counted(getattr(ops, name), "step"))
    return dev, counts


def _tiny(dev):
    import test_beam_inflight_cpu as tbi
    model, gpt, ids, qf, _, _ = tbi._inputs(dev)
    term = _gen()._gen_config(gpt).eod_id
    return gpt, ids, qf, term


def _phrases(term, ids):
    """12 phrases of 1..4 tokens with shared prefixes, one the prefix of another, one given twice; tokens the prompts also hold"""
    a = [t for t in dict.fromkeys(ids.reshape(-1).tolist()) if t != term][:6]
    return [[a[0]], [a[0], a[1]], [a[0], a[1], a[2]], [a[0], a[3]], [a[1], a[0]], [a[1], a[1], a[4], a[5]], [a[2]], [a[3], a[3]], [a[4], a[0], a[1]],
            [a[5], a[2]], [a[5], a[4]], [a[0], a[1]]]


def _assert_phrase_rows(rows, pl, term, trie, index=None):
    for i, row in enumerate(rows.tolist()):
        gen = _gen().generated_part(row, pl, term)
        assert trie.lookup(gen) >= 0 and row[pl + len(gen)] == term, (pl, row)    # a phrase, followed by the termination id
        assert index is None or int(index[i]) == trie.lookup(gen)


LENGTHS = [3, 1, 4, 2, 3]


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("kv,mixed", [("per_sequence", False), ("shared_prefix", False), ("shared_prefix", True)])
def test_lockstep_beams_return_phrases_and_mask_once_per_step(monkeypatch, groups, kv, mixed):
    dev, counts = _on_cpu(monkeypatch)
    gpt, ids, qf, term = _tiny(dev)
    trie = _gen().PhraseTrie(_phrases(term, ids), 1024)
    gkw = dict(beam_groups=2, diversity_penalty=0.5) if groups == 2 else {}
    kw = dict(query_embeds=qf[:3], beam_size=3, num_return_gen=2, stop_token=term, kv=kv, prompt_length=LENGTHS[:3] if mixed else 2, **gkw)
    for c in (None, _gen().LogitsConstraints()):                             # no trie: the function is never called
        gpt.beam_search_batched(ids[:3], constraints=c, **kw)
        assert counts["trie"] == 0 and counts["step"] > 0
    counts.update(trie=0, step=0)
    out = gpt.beam_search_batched(ids[:3], constraints=_gen().LogitsConstraints(allowed_phrases=trie), **kw)
    assert counts["trie"] == counts["step"] <= trie.max_len + 2                # once per step; the search ends when the phrases do
    for c, o in enumerate(out):
        pl = LENGTHS[c] if mixed else 2
        assert 1 <= o.sequences.shape[0] <= 2 and o.phrase_index.shape == o.scores.shape and torch.isfinite(o.scores).all()
        _assert_phrase_rows(o.sequences, pl, term, trie, o.phrase_index)
        assert torch.equal(o.sequences[:, :pl].cpu(), ids[c, :pl].expand(o.sequences.shape[0], -1))
        if groups == 1:
            assert o.sequences.shape[0] == 2 and o.scores[0] >= o.scores[1] and o.phrase_index[0] != o.phrase_index[1]
    # a ban still wins: the constraint runs first, the trie cannot bring a banned token back
    first = {int(o.sequences[0, LENGTHS[c] if mixed else 2]) for c, o in enumerate(out)}
    ban = _gen().LogitsConstraints(allowed_phrases=trie, banned_token_ids=tuple(first))
    for c, o in enumerate(gpt.beam_search_batched(ids[:3], constraints=ban, **kw)):
        assert not (set(o.sequences[:, LENGTHS[c] if mixed else 2].tolist()) & first)


@pytest.mark.parametrize("kv,mixed", [("per_sequence", False), ("shared_prefix", False), ("shared_prefix", True)])
def test_lockstep_samples_are_phrases_with_renormalised_scores(monkeypatch, kv, mixed):
    dev, counts = _on_cpu(monkeypatch)
    gpt, ids, qf, term = _tiny(dev)
    trie = _gen().PhraseTrie(_phrases(term, ids), 1024)
    lens = LENGTHS[:3] if mixed else [2, 2, 2]
    kw = dict(query_embeds=qf[:3], prompt_length=lens if mixed else torch.tensor(lens), termination_id=term, num_samples=4, seed=3, temperature=1.3,
              top_p=0.95, kv=kv, mixed_prompts=mixed)
    gpt.sample_batched(ids[:3], constraints=_gen().LogitsConstraints(), **kw)
    assert counts["trie"] == 0 and counts["step"] > 0
    counts.update(trie=0, step=0)
    out, sc = gpt.sample_batched(ids[:3], constraints=_gen().LogitsConstraints(allowed_phrases=trie), return_scores=True, **kw)
    assert counts["trie"] == counts["step"] <= trie.max_len + 1
    seen = set()
    for r in range(out.shape[0]):
        pl = lens[r // 4]
        _assert_phrase_rows(out[r:r + 1], pl, term, trie)
        gen = _gen().generated_part(out[r], pl, term)
        seen.add(trie.lookup(gen))
        assert int(sc.count[r]) == len(gen) + 1 and torch.isfinite(sc.sum_logprob[r]) and float(sc.sum_logprob[r]) <= 0.0
        forced = [i for i in range(len(gen) + 1) if len(ref_trie.allowed_tokens(ref_trie.build(_phrases(term, ids)), gen[:i], [term], 1024)[0]) == 1]
        assert all(float(sc.token_logprob[r, pl + i]) == 0.0 for i in forced)    # one allowed token: renormalised probability 1
    assert len(seen) > 1


def test_inflight_loops_return_phrases_within_the_trie_budget(monkeypatch):
    dev, counts = _on_cpu(monkeypatch)
    gpt, ids, qf, term = _tiny(dev)
    trie = _gen().PhraseTrie(_phrases(term, ids), 1024)
    c = _gen().LogitsConstraints(allowed_phrases=trie)
    kw = dict(query_embeds=qf, prompt_length=LENGTHS, slots=2, refill_min=1)
    gpt.beam_search_inflight(ids, beam_size=3, num_return_gen=2, stop_token=term, constraints=_gen().LogitsConstraints(), max_new_tokens=3, **kw)
    assert counts["trie"] == 0 and counts["step"] > 0
    counts.update(trie=0, step=0)
    out = gpt.beam_search_inflight(ids, beam_size=3, num_return_gen=2, stop_token=term, constraints=c, **kw)
    assert counts["trie"] == counts["step"] and max(out.advances) <= trie.max_len + 1      # the default budget: the longest phrase and its end
    for i, o in enumerate(out.results):
        assert o.sequences.shape[0] == 2 and torch.isfinite(o.scores).all()
        _assert_phrase_rows(o.sequences, LENGTHS[i], term, trie, o.phrase_index)
    alone = gpt.beam_search_batched(ids[3:4], query_embeds=qf[3:4], beam_size=3, num_return_gen=2, stop_token=term, kv="shared_prefix",
                                    prompt_length=LENGTHS[3], constraints=c)[0]
    assert torch.equal(alone.sequences, out.results[3].sequences) and torch.equal(alone.phrase_index, out.results[3].phrase_index)
    counts.update(trie=0, step=0)
    smp = gpt.sample_inflight(ids, num_samples=3, seed=5, top_p=0.9, termination_id=term, constraints=c, return_scores=True, **kw)
    assert counts["trie"] == counts["step"]
    assert all(w - pl <= trie.max_len + 1 for w, pl in zip(smp.written, LENGTHS))
    for r in range(smp.tokens.shape[0]):
        _assert_phrase_rows(smp.tokens[r:r + 1], LENGTHS[r // 3], term, trie)
    assert torch.isfinite(smp.scores.sum_logprob).all()


def test_what_cannot_work_is_raised_before_the_first_launch(monkeypatch):
    dev, counts = _on_cpu(monkeypatch)
    gpt, ids, qf, term = _tiny(dev)
    g = _gen()
    trie = g.PhraseTrie(_phrases(term, ids), 1024)
    with_term = g.PhraseTrie([[9, term]], 1024)
    bkw = dict(query_embeds=qf[:2], beam_size=3, stop_token=term, prompt_length=2)
    skw = dict(query_embeds=qf[:2], prompt_length=torch.tensor([2, 2]), termination_id=term)
    ikw = dict(query_embeds=qf[:2], prompt_length=[2, 2], slots=2)
    for c, shown in ((g.LogitsConstraints(allowed_phrases=trie, min_new_tokens=1), "min_new_tokens"),
                     (g.LogitsConstraints(allowed_phrases=with_term), f"termination id {term}")):
        for call in (lambda: gpt.beam_search_batched(ids[:2], constraints=c, **bkw), lambda: gpt.sample_batched(ids[:2], constraints=c, **skw),
                     lambda: gpt.beam_search_inflight(ids[:2], constraints=c, beam_size=3, stop_token=term, **ikw),
                     lambda: gpt.sample_inflight(ids[:2], constraints=c, termination_id=term, **ikw)):
            with pytest.raises(ValueError, match=shown):
                call()
    c = g.LogitsConstraints(allowed_phrases=trie)
    for stop in (dict(stop_on_eol=True), dict(stop_on_double_eol=True)):
        with pytest.raises(ValueError, match="stop_on_eol"):
            gpt.sample_batched(ids[:2], constraints=c, **skw, **stop)
        with pytest.raises(ValueError, match="stop_on_eol"):
            gpt.sample_inflight(ids[:2], constraints=c, termination_id=term, **ikw, **stop)
    cfg = g._gen_config(gpt)
    for loop, more in ((g.beam_search_batched_loop, dict(topk_fn=1, advance_fn=1)), (g.sample_batched_loop, dict(advance_fn=1)),
                       (g.beam_inflight_loop, dict(topk_fn=1, advance_fn=1, prompt_length=[2, 2])),
                       (g.sample_inflight_loop, dict(advance_fn=1, prompt_length=[2, 2]))):
        with pytest.raises(ValueError, match="trie_fn"):                     # a trie without the function that applies it is never ignored
            loop(cfg, None, ids[:2], constraints=c, **more)
    for kw in (dict(), dict(do_sample=False), dict(do_sample=False, sampler="device")):
        with pytest.raises(ValueError, match="constraints"):                 # the per-clip host loops refuse it
            gpt.generate(ids[:1], constraints=c, **kw)
    for loop in (g.beam_search_loop, g.sample_loop):
        with pytest.raises(TypeError):
            loop(cfg, None, ids[:1], trie_fn=stt.logits_trie_mask)
    assert counts == dict(trie=0, step=0)


# ------------------------------------------------------------------------------ the exhaustive check on the stub decoder
def _stub_search(phrases, K, n_ret, **more):
    import standin_beam
    import test_beam_batched_cpu as tb
    from oracle.gen_golden import StubLogits
    g = _gen()
    vocab, cfg, tokens = tb._case(0)
    assert vocab == tc.STUB_VOCAB and tokens[0, :tb.PROMPT].tolist() == tc.PROMPT and cfg.eod_id == tc.EOS
    stubs = [StubLogits(vocab=vocab, stop=tc.EOS, seed=s) for s in tc.STUB_SEEDS]

    class Padded(tb._BatchedStubState):                                      # the kernel's vocab % 8 == 0: -inf columns, never a candidate
        def _logits(self):
            lg = super()._logits()
            return torch.cat([lg, torch.full((lg.shape[0], tc.STUB_PAD - lg.shape[1]), float("-inf"))], dim=1)
    trie = g.PhraseTrie(phrases, tc.STUB_PAD)
    out = g.beam_search_batched_loop(cfg, lambda b, m: Padded(stubs, b, m), tokens.repeat(len(stubs), 1), beam_size=K, num_return_gen=n_ret,
                                     prompt_length=tb.PROMPT, topk_fn=tb._torch_topk, advance_fn=standin_beam.beam_advance,
                                     constraints=g.LogitsConstraints(allowed_phrases=trie), trie_fn=stt.logits_trie_mask, **more)
    return out, trie, tokens.shape[1] + cfg.tokens_to_generate


@pytest.mark.parametrize("case", tc.EXHAUSTIVE, ids=lambda e: f"K{e['K']}-P{e['P']}")
def test_lockstep_search_returns_exactly_the_phrases_in_reference_order(case):
    """P <= K phrases: the search returns exactly the P phrases (a trie of P phrases has at most P allowed candidates per clip and
    step, so none is ever cut), ranked as the fp64 reference ranks them, with scores = reference sum / row length within atol 1e-5 --
    the gate of tests/test_beam_batched_cpu.py::_check_against_golden for the lockstep search against the per-clip one.  With P < K
    the candidates include banned tokens, whose hypotheses reach the store: none comes back, and no score is NaN."""
    import test_beam_batched_cpu as tb
    K, P, phrases = case["K"], case["P"], case["phrases"]
    assert phrases == tc.find_set(K, P, case["first_seed"]) and len(phrases) == P
    out, trie, row_len = _stub_search(phrases, K, K)
    for o, seed in zip(out, tc.STUB_SEEDS):
        ref = tc.reference_scores(phrases, seed)
        ranked = sorted(range(P), key=lambda i: -ref[i])
        assert all(ref[a] - ref[b] >= tc.GAP for a, b in zip(ranked, ranked[1:]))
        assert o.phrase_index.tolist() == ranked, (o.phrase_index.tolist(), ranked, ref)             # the set AND the order
        assert o.sequences.shape[0] == P and not torch.isnan(o.scores).any()
        for row, i in zip(o.sequences.tolist(), ranked):
            assert row[:tb.PROMPT] == tc.PROMPT and _gen().generated_part(row, tb.PROMPT, tc.EOS) == phrases[i]
        want = torch.tensor([ref[i] / row_len for i in ranked], dtype=torch.float32)
        assert torch.allclose(o.scores, want, rtol=0, atol=1e-5), (o.scores.tolist(), want.tolist())


def test_two_groups_on_the_stub_return_phrases_only():
    import standin_beam_groups as sg
    phrases = tc.EXHAUSTIVE[3]["phrases"]                                     # two phrases, 2 x 2 beams
    out, trie, _ = _stub_search(phrases, 2, 4, beam_groups=2, diversity_penalty=0.5, group_advance_fn=sg.beam_advance_groups)
    for o in out:
        assert 2 <= o.sequences.shape[0] <= 4 and not torch.isnan(o.scores).any() and o.group.shape == o.phrase_index.shape
        assert set(o.phrase_index.tolist()) <= {0, 1} and set(o.phrase_index[o.group == 0].tolist()) == {0, 1}
        for row, i in zip(o.sequences.tolist(), o.phrase_index.tolist()):
            assert _gen().generated_part(row, 3, tc.EOS) == phrases[i]


# ------------------------------------------------------------------------------ the caption model and the entry point on the stand-ins
def test_caption_generate_allowed_phrases_on_standins(monkeypatch):
    import test_decode_ragged_cpu as tdr
    dev, counts = _on_cpu(monkeypatch)
    model, cfg, term, vid, text = tdr._setup(dev, lengths=LENGTHS)
    g = _gen()
    phrases = _phrases(term, text.input_ids)
    trie = g.PhraseTrie(phrases, 1024)
    with pytest.raises(ValueError, match="batched=True or do_sample=True"):
        model.generate(vid, text, termination_id=term, allowed_phrases=phrases)
    with pytest.raises(ValueError, match="rerank_by_logprob"):
        model.generate(vid, text, termination_id=term, batched=True, rerank_by_logprob=True, allowed_phrases=phrases)
    with pytest.raises(ValueError, match="tokenizer"):
        model.generate(vid, text, termination_id=term, batched=True, allowed_phrases=["ab"])
    model.generate(vid, text, termination_id=term, batched=True, kv_cache="shared_prefix")
    assert counts["trie"] == 0                                               # None: no call is added
    res, info = model.generate(vid, text, termination_id=term, batched=True, kv_cache="shared_prefix", allowed_phrases=phrases, beam_size=3, num_return_gen=2)
    mixed, minfo = model.generate(vid, text, termination_id=term, batched=True, kv_cache="shared_prefix", mixed_prompts=True, allowed_phrases=trie,
                                  beam_size=3, num_return_gen=2)
    fly, finfo = model.generate(vid, text, termination_id=term, batched=True, kv_cache="shared_prefix", beam_inflight=True, clips_per_search=2,
                                allowed_phrases=trie, beam_size=3, num_return_gen=2)
    assert counts["trie"] > 0
    for i in range(len(LENGTHS)):
        assert res[i].shape == (2, text.input_ids.shape[1] + model.text_decoder.config.extra["tokens_to_generate"])
        _assert_phrase_rows(res[i], LENGTHS[i], term, trie, info[i]["phrase_index"])
        assert info[i]["scores"].shape == (2,)
        for other, oinfo in ((mixed, minfo), (fly, finfo)):                  # the same search whichever loop runs it
            assert torch.equal(other[i], res[i]) and torch.equal(oinfo[i]["phrase_index"], info[i]["phrase_index"])
    smp, sc = model.generate(vid, text, termination_id=term, do_sample=True, num_samples=3, seed=5, allowed_phrases=trie, return_scores=True)
    plain = model.generate(vid, text, termination_id=term, do_sample=True, num_samples=3, seed=5, allowed_phrases=trie)
    for i in range(len(LENGTHS)):
        _assert_phrase_rows(smp[i], LENGTHS[i], term, trie, sc[i]["phrase_index"])
        assert torch.equal(plain[i], smp[i])


def test_caption_entrypoint_allowed_phrases_flag_on_standins(tmp_path, monkeypatch):
    """--eval_allowed_phrases FILE defaults off, is refused without --eval_batched_beam, and makes pred_caption the best phrase of the
    file and pred_candidates the best with their scores"""
    import json
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
    monkeypatch.setenv("MASTER_PORT", str(44000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    seen = []
    gen = downstream.DistributedGPT3_Caption.generate

    def spy(self, image, text, *a, **kw):
        seen.append(kw)
        return gen(self, image, text, *a, **kw)
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    ch = lambda *ks: "".join(chr(0x4E00 + k) for k in ks)
    phrases = [ch(3), ch(3, 4), ch(3, 4, 5), ch(9, 3), ch(20), ch(21, 22), ch(3, 4)]
    listing = tmp_path / "phrases.txt"
    listing.write_text("\n".join(phrases[:3] + ["", "  "] + phrases[3:]) + "\n", encoding="utf-8")
    try:
        out = str(tmp_path / "closed")
        base = ["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only"]
        assert entry.get_args(base)[0].eval_allowed_phrases is None
        assert entry.read_phrases(str(listing)) == phrases
        for more in ([], ["--eval_batched_beam", "--eval_beam_groups", "2"], ["--eval_batched_beam", "--eval_sample_best_of", "2"],
                     ["--eval_batched_beam", "--eval_min_new_tokens", "1"]):
            with pytest.raises(ValueError, match="--eval_allowed_phrases needs --eval_batched_beam"):
                entry.get_args(base + ["--eval_allowed_phrases", str(listing)] + more)
        args, config = entry.get_args(base + ["--eval_allowed_phrases", str(listing), "--eval_batched_beam", "--eval_shared_kv"])
        entry.main(args, config)
        assert seen and all(kw.get("batched") and kw["allowed_phrases"].n_phrases == len(phrases) for kw in seen)
        result = json.load(open(os.path.join(out, "result", "val_caption_result.json")))
        assert result
        for rec in result:
            cands = rec["pred_candidates"]
            assert 1 <= len(cands) <= 5 and rec["pred_caption"] == cands[0]["caption"] and rec["pred_caption"] in phrases
            assert all(phrases[c["phrase_index"]] == c["caption"] and c["phrase_index"] != 6 and math.isfinite(c["score"]) for c in cands)
            assert [c["score"] for c in cands] == sorted((c["score"] for c in cands), reverse=True)
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
