"""Diverse (group) beam search in lockstep, on CPU: tests/standin_beam_groups.py (the restatement of mpv_beam_advance_groups,
include/mpv.h) against tests/standin_beam.py at one group, against the whole-vocabulary definition written directly
(tests/beam_groups_cases.py: definition_advance) and, through generation.beam_search_batched_loop(beam_groups=...) on
oracle/gen_golden.py's StubLogits, against tests/golden/search_stub.pt -- written by the reference's own beam_search: at
diversity_penalty 0 every group of every clip IS that search.  Then DistributedGPT3_Caption.generate(beam_groups=...,
rerank_by_logprob=True) and the caption entry point's --eval_beam_groups on the stand-ins of tests/standin_ops.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest
import torch

import beam_groups_cases as bg
import standin_beam
import standin_beam_groups as sg
import test_beam_batched_cpu as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
VOCAB, STOP = 41, 7


# ------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_one_group_is_the_existing_standin_bit_for_bit(K):
    """G = 1: the restatement equals tests/standin_beam.py's advance on every state array, whatever lambda is -- batches of 1 to 9 clips,
    a one-clip batch that is frozen and one that finishes in the call included, with additions to the stores and evictions (counted)"""
    events = [0, 0, 0]
    cases = ((1, 1, False, 0.0, (), ()), (1, 7, False, 2.0, (0,), ()), (1, 4, True, 0.5, (), (0,)), (3, 9, False, 0.5, (1,), (2,)),
             (4, 17, True, 1e4, (1,), (2,)), (5, 6, False, 3.0, (1,), (2,)), (9, 3, False, 0.25, (), ()), (9, 12, True, 1.0, (4,), (8,)))
    for seed, (B, Lt, first, lam, frozen, finishing) in enumerate(cases * 4):     # four draws of every case
        st, vals, idxs = bg.random_state(B, 1, K, Lt, vocab=VOCAB, stop=STOP, pos=Lt // 2, seed=100 * K + seed, first=first, frozen=frozen,
                                         finishing=finishing, banned_rows=(0,) if seed % 8 == 5 else ())
        a, b = bg.clone_state(st), bg.clone_state(st)
        step = dict(vocab=VOCAB, pos=Lt // 2, cur_len=Lt, first=first, stop_token=STOP)
        standin_beam.beam_advance(vals, idxs, a, **step)
        sg.beam_advance_groups(vals, idxs, b, groups=1, diversity_penalty=lam, **step)
        bg.assert_states_equal(a, b, (K, seed))
        for p in frozen + finishing:
            assert int(a.done[p]) == 1
        for p in finishing:
            assert int(a.hyp_count[p]) == K
        events = [x + y for x, y in zip(events, bg.store_events(st, a))]
    assert events[0] > events[1] > 0, events


def _tied_logprobs(B, G, K, seed, stop_high_rows=(), stop_mid_rows=()):
    """stub logits (vocab 37) on a grid of halves and beam scores on a grid of halves: rows 0 and 1 of every group are equal row for
    row (ties across beams at different AND at equal tokens), every row has runs of equal logits; the stop token is the row's best
    in stop_high_rows (rank below K) and among the row's middle in stop_mid_rows (rank at or above K for most K)"""
    g = torch.Generator().manual_seed(seed)
    V, rows = 37, B * G * K
    logits = torch.randint(-4, 5, (rows, V), generator=g).float() * 0.5
    scores = -torch.randint(0, 4, (rows,), generator=g).float() * 0.5
    for p in range(B * G):
        if K > 1:
            logits[p * K + 1], scores[p * K + 1] = logits[p * K], scores[p * K]
    for r in stop_high_rows:
        logits[r, STOP] = 3.0
    for r in stop_mid_rows:
        logits[r, STOP] = 1.0
    if G > 1:                                                    # the groups of clip 0 see the same distribution: the penalty must bite
        for g2 in range(1, G):
            logits[g2 * K:(g2 + 1) * K], scores[g2 * K:(g2 + 1) * K] = logits[:K], scores[:K]
    return (torch.log_softmax(logits, dim=-1) + scores[:, None]).contiguous(), scores


@pytest.mark.parametrize("lam", [0.5, 2.0, 1e4])
@pytest.mark.parametrize("K,G", [(1, 2), (2, 4), (4, 2), (3, 3), (8, 2), (2, 8)])
def test_candidate_lists_stand_for_the_whole_vocabulary(K, G, lam):
    """One advance of the restatement from the m = 2K' + (G-1)K' best of every row equals, on every state array, the definition over
    the whole vocabulary: the full log-softmax matrix, the penalty on whole rows, a full sort (DESIGN.md section 21 has the argument).
    Vocabulary 37 < what three groups' candidates cover, tied logits, stop tokens below and at rank K', first step and later steps,
    a frozen group between live ones, a group that finishes in the call, and full hypothesis stores in the groups whose best
    candidate is the stop token, with stored scores on both sides of its score: evictions, counted."""
    B, V, Lt = 3, 37, 6
    M = 2 * K + (G - 1) * K
    events = [0, 0, 0]
    for first, draw in ((True, 0), (False, 0), (True, 1), (False, 1)):
        seed = 1000 * K + 10 * G + int(first) + 100 * draw
        lp, scores = _tied_logprobs(B, G, K, seed, stop_high_rows=(0, G * K + 1 if K > 1 else G * K), stop_mid_rows=(K * (G - 1), 2 * G * K))
        st, _, _ = bg.random_state(B, G, K, Lt, vocab=V, stop=STOP, pos=3, seed=seed, first=first, frozen=(G + 1,) if G > 2 else (),
                                   finishing=(2 * G,), full=(0,))
        st.scores = scores.view(B * G, K).clone()
        # the two groups whose best candidate is the stop token (about -2 / Lt): a full store with scores around that, and an empty one
        st.hyp_score[0] = (-0.5 * torch.randint(1, 9, (K,), generator=torch.Generator().manual_seed(seed)).double()) / Lt
        st.worst[0] = st.hyp_score[0].min()
        st.hyp_count[G], st.hyp_next[G], st.worst[G] = 0, 0, 1e9
        if G > 1:                                                # clip 0's groups are in the same state too
            for n in ("hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "hyp_next", "worst", "tokens"):
                getattr(st, n)[1:G] = getattr(st, n)[0:1]
        if (2 * G) in range(B * G):                              # the finishing group: nothing the candidates reach beats its store
            lp[2 * G * K:(2 * G + 1) * K] -= 50.0
        a, b = bg.clone_state(st), bg.clone_state(st)
        step = dict(groups=G, diversity_penalty=lam, vocab=V, pos=3, cur_len=Lt, first=first, stop_token=STOP)
        vals, idxs = bg.full_logprob_lists(lp, M)
        sg.beam_advance_groups(vals, idxs, a, **step)
        bg.definition_advance(lp, b, **step)
        bg.assert_states_equal(a, b, (K, G, lam, first))
        events = [x + y for x, y in zip(events, bg.store_events(st, a))]
        assert int(a.done[2 * G]) == 1
        if G > 1 and lam == 1e4 and first:                       # the penalty did bite: clip 0's groups chose different tokens
            t0, t1 = a.next_tok[:K].tolist(), a.next_tok[K:2 * K].tolist()
            assert STOP in t0 or not set(t0) & set(t1), (t0, t1)
    assert events[0] > events[1] > 0, events


def test_large_penalty_makes_the_first_step_disjoint():
    """lambda = 1e4, first step: every group of a clip reads the same distribution; no token chosen by group g is among those chosen
    by the groups before it (37 tokens, at most 16 beams: the vocabulary allows it)"""
    from youku_mplug_amd.generation import BeamState
    for K, G in ((1, 8), (2, 4), (4, 4), (8, 2), (3, 5)):
        B, V, Lt = 2, 37, 5
        g = torch.Generator().manual_seed(K * 10 + G)
        logits = torch.randn(B, V, generator=g)
        logits[:, STOP] = -30.0
        lp = torch.log_softmax(logits, dim=-1).repeat_interleave(G * K, 0).contiguous()
        st = BeamState(torch.zeros(B * G, Lt, dtype=torch.long), K)
        vals, idxs = bg.full_logprob_lists(lp, 2 * K + (G - 1) * K)
        sg.beam_advance_groups(vals, idxs, st, groups=G, diversity_penalty=1e4, vocab=V, pos=2, cur_len=1, first=True, stop_token=STOP)
        for clip in range(B):
            seen = set()
            for grp in range(G):
                toks = st.next_tok[(clip * G + grp) * K:(clip * G + grp + 1) * K].tolist()
                assert len(set(toks)) == K and not seen & set(toks), (K, G, clip, grp, toks, seen)
                seen |= set(toks)
        # and with lambda = 0 every group chooses what group 0 chooses
        st0 = BeamState(torch.zeros(B * G, Lt, dtype=torch.long), K)
        sg.beam_advance_groups(vals, idxs, st0, groups=G, diversity_penalty=0.0, vocab=V, pos=2, cur_len=1, first=True, stop_token=STOP)
        nt = st0.next_tok.view(B, G, K)
        assert (nt == nt[:, :1]).all() and torch.equal(nt[:, 0], st.next_tok.view(B, G, K)[:, 0])


REFUSALS = [dict(K=9), dict(K=0), dict(G=9), dict(G=0), dict(K=5, G=4), dict(K=8, G=3), dict(lam=-1.0), dict(lam=float("nan")),
            dict(lam=float("inf")), dict(Lt=2049), dict(pos=-1), dict(pos=12), dict(cur_len=0), dict(vocab=0)]


def test_standin_refuses_what_the_kernel_refuses():
    from youku_mplug_amd.generation import BeamState
    for over in REFUSALS:
        c = dict(dict(K=2, G=2, lam=0.5, Lt=12, pos=3, cur_len=1, vocab=37), **over)
        K, G = c["K"], c["G"]
        st = BeamState(torch.zeros(max(G, 1), c["Lt"], dtype=torch.long), max(K, 1))
        st.beams = K
        m = max(1, (G + 1) * K)
        with pytest.raises(AssertionError):
            sg.beam_advance_groups(torch.zeros(max(G * K, 1), m), torch.zeros(max(G * K, 1), m, dtype=torch.long), st, groups=G,
                                   diversity_penalty=c["lam"], vocab=c["vocab"], pos=c["pos"], cur_len=c["cur_len"], first=True, stop_token=7)


def _group_desc(**over):
    from youku_mplug_amd import _lib
    d = _lib.BeamAdvanceGroupsDesc()
    for n, _ in _lib.BeamAdvanceGroupsDesc._fields_[:14]:
        setattr(d, n, 64 * (1 + len(n)))                                      # non-NULL, never dereferenced: a refusal comes before any launch
    d.tokens_out = 8
    d.batch, d.beams, d.groups, d.row_len, d.vocab, d.pos, d.cur_len, d.first, d.diversity_penalty, d.stop_token = 1, 2, 2, 12, 37, 3, 1, 1, 0.5, 7
    names = dict(K="beams", G="groups", lam="diversity_penalty", Lt="row_len")
    for k, v in over.items():
        setattr(d, names.get(k, k), v)
    return d


def test_library_exports_the_symbol_and_refuses_on_the_host():
    """every refusal of include/mpv.h comes back negative before anything is launched (the pointers are not memory: a launch would fault)"""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    assert "mpv_beam_advance_groups" in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "mpv_beam_advance_groups")
    fn = _lib.lib().mpv_beam_advance_groups
    for over in REFUSALS + [dict(batch=0), dict(scores=None), dict(next_tok=None), dict(tokens_out=64 * (1 + len("tokens_in")))]:
        assert fn(ctypes.byref(_group_desc(**over)), None) < 0, over
        assert b"mpv_beam_advance_groups" in _lib.lib().mpv_last_error()
    assert fn(None, None) < 0


def test_ctypes_descriptor_layout_follows_the_header_without_a_compiler():
    """the header's field declarations laid out by the C rules (natural alignment; pointers and int64_t 8 bytes, int and float 4):
    names, offsets and size equal the ctypes structure's -- a check that needs no gcc (the test below asks the compiler itself)"""
    from youku_mplug_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    cname, ct = "mpv_beam_advance_groups_desc", _lib.BeamAdvanceGroupsDesc
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, re.S).group(1)
    at, fields = 0, []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        base = decl.replace("const ", "").split()[0].rstrip("*")
        for part in decl.split(","):
            size = 8 if "*" in part else {"int": 4, "float": 4, "int64_t": 8, "double": 8, "int32_t": 4}[base]     # a declarator with * is a pointer
            at = (at + size - 1) // size * size
            fields.append((re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1], at))
            at += size
    assert fields == [(f[0], getattr(ct, f[0]).offset) for f in ct._fields_], fields
    assert (at + 7) // 8 * 8 == ctypes.sizeof(ct)


def test_ctypes_descriptor_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    cname, ct = "mpv_beam_advance_groups_desc", _lib.BeamAdvanceGroupsDesc
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


# ------------------------------------------------------------------------------ the loop against the reference's golden
def run_stub_groups(seeds, Q, *, advance, G=2, lam=0.0, K=tb.K, n_ret=2 * tb.N_RET, make_state=None, topk=tb._torch_topk, device="cpu"):
    """generation.beam_search_batched_loop(beam_groups=G) over one StubLogits clip per seed (shared with the GPU test)"""
    from oracle.gen_golden import StubLogits
    from youku_mplug_amd import generation
    vocab, cfg, tokens = tb._case(Q)
    stubs = [StubLogits(vocab=vocab, stop=7, seed=s) for s in seeds]
    B = len(seeds)
    qe = torch.zeros(B, Q, 4, device=device) if Q else None
    make_state = make_state or (lambda b, m: tb._BatchedStubState(stubs, b, m))
    return generation.beam_search_batched_loop(cfg, make_state, tokens.repeat(B, 1).to(device), query_embeds=qe, beam_size=K, num_return_gen=n_ret,
                                               prompt_length=tb.PROMPT, topk_fn=topk, beam_groups=G, diversity_penalty=lam,
                                               group_advance_fn=advance)


def check_groups_against_golden(out, seeds, Q, G=2, per_group=tb.N_RET):
    """every group of every clip reproduces the reference's beam_search (beam 4, 3 returned): tokens equal, scores within 1e-5"""
    ref = torch.load(os.path.join(GOLD, "search_stub.pt"))["beam"]
    assert len(out) == len(seeds)
    for o, s in zip(out, seeds):
        r = ref[(s, Q)]
        n = r["sequences"].shape[0]
        assert n == per_group and o.sequences.shape == (G * n, r["sequences"].shape[1]) and o.scores.shape == (G * n,)
        assert o.group.dtype == torch.int64 and o.group.tolist() == [g for g in range(G) for _ in range(n)]
        for g in range(G):
            rows = slice(g * n, (g + 1) * n)
            assert torch.equal(o.sequences[rows].cpu(), r["sequences"]), (s, Q, g, o.sequences[rows].tolist(), r["sequences"].tolist())
            assert torch.allclose(o.scores[rows], r["scores"], atol=1e-5), (s, Q, g)


@pytest.mark.parametrize("Q", [0, 3])
def test_every_group_reproduces_the_reference_golden_at_penalty_zero(Q):
    seeds = (1, 2, 3, 4)
    out = run_stub_groups(seeds, Q, advance=sg.beam_advance_groups)
    check_groups_against_golden(out, seeds, Q)
    # with a penalty group 0 is still that search; the groups behind it are not (the feature does something)
    div = run_stub_groups(seeds, Q, advance=sg.beam_advance_groups, lam=2.0)
    differs = 0
    for o, d in zip(out, div):
        assert torch.equal(d.sequences[d.group == 0], o.sequences[:tb.N_RET]) and torch.equal(d.scores[d.group == 0], o.scores[:tb.N_RET])
        differs += int(not torch.equal(d.sequences[d.group == 1], o.sequences[tb.N_RET:]))
    assert differs > 0


def test_loop_argument_checks_and_the_unchanged_default():
    from youku_mplug_amd import generation
    for bad in (dict(n_ret=5), dict(n_ret=10), dict(n_ret=0), dict(lam=-0.5), dict(lam=float("nan")), dict(G=0)):
        with pytest.raises(ValueError):
            run_stub_groups((1,), 0, advance=sg.beam_advance_groups, **bad)
    with pytest.raises(ValueError):
        run_stub_groups((1,), 0, advance=None)
    with pytest.raises(ValueError):                                          # return_scores stays refused
        generation.beam_search_batched_loop(None, None, torch.zeros(1, 3, dtype=torch.long), return_scores=True, beam_groups=2)

    # beam_groups = 1: group_advance_fn is never called, the result has no `group` field: today's calls
    def never(*a, **k):
        raise AssertionError("group_advance_fn called at beam_groups = 1")
    from oracle.gen_golden import StubLogits
    vocab, cfg, tokens = tb._case(0)
    stubs = [StubLogits(vocab=vocab, stop=7, seed=1)]
    out = generation.beam_search_batched_loop(cfg, lambda b, m: tb._BatchedStubState(stubs, b, m), tokens, beam_size=tb.K, num_return_gen=tb.N_RET,
                                              prompt_length=tb.PROMPT, topk_fn=tb._torch_topk, advance_fn=standin_beam.beam_advance,
                                              beam_groups=1, diversity_penalty=3.0, group_advance_fn=never)
    tb._check_against_golden(out, (1,), 0)
    assert not hasattr(out[0], "group")


# ------------------------------------------------------------------------------ the model and the entry point on the stand-ins
def _on_cpu(monkeypatch):
    import standin_decode_shared
    import standin_prefix_packed
    import test_sample_score_cpu as tsc
    from youku_mplug_amd import ops
    dev = tsc._on_cpu(monkeypatch)
    standin_decode_shared.install(monkeypatch)
    standin_prefix_packed.install(monkeypatch)
    monkeypatch.setattr(ops, "beam_advance_groups", sg.beam_advance_groups)
    return dev


def test_caption_generate_groups_and_rerank_on_standins(monkeypatch):
    """DistributedGPT3_Caption.generate(batched=True, beam_groups=2, rerank_by_logprob=True) on ragged prompts (two prompt-length
    groups): shapes, the group field, every clip's rows ordered by the returned normalised score, the scores those of a direct
    score_captions call on the same candidates; without rerank the rows come group by group."""
    import caption_score_cases as cs
    dev = _on_cpu(monkeypatch)
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    term = g["meta"]["eod_id"]
    sel = [0, 1, 0]
    text = cs.text_of(ids, mask, sel, dev)
    vid = video[sel].to(torch.bfloat16)
    Lt = ids.shape[1] + g["meta"]["tokens_to_generate"]
    kw = dict(termination_id=term, batched=True, beam_groups=2, diversity_penalty=1.5, beam_size=3, num_return_gen=4)
    plain = model.generate(vid, text, **kw)
    assert isinstance(plain, list) and len(plain) == 3 and all(p.shape == (4, Lt) and not p.is_cuda for p in plain)
    assert torch.equal(plain[0], plain[2])
    for lp_exp in (1.0, 0.0):
        res, scores = model.generate(vid, text, rerank_by_logprob=True, length_penalty=lp_exp, **kw)
        assert len(res) == len(scores) == 3
        for i, (r, sc, p) in enumerate(zip(res, scores, plain)):
            assert r.shape == (4, Lt) and set(sc) == {"sum_logprob", "count", "token_logprob", "group", "best"} and sc["best"] == 0
            assert sorted(sc["group"].tolist()) == [0, 0, 1, 1] and sc["group"].dtype == torch.int64
            pl = int(mask[sel[i]].sum()) - 1
            assert (r[:, :pl] == ids[sel[i], :pl]).all()
            norm = [s / float(c) ** lp_exp for s, c in zip(sc["sum_logprob"].tolist(), sc["count"].tolist())]
            assert norm == sorted(norm, reverse=True), (i, norm)
            rows_p, rows_r = [tuple(x) for x in p.tolist()], [tuple(x) for x in r.tolist()]
            assert sorted(rows_p) == sorted(rows_r)                              # a permutation of the search's rows
            for row, grp in zip(rows_r, sc["group"].tolist()):
                assert grp in {k // 2 for k, q in enumerate(rows_p) if q == row}
            # the candidates as the model cut them, scored directly
            cands = []
            for row in r[:, pl:].tolist():
                cands.append(row[:row.index(term)] if term in row else row)
            assert sc["count"].tolist() == [len(c) + 1 for c in cands]
        direct = model.score_captions(vid, text, [[row[:row.index(term)] if term in row else row
                                                   for row in r[:, int(mask[s].sum()) - 1:].tolist()] for r, s in zip(res, sel)],
                                      termination_id=term, length_penalty=lp_exp)
        for sc, d in zip(scores, direct):
            assert torch.equal(sc["sum_logprob"], d["sum_logprob"]) and torch.equal(sc["count"], d["count"]) and d["best"] == 0
            assert torch.equal(sc["token_logprob"], d["token_logprob"])
    # refusals
    for bad in (dict(batched=False), dict(do_sample=True), dict(num_return_gen=3), dict(beam_size=1), dict(diversity_penalty=-1.0)):
        with pytest.raises(ValueError):
            model.generate(vid, text, **dict(kw, **bad))
    with pytest.raises(ValueError):
        model.generate(vid, text, termination_id=term, rerank_by_logprob=True)
    with pytest.raises(ValueError):
        model.generate(vid, text, return_scores=True, **kw)
    # rerank without groups: the plain batched search's n-best, re-ranked; group is all zero
    res1, sc1 = model.generate(vid, text, termination_id=term, batched=True, num_return_gen=3, rerank_by_logprob=True)
    assert all(r.shape == (3, Lt) for r in res1) and all(s["group"].tolist() == [0, 0, 0] for s in sc1)


def test_rerank_scores_a_hypothesis_that_fills_the_row_at_the_position_limit(monkeypatch):
    """The termination token banned and tokens_to_generate chosen so that query slots + row = max_position_embeddings: every hypothesis
    fills its row, the re-rank scores it whole plus the terminator -- whose input sits at the last row of the position table, one
    position more than the search fed -- and nothing falls outside the table."""
    import caption_score_cases as cs
    dev = _on_cpu(monkeypatch)
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    term = g["meta"]["eod_id"]
    max_pos = model.text_decoder.config.max_position_embeddings
    model.text_decoder.config.extra.update(tokens_to_generate=max_pos - model.num_learnable_token - ids.shape[1])
    text = cs.text_of(ids, mask, [0, 1], dev)
    res, scores = model.generate(video.to(torch.bfloat16), text, termination_id=term, batched=True, beam_groups=2, diversity_penalty=1.0, beam_size=2,
                                 num_return_gen=2, rerank_by_logprob=True, banned_token_ids=[term])
    Lt = max_pos - model.num_learnable_token
    for i, (r, sc) in enumerate(zip(res, scores)):
        pl = int(mask[i].sum()) - 1
        assert r.shape == (2, Lt) and not (r[:, pl:] == term).any()
        assert sc["count"].tolist() == [Lt - pl + 1] * 2 and torch.isfinite(sc["sum_logprob"]).all()


def test_caption_entrypoint_group_flags_on_standins(tmp_path, monkeypatch):
    """downstream/run_caption_distributed_gpt3.py --evaluate_only with --eval_beam_groups / --eval_diversity_penalty on the stand-ins:
    pred_candidates beside pred_caption (its first entry), combined with --eval_shared_kv and a constraint flag; without the flags the
    generate calls carry none of the new keywords and the records have the parent's keys."""
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
        seen.append(dict(kw))
        return gen(self, image, text, *a, **kw)
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    merged = {}
    base = ["--config", cfg, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only"]
    try:
        for name, flags in (("plain", []), ("groups", ["--eval_beam_groups", "2", "--eval_diversity_penalty", "1.5"]),
                            ("combined", ["--eval_beam_groups", "4", "--eval_diversity_penalty", "0.5", "--eval_shared_kv", "--eval_no_repeat_ngram", "2"])):
            out = str(tmp_path / name)
            args, config = entry.get_args(base + ["--output_dir", out] + flags)
            assert args.eval_beam_groups == (1 if not flags else int(flags[1]))
            seen.clear()
            entry.main(args, config)
            new = {"beam_groups", "diversity_penalty", "rerank_by_logprob"}
            if flags:
                G = int(flags[1])
                assert seen and all(s["beam_groups"] == G and s["batched"] and s["rerank_by_logprob"] and s["beam_size"] == min(5, 16 // G) for s in seen)
                assert name != "combined" or all(s["kv_cache"] == "shared_prefix" and s["no_repeat_ngram_size"] == 2 for s in seen)
            else:
                assert seen and all(s == {} for s in seen), seen                            # the parent's calls: no keyword at all
            merged[name] = json.load(open(os.path.join(out, "result", "val_caption_result.json")))
        for bad in (["--eval_beam_groups", "9"], ["--eval_beam_groups", "0"], ["--eval_diversity_penalty", "1.0"],
                    ["--eval_beam_groups", "2", "--eval_diversity_penalty", "-1"], ["--eval_beam_groups", "2", "--eval_sample_best_of", "2"]):
            with pytest.raises(ValueError):
                entry.get_args(base + ["--output_dir", str(tmp_path / "bad")] + bad)
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert len(merged["plain"]) == 5 and all(set(r) == {"video_id", "pred_caption", "gold_caption"} for r in merged["plain"])
    for name, n in (("groups", 10), ("combined", 16)):
        assert len(merged[name]) == 5
        for x, y in zip(merged["plain"], merged[name]):
            assert set(y) == {"video_id", "pred_caption", "gold_caption", "pred_candidates"}
            assert x["video_id"] == y["video_id"] and x["gold_caption"] == y["gold_caption"]
            assert 1 <= len(y["pred_candidates"]) <= n and y["pred_caption"] == y["pred_candidates"][0]
            assert all(isinstance(c, str) for c in y["pred_candidates"])
