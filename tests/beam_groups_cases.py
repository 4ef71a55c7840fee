"""Shared by tests/test_beam_groups_cpu.py and tests/test_beam_groups_gpu.py: random mid-search states of the group beam search
(generation.BeamState over (clip, group) pseudo-clips) with candidate lists shaped like mpv_logprob_topk's output, the comparison of
two states on every array, and the whole-vocabulary definition of one advance written directly (a full log-probability matrix, the
penalty applied to whole rows, a sort, then tests/standin_beam.py's iteration per group)."""
import types

import torch

import standin_beam

STATE_ARRAYS = ("tokens", "tokens_alt", "scores", "hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "hyp_next", "worst", "done", "src_row",
                "next_tok")
CANARY = {torch.int64: -77, torch.int32: -77, torch.float32: -77.5, torch.float64: -77.5}


def random_state(B, G, K, Lt, *, vocab, stop, pos, seed, first=False, frozen=(), finishing=(), banned_rows=(), full=(), levels=4, stop_rate=0.4):
    """-> (BeamState of B * G pseudo-clips x K beams, cand_val, cand_idx [B*G*K, m]).  The candidate rows are what a top-m writes:
    values descending, distinct tokens, the lower token first among equal values.  Values are drawn from `levels` steps of 0.25, so
    ties within a row, across the beams of a group and across groups are the rule, not the exception; about `stop_rate` of the rows
    carry the stop token, half of them among the row's best two (rank below K), half at a random rank (at and above K included).
    The hypothesis stores: about half are full (and every one in `full`), and the stored scores lie on the grid of the scores a stop
    candidate can get -- double(-0.25 n) / Lt for the candidates' range of n and one step beyond on either side -- so a full store
    sees candidates below `worst` (refused), equal to it (refused) and above it (the lowest goes: eviction), with equal stored scores
    under different insertion numbers (the eviction's tie rule).  frozen: pseudo-clips whose done flag is set; finishing:
    pseudo-clips built to pass the done test in this call (a full store with a worst score above anything the candidates reach);
    banned_rows: rows whose candidate values are all -inf.  Every array the call writes conditionally holds a canary first."""
    from youku_mplug_amd.generation import BeamState
    g = torch.Generator().manual_seed(seed)
    P, M = B * G, 2 * K + (G - 1) * K
    assert M <= vocab - 1 and 0 <= pos < Lt
    st = BeamState(torch.zeros(P, Lt, dtype=torch.long), K)
    st.tokens = torch.randint(0, vocab, (P, K, Lt), generator=g)
    st.tokens_alt = torch.full_like(st.tokens, CANARY[torch.int64])
    st.scores = -torch.randint(0, 3 * levels, (P, K), generator=g).float() * 0.25
    st.hyp_tokens = torch.randint(0, vocab, (P, K, Lt), generator=g)
    st.src_row = torch.full((P * K,), CANARY[torch.int64], dtype=torch.int64)
    st.next_tok = torch.full((P * K,), CANARY[torch.int64], dtype=torch.int64)
    for p in range(P):
        count = int(torch.randint(0, K + 1, (1,), generator=g))
        if p in finishing or p in full or float(torch.rand(1, generator=g)) < 0.5:
            count = K
        order = torch.randperm(K, generator=g)[:count]
        st.hyp_count[p], st.hyp_next[p] = count, count + int(torch.randint(0, 3, (1,), generator=g))
        st.hyp_order[p, :count] = order.to(torch.int32)
        hs = (-0.25 * torch.randint(3, 6 * levels - 4, (count,), generator=g).double()) / Lt       # candidates: n in [4, 4 * levels + 2]
        if p in finishing:
            hs = torch.full((K,), -1e-6, dtype=torch.float64)
        st.hyp_score[p, :count] = hs
        st.worst[p] = float(hs.min()) if count == K else (float(hs.min()) if count else 1e9)
        st.done[p] = 1 if p in frozen else 0
    vals = torch.empty(P * K, M)
    idxs = torch.empty(P * K, M, dtype=torch.int64)
    for r in range(P * K):
        toks = torch.randperm(vocab, generator=g)
        toks = toks[toks != stop][:M]
        if float(torch.rand(1, generator=g)) < stop_rate:
            toks[int(torch.randint(0, 2 if float(torch.rand(1, generator=g)) < 0.5 else M, (1,), generator=g))] = stop
        v = (st.scores.view(-1)[r] - 1.0 - torch.randint(0, levels, (M,), generator=g).float() * 0.25).sort(descending=True).values
        if r // K in finishing:
            v = v - 50.0
        if r in banned_rows:
            v = torch.full((M,), float("-inf"))
        # within equal values the lower token comes first, as mpv_logprob_topk orders them
        pairs = sorted(zip(v.tolist(), toks.tolist()), key=lambda x: (-x[0], x[1]))
        vals[r], idxs[r] = torch.tensor([x for x, _ in pairs]), torch.tensor([t for _, t in pairs])
    return st, vals.contiguous(), idxs.contiguous()


def clone_state(st, device=None):
    c = types.SimpleNamespace(batch=st.batch, beams=st.beams, row_len=st.row_len)
    for n in STATE_ARRAYS:
        setattr(c, n, getattr(st, n).clone().to(device or getattr(st, n).device))
    return c


def assert_states_equal(a, b, what=""):
    """every state array and output, bit for bit (NaN-free by construction; -inf compares equal to -inf)"""
    for n in STATE_ARRAYS:
        x, y = getattr(a, n).cpu(), getattr(b, n).cpu()
        assert x.dtype == y.dtype and x.shape == y.shape, (what, n)
        assert torch.equal(x, y), (what, n, (x != y).nonzero()[:4].tolist())


def store_events(before, after):
    """what one advance did to the hypothesis stores, read off the state arrays: (additions, evictions, evictions out of a store whose
    lowest score was held by more than one entry).  An eviction is an addition that did not raise the count."""
    add = ev = tied = 0
    for p in range(before.batch):
        d_next = int(after.hyp_next[p]) - int(before.hyp_next[p])
        e = d_next - (int(after.hyp_count[p]) - int(before.hyp_count[p]))
        add, ev = add + d_next, ev + e
        if e and int(before.hyp_count[p]) == before.beams:
            hs = before.hyp_score[p].cpu()
            tied += int((hs == hs.min()).sum() > 1)
    return add, ev, tied


def full_logprob_lists(lp, m):
    """the m best of every row of a full [rows, V] matrix: value descending, lower token first (a stable sort), as mpv_logprob_topk"""
    v, i = torch.sort(lp, dim=-1, descending=True, stable=True)
    return v[:, :m].contiguous(), i[:, :m].contiguous()


def definition_advance(lp, st, *, groups, diversity_penalty, vocab, pos, cur_len, first, stop_token):
    """One call of the contract from its DEFINITION over the whole vocabulary: lp fp32 [B*G*K, V] is log_softmax + scores of every
    row.  Per clip, group after group: the group's whole rows are lowered by lambda * c(token) (fp32 product, fp32 difference, rows of
    c = 0 untouched), sorted in full, and the group -- seen as a one-clip BeamState -- goes through ONE iteration of the ungrouped
    contract (tests/standin_beam.py) on the first 2K of every row.  What it emitted (a live group's real next beams) is counted
    for the groups behind it."""
    G, K = groups, st.beams
    B = st.batch // G
    lam = torch.tensor(float(diversity_penalty), dtype=torch.float32)
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (st.batch * K, vocab)
    out_tokens = st.tokens.clone()
    for clip in range(B):
        counts = torch.zeros(vocab, dtype=torch.float32)
        for g in range(G):
            p = clip * G + g
            rows = lp[p * K:(p + 1) * K]
            pen = lam * counts                                              # fp32 product
            rows = torch.where(counts[None] > 0, rows - pen[None], rows)    # fp32 difference
            v, i = full_logprob_lists(rows, 2 * K)
            sub = types.SimpleNamespace(batch=1, beams=K, row_len=st.row_len)
            for n in STATE_ARRAYS:
                t = getattr(st, n)
                setattr(sub, n, (t[p * K:(p + 1) * K] if n in ("src_row", "next_tok") else t[p:p + 1]).clone())
            was_done = bool(sub.done[0])
            standin_beam.beam_advance(v, i, sub, vocab=vocab, pos=pos, cur_len=cur_len, first=first, stop_token=stop_token)
            sub.src_row += p * K                                            # the one-clip call numbers its rows from 0
            for n in STATE_ARRAYS:
                if n in ("tokens", "tokens_alt"):
                    continue
                t = getattr(st, n)
                (t[p * K:(p + 1) * K] if n in ("src_row", "next_tok") else t[p:p + 1]).copy_(getattr(sub, n))
            out_tokens[p] = sub.tokens[0]                                   # the stand-in has swapped: tokens is the table it wrote
            if not was_done and not bool(sub.done[0]):
                for j in range(K):
                    if int(sub.next_tok[j]) != stop_token:                  # a real next beam (a slot left over carries the stop token)
                        counts[int(sub.next_tok[j])] += 1
    st.tokens_alt.copy_(out_tokens)
    st.tokens, st.tokens_alt = st.tokens_alt, st.tokens
    return st.src_row, st.next_tok
