"""Test-only restatement of mpv_beam_advance_groups (include/mpv.h; youku_mplug_amd.ops.beam_advance_groups) in torch / Python on
the same state arrays: a generation.BeamState whose st.batch pseudo-clips are (clip, group) pairs, `groups` consecutive ones per
clip.  It is the `group_advance_fn` of generation.beam_search_batched_loop on CPU, and what the kernel is compared with bit for bit
on the GPU.  Per (clip, group) it is tests/standin_beam.py's iteration on the penalised values; the penalty is fp32 (one rounded
product, then one rounded difference), everything behind it Python floats (fp64), as in the kernel."""
import math
import struct

import torch

MAX_BEAMS, MAX_GROUPS, MAX_SEQ, MAX_ROW_LEN = 8, 8, 16, 2048


def _f32(x: float) -> float:
    try:
        return struct.unpack("f", struct.pack("f", x))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def penalised(v: float, lam: float, c: int) -> float:
    """v - lam * c as the kernel rounds it: an fp32 product, then an fp32 difference; v itself when c = 0.  Both are computed in fp64
    and rounded to fp32: for fp32 operands the fp64 product is exact and the fp64 difference is rounded with more than 2 * 24 + 2
    bits, so the second rounding gives the correctly rounded fp32 result."""
    if c == 0:
        return v
    return _f32(_f32(v) - _f32(_f32(lam) * float(c)))


def beam_advance_groups(cand_val, cand_idx, st, *, groups, diversity_penalty, vocab, pos, cur_len, first, stop_token):
    G, K, Lt = int(groups), st.beams, st.row_len
    lam = float(diversity_penalty)
    assert 1 <= K <= MAX_BEAMS and 1 <= G <= MAX_GROUPS and G * K <= MAX_SEQ
    assert math.isfinite(lam) and lam >= 0.0
    assert 1 <= Lt <= MAX_ROW_LEN and 0 <= pos < Lt and cur_len >= 1 and vocab >= 1
    assert st.batch >= G and st.batch % G == 0
    B, M = st.batch // G, 2 * K + (G - 1) * K
    assert cand_val.dtype == torch.float32 and cand_idx.dtype == torch.int64 and tuple(cand_val.shape) == tuple(cand_idx.shape) == (B * G * K, M)
    dev = cand_val.device
    vals, idxs = cand_val.cpu().view(B * G, K, M).tolist(), cand_idx.cpu().view(B * G, K, M).tolist()
    host = {n: getattr(st, n).cpu() for n in ("tokens", "scores", "hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "hyp_next", "worst",
                                              "done", "src_row", "next_tok")}
    tin, tout = host["tokens"], host["tokens"].clone()          # a frozen group's rows go to the other table unchanged
    stop_token = int(stop_token)
    for clip in range(B):
        emitted = []                                            # the tokens of this call's next beams of the groups before, with multiplicity
        for g in range(G):
            b = clip * G + g
            rows = range(b * K, (b + 1) * K)
            if int(host["done"][b]):
                for r in rows:
                    host["src_row"][r], host["next_tok"][r] = r, stop_token
                continue
            cand = [(penalised(vals[b][beam][j], lam, emitted.count(idxs[b][beam][j])), beam, idxs[b][beam][j], beam * M + j)
                    for beam in range(1 if first else K) for j in range(M)]
            cand.sort(key=lambda c: (-c[0], c[1] * vocab + c[2], c[3]))
            cand = cand[:2 * K]
            count, nxt, worst = int(host["hyp_count"][b]), int(host["hyp_next"][b]), float(host["worst"][b])
            next_beams = []
            for rank, (v, beam, tok, _) in enumerate(cand):
                if len(next_beams) == K:
                    break
                if tok != stop_token:
                    next_beams.append((v, beam, tok))
                    continue
                if rank >= K:
                    continue
                score = v / float(Lt)
                if not (count < K or score > worst):
                    continue
                if count < K:
                    slot, count, worst = count, count + 1, min(score, worst)
                else:
                    slot = min(range(K), key=lambda s: (float(host["hyp_score"][b, s]), int(host["hyp_order"][b, s])))
                    worst = min([score] + [float(host["hyp_score"][b, s]) for s in range(K) if s != slot])
                host["hyp_score"][b, slot], host["hyp_order"][b, slot] = score, nxt
                host["hyp_tokens"][b, slot] = tin[b, beam]
                nxt += 1
            done = count == K and worst >= cand[0][0] / float(cur_len)
            host["hyp_count"][b], host["hyp_next"][b], host["worst"][b], host["done"][b] = count, nxt, worst, int(done)
            for j, r in enumerate(rows):
                if done:
                    host["src_row"][r], host["next_tok"][r] = r, stop_token
                    continue
                v, beam, tok = next_beams[j] if j < len(next_beams) else (float("-inf"), j, stop_token)
                tout[b, j] = tin[b, beam]
                tout[b, j, pos] = tok
                host["scores"][b, j], host["src_row"][r], host["next_tok"][r] = v, b * K + beam, tok
            if not done:
                emitted += [tok for _, _, tok in next_beams]
    for n, t in host.items():
        if n != "tokens":
            getattr(st, n).copy_(t.to(dev))
    st.tokens_alt.copy_(tout.to(dev))
    st.tokens, st.tokens_alt = st.tokens_alt, st.tokens
    return st.src_row, st.next_tok
