"""Test-only restatement of mpv_beam_advance (include/mpv.h; youku_mplug_amd.ops.beam_advance) in torch / Python on the same state
arrays (generation.BeamState): the `advance_fn` of generation.beam_search_batched_loop on CPU, and what the kernel is compared with
bit for bit on the GPU.  Per clip it is one iteration of generation.beam_search_loop, written on arrays instead of Python objects;
Python floats are fp64, as the kernel's heap arithmetic."""
import torch

MAX_BEAMS, MAX_ROW_LEN = 8, 2048


def beam_advance(cand_val, cand_idx, st, *, vocab, pos, cur_len, first, stop_token):
    B, K, Lt = st.batch, st.beams, st.row_len
    assert 1 <= K <= MAX_BEAMS and 1 <= Lt <= MAX_ROW_LEN and 0 <= pos < Lt and cur_len >= 1
    assert cand_val.dtype == torch.float32 and cand_idx.dtype == torch.int64 and tuple(cand_val.shape) == tuple(cand_idx.shape) == (B * K, 2 * K)
    dev = cand_val.device
    vals, idxs = cand_val.cpu().view(B, K, 2 * K).tolist(), cand_idx.cpu().view(B, K, 2 * K).tolist()
    host = {n: getattr(st, n).cpu() for n in ("tokens", "scores", "hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "hyp_next", "worst",
                                              "done", "src_row", "next_tok")}
    tin, tout = host["tokens"], host["tokens"].clone()          # a frozen clip's rows go to the other table unchanged
    stop_token = int(stop_token)
    for b in range(B):
        rows = range(b * K, (b + 1) * K)
        if int(host["done"][b]):
            for j, r in enumerate(rows):
                host["src_row"][r], host["next_tok"][r] = r, stop_token
            continue
        cand = [(vals[b][beam][j], beam, idxs[b][beam][j], beam * 2 * K + j) for beam in range(1 if first else K) for j in range(2 * K)]
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
    for n, t in host.items():
        if n != "tokens":
            getattr(st, n).copy_(t.to(dev))
    st.tokens_alt.copy_(tout.to(dev))
    st.tokens, st.tokens_alt = st.tokens_alt, st.tokens
    return st.src_row, st.next_tok
