"""The reference of the CIDEr tests, TEST INFRASTRUCTURE ONLY: what include/mpv.h (mpv_caption_cider) states, restated with dicts in
plain fp64 Python, independently of generation.CiderStats and of the kernel -- n-gram counts per caption, document frequencies per
clip, tf-idf vectors, clipped cosine and the Gaussian length penalty -- and the self-critical loss of
DistributedGPT3_Caption.forward_scst, restated on oracle.restate's fp32 decoder for autograd.  Checked itself against the recorded scores
of the reference project's scorer (tests/golden/cider_reference.json, tools/gen_golden_cider.py) in tests/test_cider_cpu.py."""
import math

ORDERS = 4
MASK64 = (1 << 64) - 1


def candidate(row, start, term, width):
    """the caption of a table row: the tokens from `start` up to the first `term` at or behind it, or the width"""
    out = []
    for t in row[start:width]:
        if t == term:
            break
        out.append(int(t))
    return out


def counts(caption):
    """{n-gram tuple: occurrences} over the orders 1 .. 4"""
    c = {}
    for n in range(1, ORDERS + 1):
        for i in range(len(caption) - n + 1):
            g = tuple(caption[i:i + n])
            c[g] = c.get(g, 0) + 1
    return c


def doc_freq(reference_sets):
    """-> ({n-gram: number of clips with a reference that holds it}, log(number of clips))"""
    df = {}
    for refs in reference_sets:
        for g in set(g for ref in refs for g in counts(ref)):
            df[g] = df.get(g, 0) + 1
    return df, math.log(float(len(reference_sets)))


def vectors(caption, df, log_ref_len):
    """-> (vec: one {n-gram: tf * idf} per order, norm: one float per order)"""
    vec = [dict() for _ in range(ORDERS)]
    sq = [0.0] * ORDERS
    for g, tf in counts(caption).items():
        n = len(g) - 1
        vec[n][g] = float(tf) * (log_ref_len - math.log(max(1.0, float(df.get(g, 0)))))
        sq[n] += vec[n][g] ** 2
    return vec, [math.sqrt(x) for x in sq]


def pair_values(cand, ref, df, log_ref_len, sigma=6.0):
    """the four per-order similarities of one (candidate, reference) pair after the length penalty"""
    vc, nc = vectors(cand, df, log_ref_len)
    vr, nr = vectors(ref, df, log_ref_len)
    delta = float(len(cand) - len(ref))
    out = []
    for n in range(ORDERS):
        val = 0.0
        for g, x in vc[n].items():
            y = vr[n].get(g, 0.0)
            val += min(x, y) * y
        if nc[n] != 0 and nr[n] != 0:
            val /= nc[n] * nr[n]
        out.append(val * math.exp(-(delta ** 2) / (2 * sigma ** 2)))
    return out


def score_of(pairs):
    """a candidate's score from its pairs' values: 10 * mean_n(sum_r pair / R), 0.0 without references"""
    if not pairs:
        return 0.0
    return 10.0 * sum(sum(p[n] for p in pairs) / len(pairs) for n in range(ORDERS)) / ORDERS


def case_values(case, sigma=6.0):
    """a case of tests/cider_cases.py -> (pair [pairs][4], score [rows_a]) in the kernel's order, from the TABLES (not from the lists
    the tables were built from)"""
    ca = [candidate(r, s, case["term"], case["width_a"]) for r, s in zip(case["tok_a"].tolist(), case["start_a"])]
    cb = [candidate(r, s, case["term"], case["width_b"]) for r, s in zip(case["tok_b"].tolist(), case["start_b"])]
    df, log_ref_len = doc_freq(case["corpus"])
    pair, score = [], []
    for g in range(len(case["begin_a"]) - 1):
        for i in range(case["begin_a"][g], case["begin_a"][g + 1]):
            mine = [pair_values(ca[i], cb[j], df, log_ref_len, sigma) for j in range(case["begin_b"][g], case["begin_b"][g + 1])]
            pair += mine
            score.append(score_of(mine))
    return pair, score


def corpus_cider(hyps, reference_sets, sigma=6.0):
    """one hypothesis per clip against its references, df from these references -> (mean, per-clip scores)"""
    df, log_ref_len = doc_freq(reference_sets)
    scores = [score_of([pair_values(h, r, df, log_ref_len, sigma) for r in refs]) for h, refs in zip(hyps, reference_sets)]
    return sum(scores) / len(scores), scores


def mix(x):
    """the splitmix64 finaliser, restated: the slot rule of the corpus table"""
    x &= MASK64
    x ^= x >> 30
    x = x * 0xbf58476d1ce4e5b9 & MASK64
    x ^= x >> 27
    x = x * 0x94d049bb133111eb & MASK64
    return x ^ x >> 31


def key_of(ngram):
    return sum((int(t) + 1) << (16 * i) for i, t in enumerate(ngram))


# ------------------------------------------------------------------------------------------------ the self-critical loss
def scst_weights(table, rewards, prompt_len, term, baseline="mean_others", greedy=None):
    """table: the padded rollouts [B * N][W] (row b * N + s, lists), rewards [B][N], greedy [B] -> (weights [B * N][W - prompt_len] over
    the generated columns: A / T up to and including the first `term`, 0 behind it; T), in fp64 on the host"""
    B, N = len(rewards), len(rewards[0])
    live, T = [], 0
    for row in table:
        gen = row[prompt_len:]
        n = gen.index(term) + 1 if term in gen else len(gen)
        live.append([1.0] * n + [0.0] * (len(gen) - n))
        T += n
    out = []
    for b in range(B):
        for s in range(N):
            if baseline == "greedy":
                adv = rewards[b][s] - greedy[b]
            else:
                adv = rewards[b][s] - sum(rewards[b][m] for m in range(N) if m != s) / (N - 1)
            out.append([adv * x / T for x in live[b * N + s]])
    return out, T


def scst_loss(video, prompts, table, weights, sd, cfg):
    """fp32 autograd restatement of forward_scst's loss on oracle.restate: video [B, ...], prompts: unused beyond the table (the table
    rows carry them), table int64 [B * N, W] (row b * N + s), weights fp32 [B * N, W - pl] -> (loss, query_features [B, Q, H] with
    retained grad).  sd: the fp32 state dict; tensors in it that require grad receive gradients."""
    import torch
    import torch.nn.functional as F
    from oracle import restate
    B = video.shape[0]
    R, W = table.shape
    N = R // B
    pl = W - weights.shape[1]
    image_embeds = restate.timesformer(video, sd, cfg)
    image_query = restate.attention_pool(sd["learnable_queries"].repeat(B, 1, 1), image_embeds, sd, cfg)
    qf = restate.visual_connect(image_query, sd)
    qf.retain_grad()
    Q = qf.shape[1]
    rows = qf.repeat_interleave(N, dim=0)                                                      # row b * N + s
    emb = F.embedding(table, sd["text_decoder.dist_model.language_model.embedding.word_embeddings.weight"])
    targets = torch.cat([table[:, 1:], table[:, :1]], dim=1)
    targets = torch.cat([torch.full((R, Q), 100, dtype=torch.long, device=table.device), targets], dim=1)
    dummy = torch.ones((R, Q + W - 1), device=table.device)
    out = restate.gpt_forward(torch.cat([rows, emb], dim=1), targets, dummy, sd, cfg)
    ce = out["losses"][:, Q + pl - 1:Q + W - 1]                                                # position Q + c - 1 predicts column c
    return (ce * weights.to(ce.dtype)).sum(), qf
