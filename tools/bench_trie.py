"""What closed-vocabulary decoding costs, on one GPU: the decoder, the constants and the method of
tools/bench_caption_batched.py (the 1.3B dims with synthetic weights, 256 query slots, 8-token prompts, kv="shared_prefix").

  (a) mask      ops.logits_trie_mask alone, on 160 and 512 rows x 51200 columns, for synthetic tries of 45, 10 000 and 100 000 phrases
                of 2..6 tokens, with every row at the root, at mid depth (two tokens into a phrase) or dead.  HIP events around 20
                launches; every configuration runs once before the timed rounds and the configurations alternate inside a round.
  (b) loops     a 32 clips x 5 beams lockstep beam search and a 128-clips-through-32-slots in-flight beam search, with and without
                a 10 000-phrase trie whose phrases all hold 6 tokens, alternated.  Both runs are given 7 steps per clip: the
                unconstrained one (constraints=None) a budget of 7 (tokens_to_generate / max_new_tokens; a random-weight decoder
                closes no hypothesis store before it), the constrained one ends every phrase at step 7.  The decoder steps and the
                mask launches of every run are counted and written next to the times.  The timing condition: the median with the
                trie exceeds the median without it by no more than mask launches x the mask launch's own time from (a) plus the
                larger run-to-run spread of the two; the baseline is the unconstrained loop of this process.
  (c) crossover for 45 and 1000 phrases of 2..6 tokens and 8 clips: the constrained search (5 beams) against scoring every phrase of
                every clip, one packed continuation pass per clip over all phrases (forward_prefix + forward_continuation_packed,
                what DistributedGPT3_Caption.score_captions runs).

    python tools/bench_trie.py [--out profiles/trie_decode.json] [--rounds 3]

No ratio is promised: the JSON holds medians and run-to-run spreads.  The process exits with status 1 if the timing condition of (b)
does not hold."""
import argparse
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_caption_batched as base  # noqa: E402  (the decoder's dims and the constants of the caption benchmark)
from bench_mixed_prompts import summary, timed  # noqa: E402

ROWS, SIZES, LAUNCHES = (160, 512), (45, 10000, 100000), 20
CLIPS_LOCKSTEP, CLIPS_INFLIGHT, SLOTS, BEAMS, PHRASE_LEN = 32, 128, 32, 5, 6
CROSS_CLIPS, CROSS_SIZES = 8, (45, 1000)


def synthetic_phrases(n, seed, lo=2, hi=6):
    """n distinct phrases of lo..hi tokens over [8, VOCAB); first tokens from a skewed alphabet, so that prefixes are shared"""
    rng = random.Random(seed)
    seen, out = set(), []
    heads = max(8, int(n ** 0.75))
    while len(out) < n:
        ph = [8 + rng.randrange(heads)] + [8 + rng.randrange(base.VOCAB - 8) if rng.random() < 0.5 else 8 + rng.randrange(64)
                                           for _ in range(rng.randint(lo, hi) - 1)]
        if tuple(ph) not in seen:
            seen.add(tuple(ph))
            out.append(ph)
    return out


def mask_section(dev, rounds):
    from youku_mplug_amd import generation, ops
    gen = torch.Generator().manual_seed(3)
    configs = []
    for n in SIZES:
        phrases = synthetic_phrases(n, n)
        trie = generation.PhraseTrie(phrases, base.VOCAB)
        for rows in ROWS:
            logits = (torch.randn(rows, base.VOCAB, generator=gen) * 3.0).to(torch.bfloat16).to(dev)
            for where in ("root", "mid", "dead"):
                tokens = torch.full((rows, 16), base.STOP, dtype=torch.int64)
                for r in range(rows):
                    ph = phrases[(r * 7919) % n]
                    tokens[r, 8:10] = torch.tensor(ph[:2] if where != "dead" else [base.STOP, ph[0]])
                pos = 8 if where == "root" else 10
                configs.append(dict(name=f"{n}_phrases_{rows}_rows_{where}", trie=trie, logits=logits, work=logits.clone(), tokens=tokens.to(dev),
                                    pos=pos, root_children=trie.child_begin[1], nodes=trie.n_nodes))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(c):
        c["work"].copy_(c["logits"])
        start.record()
        for _ in range(LAUNCHES):
            ops.logits_trie_mask(c["work"], c["tokens"], pos=c["pos"], trie=c["trie"], prompt_len_all=8, eos_ids=[base.STOP],
                                 ban_value=generation.BAN_BEAM)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / LAUNCHES              # us per launch
    for c in configs:
        run(c)
    times = {c["name"]: [] for c in configs}
    for _ in range(rounds):
        for c in configs:
            times[c["name"]].append(run(c))
    out = {}
    for c in configs:
        v = times[c["name"]]
        med = sorted(v)[len(v) // 2]
        out[c["name"]] = dict(us_per_launch=v, median_us=med, run_to_run_spread=(max(v) - min(v)) / med, root_children=c["root_children"],
                              nodes=c["nodes"], bytes_written_at_most=c["logits"].numel() * 2)
        print(f"[mask] {c['name']}: {med:.1f} us ({out[c['name']]['run_to_run_spread']:.1%})", flush=True)
    return out


def loops_section(gpt, dev, rounds, mask_us):
    from youku_mplug_amd import generation, ops
    counts = dict(steps=0, masks=0)
    step, masks = generation.SharedPrefixDecodeState.step, {n: getattr(ops, n) for n in ("logits_trie_mask", "logits_trie_mask_steps")}

    def counted_step(self, *a, **k):
        counts["steps"] += 1
        return step(self, *a, **k)

    def counted_mask(fn):
        def run(*a, **k):
            counts["masks"] += 1
            return fn(*a, **k)
        return run
    generation.SharedPrefixDecodeState.step = counted_step
    for n, fn in masks.items():
        setattr(ops, n, counted_mask(fn))
    gen = torch.Generator().manual_seed(1)
    phrases = synthetic_phrases(10000, 6, lo=PHRASE_LEN, hi=PHRASE_LEN)
    trie = generation.PhraseTrie(phrases, base.VOCAB)
    steps = PHRASE_LEN + 1
    gpt.config.extra["tokens_to_generate"] = steps
    plain = None
    closed = generation.LogitsConstraints(allowed_phrases=trie)
    qe = (torch.randn(CLIPS_INFLIGHT, base.Q, base.HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
    tokens = torch.randint(8, base.VOCAB, (CLIPS_INFLIGHT, base.PROMPT), generator=gen).to(dev)
    kw = dict(beam_size=BEAMS, num_return_gen=1, stop_token=base.STOP)
    seen = {}

    def lockstep_plain():
        counts.update(steps=0, masks=0)
        gpt.beam_search_batched(tokens[:CLIPS_LOCKSTEP], query_embeds=qe[:CLIPS_LOCKSTEP].contiguous(), prompt_length=base.PROMPT, kv="shared_prefix",
                                constraints=plain, **kw)
        seen["lockstep_plain_steps"] = counts["steps"]

    def lockstep_trie():
        counts.update(steps=0, masks=0)
        out = gpt.beam_search_batched(tokens[:CLIPS_LOCKSTEP], query_embeds=qe[:CLIPS_LOCKSTEP].contiguous(), prompt_length=base.PROMPT,
                                      kv="shared_prefix", constraints=closed, **kw)
        seen["lockstep_trie_steps"], seen["lockstep_trie_masks"] = counts["steps"], counts["masks"]
        seen["lockstep_phrases"] = sum(int(o.phrase_index.numel() == 1 and o.phrase_index[0] >= 0) for o in out)

    def inflight_plain():
        out = gpt.beam_search_inflight(tokens, query_embeds=qe, prompt_length=[base.PROMPT] * CLIPS_INFLIGHT, slots=SLOTS, max_new_tokens=steps,
                                       constraints=plain, **kw)
        seen["inflight_plain_steps"] = out.steps

    def inflight_trie():
        counts.update(steps=0, masks=0)
        out = gpt.beam_search_inflight(tokens, query_embeds=qe, prompt_length=[base.PROMPT] * CLIPS_INFLIGHT, slots=SLOTS, constraints=closed, **kw)
        seen["inflight_trie_steps"], seen["inflight_trie_masks"] = out.steps, counts["masks"]
        seen["inflight_phrases"] = sum(int(o.phrase_index.numel() == 1 and o.phrase_index[0] >= 0) for o in out.results)
    rec = {}
    for name, fns, key in (("lockstep_32x5", [lockstep_plain, lockstep_trie], "lockstep_trie_masks"),
                           ("inflight_128_through_32", [inflight_plain, inflight_trie], "inflight_trie_masks")):
        times = timed(fns, rounds)
        med, spread = summary(times)
        a, b = fns[0].__name__, fns[1].__name__
        n_masks = seen[key]
        allowance = n_masks * mask_us * 1e-6 + max(spread[a] * med[a], spread[b] * med[b])
        rec[name] = dict(seconds=times, median_s=med, run_to_run_spread=spread, mask_launches=n_masks, mask_us_per_launch=mask_us,
                         trie_minus_plain_s=med[b] - med[a], allowance_s=allowance, condition_holds=bool(med[b] - med[a] <= allowance),
                         counted=dict(seen))
        print(f"[loops] {name}: plain {med[a]:.4f} s ({spread[a]:.1%})  trie {med[b]:.4f} s ({spread[b]:.1%})  "
              f"difference {med[b] - med[a]:+.4f} s, allowance {allowance:.4f} s -> {'ok' if rec[name]['condition_holds'] else 'NOT MET'}", flush=True)
    generation.SharedPrefixDecodeState.step = step
    for n, fn in masks.items():
        setattr(ops, n, fn)
    return rec


def crossover_section(gpt, dev, rounds):
    from youku_mplug_amd import generation, ops
    gen = torch.Generator().manual_seed(2)
    gpt.config.extra["tokens_to_generate"] = 8
    qe = (torch.randn(CROSS_CLIPS, base.Q, base.HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
    prompt = torch.randint(8, base.VOCAB, (CROSS_CLIPS, base.PROMPT), generator=gen).to(dev)
    rec = {}
    for n in CROSS_SIZES:
        phrases = synthetic_phrases(n, 100 + n)
        trie = generation.PhraseTrie(phrases, base.VOCAB)
        closed = generation.LogitsConstraints(allowed_phrases=trie)
        lens = [len(p) + 1 for p in phrases]                                  # the phrase and its termination id
        layout = ops.PackedLayout(lens, [n], device=dev)
        best = {}

        def search():
            out = gpt.beam_search_batched(prompt, query_embeds=qe, prompt_length=base.PROMPT, kv="shared_prefix", constraints=closed, beam_size=BEAMS,
                                          num_return_gen=1, stop_token=base.STOP)
            best["search"] = [int(o.phrase_index[0]) for o in out]

        def score_all():
            picks = []
            for c in range(CROSS_CLIPS):
                rows_in = torch.tensor([x for p in phrases for x in [int(prompt[c, -1])] + p], dtype=torch.long, device=dev)
                target = torch.tensor([x for p in phrases for x in p + [base.STOP]], dtype=torch.long, device=dev)
                prefix = gpt.forward_prefix(qe[c].reshape(-1, base.HIDDEN), prompt[c:c + 1, :-1].contiguous())
                lp = gpt.forward_continuation_packed(prefix, rows_in, layout, labels=target)["token_logprob"]
                seg = torch.repeat_interleave(torch.arange(n, device=dev), torch.tensor(lens, device=dev))
                total = torch.zeros(n, dtype=torch.float32, device=dev).index_add_(0, seg, lp.float())
                picks.append(int(total.argmax()))
            best["score_all"] = picks
        times = timed([search, score_all], rounds)
        med, spread = summary(times)
        rec[f"{n}_phrases"] = dict(clips=CROSS_CLIPS, beams=BEAMS, seconds=times, median_s=med, run_to_run_spread=spread,
                                   score_all_over_search=med["score_all"] / med["search"],
                                   same_best_phrase=sum(int(a == b) for a, b in zip(best["search"], best["score_all"])),
                                   note="the search ranks by the renormalised, length-normalised beam score; the scoring by the model's "
                                        "likelihood over the whole vocabulary: the best phrases need not agree")
        print(f"[crossover] {n} phrases x {CROSS_CLIPS} clips: search {med['search']:.4f} s  score all {med['score_all']:.4f} s", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trie_decode.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip", nargs="*", default=[], choices=["loops", "crossover"])
    args = ap.parse_args()
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    dev = torch.device("cuda:0")
    rec = {"decoder": dict(hidden=base.HIDDEN, layers=base.LAYERS, heads=base.HEADS, ffn=base.FFN, vocab=base.VOCAB), "query_slots": base.Q,
           "prompt_tokens": base.PROMPT, "rounds": args.rounds, "launches_per_timing": LAUNCHES, "device": torch.cuda.get_device_name(0)}
    t0 = time.perf_counter()
    with torch.no_grad():
        rec["mask"] = mask_section(dev, args.rounds)
        mask_us = rec["mask"]["10000_phrases_160_rows_mid"]["median_us"]
        cfg = GPT3Config(vocab_size=base.VOCAB, hidden_size=base.HIDDEN, ffn_hidden_size=base.FFN, num_hidden_layers=base.LAYERS,
                         num_attention_heads=base.HEADS, max_position_embeddings=base.MAX_POS, layernorm_epsilon=base.LN_EPS,
                         tokens_to_generate=PHRASE_LEN + 1, eod_id=base.STOP)
        torch.manual_seed(0)
        gpt = DistributedGPT3(config=cfg, device=dev).eval()
        for name, fn in (("loops", lambda: loops_section(gpt, dev, args.rounds, mask_us)), ("crossover", lambda: crossover_section(gpt, dev, args.rounds))):
            if name in args.skip:
                continue
            try:
                rec[name] = fn()
            except Exception as e:                                           # the sections before keep their figures
                rec[name] = dict(error=f"{type(e).__name__}: {e}")
                print(f"[{name}] failed: {rec[name]['error']}", flush=True)
    rec["wall_s"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)
    ok = all(v.get("condition_holds", True) for v in rec.get("loops", {}).values() if isinstance(v, dict))
    sys.exit(0 if ok and "error" not in rec.get("loops", {}) else 1)


if __name__ == "__main__":
    main()
