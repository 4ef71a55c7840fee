"""Cost of the consensus caption choice on one GPU, written to profiles/consensus.json.  The decoder and the
constants are those of tools/bench_sample_inflight.py: the 1.3B dims with synthetic weights, 256 query slots, 8-token prompts,
kv="shared_prefix", top-p 0.9, 16 samples per clip, termination banned (termination id -1: a random-weight decoder would not
terminate in any case), so that every candidate is as long as tokens_to_generate: about 30 and about 100 tokens.

  1. kernel     ops.caption_overlap alone on a padded table of 32 x 16 and 128 x 16 rows, every clip's 16 x 16 pairs, at candidate
                lengths 30 and 100: random ids over the vocabulary (no n-gram ever matches: the scans leave at the first token) and
                ids over a 64-token alphabet (hits at every order).  HIP events around 20 launches after 3 warm-up ones.
  2. generate   DistributedGPT3_Caption.generate(do_sample=True, num_samples=16, query_features=...) without and with
                consensus="rouge_l", alternated in one process: 32 clips in one lockstep chunk and 128 clips in flight through 32
                slots.  The call without the keyword is the parent's behaviour.  Host clocks around calls that end in their
                download; every call once before the timed rounds.
  3. host loop  the same counts for some clips' pairs by a plain Python loop on the host (a rolling-row LCS and collections.Counter),
                timed on --host_clips clips and scaled to the call: for scale only.

    python tools/bench_consensus.py [--out profiles/consensus.json] [--rounds 3] [--host_clips 2]

No number is promised: the JSON holds medians, spreads and what was derived from them."""
import argparse
import dataclasses
import json
import os
import sys
import time
import types
from collections import Counter

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_caption_batched as base  # noqa: E402  (the decoder's dims and the constants of the caption benchmark)
from bench_mixed_prompts import summary, timed  # noqa: E402

SAMPLES, SLOTS, PROMPT, TOP_P = 16, 32, base.PROMPT, 0.9
LENGTHS = (30, 100)


def kernel_rows(dev):
    from youku_mplug_amd import ops
    out = []
    g = torch.Generator().manual_seed(3)
    for clips in (32, 128):
        for length in LENGTHS:
            for content, high in (("random_ids", base.VOCAB), ("alphabet_64", 72)):
                rows, width = clips * SAMPLES, PROMPT + length
                table = torch.randint(8, high, (rows, width), generator=g).to(dev)
                start, begin = [PROMPT] * rows, list(range(0, rows + 1, SAMPLES))
                call = lambda: ops.caption_overlap(table, start, begin, term=-1)
                for _ in range(3):
                    call()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                for _ in range(20):
                    ln, _, counts = call()
                t1.record()
                torch.cuda.synchronize()
                us = t0.elapsed_time(t1) * 1e3 / 20
                assert int(ln.min()) == length and int(counts[:, 0].max()) == length              # a row against itself
                out.append(dict(clips=clips, samples=SAMPLES, pairs=clips * SAMPLES * SAMPLES, candidate_tokens=length, content=content,
                                call_us=round(us, 1), note="wrapper included: one small upload of the starts and offsets per call"))
                print(f"kernel: {clips:4d} clips x {SAMPLES} samples, {length:3d} tokens, {content:12s}: {us:9.1f} us per call", flush=True)
    return out


def host_counts(a, b):
    row = [0] * (len(b) + 1)
    for x in a:
        prev = 0
        for j, y in enumerate(b, 1):
            prev, row[j] = row[j], (prev + 1 if x == y else max(row[j], row[j - 1]))
    out = [row[-1]]
    for n in (1, 2, 3, 4):
        ca = Counter(tuple(a[i:i + n]) for i in range(len(a) - n + 1))
        cb = Counter(tuple(b[i:i + n]) for i in range(len(b) - n + 1))
        out.append(sum(min(c, cb[k]) for k, c in ca.items()))
    return out


def host_rows(clips_timed):
    out = []
    g = torch.Generator().manual_seed(4)
    for length in LENGTHS:
        cands = torch.randint(8, 72, (clips_timed * SAMPLES, length), generator=g).tolist()
        t0 = time.perf_counter()
        for c in range(clips_timed):
            rows = cands[c * SAMPLES:(c + 1) * SAMPLES]
            for a in rows:
                for b in rows:
                    host_counts(a, b)
        per_clip = (time.perf_counter() - t0) / clips_timed
        out.append(dict(candidate_tokens=length, clips_timed=clips_timed, seconds_per_clip=round(per_clip, 4),
                        scaled_to_32_clips_s=round(per_clip * 32, 2), scaled_to_128_clips_s=round(per_clip * 128, 2)))
        print(f"host loop: {length:3d} tokens: {per_clip:.3f} s per clip of {SAMPLES * SAMPLES} pairs -> {per_clip * 128:.1f} s for 128 clips", flush=True)
    return out


def generate_rows(dev, rounds):
    from oracle.weights import CONFIG_TINY
    from youku_mplug_amd.downstream import synthetic_gencls_model
    shapes = dataclasses.replace(CONFIG_TINY, hidden=base.HIDDEN, layers=base.LAYERS, heads=base.HEADS, ffn=base.FFN, vocab=base.VOCAB,
                                 max_pos=base.MAX_POS, num_queries=base.Q, gpt_ln_eps=base.LN_EPS)       # (the tiny ViT is never run)
    torch.manual_seed(0)
    model = synthetic_gencls_model(shapes, "caption", device=dev).eval()
    gen = torch.Generator().manual_seed(1)
    out = []
    for length in LENGTHS:
        model.text_decoder.config.extra.update(tokens_to_generate=length, eod_id=base.STOP)
        for name, clips, more in (("lockstep_32_clips", 32, dict(sample_mixed_prompts=True)), ("inflight_128_clips", 128, dict(inflight=True))):
            qf = (torch.randn(clips * base.Q, base.HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
            ids = torch.randint(8, base.VOCAB, (clips, PROMPT + 1), generator=gen).to(dev)
            text = types.SimpleNamespace(input_ids=ids, attention_mask=torch.ones_like(ids))
            kw = dict(termination_id=-1, do_sample=True, num_samples=SAMPLES, seed=5, top_p=TOP_P, kv_cache="shared_prefix", clips_per_search=SLOTS,
                      query_features=qf, **more)
            last = {}

            def plain():
                last["plain"] = model.generate(None, text, **kw)

            def consensus():
                last["consensus"] = model.generate(None, text, consensus="rouge_l", **kw)
            times = timed([plain, consensus], rounds)
            med, spread = summary(times)
            assert all(any(torch.equal(c, p[s:s + 1]) for s in range(SAMPLES)) for c, p in zip(last["consensus"], last["plain"]))
            noise = max(spread["plain"] * med["plain"], spread["consensus"] * med["consensus"])
            out.append(dict(case=name, clips=clips, candidate_tokens=length, seconds={k: [round(x, 4) for x in v] for k, v in times.items()},
                            median_s={k: round(v, 4) for k, v in med.items()}, run_to_run_spread={k: round(v, 4) for k, v in spread.items()},
                            consensus_minus_plain_s=round(med["consensus"] - med["plain"], 4), larger_spread_s=round(noise, 4),
                            beyond_spread=bool(abs(med["consensus"] - med["plain"]) > noise),
                            plain_s_per_generated_position=round(med["plain"] / length, 5)))
            print(f"generate: {name}, {length:3d} tokens: plain {med['plain']:.4f} s ({spread['plain']:.1%}), consensus {med['consensus']:.4f} s "
                  f"({spread['consensus']:.1%})", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host_clips", type=int, default=2)
    args = ap.parse_args()
    import youku_mplug_amd  # noqa: F401
    dev = torch.device("cuda:0")
    rec = {"decoder": dict(hidden=base.HIDDEN, layers=base.LAYERS, heads=base.HEADS, ffn=base.FFN, vocab=base.VOCAB), "query_slots": base.Q,
           "samples_per_clip": SAMPLES, "slots": SLOTS, "prompt_tokens": PROMPT, "top_p": TOP_P, "rounds": args.rounds, "termination": "banned",
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        rec["kernel"] = kernel_rows(dev)
        rec["host_python_loop"] = host_rows(args.host_clips)
        rec["generate"] = generate_rows(dev, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
