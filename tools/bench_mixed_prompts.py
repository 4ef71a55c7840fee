"""Lockstep beam search over clips whose prompts differ in length, on one GPU: tools/bench_caption_batched.py's decoder (the 1.3B
dims with synthetic weights, 256 query slots, beam 5, kv="shared_prefix") in two comparisons, same process, alternated:

(a) 32 clips with 32 different prompt lengths (8 .. 39): the grouped path -- one beam_search_batched call per distinct length, as
    DistributedGPT3_Caption.generate(batched=True) makes them: here 32 searches of one clip each -- beside the mixed mode, ONE call
    with the 32 lengths (generate(mixed_prompts=True)).
(b) 32 clips with equal prompts (8 tokens): the uniform lockstep call beside the mixed mode on the same clips -- what the per-group
    prefix length costs when it buys nothing.

    python tools/bench_mixed_prompts.py [--out profiles/mixed_prompts.json] [--rounds 3] [--positions 24]

Times are host clocks around calls that end in a download of the search state (a device synchronise precedes and follows); every path
is run once before the timed rounds.  The stop token of a random-weight decoder practically never collects five finished hypotheses,
so every clip generates its whole budget: tokens_to_generate + (row width - its prompt length) positions; the decode steps issued are
counted and written next to the times.  Outputs are compared too: in (b) rows and scores of the two paths, in (a) the rows clip by
clip (the paths run different row counts per step, so near-ties may resolve differently: the count of equal clips is recorded, not
asserted).  No ratio is promised; the JSON holds medians and run-to-run spreads, and for (b) the difference round by round as well: a
cost smaller than the spread of either path can still have one sign in every alternation."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_caption_batched as base  # noqa: E402  (the decoder's dims and the constants of the caption benchmark)

CLIPS, SHORTEST = 32, base.PROMPT


def timed(fns, rounds):
    """every fn once (warm-up), then `rounds` alternated passes -> {name: [seconds]}"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = {fn.__name__: [] for fn in fns}
    for _ in range(rounds):
        for fn in fns:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[fn.__name__].append(time.perf_counter() - t0)
    return times


def summary(times):
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return med, {k: (max(v) - min(v)) / med[k] for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_prompts.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--positions", type=int, default=24)
    args = ap.parse_args()
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import generation
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    dev = torch.device("cuda:0")
    cfg = GPT3Config(vocab_size=base.VOCAB, hidden_size=base.HIDDEN, ffn_hidden_size=base.FFN, num_hidden_layers=base.LAYERS,
                     num_attention_heads=base.HEADS, max_position_embeddings=base.MAX_POS, layernorm_epsilon=base.LN_EPS,
                     tokens_to_generate=args.positions, eod_id=base.STOP)
    torch.manual_seed(0)
    gpt = DistributedGPT3(config=cfg, device=dev).eval()
    steps = [0]
    step = generation.SharedPrefixDecodeState.step

    def counted(self, *a, **k):
        steps[0] += 1
        return step(self, *a, **k)
    generation.SharedPrefixDecodeState.step = counted
    gen = torch.Generator().manual_seed(1)
    kw = dict(beam_size=base.BEAMS, stop_token=base.STOP, kv="shared_prefix")
    rec = {"decoder": dict(hidden=base.HIDDEN, layers=base.LAYERS, heads=base.HEADS, ffn=base.FFN, vocab=base.VOCAB), "query_slots": base.Q,
           "beams": base.BEAMS, "clips": CLIPS, "tokens_to_generate": args.positions, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    with torch.no_grad():
        qe = (torch.randn(CLIPS, base.Q, base.HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
        # ---- (a) 32 different prompt lengths in rows of one width, as a tokenizer pads them
        lens = list(range(SHORTEST, SHORTEST + CLIPS))
        width = max(lens) + 1
        tokens = torch.randint(8, base.VOCAB, (CLIPS, width), generator=gen).to(dev)
        last = {}

        def grouped():
            out = [None] * CLIPS
            for pl in sorted(set(lens)):
                sel = [i for i, x in enumerate(lens) if x == pl]
                for i, o in zip(sel, gpt.beam_search_batched(tokens[sel], query_embeds=qe[sel].contiguous(), prompt_length=pl, **kw)):
                    out[i] = o
            last["grouped"] = out

        def mixed():
            last["mixed"] = gpt.beam_search_batched(tokens, query_embeds=qe, prompt_length=lens, **kw)
        nsteps = {}
        for fn in (grouped, mixed):
            steps[0] = 0
            fn()
            nsteps[fn.__name__] = steps[0]
        times = timed((grouped, mixed), args.rounds)
        med, spread = summary(times)
        same = sum(int(torch.equal(a.sequences, b.sequences)) for a, b in zip(last["grouped"], last["mixed"]))
        gain = med["grouped"] - med["mixed"]
        noise = max(spread["grouped"] * med["grouped"], spread["mixed"] * med["mixed"])
        rec["cases"]["a_32_lengths"] = dict(prompt_lengths=lens, row_width=width, seconds=times, median_s=med, run_to_run_spread=spread,
                                            decode_steps=nsteps, searches=dict(grouped=len(set(lens)), mixed=1),
                                            clips_with_equal_rows=same, grouped_minus_mixed_s=gain, larger_spread_s=noise,
                                            mixed_below_grouped_by_more_than_spread=bool(gain > noise))
        print(f"(a) grouped {med['grouped']:.4f} s (spread {spread['grouped']:.1%}, {nsteps['grouped']} steps)  mixed {med['mixed']:.4f} s "
              f"(spread {spread['mixed']:.1%}, {nsteps['mixed']} steps)  equal rows in {same}/{CLIPS} clips", flush=True)
        # ---- (b) 32 equal prompts
        eq = tokens[:, :SHORTEST].contiguous()

        def uniform():
            last["uniform"] = gpt.beam_search_batched(eq, query_embeds=qe, prompt_length=SHORTEST, **kw)

        def mixed_equal():
            last["mixed_equal"] = gpt.beam_search_batched(eq, query_embeds=qe, prompt_length=[SHORTEST] * CLIPS, **kw)
        nsteps = {}
        for fn in (uniform, mixed_equal):
            steps[0] = 0
            fn()
            nsteps[fn.__name__] = steps[0]
        times = timed((uniform, mixed_equal), args.rounds)
        med, spread = summary(times)
        same = all(torch.equal(a.sequences, b.sequences) and torch.equal(a.scores, b.scores) for a, b in zip(last["uniform"], last["mixed_equal"]))
        cost = med["mixed_equal"] - med["uniform"]
        paired = [m - u for u, m in zip(times["uniform"], times["mixed_equal"])]       # round by round: the two ran back to back
        noise = max(spread["uniform"] * med["uniform"], spread["mixed_equal"] * med["mixed_equal"])
        rec["cases"]["b_equal_prompts"] = dict(prompt_length=SHORTEST, seconds=times, median_s=med, run_to_run_spread=spread, decode_steps=nsteps,
                                               rows_and_scores_equal=bool(same), mixed_minus_uniform_s=cost, larger_spread_s=noise,
                                               cost_above_spread=bool(cost > noise), paired_mixed_minus_uniform_s=paired,
                                               mixed_slower_in_rounds=sum(d > 0 for d in paired),
                                               cost_per_decode_step_s=cost / max(nsteps["mixed_equal"], 1))
        print(f"(b) uniform {med['uniform']:.4f} s (spread {spread['uniform']:.1%})  mixed {med['mixed_equal']:.4f} s "
              f"(spread {spread['mixed_equal']:.1%})  mixed - uniform {cost * 1e3:.3f} ms (larger spread {noise * 1e3:.3f} ms, slower in "
              f"{sum(d > 0 for d in paired)}/{len(paired)} rounds)  rows and scores equal: {same}", flush=True)
    generation.SharedPrefixDecodeState.step = step
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
