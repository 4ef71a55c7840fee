"""Sampled captions over clips whose prompts differ in length, on one GPU: the decoder and the constants of
tools/bench_mixed_prompts.py (the 1.3B dims with synthetic weights, 256 query slots, kv="shared_prefix", tokens_to_generate 24), 16
samples per clip, top-p 0.9, early termination off (a random-weight decoder would not terminate in any case), in two comparisons, same
process, alternated:

(a) 32 clips with 32 different prompt lengths (8 .. 39): the grouped path -- one sample_batched call per distinct length, as
    DistributedGPT3_Caption.generate(do_sample=True) makes them: here 32 loops of 16 rows each -- beside the mixed mode, ONE call of
    512 rows with the 32 lengths (generate(do_sample=True, sample_mixed_prompts=True)).
(b) 32 clips with equal prompts (8 tokens): today's uniform loop beside the mixed loop on the same clips -- what the per-row column of
    the three ragged kernels, the ragged prefill and the ragged step cost when they buy nothing.

    python tools/bench_mixed_sampling.py [--out profiles/mixed_sampling.json] [--rounds 9] [--positions 24] [--scores]

Times are host clocks around calls that end in a download of the token table (a device synchronise precedes and follows); every path is
run once before the timed rounds; the decode steps issued are counted and written next to the times.  Outputs are compared too: in (b)
the rows of the two paths (the same row count per step: equal bit for bit is expected and recorded), in (a) the rows clip by clip (the
paths run 16-row and 512-row steps, whose logits differ in the last bf16 digit, so a draw near a boundary may differ: the count of equal
clips is recorded, not asserted).  No ratio is promised; the JSON holds medians, run-to-run spreads and, for (b), the difference round
by round."""
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
from bench_mixed_prompts import summary, timed  # noqa: E402

CLIPS, SHORTEST, SAMPLES, TOP_P = 32, base.PROMPT, 16, 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_sampling.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--positions", type=int, default=24)
    ap.add_argument("--scores", action="store_true", help="return_scores=True in every call (one more launch per step)")
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
    kw = dict(num_samples=SAMPLES, seed=5, top_p=TOP_P, top_k=0, temperature=1.0, kv="shared_prefix", termination_id=base.STOP,
              use_eod_token_for_early_termination=False, **(dict(return_scores=True) if args.scores else {}))
    rows_of = (lambda out: out[0]) if args.scores else (lambda out: out)
    rec = {"decoder": dict(hidden=base.HIDDEN, layers=base.LAYERS, heads=base.HEADS, ffn=base.FFN, vocab=base.VOCAB), "query_slots": base.Q,
           "samples_per_clip": SAMPLES, "top_p": TOP_P, "clips": CLIPS, "tokens_to_generate": args.positions, "rounds": args.rounds,
           "return_scores": bool(args.scores), "early_termination": False, "device": torch.cuda.get_device_name(0), "cases": {}}

    def streams(sel):
        return (torch.as_tensor(sel)[:, None] * SAMPLES + torch.arange(SAMPLES)[None]).reshape(-1)

    def count_steps(fns):
        n = {}
        for fn in fns:
            steps[0] = 0
            fn()
            n[fn.__name__] = steps[0]
        return n
    with torch.no_grad():
        qe = (torch.randn(CLIPS, base.Q, base.HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
        # ---- (a) 32 different prompt lengths in rows of one width, as a tokenizer pads them
        lens = list(range(SHORTEST, SHORTEST + CLIPS))
        width = max(lens) + 1
        final = width + args.positions
        tokens = torch.randint(8, base.VOCAB, (CLIPS, width), generator=gen).to(dev)
        last = {}

        def grouped():
            out = [None] * CLIPS
            for pl in sorted(set(lens)):
                sel = [i for i, x in enumerate(lens) if x == pl]
                rows = rows_of(gpt.sample_batched(tokens[sel], query_embeds=qe[sel].contiguous(), streams=streams(sel),
                                                  prompt_length=torch.full((len(sel),), pl, device=dev), **kw))[:, :final].cpu()
                for j, i in enumerate(sel):
                    out[i] = rows[j * SAMPLES:(j + 1) * SAMPLES]
            last["grouped"] = out

        def mixed():
            rows = rows_of(gpt.sample_batched(tokens, query_embeds=qe, streams=streams(range(CLIPS)), prompt_length=lens, mixed_prompts=True,
                                              **kw))[:, :final].cpu()
            last["mixed"] = [rows[i * SAMPLES:(i + 1) * SAMPLES] for i in range(CLIPS)]
        nsteps = count_steps((grouped, mixed))
        times = timed((grouped, mixed), args.rounds)
        med, spread = summary(times)
        same = sum(int(a.shape == b.shape and torch.equal(a, b)) for a, b in zip(last["grouped"], last["mixed"]))
        same_rows = sum(int(torch.equal(x, y)) for a, b in zip(last["grouped"], last["mixed"]) if a.shape == b.shape for x, y in zip(a, b))
        # the same two paths once more with greedy draws (top_k = 1): an arg-max survives a last-digit difference of the logits far more
        # often than a draw from a nearly flat distribution does, so this count says whether the two paths follow the same sequences
        sampled = dict(last)
        kw.update(top_k=1, top_p=0.0)
        grouped()
        mixed()
        kw.update(top_k=0, top_p=TOP_P)
        greedy_same = sum(int(torch.equal(x, y)) for a, b in zip(last["grouped"], last["mixed"]) for x, y in zip(a[:1], b[:1]))
        greedy_first = sum(int(a[0, n] == b[0, n]) for a, b, n in zip(last["grouped"], last["mixed"], lens))
        last.update(sampled)
        gain = med["grouped"] - med["mixed"]
        noise = max(spread["grouped"] * med["grouped"], spread["mixed"] * med["mixed"])
        rec["cases"]["a_32_lengths"] = dict(prompt_lengths=lens, row_width=width, seconds=times, median_s=med, run_to_run_spread=spread,
                                            decode_steps=nsteps, loops=dict(grouped=len(set(lens)), mixed=1),
                                            rows_per_step=dict(grouped=SAMPLES, mixed=CLIPS * SAMPLES), clips_with_equal_rows=same,
                                            equal_rows=same_rows, greedy_clips_with_equal_rows=greedy_same,
                                            greedy_clips_with_equal_first_token=greedy_first, grouped_minus_mixed_s=gain, larger_spread_s=noise,
                                            mixed_below_grouped_by_more_than_spread=bool(gain > noise))
        print(f"(a) grouped {med['grouped']:.4f} s (spread {spread['grouped']:.1%}, {nsteps['grouped']} steps)  mixed {med['mixed']:.4f} s "
              f"(spread {spread['mixed']:.1%}, {nsteps['mixed']} steps)  equal rows in {same}/{CLIPS} clips, {same_rows}/{CLIPS * SAMPLES} rows; "
              f"greedy: equal rows in {greedy_same}/{CLIPS} clips, equal first token in {greedy_first}/{CLIPS}", flush=True)
        # ---- (b) 32 equal prompts
        eq = tokens[:, :SHORTEST].contiguous()

        def uniform():
            last["uniform"] = rows_of(gpt.sample_batched(eq, query_embeds=qe, streams=streams(range(CLIPS)),
                                                         prompt_length=torch.full((CLIPS,), SHORTEST, device=dev), **kw)).cpu()

        def mixed_equal():
            last["mixed_equal"] = rows_of(gpt.sample_batched(eq, query_embeds=qe, streams=streams(range(CLIPS)), prompt_length=[SHORTEST] * CLIPS,
                                                             mixed_prompts=True, **kw)).cpu()
        nsteps = count_steps((uniform, mixed_equal))
        times = timed((uniform, mixed_equal), args.rounds)
        med, spread = summary(times)
        same = last["uniform"].shape == last["mixed_equal"].shape and torch.equal(last["uniform"], last["mixed_equal"])
        cost = med["mixed_equal"] - med["uniform"]
        paired = [m - u for u, m in zip(times["uniform"], times["mixed_equal"])]       # round by round: the two ran back to back
        noise = max(spread["uniform"] * med["uniform"], spread["mixed_equal"] * med["mixed_equal"])
        rec["cases"]["b_equal_prompts"] = dict(prompt_length=SHORTEST, seconds=times, median_s=med, run_to_run_spread=spread, decode_steps=nsteps,
                                               rows_equal=bool(same), mixed_minus_uniform_s=cost, larger_spread_s=noise,
                                               cost_above_spread=bool(cost > noise), paired_mixed_minus_uniform_s=paired,
                                               mixed_slower_in_rounds=sum(d > 0 for d in paired),
                                               cost_per_decode_step_s=cost / max(nsteps["mixed_equal"], 1))
        print(f"(b) uniform {med['uniform']:.4f} s (spread {spread['uniform']:.1%})  mixed {med['mixed_equal']:.4f} s "
              f"(spread {spread['mixed_equal']:.1%})  mixed - uniform {cost * 1e3:.3f} ms (larger spread {noise * 1e3:.3f} ms, slower in "
              f"{sum(d > 0 for d in paired)}/{len(paired)} rounds)  rows equal: {same}", flush=True)
    generation.SharedPrefixDecodeState.step = step
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
