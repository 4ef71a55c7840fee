"""Caption beam search on one GPU: captions/s of the per-clip path (DistributedGPT3.beam_search, one search per clip: what
DistributedGPT3_Caption.generate does by default) beside the lockstep path (DistributedGPT3.beam_search_batched: generate(batched=True))
for B = 1, 8, 32 clips -- the 1.3B decoder's dims with synthetic weights, 256 query slots + an 8-token prompt, beam 5, a fixed number
of generated positions, same process, alternated three times.

    python tools/bench_caption_batched.py [--out profiles/caption_batched.json] [--rounds 3] [--positions 24] [--batches 1,8,32]

The stop token of a random-weight decoder practically never collects five finished hypotheses, so both paths generate every position;
the decode steps actually issued are counted and written next to the times.  Prints one table and writes one JSON file."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIDDEN, LAYERS, HEADS, FFN, VOCAB, MAX_POS, LN_EPS = 2048, 24, 32, 8192, 51200, 2048, 1e-5      # bench.py's 1.3B decoder
Q, PROMPT, BEAMS, STOP = 256, 8, 5, 7
HBM_BYTES_PER_S = 6.3e12          # measured streaming read rate of one MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caption_batched.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--positions", type=int, default=24)
    ap.add_argument("--batches", default="1,8,32")
    args = ap.parse_args()
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import generation
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    dev = torch.device("cuda:0")
    cfg = GPT3Config(vocab_size=VOCAB, hidden_size=HIDDEN, ffn_hidden_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                     max_position_embeddings=MAX_POS, layernorm_epsilon=LN_EPS, tokens_to_generate=args.positions, eod_id=STOP)
    torch.manual_seed(0)
    gpt = DistributedGPT3(config=cfg, device=dev).eval()
    weight_bytes = sum(p.numel() * p.element_size() for p in gpt.parameters())
    steps = [0]
    step = generation.DecodeState.step

    def counted(self, *a, **k):
        steps[0] += 1
        return step(self, *a, **k)
    generation.DecodeState.step = counted
    gen = torch.Generator().manual_seed(1)
    rec = {"decoder": dict(hidden=HIDDEN, layers=LAYERS, heads=HEADS, ffn=FFN, vocab=VOCAB, weight_bytes=weight_bytes), "query_slots": Q,
           "prompt_tokens": PROMPT, "beams": BEAMS, "positions": args.positions, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "weight_stream_floor_ms_per_step": 1e3 * weight_bytes / HBM_BYTES_PER_S, "cases": []}
    print(f"{'B':>3} {'per-clip s':>28} {'batched s':>28} {'captions/s':>19} {'ratio':>6}")
    with torch.no_grad():
        for B in [int(b) for b in args.batches.split(",")]:
            qe = (torch.randn(B, Q, HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
            tokens = torch.randint(8, VOCAB, (B, PROMPT), generator=gen).to(dev)

            def per_clip():
                return [gpt.beam_search(tokens[i:i + 1], query_embeds=qe[i:i + 1], beam_size=BEAMS, stop_token=STOP, prompt_length=PROMPT) for i in range(B)]

            def batched():
                return gpt.beam_search_batched(tokens, query_embeds=qe, beam_size=BEAMS, stop_token=STOP, prompt_length=PROMPT)
            times, nsteps = {"per_clip": [], "batched": []}, {}
            for fn in (per_clip, batched):                     # warm-up (allocator, workspaces), and the steps each path issues
                steps[0] = 0
                fn()
                nsteps[fn.__name__] = steps[0]
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for fn in (per_clip, batched):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[fn.__name__].append(time.perf_counter() - t0)
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
            case = {"clips": B, "seconds": times, "median_s": med, "run_to_run_spread": spread, "decode_steps": nsteps,
                    "captions_per_s": {k: B / med[k] for k in med}, "batched_over_per_clip": med["per_clip"] / med["batched"],
                    "kv_bytes_batched": 2 * LAYERS * B * BEAMS * (Q + PROMPT + args.positions) * 3 * HIDDEN * 2}
            rec["cases"].append(case)
            fmt = lambda v: " ".join(f"{x:8.4f}" for x in v)
            print(f"{B:>3} {fmt(times['per_clip']):>28} {fmt(times['batched']):>28} {B / med['per_clip']:9.2f} {B / med['batched']:9.2f} "
                  f"{case['batched_over_per_clip']:6.2f}", flush=True)
            del qe, tokens
            torch.cuda.empty_cache()
    generation.DecodeState.step = step
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
