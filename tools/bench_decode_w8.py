"""Decode steps on FP8 (e4m3) decoder weights against the bf16 path, on one GPU -> profiles/decode_w8.json.

    python tools/bench_decode_w8.py [--out profiles/decode_w8.json] [--rounds 3] [--positions 24] [--sections a,b] [--rows 1,5,...]

(a) per product: the 1.3B decoder's five weight products at M = 1, 5, 16, 40, 96, 160, 512 rows, ops.gemm_w8 on the codes beside ops.gemm
    on the bf16 weight (the baseline is the existing bf16 product, never an earlier version of the new kernel), alternated in one
    process, the weights rotated through a set three times the size of the MALL so that none is cache-resident: time and weight
    bytes / s of both, and the run-to-run spread of the pair.
(b) end to end: tools/bench_caption_batched.py's decoder and constants, decode_weights "bf16" / "fp8" alternated: the per-clip beam
    search (beam 5), the lockstep search of 32 clips x 5 beams in both KV modes, 32 clips x 16 samples on the shared prefix."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_caption_batched import BEAMS, FFN, HEADS, HIDDEN, LAYERS, LN_EPS, MAX_POS, PROMPT, Q, STOP, VOCAB  # noqa: E402

PRODUCTS = [("qkv", 3 * HIDDEN, HIDDEN), ("dense", HIDDEN, HIDDEN), ("fc1", FFN, HIDDEN), ("fc2", HIDDEN, FFN), ("lm_head", VOCAB, HIDDEN)]
ROWS = [1, 5, 16, 40, 96, 160, 512]
ROTATE_BYTES = 768 << 20          # of codes per shape: three times the 256 MiB MALL (the bf16 set is twice that)


def _median(v):
    return sorted(v)[len(v) // 2]


def section_a(dev, rounds, rows=ROWS):
    from tools.bench_kernels import timeit
    from youku_mplug_amd import ops
    out = []
    print(f"{'product':>8} {'M':>4} {'bf16 us':>9} {'fp8 us':>9} {'bf16 TB/s':>10} {'fp8 TB/s':>9} {'fp8/bf16':>9} {'spread':>7}")
    for name, N, K in PRODUCTS:
        n = max(8, -(-ROTATE_BYTES // (N * K)))
        ws = [(torch.randn(N, K, device=dev) * 0.02).bfloat16() for _ in range(n)]
        qs = [ops.quantize_rows_e4m3(w) for w in ws]
        for M in rows:
            a = (torch.randn(M, K, device=dev) * 0.5).bfloat16()
            c = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            i = [0]

            def bf16():
                i[0] = (i[0] + 1) % n
                ops.gemm(a, ws[i[0]], M, N, K, out=c)

            def fp8():
                i[0] = (i[0] + 1) % n
                ops.gemm_w8(a, qs[i[0]][0], qs[i[0]][1], M, N, K, out=c)
            t = {"bf16": [], "fp8": []}
            for _ in range(rounds):
                for fn in (bf16, fp8):
                    t[fn.__name__].append(timeit(fn, iters=max(20, n)))
            med = {k: _median(v) for k, v in t.items()}
            spread = max((max(v) - min(v)) / med[k] for k, v in t.items())
            rec = {"product": name, "M": M, "N": N, "K": K, "rotated_weights": n, "seconds": t, "median_s": med,
                   "weight_bytes_per_s": {"bf16": N * K * 2 / med["bf16"], "fp8": N * K / med["fp8"]},
                   "fp8_over_bf16_time": med["fp8"] / med["bf16"], "pair_spread": spread}
            out.append(rec)
            print(f"{name:>8} {M:>4} {med['bf16'] * 1e6:9.1f} {med['fp8'] * 1e6:9.1f} {rec['weight_bytes_per_s']['bf16'] / 1e12:10.2f} "
                  f"{rec['weight_bytes_per_s']['fp8'] / 1e12:9.2f} {rec['fp8_over_bf16_time']:9.2f} {spread:7.3f}", flush=True)
        del ws, qs
        torch.cuda.empty_cache()
    return out


def section_b(dev, rounds, positions):
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    cfg = GPT3Config(vocab_size=VOCAB, hidden_size=HIDDEN, ffn_hidden_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                     max_position_embeddings=MAX_POS, layernorm_epsilon=LN_EPS, tokens_to_generate=positions, eod_id=STOP)
    torch.manual_seed(0)
    gpt = DistributedGPT3(config=cfg, device=dev).eval()
    gen = torch.Generator().manual_seed(1)
    B = 32
    qe = (torch.randn(B, Q, HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
    tokens = torch.randint(8, VOCAB, (B, PROMPT), generator=gen).to(dev)
    cases = {
        "per_clip_beam5": lambda w: gpt.beam_search(tokens[:1], query_embeds=qe[:1], beam_size=BEAMS, stop_token=STOP, prompt_length=PROMPT,
                                                    decode_weights=w),
        "lockstep_32x5_per_sequence": lambda w: gpt.beam_search_batched(tokens, query_embeds=qe, beam_size=BEAMS, stop_token=STOP,
                                                                        prompt_length=PROMPT, decode_weights=w),
        "lockstep_32x5_shared_prefix": lambda w: gpt.beam_search_batched(tokens, query_embeds=qe, beam_size=BEAMS, stop_token=STOP,
                                                                         prompt_length=PROMPT, kv="shared_prefix", decode_weights=w),
        "sample_32x16_shared_prefix": lambda w: gpt.sample_batched(tokens, query_embeds=qe, num_samples=16, seed=3, top_k=0, top_p=0.9,
                                                                   termination_id=STOP, kv="shared_prefix", decode_weights=w),
    }
    out = []
    print(f"{'case':>30} {'bf16 s':>28} {'fp8 s':>28} {'fp8/bf16':>9}")
    with torch.no_grad():
        t0 = time.perf_counter()
        q8 = gpt.quantize_decode_weights()
        torch.cuda.synchronize()
        quantise_s = time.perf_counter() - t0
        for name, fn in cases.items():
            times = {"bf16": [], "fp8": []}
            for w in times:                                    # warm-up (allocator, workspaces)
                fn(w)
            torch.cuda.synchronize()
            for _ in range(rounds):
                for w in times:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(w)
                    torch.cuda.synchronize()
                    times[w].append(time.perf_counter() - t0)
            med = {k: _median(v) for k, v in times.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
            out.append({"case": name, "seconds": times, "median_s": med, "run_to_run_spread": spread, "fp8_over_bf16_time": med["fp8"] / med["bf16"]})
            fmt = lambda v: " ".join(f"{x:8.4f}" for x in v)
            print(f"{name:>30} {fmt(times['bf16']):>28} {fmt(times['fp8']):>28} {med['fp8'] / med['bf16']:9.3f}", flush=True)
            torch.cuda.empty_cache()
    return {"decoder": dict(hidden=HIDDEN, layers=LAYERS, heads=HEADS, ffn=FFN, vocab=VOCAB), "query_slots": Q, "prompt_tokens": PROMPT,
            "beams": BEAMS, "positions": positions, "fp8_copy_bytes": q8.nbytes(), "quantise_seconds_first_call": quantise_s, "cases": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_w8.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--positions", type=int, default=24)
    ap.add_argument("--sections", default="a,b")
    ap.add_argument("--rows", default=",".join(map(str, ROWS)), help="section (a): the row counts")
    args = ap.parse_args()
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "w8_max_rows": _lib.W8_MAX_ROWS}
    if os.path.isfile(args.out):                               # a run of one section keeps the other
        with open(args.out) as f:
            rec = dict(json.load(f), **rec)
    if "a" in args.sections.split(","):
        rec["per_product"] = section_a(dev, args.rounds, [int(m) for m in args.rows.split(",")])
    if "b" in args.sections.split(","):
        rec["end_to_end"] = section_b(dev, args.rounds, args.positions)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
