"""Decode steps on FP8 (e4m3) decoder weights against the bf16 path, on one GPU -> profiles/decode_w8.json.

    python tools/bench_decode_w8.py [--out profiles/decode_w8.json] [--rounds 3] [--positions 24] [--sections a,b] [--rows 1,5,...]

(a) per product: the 1.3B decoder's five weight products at M = 1, 5, 16, 40, 96, 128, 160, 256, 384, 512 rows, ops.gemm_w8 (the
    streaming kernel) and ops.gemm_w8_tiled (the many-row kernel) on the codes beside ops.gemm on the bf16 weight (the baseline is
    the existing bf16 product, never an earlier version of a new kernel), alternated in one process, the weights rotated through a
    set three times the size of the MALL so that none is cache-resident: time and weight bytes / s of each, and the run-to-run
    spread.  Per row count the step sum 24 * (qkv + dense + fc1 + fc2) + lm_head of the bf16 products and of the products the
    FP8 step runs (streaming up to MPV_W8_MAX_ROWS rows, tiled above), and from them the row limit of the tiled kernel by the
    rule of DESIGN section 22.
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
ROWS = [1, 5, 16, 40, 96, 128, 160, 256, 384, 512]
TILED_CANDIDATES = [128, 160, 256, 384, 512]      # the row counts MPV_W8_TILED_MAX_ROWS is chosen from
ROTATE_BYTES = 768 << 20          # of codes per shape: three times the 256 MiB MALL (the bf16 set is twice that)


def _median(v):
    return sorted(v)[len(v) // 2]


def section_a(dev, rounds, rows=ROWS):
    from tools.bench_kernels import timeit
    from youku_mplug_amd import ops
    out = []
    print(f"{'product':>8} {'M':>4} {'bf16 us':>9} {'fp8 us':>9} {'tiled us':>9} {'bf16 TB/s':>10} {'fp8 TB/s':>9} {'tiled TB/s':>10} "
          f"{'fp8/bf16':>9} {'tiled/bf16':>10} {'spread':>7}")
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

            def tiled():
                i[0] = (i[0] + 1) % n
                ops.gemm_w8_tiled(a, qs[i[0]][0], qs[i[0]][1], M, N, K, out=c)
            t = {"bf16": [], "fp8": [], "tiled": []}
            for _ in range(rounds):
                for fn in (bf16, fp8, tiled):
                    t[fn.__name__].append(timeit(fn, iters=max(20, n)))
            med = {k: _median(v) for k, v in t.items()}
            spread = max((max(v) - min(v)) / med[k] for k, v in t.items())
            rec = {"product": name, "M": M, "N": N, "K": K, "rotated_weights": n, "seconds": t, "median_s": med,
                   "weight_bytes_per_s": {"bf16": N * K * 2 / med["bf16"], "fp8": N * K / med["fp8"], "tiled": N * K / med["tiled"]},
                   "fp8_over_bf16_time": med["fp8"] / med["bf16"], "tiled_over_bf16_time": med["tiled"] / med["bf16"], "pair_spread": spread}
            out.append(rec)
            bw = rec["weight_bytes_per_s"]
            print(f"{name:>8} {M:>4} {med['bf16'] * 1e6:9.1f} {med['fp8'] * 1e6:9.1f} {med['tiled'] * 1e6:9.1f} {bw['bf16'] / 1e12:10.2f} "
                  f"{bw['fp8'] / 1e12:9.2f} {bw['tiled'] / 1e12:10.2f} {rec['fp8_over_bf16_time']:9.2f} {rec['tiled_over_bf16_time']:10.2f} "
                  f"{spread:7.3f}", flush=True)
        del ws, qs
        torch.cuda.empty_cache()
    return out


def step_sums(per_product, w8_max_rows):
    """per row count: 24 * (qkv + dense + fc1 + fc2) + lm_head per round -> median and run-to-run spread, for the bf16 products and for
    the FP8 step's (streaming up to w8_max_rows rows, tiled above), and whether FP8 is below bf16 by more than the larger spread"""
    out = []
    for M in sorted({r["M"] for r in per_product}):
        by = {r["product"]: r["seconds"] for r in per_product if r["M"] == M}
        if set(by) != {name for name, _, _ in PRODUCTS}:
            continue
        kernel = "fp8" if M <= w8_max_rows else "tiled"
        rec = {"M": M, "fp8_kernel": kernel}
        for key, col in (("bf16", "bf16"), ("fp8", kernel)):
            sums = [LAYERS * sum(by[p][col][i] for p in ("qkv", "dense", "fc1", "fc2")) + by["lm_head"][col][i] for i in range(len(by["qkv"][col]))]
            rec[key + "_s"] = _median(sums)
            rec[key + "_spread"] = (max(sums) - min(sums)) / _median(sums)
        rec["fp8_over_bf16_time"] = rec["fp8_s"] / rec["bf16_s"]
        rec["fp8_wins"] = rec["fp8_s"] < rec["bf16_s"] * (1 - max(rec["bf16_spread"], rec["fp8_spread"]))
        out.append(rec)
    return out


def tiled_limit_by_rule(sums, w8_max_rows):
    """the largest of TILED_CANDIDATES such that FP8 wins there and at every smaller measured row count above w8_max_rows
    (None: not even the smallest, or a candidate was not measured)"""
    measured = {r["M"]: r["fp8_wins"] for r in sums if r["M"] > w8_max_rows}
    best = None
    for M in sorted(measured):
        if not measured[M]:
            break
        if M in TILED_CANDIDATES:
            best = M
    return best


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
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "w8_max_rows": _lib.W8_MAX_ROWS,
           "w8_tiled_max_rows": _lib.W8_TILED_MAX_ROWS}
    if os.path.isfile(args.out):                               # a run of one section keeps the other
        with open(args.out) as f:
            rec = dict(json.load(f), **rec)
    if "a" in args.sections.split(","):
        rec["per_product"] = section_a(dev, args.rounds, [int(m) for m in args.rows.split(",")])
        rec["step_sums"] = step_sums(rec["per_product"], _lib.W8_MAX_ROWS)
        rec["w8_tiled_max_rows_by_rule"] = tiled_limit_by_rule(rec["step_sums"], _lib.W8_MAX_ROWS)
        print(f"{'M':>4} {'bf16 step us':>13} {'fp8 step us':>12} {'kernel':>7} {'fp8/bf16':>9} {'spreads':>15} wins")
        for r in rec["step_sums"]:
            print(f"{r['M']:>4} {r['bf16_s'] * 1e6:13.1f} {r['fp8_s'] * 1e6:12.1f} {r['fp8_kernel']:>7} {r['fp8_over_bf16_time']:9.3f} "
                  f"{r['bf16_spread']:7.3f} {r['fp8_spread']:7.3f} {r['fp8_wins']}")
        print("tiled row limit by the rule:", rec["w8_tiled_max_rows_by_rule"], "-- built with", _lib.W8_TILED_MAX_ROWS)
    if "b" in args.sections.split(","):
        rec["end_to_end"] = section_b(dev, args.rounds, args.positions)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
