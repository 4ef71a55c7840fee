"""Decode against a per-clip shared prefix KV cache on one GPU.

1. Kernel level, the 1.3B decoder's attention dims (32 heads x 64), 264 shared positions + 12 generated ones: today's decode
   attention (mpv_attn_fwd with sq = 1 on per-sequence caches) beside mpv_attn_decode_shared_fwd (prefix cache + suffix cache) for
   (clips, sequences per clip) = (1, 5), (8, 5), (32, 5), (32, 16).  HIP events, 3 warm-up + 20 timed launches (the protocol of
   tools/bench_temporal_long.py); microseconds and algorithmic GB/s (the K and V rows each formulation has to read: sequences x 276
   against clips x 264 + sequences x 12, 8 KB per row), shader clock and package power sampled as bench.py samples them.
2. End to end, the protocol and constants of tools/bench_caption_batched.py (1.3B decoder, synthetic weights, 256 query slots + an
   8-token prompt, 24 generated positions): beam 5 at 8 and 32 clips and 16 samples at 32 clips, kv="per_sequence" and
   "shared_prefix" alternated three times in one process: median seconds and spread, kv_bytes() of the state and
   torch.cuda.max_memory_allocated of each.

    python tools/bench_decode_shared.py [--out profiles/decode_shared_prefix.json] [--rounds 3] [--skip_e2e]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_caption_batched import BEAMS, FFN, HEADS, HIDDEN, LAYERS, LN_EPS, MAX_POS, PROMPT, Q, STOP, VOCAB  # noqa: E402
from bench_temporal_long import timeit  # noqa: E402

HD = HIDDEN // HEADS
PREFIX, OWN, SUFFIX_MAX = Q + PROMPT, 12, 36
ROW_BYTES = 2 * HIDDEN * 2                       # K and V of one position, all heads


def kernel_rows(dev, sampler_cls):
    from youku_mplug_amd import ops
    H, out = HIDDEN, []
    for G, K in ((1, 5), (8, 5), (32, 5), (32, 16)):
        n = G * K
        ML = PREFIX + SUFFIX_MAX
        cache = (torch.randn(n * ML, 3 * H, device=dev) * 0.5).bfloat16()
        prefix = (torch.randn(G * PREFIX, 3 * H, device=dev) * 0.5).bfloat16()
        suffix = (torch.randn(n * SUFFIX_MAX, 3 * H, device=dev) * 0.5).bfloat16()
        o = torch.empty(n, H, dtype=torch.bfloat16, device=dev)
        cs = (ML * 3 * H, 3 * HD, 3 * H)
        lay = ops.AttnLayout(cs, cs, cs, (H, HD, H))
        ss = (SUFFIX_MAX * 3 * H, 3 * HD, 3 * H)
        slay = ops.AttnLayout(ss, ss, ss, (H, HD, H))
        ps = (PREFIX * 3 * H, 3 * HD, 3 * H)
        sk, scale = PREFIX + OWN, HD ** -0.5
        cf, sf, pf = cache.view(-1), suffix.view(-1), prefix.view(-1)

        def per_sequence():
            ops.attn_fwd(cf[(sk - 1) * 3 * H:], cf[HD:], cf[2 * HD:], o, lay, n, HEADS, 1, sk, HD, causal=True, scale=scale)

        def shared():
            ops.attn_decode_shared_fwd(sf[(OWN - 1) * 3 * H:], sf[HD:], sf[2 * HD:], pf[HD:], pf[2 * HD:], o, slay, (ps, ps), n, K, HEADS, PREFIX, OWN,
                                       HD, scale=scale)
        with sampler_cls(0) as sampler:
            ta, tb = timeit(per_sequence), timeit(shared)
        tel = sampler.summary()
        ba, bb = n * sk * ROW_BYTES, (G * PREFIX + n * OWN) * ROW_BYTES
        row = dict(clips=G, per_clip=K, sequences=n, per_sequence_us=round(ta * 1e6, 1), shared_us=round(tb * 1e6, 1),
                   per_sequence_bytes=ba, shared_bytes=bb, per_sequence_gbps=round(ba / ta / 1e9), shared_gbps=round(bb / tb / 1e9),
                   speedup=round(ta / tb, 2), sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"], clock_power_source=tel["clock_power_source"])
        print(f"kernel {G:2d} x {K:2d}: per-sequence {row['per_sequence_us']:7.1f} us ({row['per_sequence_gbps']:5d} GB/s)  shared "
              f"{row['shared_us']:7.1f} us ({row['shared_gbps']:5d} GB/s)  x{row['speedup']:.2f}  {tel['sclk_mhz']} MHz {tel['power_w']} W", flush=True)
        out.append(row)
        del cache, prefix, suffix, o
        torch.cuda.empty_cache()
    return out


def end_to_end(dev, rounds, positions):
    from youku_mplug_amd import generation
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    cfg = GPT3Config(vocab_size=VOCAB, hidden_size=HIDDEN, ffn_hidden_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                     max_position_embeddings=MAX_POS, layernorm_epsilon=LN_EPS, tokens_to_generate=positions, eod_id=STOP)
    torch.manual_seed(0)
    gpt = DistributedGPT3(config=cfg, device=dev).eval()
    states = []
    make = generation.make_state_fn

    def recording(g, kv="per_sequence"):
        inner = make(g, kv)

        def make_state(batch, max_len):
            states.append(inner(batch, max_len))
            return states[-1]
        return make_state
    generation.make_state_fn = recording
    gen = torch.Generator().manual_seed(1)
    P, S, row3 = Q + PROMPT, positions, 3 * HIDDEN * 2
    cases = []
    try:
        with torch.no_grad():
            for mode, B, K in (("beam", 8, BEAMS), ("beam", 32, BEAMS), ("sample", 32, 16)):
                qe = (torch.randn(B, Q, HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
                tokens = torch.randint(8, VOCAB, (B, PROMPT), generator=gen).to(dev)

                def run(kv):
                    if mode == "beam":
                        return gpt.beam_search_batched(tokens, query_embeds=qe, beam_size=K, stop_token=STOP, prompt_length=PROMPT, kv=kv)
                    return gpt.sample_batched(tokens, query_embeds=qe, num_samples=K, seed=1, use_eod_token_for_early_termination=False, kv=kv)
                kvs = ("per_sequence", "shared_prefix")
                times, kvb, peak = {k: [] for k in kvs}, {}, {}
                for kv in kvs:                                   # warm-up (allocator, workspaces)
                    run(kv)
                    states.clear()
                torch.cuda.synchronize()
                for _ in range(rounds):
                    for kv in kvs:
                        torch.cuda.empty_cache()
                        torch.cuda.reset_peak_memory_stats(dev)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        run(kv)
                        torch.cuda.synchronize()
                        times[kv].append(time.perf_counter() - t0)
                        peak[kv] = torch.cuda.max_memory_allocated(dev)
                        kvb[kv] = states[-1].kv_bytes()
                        states.clear()
                med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
                spread = {k: max(v) - min(v) for k, v in times.items()}
                copies = 2 if mode == "beam" else 1
                formula = {"per_sequence": LAYERS * 2 * B * K * (P + S) * row3, "shared_prefix": LAYERS * (B * P + copies * B * K * S) * row3}
                case = dict(mode=mode, clips=B, per_clip=K, positions=positions, seconds=times, median_s=med, spread_s=spread, kv_bytes=kvb,
                            kv_bytes_formula=formula, max_memory_allocated=peak,
                            shared_minus_per_sequence_s=med["shared_prefix"] - med["per_sequence"], larger_spread_s=max(spread.values()))
                assert kvb == formula, (kvb, formula)
                cases.append(case)
                print(f"{mode:6s} {B:2d} x {K:2d}: per-sequence {med['per_sequence']:.4f} s (spread {spread['per_sequence']:.4f})  shared "
                      f"{med['shared_prefix']:.4f} s (spread {spread['shared_prefix']:.4f})  KV {kvb['per_sequence'] / 2**30:.2f} -> "
                      f"{kvb['shared_prefix'] / 2**30:.2f} GiB  peak {peak['per_sequence'] / 2**30:.2f} -> {peak['shared_prefix'] / 2**30:.2f} GiB",
                      flush=True)
                del qe, tokens
                torch.cuda.empty_cache()
    finally:
        generation.make_state_fn = make
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_shared_prefix.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--positions", type=int, default=24)
    ap.add_argument("--skip_e2e", action="store_true")
    a = ap.parse_args()
    import bench
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    dev = torch.device("cuda:0")
    _lib.check(_lib.lib().mpv_check_device(), "mpv_check_device")
    res = {"device": torch.cuda.get_device_name(0),
           "kernel_dims": dict(heads=HEADS, head_dim=HD, prefix_len=PREFIX, own_len=OWN, row_bytes=ROW_BYTES),
           "kernel_protocol": "HIP events, 3 warm-up + 20 timed launches per figure",
           "kernel": kernel_rows(dev, bench.ClockPowerSampler)}
    if not a.skip_e2e:
        res["end_to_end_protocol"] = f"tools/bench_caption_batched.py's decoder and constants; {a.rounds} alternated rounds in one process"
        res["end_to_end"] = end_to_end(dev, a.rounds, a.positions)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
