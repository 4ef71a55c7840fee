"""Cost of sampled generation on one GPU, measured two ways and written to profiles/sampling_cost.json.

(a) One sampling step: the fused launch (ops.sample_advance: filter, draw and the loop body's bookkeeping) beside generation.sample_token
    -- the chain of torch calls of the host loop, untouched by the fused path -- in the same process, on the same bf16 logits:
    rows in {1, 32, 160} x V = 51200, for top-p 0.9, top-k 50 and plain sampling.  HIP events, 3 warm-up + 20 timed calls per figure,
    the two sides alternated over --rounds rounds; shader clock and package power sampled as bench.py samples them.
(b) A whole generation: tokens/s of DistributedGPT3.sample (the host loop, 160 sequences with the prefix repeated per sample) beside
    DistributedGPT3.sample_batched (32 clips x 5 samples, prefill once per clip) at the 1.3B decoder's dims with synthetic weights,
    256 query slots + an 8-token prompt, 30 generated tokens, top-p 0.9, early termination off so that both generate every position.

    python tools/bench_sampling.py [--out profiles/sampling_cost.json] [--rounds 3] [--no-generation]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIDDEN, LAYERS, HEADS, FFN, VOCAB, MAX_POS, LN_EPS = 2048, 24, 32, 8192, 51200, 2048, 1e-5      # bench.py's 1.3B decoder
Q, PROMPT, CLIPS, SAMPLES, POSITIONS = 256, 8, 32, 5, 30
FILTERS = (("top_p_0.9", dict(top_k=0, top_p=0.9)), ("top_k_50", dict(top_k=50, top_p=0.0)), ("plain", dict(top_k=0, top_p=0.0)))


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3      # us


def step_rows(dev, sampler_cls, rounds):
    from youku_mplug_amd import generation, ops
    out = []
    g = torch.Generator().manual_seed(0)
    for rows in (1, 32, 160):
        logits = (torch.randn(rows, VOCAB, generator=g) * 2.0 - 20.0)
        hot = torch.randint(0, VOCAB, (rows, 40), generator=g)
        logits.scatter_(1, hot, -6.0 * torch.rand(rows, 40, generator=g))
        logits = logits.to(dev).to(torch.bfloat16)
        st = generation.SampleState(torch.zeros((rows, 8), dtype=torch.int64, device=dev), torch.zeros(rows, dtype=torch.int64, device=dev))
        for name, f in FILTERS:
            fused = lambda: ops.sample_advance(logits, st, pos=3, temperature=1.0, seed=1, vocab_size=VOCAB, termination_id=7, **f)
            chain = lambda: generation.sample_token(logits, temperature=1.0, vocab_size=VOCAB, **f)
            t = {"fused": [], "chain": []}
            with sampler_cls(0) as sampler:
                for _ in range(rounds):
                    t["fused"].append(timeit(fused))
                    t["chain"].append(timeit(chain))
            tel = sampler.summary()
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            row = dict(rows=rows, vocab=VOCAB, filter=name, fused_us=[round(x, 1) for x in t["fused"]], chain_us=[round(x, 1) for x in t["chain"]],
                       fused_median_us=round(med["fused"], 1), chain_median_us=round(med["chain"], 1), chain_over_fused=round(med["chain"] / med["fused"], 2),
                       logits_bytes=rows * VOCAB * 2, sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"], clock_power_source=tel["clock_power_source"])
            out.append(row)
            print(f"rows {rows:4d} {name:10s} fused {med['fused']:8.1f} us   torch chain {med['chain']:8.1f} us   x{row['chain_over_fused']:.2f}   "
                  f"{tel['sclk_mhz']} MHz {tel['power_w']} W", file=sys.stderr, flush=True)
    return out


def generation_row(dev, sampler_cls, rounds):
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    cfg = GPT3Config(vocab_size=VOCAB, hidden_size=HIDDEN, ffn_hidden_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                     max_position_embeddings=MAX_POS, layernorm_epsilon=LN_EPS, tokens_to_generate=POSITIONS, eod_id=7, top_k=0, top_p=0.9)
    torch.manual_seed(0)
    gpt = DistributedGPT3(config=cfg, device=dev).eval()
    gen = torch.Generator().manual_seed(1)
    qe = (torch.randn(CLIPS, Q, HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
    tokens = torch.randint(8, VOCAB, (CLIPS, PROMPT), generator=gen).to(dev)
    lengths = torch.full((CLIPS,), PROMPT, device=dev)
    kw = dict(use_eod_token_for_early_termination=False)

    def host_loop():
        return gpt.sample(tokens.repeat_interleave(SAMPLES, 0), query_embeds=qe.repeat_interleave(SAMPLES, 0), prompt_length=lengths.repeat_interleave(SAMPLES), **kw)

    def batched():
        return gpt.sample_batched(tokens, query_embeds=qe, prompt_length=lengths, num_samples=SAMPLES, seed=1, **kw)
    times = {"host_loop": [], "batched": []}
    with torch.no_grad(), sampler_cls(0) as sampler:
        for fn in (host_loop, batched):
            out = fn()
            assert out.shape[0] == CLIPS * SAMPLES and out.shape[1] >= PROMPT + POSITIONS
        torch.cuda.synchronize()
        for _ in range(rounds):
            for fn in (host_loop, batched):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[fn.__name__].append(time.perf_counter() - t0)
    tel = sampler.summary()
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    n_tok = CLIPS * SAMPLES * POSITIONS
    row = dict(workload=f"{CLIPS} clips x {SAMPLES} samples x {POSITIONS} tokens, 1.3B dims, {Q} query slots + {PROMPT}-token prompt, top-p 0.9",
               seconds={k: [round(x, 4) for x in v] for k, v in times.items()}, median_s={k: round(v, 4) for k, v in med.items()},
               tokens_per_s={k: round(n_tok / v, 1) for k, v in med.items()}, batched_over_host_loop=round(med["host_loop"] / med["batched"], 2),
               sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"], clock_power_source=tel["clock_power_source"])
    print(f"generation: host loop {med['host_loop']:.3f} s, batched {med['batched']:.3f} s, x{row['batched_over_host_loop']:.2f}", file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_cost.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-generation", action="store_true")
    a = ap.parse_args()
    import bench
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    dev = torch.device("cuda:0")
    _lib.check(_lib.lib().mpv_check_device(), "mpv_check_device")
    res = {"device": torch.cuda.get_device_name(0), "protocol": f"HIP events, 3 warm-up + 20 timed calls per figure, {a.rounds} alternated rounds, medians",
           "step": step_rows(dev, bench.ClockPowerSampler, a.rounds)}
    if not a.no_generation:
        res["generation"] = generation_row(dev, bench.ClockPowerSampler, a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
