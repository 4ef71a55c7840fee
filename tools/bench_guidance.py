"""Cost of guided decoding on one GPU, measured two ways and written to profiles/guidance.json.

(a) The launch alone: ops.logits_guide (scale 3, alpha 0.1) at 160 and 512 rows of the 1.3B vocabulary (51200), beside its byte floor
    3 * rows * vocab * 2 B (cond and uncond read once, cond written once) at 6.3 TB/s.  HIP events, 3 warm-up + 20 timed launches per
    figure; shader clock and package power sampled as bench.py samples them.
(b) Whole generations at 1.3B dims (256 query slots + an 8-token prompt, 30 tokens, kv="shared_prefix", early termination off):
    16 clips x 16 samples (top-p 0.9) and 32 clips x 5 beams, each three ways -- guided (scale 3), unguided on the same clips, and
    unguided on twice the clips (the rows the guided call's state holds) -- alternated --rounds times in one process; median and
    max - min spread of each.

    python tools/bench_guidance.py [--out profiles/guidance.json] [--rounds 3] [--no-generation]

No caption-quality figure is taken: the weights are random, no checkpoint exists here."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sampling import FFN, HEADS, HIDDEN, LAYERS, LN_EPS, MAX_POS, POSITIONS, PROMPT, Q, VOCAB, timeit  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
SAMPLE_SHAPE, BEAM_SHAPE = (16, 16), (32, 5)          # clips x fan


def launch_rows(dev, sampler_cls):
    from youku_mplug_amd import ops
    out = []
    g = torch.Generator().manual_seed(0)
    for rows in (160, 512):
        both = (torch.randn(2 * rows, VOCAB, generator=g) * 2.0).to(dev).to(torch.bfloat16)       # the two halves of one step's logits
        guide = lambda: ops.logits_guide(both[:rows], both[rows:], scale=3.0, alpha=0.1)          # in place: the time does not depend on the values
        with sampler_cls(0) as sampler:
            t = timeit(guide)
        tel = sampler.summary()
        floor = 3 * rows * VOCAB * 2 / HBM_BYTES_PER_S * 1e6
        out.append(dict(vocab=VOCAB, rows=rows, guide_us=round(t, 1), byte_floor_us=round(floor, 1), over_floor=round(t / floor, 2),
                        sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"], clock_power_source=tel["clock_power_source"]))
        print(f"rows {rows:4d} vocab {VOCAB}: guide {t:7.1f} us, floor {floor:6.1f} us   {tel['sclk_mhz']} MHz {tel['power_w']} W", file=sys.stderr,
              flush=True)
    return out


def _alternate(runs, rounds, sampler_cls):
    times = {k: [] for k in runs}
    with torch.no_grad(), sampler_cls(0) as sampler:
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
    tel = sampler.summary()
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return dict(seconds={k: [round(x, 4) for x in v] for k, v in times.items()}, median_s={k: round(v, 4) for k, v in med.items()},
                spread_s={k: round(max(v) - min(v), 4) for k, v in times.items()}, guided_over_unguided=round(med["guided"] / med["unguided"], 4),
                guided_over_twice_the_rows=round(med["guided"] / med["unguided_twice_the_rows"], 4),
                guided_minus_twice_the_rows_per_step_us=round((med["guided"] - med["unguided_twice_the_rows"]) / POSITIONS * 1e6, 1),
                sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"], clock_power_source=tel["clock_power_source"])


def generation_rows(dev, sampler_cls, rounds):
    from youku_mplug_amd.generation import Guidance
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    cfg = GPT3Config(vocab_size=VOCAB, hidden_size=HIDDEN, ffn_hidden_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                     max_position_embeddings=MAX_POS, layernorm_epsilon=LN_EPS, tokens_to_generate=POSITIONS, eod_id=7, top_k=0, top_p=0.9)
    torch.manual_seed(0)
    gpt = DistributedGPT3(config=cfg, device=dev).eval()
    gen = torch.Generator().manual_seed(1)
    most = 2 * max(SAMPLE_SHAPE[0], BEAM_SHAPE[0])
    qe = (torch.randn(most, Q, HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
    null = (torch.randn(Q, HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
    tokens = torch.randint(8, VOCAB, (most, PROMPT), generator=gen).to(dev)
    guidance = Guidance(3.0, 0.0, null)
    out = {}
    clips, fan = SAMPLE_SHAPE
    skw = lambda n: dict(query_embeds=qe[:n], prompt_length=torch.full((n,), PROMPT, device=dev), num_samples=fan, seed=1, kv="shared_prefix",
                         use_eod_token_for_early_termination=False)
    runs = {"unguided": lambda: gpt.sample_batched(tokens[:clips], **skw(clips)),
            "guided": lambda: gpt.sample_batched(tokens[:clips], guidance=guidance, **skw(clips)),
            "unguided_twice_the_rows": lambda: gpt.sample_batched(tokens[:2 * clips], **skw(2 * clips))}
    out["samples"] = dict(workload=f"{clips} clips x {fan} samples x {POSITIONS} tokens, 1.3B dims, {Q} query slots + {PROMPT}-token prompt, top-p 0.9, "
                                   "shared-prefix KV; guided: scale 3", **_alternate(runs, rounds, sampler_cls))
    clips, fan = BEAM_SHAPE
    # a stop token the random decoder never prefers: the searches run their full length
    bkw = lambda n: dict(query_embeds=qe[:n], beam_size=fan, num_return_gen=1, stop_token=7, prompt_length=PROMPT, kv="shared_prefix")
    runs = {"unguided": lambda: gpt.beam_search_batched(tokens[:clips], **bkw(clips)),
            "guided": lambda: gpt.beam_search_batched(tokens[:clips], guidance=guidance, **bkw(clips)),
            "unguided_twice_the_rows": lambda: gpt.beam_search_batched(tokens[:2 * clips], **bkw(2 * clips))}
    out["beams"] = dict(workload=f"{clips} clips x {fan} beams x up to {POSITIONS} tokens, 1.3B dims, {Q} query slots + {PROMPT}-token prompt, "
                                 "shared-prefix KV; guided: scale 3", **_alternate(runs, rounds, sampler_cls))
    for k, v in out.items():
        print(f"{k}: unguided {v['median_s']['unguided']:.4f} s, guided {v['median_s']['guided']:.4f} s, unguided at twice the rows "
              f"{v['median_s']['unguided_twice_the_rows']:.4f} s", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-generation", action="store_true")
    a = ap.parse_args()
    import bench
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    dev = torch.device("cuda:0")
    _lib.check(_lib.lib().mpv_check_device(), "mpv_check_device")
    res = {"device": torch.cuda.get_device_name(0), "protocol": "HIP events, 3 warm-up + 20 timed launches per figure; generation: wall clock, "
           f"{a.rounds} alternated rounds, median and max - min; one run; no caption-quality figure (random weights)",
           "launch": launch_rows(dev, bench.ClockPowerSampler)}
    if not a.no_generation:
        res["generation"] = generation_rows(dev, bench.ClockPowerSampler, a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
