"""Cost of the generation constraints on one GPU, measured two ways and written to profiles/logits_constrain_cost.json.

(a) The launch alone: ops.logits_constrain with every constraint on (penalty 1.3, no-repeat bigrams, min_new_tokens, three banned ids)
    beside ops.sample_advance (top-p 0.9) on the same bf16 logits in the same run: rows in {160, 512} x history in {8, 32, 128}, at
    the 1.3B vocabulary (51200) and again at 8192 -- the constraint launch follows the history, not the vocabulary.  HIP events, 3
    warm-up + 20 timed launches per figure; shader clock and package power sampled as bench.py samples them.
(b) A whole generation with tools/bench_sampling.py's constants (32 clips x 5 samples x 30 tokens, 1.3B dims, 256 query slots + an
    8-token prompt, top-p 0.9, early termination off): DistributedGPT3.sample_batched with constraints off and on, alternated
    --rounds times in one process; median and max - min spread of each.

    python tools/bench_logits_constrain.py [--out profiles/logits_constrain_cost.json] [--rounds 3] [--no-generation]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sampling import CLIPS, FFN, HEADS, HIDDEN, LAYERS, LN_EPS, MAX_POS, POSITIONS, PROMPT, Q, SAMPLES, VOCAB, timeit  # noqa: E402

PROMPT_COLS = 8


def all_on():
    from youku_mplug_amd.generation import LogitsConstraints
    return LogitsConstraints(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=10 ** 6, banned_token_ids=(11, 12, 13))


def launch_rows(dev, sampler_cls):
    from youku_mplug_amd import generation, ops
    out = []
    g = torch.Generator().manual_seed(0)
    for vocab in (VOCAB, 8192):
        for rows in (160, 512):
            base = (torch.randn(rows, vocab, generator=g) * 2.0 - 20.0).to(dev).to(torch.bfloat16)
            for hist in (8, 32, 128):
                pos = PROMPT_COLS + hist
                tokens = torch.randint(0, vocab, (rows, pos + 2), generator=g).to(dev)
                st = generation.SampleState(tokens, torch.full((rows,), PROMPT_COLS, dtype=torch.int64, device=dev))
                logits = base.clone()                                       # the launch edits in place: the time does not depend on the values
                c = all_on()
                constrain = lambda: ops.logits_constrain(logits, st.tokens, pos=pos, constraints=c, prompt_len=st.prompt_len, eos_ids=[7])
                sample = lambda: ops.sample_advance(logits, st, pos=pos, temperature=1.0, top_k=0, top_p=0.9, seed=1, vocab_size=vocab, termination_id=7)
                with sampler_cls(0) as sampler:
                    t_c, t_s = timeit(constrain), timeit(sample)
                tel = sampler.summary()
                row = dict(vocab=vocab, rows=rows, history=hist, constrain_us=round(t_c, 1), sample_advance_us=round(t_s, 1),
                           constrain_over_sample=round(t_c / t_s, 3), sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"],
                           clock_power_source=tel["clock_power_source"])
                out.append(row)
                print(f"vocab {vocab:6d} rows {rows:4d} history {hist:4d}: constrain {t_c:7.1f} us   sample_advance {t_s:7.1f} us   "
                      f"{tel['sclk_mhz']} MHz {tel['power_w']} W", file=sys.stderr, flush=True)
    return out


def generation_row(dev, sampler_cls, rounds):
    from youku_mplug_amd.generation import LogitsConstraints
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    cfg = GPT3Config(vocab_size=VOCAB, hidden_size=HIDDEN, ffn_hidden_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                     max_position_embeddings=MAX_POS, layernorm_epsilon=LN_EPS, tokens_to_generate=POSITIONS, eod_id=7, top_k=0, top_p=0.9)
    torch.manual_seed(0)
    gpt = DistributedGPT3(config=cfg, device=dev).eval()
    gen = torch.Generator().manual_seed(1)
    qe = (torch.randn(CLIPS, Q, HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
    tokens = torch.randint(8, VOCAB, (CLIPS, PROMPT), generator=gen).to(dev)
    lengths = torch.full((CLIPS,), PROMPT, device=dev)
    kw = dict(query_embeds=qe, prompt_length=lengths, num_samples=SAMPLES, seed=1, use_eod_token_for_early_termination=False)
    c = LogitsConstraints(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=5)
    runs = {"off": lambda: gpt.sample_batched(tokens, **kw), "on": lambda: gpt.sample_batched(tokens, constraints=c, **kw)}
    times = {k: [] for k in runs}
    with torch.no_grad(), sampler_cls(0) as sampler:
        for fn in runs.values():
            assert fn().shape[0] == CLIPS * SAMPLES
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
    row = dict(workload=f"{CLIPS} clips x {SAMPLES} samples x {POSITIONS} tokens, 1.3B dims, {Q} query slots + {PROMPT}-token prompt, top-p 0.9; "
                        "on: penalty 1.3, no-repeat bigrams, min_new_tokens 5",
               seconds={k: [round(x, 4) for x in v] for k, v in times.items()}, median_s={k: round(v, 4) for k, v in med.items()},
               spread_s={k: round(max(v) - min(v), 4) for k, v in times.items()}, on_over_off=round(med["on"] / med["off"], 4),
               per_step_us=round((med["on"] - med["off"]) / POSITIONS * 1e6, 1), sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"],
               clock_power_source=tel["clock_power_source"])
    print(f"generation: constraints off {med['off']:.4f} s, on {med['on']:.4f} s (x{row['on_over_off']:.4f})", file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logits_constrain_cost.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-generation", action="store_true")
    a = ap.parse_args()
    import bench
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    dev = torch.device("cuda:0")
    _lib.check(_lib.lib().mpv_check_device(), "mpv_check_device")
    res = {"device": torch.cuda.get_device_name(0), "protocol": "HIP events, 3 warm-up + 20 timed launches per figure; generation: wall clock, "
           f"{a.rounds} alternated rounds, median and max - min", "launch": launch_rows(dev, bench.ClockPowerSampler)}
    if not a.no_generation:
        res["generation"] = generation_row(dev, bench.ClockPowerSampler, a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
