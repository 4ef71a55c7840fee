"""Cost of the sequence scores of sampled generation on one GPU, measured three ways and written to
profiles/sample_scores_cost.json.

(a) The launch alone: ops.sample_score beside ops.sample_advance (top-p 0.9) on the same bf16 logits in the same run: rows in
    {160, 512} at the 1.3B vocabulary (51200) and again at 8192.  HIP events, 3 warm-up + 20 timed launches per figure; shader clock
    and package power sampled as bench.py samples them.
(b) A whole generation with tools/bench_sampling.py's constants (32 clips x 5 samples x 30 tokens, 1.3B dims, 256 query slots + an
    8-token prompt, top-p 0.9, early termination off): DistributedGPT3.sample_batched with return_scores off and on, alternated
    --rounds times in one process; median and max - min spread of each.
(c) The plain path (no keyword of this feature) on another tree and on this tree -- `--parent DIR`, a built checkout of the parent
    commit -- one process per figure, alternated --rounds times: does the tree with the score kernel leave the unscored generation
    where it was?  It passes when the difference of the medians is within the larger max - min of the two sides.

Without --step this file is only a driver and does not touch the GPU: every measuring step is a child process under its own
`timeout -k 10`, the steps are chained (the first one that fails, faults or runs out of time ends the job, nothing is started behind
it) and their JSON lines are merged into the output file.

    python tools/bench_sample_scores.py [--out profiles/sample_scores_cost.json] [--rounds 3] [--parent DIR] [--no-generation]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = {"launch": 240, "generation": 420, "plain": 300}


def _use_tree(tree):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.abspath(tree))


def launch_rows(dev, sampler_cls):
    import torch
    from bench_sampling import VOCAB, timeit
    from youku_mplug_amd import generation, ops
    out = []
    g = torch.Generator().manual_seed(0)
    for vocab in (VOCAB, 8192):
        for rows in (160, 512):
            logits = (torch.randn(rows, vocab, generator=g) * 2.0 - 20.0).to(dev).to(torch.bfloat16)
            st = generation.SampleState(torch.randint(0, vocab, (rows, 40), generator=g).to(dev), torch.full((rows,), 8, dtype=torch.int64, device=dev))
            sc = generation.SampleScores(rows, 40, dev)
            # termination_id -1: no row ever ends, so every timed launch scores every row (a finished row would return at once)
            sample = lambda: ops.sample_advance(logits, st, pos=20, temperature=1.0, top_k=0, top_p=0.9, seed=1, vocab_size=vocab, termination_id=-1)
            score = lambda: ops.sample_score(logits, st, sc, pos=20)
            with sampler_cls(0) as sampler:
                t_a, t_s = timeit(sample), timeit(score)
            tel = sampler.summary()
            assert int(sc.count.min()) == 23 and int(sc.live.min()) == 1
            row = dict(vocab=vocab, rows=rows, sample_score_us=round(t_s, 1), sample_advance_us=round(t_a, 1), score_over_sample=round(t_s / t_a, 3),
                       logits_bytes=rows * vocab * 2, sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"], clock_power_source=tel["clock_power_source"])
            out.append(row)
            print(f"vocab {vocab:6d} rows {rows:4d}: sample_score {t_s:7.1f} us   sample_advance {t_a:7.1f} us   {tel['sclk_mhz']} MHz {tel['power_w']} W",
                  file=sys.stderr, flush=True)
    return out


def _generation_setup(dev):
    import torch
    from bench_sampling import CLIPS, FFN, HEADS, HIDDEN, LAYERS, LN_EPS, MAX_POS, POSITIONS, PROMPT, Q, SAMPLES, VOCAB
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    cfg = GPT3Config(vocab_size=VOCAB, hidden_size=HIDDEN, ffn_hidden_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                     max_position_embeddings=MAX_POS, layernorm_epsilon=LN_EPS, tokens_to_generate=POSITIONS, eod_id=7, top_k=0, top_p=0.9)
    torch.manual_seed(0)
    gpt = DistributedGPT3(config=cfg, device=dev).eval()
    gen = torch.Generator().manual_seed(1)
    qe = (torch.randn(CLIPS, Q, HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
    tokens = torch.randint(8, VOCAB, (CLIPS, PROMPT), generator=gen).to(dev)
    kw = dict(query_embeds=qe, prompt_length=torch.full((CLIPS,), PROMPT, device=dev), num_samples=SAMPLES, seed=1,
              use_eod_token_for_early_termination=False)
    what = f"{CLIPS} clips x {SAMPLES} samples x {POSITIONS} tokens, 1.3B dims, {Q} query slots + {PROMPT}-token prompt, top-p 0.9"
    return gpt, tokens, kw, what, CLIPS * SAMPLES, POSITIONS


def _alternate(runs, rounds):
    import torch
    times = {k: [] for k in runs}
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
    return times


def generation_row(dev, sampler_cls, rounds):
    import torch
    gpt, tokens, kw, what, R, positions = _generation_setup(dev)
    runs = {"off": lambda: gpt.sample_batched(tokens, **kw), "on": lambda: gpt.sample_batched(tokens, return_scores=True, **kw)}
    with torch.no_grad(), sampler_cls(0) as sampler:
        toks, sc = runs["on"]()
        assert toks.shape[0] == R and torch.equal(toks, runs["off"]()) and bool(torch.isfinite(sc.sum_logprob).all()) and int(sc.count.max()) <= positions
        times = _alternate(runs, rounds)
    tel = sampler.summary()
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    row = dict(workload=what + "; on: return_scores=True", seconds={k: [round(x, 4) for x in v] for k, v in times.items()},
               median_s={k: round(v, 4) for k, v in med.items()}, spread_s={k: round(max(v) - min(v), 4) for k, v in times.items()},
               on_over_off=round(med["on"] / med["off"], 4), per_step_us=round((med["on"] - med["off"]) / positions * 1e6, 1),
               sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"], clock_power_source=tel["clock_power_source"])
    print(f"generation: return_scores off {med['off']:.4f} s, on {med['on']:.4f} s (x{row['on_over_off']:.4f})", file=sys.stderr, flush=True)
    return row


def plain_row(dev, sampler_cls):
    """one figure of case (c): the generation without any keyword of this feature, on whatever tree is first on sys.path"""
    import torch
    gpt, tokens, kw, what, R, _ = _generation_setup(dev)
    with torch.no_grad(), sampler_cls(0) as sampler:
        times = _alternate({"plain": lambda: gpt.sample_batched(tokens, **kw)}, 3)["plain"]
    tel = sampler.summary()
    return dict(batched_s=round(sorted(times)[1], 4), seconds=[round(x, 4) for x in times], sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"])


def run_step(step, tree, rounds):
    _use_tree(tree)
    import torch
    import bench
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    dev = torch.device("cuda:0")
    _lib.check(_lib.lib().mpv_check_device(), "mpv_check_device")
    res = {"launch": lambda: launch_rows(dev, bench.ClockPowerSampler), "generation": lambda: generation_row(dev, bench.ClockPowerSampler, rounds),
           "plain": lambda: plain_row(dev, bench.ClockPowerSampler)}[step]()
    print("RESULT " + json.dumps({"device": torch.cuda.get_device_name(0), "result": res}), flush=True)


def _child(step, tree, rounds):
    """one measuring step as a child process under its own time limit -> its result, or None (then the job ends)"""
    cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--tree", tree, "--rounds", str(rounds)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=tree)
    line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
    if p.returncode != 0 or line is None:
        print(f"step {step} on {tree} ended with status {p.returncode}: nothing more is started", file=sys.stderr, flush=True)
        return None
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_scores_cost.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: case (c)")
    ap.add_argument("--no-generation", action="store_true")
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None, help="(internal) run one measuring step in this process")
    ap.add_argument("--tree", default=ROOT, help="(internal) the tree the step imports the package from")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a.tree, a.rounds)
    res = {"protocol": "one child process per step, each under its own timeout; launch: HIP events, 3 warm-up + 20 timed launches per figure; "
           f"generation: wall clock, {a.rounds} alternated rounds, median and max - min", "not_run": []}
    ok = True
    steps = [("launch", "launch")] + ([] if a.no_generation else [("generation", "generation")])
    for key, step in steps:
        r = _child(step, ROOT, a.rounds) if ok else None
        if r is None:
            ok = False
            res["not_run"].append(key)
            continue
        res["device"], res[key] = r["device"], r["result"]
    if a.parent and not a.no_generation:
        sides = {"parent": [], "this_tree": []}
        for _ in range(a.rounds):
            for side, tree in (("parent", os.path.abspath(a.parent)), ("this_tree", ROOT)):
                r = _child("plain", tree, a.rounds) if ok else None
                if r is None:
                    ok = False
                    continue
                sides[side].append(r["result"])
        if ok:
            med = {k: sorted(x["batched_s"] for x in v)[len(v) // 2] for k, v in sides.items()}
            spread = {k: round(max(x["batched_s"] for x in v) - min(x["batched_s"] for x in v), 4) for k, v in sides.items()}
            margin = max(spread.values())
            res["plain_ab"] = dict(workload="case (c): sample_batched without any keyword of this feature; the parent commit's tree and this tree, "
                                   f"one process per figure (median of 3 timed generations), alternated {a.rounds} times in one job", **sides,
                                   parent_median_s=med["parent"], this_tree_median_s=med["this_tree"], parent_spread_s=spread["parent"],
                                   this_tree_spread_s=spread["this_tree"], margin_s=margin, not_slower=bool(med["this_tree"] - med["parent"] <= margin))
        else:
            res["not_run"].append("plain_ab")
    else:
        res["not_run"].append("plain_ab (no --parent tree given)" if not a.parent else "plain_ab")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
