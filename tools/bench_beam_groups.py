"""Cost of the diverse (group) beam search on one GPU, written to profiles/beam_groups_cost.json.

(a) The bookkeeping kernel alone, 32 clips x 8 sequences: ops.beam_advance at K = 8 against ops.beam_advance_groups at 4 beams x 2
    groups and at 2 beams x 4 groups, each on its own candidate lists (2K, and 2K' + (G-1)K' per row) without stop tokens, so no clip
    ever finishes.  HIP events, 3 warm-up + 20 timed launches per kernel, alternated launch by launch.
(b) End to end on the 1.3B decoder with synthetic weights (the constants of tools/bench_caption_batched.py), 32 clips: the plain
    lockstep search at beam 8 against the group search at 4 x 2 and 2 x 4 -- the same 8 sequences per clip, the stop token banned
    (banned_token_ids) so that all three generate every position -- alternated --rounds times in one process.  The group search may
    be slower than the plain search of the same run by no more than the larger max - min of the two over the rounds.

Without --step this file is only a driver and does not touch the GPU: every measuring step is a child process under its own
`timeout -k 10`, the steps are chained (the first one that fails, faults or runs out of time ends the job, nothing is started behind
it) and their JSON lines are merged into the output file.  Clock and power are sampled as bench.py samples them.

    python tools/bench_beam_groups.py [--out profiles/beam_groups_cost.json] [--rounds 3] [--positions 24]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = {"kernel": 180, "end_to_end": 420}
CLIPS, SEQS = 32, 8
SHAPES = {"plain_8": (8, 1), "groups_4x2": (4, 2), "groups_2x4": (2, 4)}          # name -> (beams per group, groups)
PENALTY = 0.5


def _timeit_alternated(fns, iters=20, warm=3):
    import torch
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in fns}
    for i in range(iters):
        for k, fn in fns.items():
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    t = {k: sorted(s.elapsed_time(e) * 1e3 for s, e in v) for k, v in ev.items()}
    return {k: dict(median_us=round(v[len(v) // 2], 1), min_us=round(v[0], 1), max_us=round(v[-1], 1)) for k, v in t.items()}


def kernel_rows(dev, sampler_cls, positions):
    import torch
    from bench_caption_batched import PROMPT, STOP, VOCAB
    from youku_mplug_amd import ops
    from youku_mplug_amd.generation import BeamState
    Lt = PROMPT + positions
    g = torch.Generator().manual_seed(1)
    fns, shapes = {}, {}
    for name, (K, G) in SHAPES.items():
        m, rows = (G + 1) * K, CLIPS * G * K
        st = BeamState(torch.randint(8, VOCAB, (CLIPS * G, Lt), generator=g).to(dev), K)
        idx = torch.stack([torch.randperm(VOCAB - 8, generator=g)[:m] + 8 for _ in range(rows)]).to(dev)       # no stop token: nobody finishes
        val = (-torch.rand(rows, m, generator=g) * 4).sort(dim=1, descending=True).values.contiguous().to(dev)
        kw = dict(vocab=VOCAB, pos=PROMPT + 1, cur_len=2, first=False, stop_token=STOP)
        shapes[name] = dict(beams_per_group=K, groups=G, candidates_per_row=m, rows=rows, row_len=Lt)
        if G == 1:
            fns[name] = lambda st=st, val=val, idx=idx, kw=kw: ops.beam_advance(val, idx, st, **kw)
        else:
            fns[name] = lambda st=st, val=val, idx=idx, kw=kw, G=G: ops.beam_advance_groups(val, idx, st, groups=G, diversity_penalty=PENALTY, **kw)
    with sampler_cls(0) as sampler:
        t = _timeit_alternated(fns)
    tel = sampler.summary()
    for name in SHAPES:
        print(f"kernel {name}: {t[name]['median_us']} us ({t[name]['min_us']} - {t[name]['max_us']})", file=sys.stderr, flush=True)
    return dict(clips=CLIPS, shapes=shapes, diversity_penalty=PENALTY, times=t, sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"],
                clock_power_source=tel["clock_power_source"])


def end_to_end_rows(dev, sampler_cls, rounds, positions):
    import torch
    from bench_caption_batched import FFN, HEADS, HIDDEN, LAYERS, LN_EPS, MAX_POS, PROMPT, Q, STOP, VOCAB
    from youku_mplug_amd import generation
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    cfg = GPT3Config(vocab_size=VOCAB, hidden_size=HIDDEN, ffn_hidden_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                     max_position_embeddings=MAX_POS, layernorm_epsilon=LN_EPS, tokens_to_generate=positions, eod_id=STOP)
    torch.manual_seed(0)
    gpt = DistributedGPT3(config=cfg, device=dev).eval()
    gen = torch.Generator().manual_seed(1)
    qe = (torch.randn(CLIPS, Q, HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
    tokens = torch.randint(8, VOCAB, (CLIPS, PROMPT), generator=gen).to(dev)
    ban = generation.LogitsConstraints(banned_token_ids=(STOP,))
    steps = [0]
    step = generation.DecodeState.step

    def counted(self, *a, **k):
        steps[0] += 1
        return step(self, *a, **k)
    generation.DecodeState.step = counted

    def run(K, G):
        more = dict(beam_groups=G, diversity_penalty=PENALTY, num_return_gen=G) if G > 1 else {}
        return gpt.beam_search_batched(tokens, query_embeds=qe, beam_size=K, stop_token=STOP, prompt_length=PROMPT, constraints=ban, **more)
    times, nsteps, distinct = {k: [] for k in SHAPES}, {}, {}
    with torch.no_grad(), sampler_cls(0) as sampler:
        for name, (K, G) in SHAPES.items():                   # warm-up (allocator, workspaces), and the steps each search issues
            steps[0] = 0
            out = run(K, G)
            nsteps[name] = steps[0]
            if G > 1:                                         # how many of a clip's G best-per-group captions differ, on average
                distinct[name] = sum(len({tuple(r) for r in o.sequences.tolist()}) for o in out) / len(out)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, (K, G) in SHAPES.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(K, G)
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
    generation.DecodeState.step = step
    tel = sampler.summary()
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    row = dict(clips=CLIPS, sequences_per_clip=SEQS, query_slots=Q, prompt_tokens=PROMPT, positions=positions, rounds=rounds, diversity_penalty=PENALTY,
               decode_steps=nsteps, distinct_best_per_group_captions_per_clip=distinct, seconds={k: [round(x, 4) for x in v] for k, v in times.items()},
               median_s={k: round(v, 4) for k, v in med.items()}, spread_s={k: round(v, 4) for k, v in spread.items()},
               ms_per_position={k: round(1e3 * med[k] / positions, 3) for k in med},
               sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"], clock_power_source=tel["clock_power_source"], condition={})
    for name in SHAPES:
        if name == "plain_8":
            continue
        margin = max(spread["plain_8"], spread[name])
        row["condition"][name] = dict(slower_by_s=round(med[name] - med["plain_8"], 4), margin_s=round(margin, 4),
                                      not_slower=bool(med[name] - med["plain_8"] <= margin))
    print("end to end: " + ", ".join(f"{k} {med[k]:.4f} s (+- {spread[k]:.4f})" for k in SHAPES), file=sys.stderr, flush=True)
    return row


def run_step(step, rounds, positions):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    dev = torch.device("cuda:0")
    _lib.check(_lib.lib().mpv_check_device(), "mpv_check_device")
    res = {"kernel": lambda: kernel_rows(dev, bench.ClockPowerSampler, positions),
           "end_to_end": lambda: end_to_end_rows(dev, bench.ClockPowerSampler, rounds, positions)}[step]()
    print("RESULT " + json.dumps({"device": torch.cuda.get_device_name(0), "result": res}), flush=True)


def _child(step, rounds, positions):
    """one measuring step as a child process under its own time limit -> its result, or None (then the job ends)"""
    cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(rounds),
           "--positions", str(positions)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
    if p.returncode != 0 or line is None:
        print(f"step {step} ended with status {p.returncode}: nothing more is started", file=sys.stderr, flush=True)
        return None
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_groups_cost.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--positions", type=int, default=24)
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None, help="(internal) run one measuring step in this process")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a.rounds, a.positions)
    res = {"protocol": "one child process per step, each under its own timeout; kernel: HIP events, 3 warm-up + 20 timed launches per kernel, "
           f"alternated launch by launch, median / min / max; end to end: wall clock, {a.rounds} alternated rounds in one process, median and max - min",
           "not_run": []}
    ok = True
    for step in ("kernel", "end_to_end"):
        r = _child(step, a.rounds, a.positions) if ok else None
        if r is None:
            ok = False
            res["not_run"].append(step)
            continue
        res["device"], res[step] = r["device"], r["result"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
