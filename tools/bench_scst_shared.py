"""Cost of the self-critical training pass on a shared prefix against the per-sequence pass, one GPU, written
to profiles/scst_shared_prefix.json.  The decoder and the constants are tools/bench_scst.py's: the 1.3B dims with synthetic weights
(frozen), the tiny ViT, 256 query slots, 8-token prompts, 16 samples per clip.

  a. attention  mpv_attn_prefix_packed_fwd_lse and mpv_attn_prefix_packed_bwd alone at 32 heads x 64, P = 264, 16 groups x 16
                continuations of 30 rows, and ragged 6 .. 30 rows: HIP events around 20 launches after 3 warm-up ones.
  b. pass       forward_scst + backward with GIVEN rollouts (no sampling; the tiny encoder and the reward call are in both arms) in
                the two training_pass modes, same process, alternated `--rounds` times; 16 clips x 16 samples x 30 tokens and
                8 x 16 x 100; peak allocation of each mode.
  c. wide       32 clips x 16 samples x 30 tokens in ONE shared-prefix call beside two per-sequence micro-batches of 16 clips.

Every step runs in a child process of its own under its own time limit, with the shader clock and package power sampled as bench.py
samples them; a step that fails or runs out of time is recorded as such and no further step is started.

    python tools/bench_scst_shared.py [--out profiles/scst_shared_prefix.json] [--rounds 3]

No number is promised and no caption-quality claim is made: there is no trained checkpoint and no data set behind these figures."""
import argparse
import dataclasses
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "tests")]

SAMPLES, REFS = 16, 5
STEPS = {"attention": 240, "pass": 420, "wide": 300}         # child time limits, seconds


def _sampler():
    import bench
    return bench.ClockPowerSampler(0)


def attention_step(args):
    import torch
    from youku_mplug_amd import ops
    dev = torch.device("cuda:0")
    heads, hd, P, G, C = 32, 64, 264, 16, 16
    H = heads * hd
    gen = torch.Generator().manual_seed(2)
    out = []
    for name, lens in (("uniform_30", [30] * (G * C)), ("ragged_6_30", torch.randint(6, 31, (G * C,), generator=gen).tolist())):
        layout = ops.PackedLayout(lens, [C] * G, device=dev)
        R = layout.rows
        qkv = torch.randn(R, 3 * H, generator=gen).to(torch.bfloat16).to(dev)
        pq = torch.randn(G * P, 3 * H, generator=gen).to(torch.bfloat16).to(dev)
        do = torch.randn(R, H, generator=gen).to(torch.bfloat16).to(dev)
        o = torch.empty(R, H, dtype=torch.bfloat16, device=dev)
        dqkv, dpq = torch.empty_like(qkv), torch.zeros_like(pq)
        st = ((3 * H, 3 * hd),) * 3 + ((H, hd),)
        pst = (P * 3 * H, 3 * hd, 3 * H)
        lse = torch.empty(heads, R, dtype=torch.float32, device=dev)
        fwd = lambda: ops.attn_prefix_packed_fwd_lse(qkv, qkv[:, hd:], qkv[:, 2 * hd:], pq[:, hd:], pq[:, 2 * hd:], o, st, (pst, pst), layout,      # noqa: E731
                                                     heads, P, hd, scale=hd ** -0.5, lse=lse)
        plain = lambda: ops.attn_prefix_packed_fwd(qkv, qkv[:, hd:], qkv[:, 2 * hd:], pq[:, hd:], pq[:, 2 * hd:], o, st, (pst, pst), layout,        # noqa: E731
                                                   heads, P, hd, scale=hd ** -0.5)
        bwd = lambda: ops.attn_prefix_packed_bwd(qkv, qkv[:, hd:], qkv[:, 2 * hd:], pq[:, hd:], pq[:, 2 * hd:], o, lse, do, dqkv, dqkv[:, hd:],     # noqa: E731
                                                 dqkv[:, 2 * hd:], dpq[:, hd:], dpq[:, 2 * hd:], st, (pst, pst), layout, heads, P, hd,
                                                 scale=hd ** -0.5)
        row = dict(layout=name, rows=R, groups=G, continuations_per_group=C, prefix_len=P, heads=heads, head_dim=hd)
        for tag, call in (("fwd_us", plain), ("fwd_lse_us", fwd), ("bwd_us", bwd)):
            for _ in range(3):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(20):
                call()
            e1.record()
            torch.cuda.synchronize()
            row[tag] = round(e0.elapsed_time(e1) * 1e3 / 20, 1)
        # useful matrix work of the backward: 5 products of 2 x hd flops per visible (row, key) pair
        pairs = sum(n * P + n * (n + 1) // 2 for n in lens)
        row["bwd_tflops_on_visible_pairs"] = round(5 * 2 * hd * pairs * heads / (row["bwd_us"] * 1e-6) / 1e12, 1)
        print(f"attention {name}: {row}", flush=True)
        out.append(row)
    return out


def _model(dev):
    import torch
    import bench_caption_batched as base
    from oracle.weights import CONFIG_TINY
    from youku_mplug_amd.downstream import synthetic_gencls_model
    shapes = dataclasses.replace(CONFIG_TINY, hidden=base.HIDDEN, layers=base.LAYERS, heads=base.HEADS, ffn=base.FFN, vocab=base.VOCAB,
                                 max_pos=base.MAX_POS, num_queries=base.Q, gpt_ln_eps=base.LN_EPS)
    torch.manual_seed(0)
    return synthetic_gencls_model(shapes, "caption", device=dev).train(), CONFIG_TINY, base


def _problem(dev, cfg, base, clips, length, gen):
    import torch
    from youku_mplug_amd import generation
    video = torch.randn((clips, 3, cfg.num_frames, cfg.img_size, cfg.img_size), generator=gen).to(dev).to(torch.bfloat16)
    ids = torch.randint(8, base.VOCAB, (clips, base.PROMPT + 1), generator=gen).to(dev)
    text = types.SimpleNamespace(input_ids=ids, attention_mask=torch.ones_like(ids))
    refs = [torch.randint(8, 72, (REFS, length), generator=gen).tolist() for _ in range(clips)]
    roll = torch.cat([ids[:, :base.PROMPT].cpu().repeat_interleave(SAMPLES, dim=0),
                      torch.randint(8, 72, (clips * SAMPLES, length), generator=gen)], dim=1).to(dev)      # no terminator: every sample is full length
    return video, text, refs, generation.CiderStats(refs, base.VOCAB), roll


def _one(model, prob, length, mode, term):
    """one forward_scst + backward with the given rollouts -> (seconds between synchronisations, peak allocation in GB)"""
    import torch
    video, text, refs, stats, roll = prob
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    loss, _ = model.forward_scst(video, text, refs, cider=stats, num_samples=SAMPLES, rollouts=roll, max_new_tokens=length, termination_id=term,
                                 training_pass=mode)
    loss.backward()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 2 ** 30


def pass_step(args):
    import torch
    dev = torch.device("cuda:0")
    model, cfg, base = _model(dev)
    gen = torch.Generator().manual_seed(1)
    out = []
    for clips, length in ((16, 30), (8, 100)):
        prob = _problem(dev, cfg, base, clips, length, gen)
        P = base.Q + base.PROMPT - 1
        rows = dict(per_sequence=clips * SAMPLES * (base.Q + base.PROMPT + length), shared_prefix=clips * P + clips * SAMPLES * length)
        for mode in ("per_sequence", "shared_prefix"):          # warm-up, dropped
            _one(model, prob, length, mode, base.STOP)
        rounds = []
        for _ in range(args.rounds):
            r = {}
            for mode in ("per_sequence", "shared_prefix"):
                s, gb = _one(model, prob, length, mode, base.STOP)
                r[mode] = dict(seconds=round(s, 4), peak_gb=round(gb, 1))
            r["time_ratio"] = round(r["per_sequence"]["seconds"] / r["shared_prefix"]["seconds"], 2)
            rounds.append(r)
        med = sorted(r["time_ratio"] for r in rounds)[len(rounds) // 2]
        rec = dict(clips=clips, samples=SAMPLES, caption_tokens=length, decoder_rows=rows, row_ratio=round(rows["per_sequence"] / rows["shared_prefix"], 2),
                   rounds=rounds, time_ratio_median=med, shared_prefix_faster_in_every_round=all(r["time_ratio"] > 1.0 for r in rounds),
                   note="forward_scst + backward with given rollouts: the tiny encoder, the reward call and the references' upload are in both arms")
        print(f"pass {clips} x {SAMPLES} x {length}: {rec}", flush=True)
        out.append(rec)
    return out


def wide_step(args):
    import torch
    dev = torch.device("cuda:0")
    model, cfg, base = _model(dev)
    gen = torch.Generator().manual_seed(1)
    length = 30
    whole = _problem(dev, cfg, base, 32, length, gen)
    video, text, refs, stats, roll = whole
    from youku_mplug_amd import generation
    halves = []
    for a in (0, 16):
        r = refs[a:a + 16]
        halves.append((video[a:a + 16], types.SimpleNamespace(input_ids=text.input_ids[a:a + 16], attention_mask=text.attention_mask[a:a + 16]), r,
                       generation.CiderStats(r, base.VOCAB), roll[a * SAMPLES:(a + 16) * SAMPLES]))
    try:
        _one(model, whole, length, "per_sequence", base.STOP)
        refused = None
    except ValueError as e:
        refused = str(e)[:160]
    _one(model, whole, length, "shared_prefix", base.STOP)
    for h in halves:
        _one(model, h, length, "per_sequence", base.STOP)
    rounds = []
    for _ in range(args.rounds):
        two = [_one(model, h, length, "per_sequence", base.STOP) for h in halves]
        s, gb = _one(model, whole, length, "shared_prefix", base.STOP)
        rounds.append(dict(two_per_sequence_calls_of_16_s=round(sum(t for t, _ in two), 4), per_sequence_peak_gb=round(max(g for _, g in two), 1),
                           one_shared_prefix_call_of_32_s=round(s, 4), shared_prefix_peak_gb=round(gb, 1)))
    rec = dict(clips=32, samples=SAMPLES, caption_tokens=length, per_sequence_call_of_32=("refused: " + refused) if refused else "ran", rounds=rounds,
               note="the two per-sequence calls are two forward + backward passes, not one optimizer step's accumulation: the backward kernels "
                    "overwrite .grad")
    print(f"wide: {rec}", flush=True)
    return rec


def child(args):
    import torch
    import youku_mplug_amd  # noqa: F401
    fn = dict(attention=attention_step, **{"pass": pass_step}, wide=wide_step)[args.step]
    with _sampler() as s:
        res = fn(args)
    with open(args.result, "w") as f:
        json.dump(dict(result=res, clocks=s.summary(), device=torch.cuda.get_device_name(0)), f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scst_shared_prefix.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="(internal) run one step in this process")
    ap.add_argument("--result", default=None, help="(internal) where the step's process leaves its record")
    ap.add_argument("--only", nargs="*", default=None, help="run these steps only")
    args = ap.parse_args()
    if args.step:
        return child(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rec = {"decoder": "bench.py's 1.3B dims, synthetic weights, frozen", "samples_per_clip": SAMPLES, "references_per_clip": REFS,
           "clock": "HIP events (attention), host perf_counter between synchronisations (pass, wide)"}
    for step in (args.only or ["attention", "pass", "wide"]):
        part = os.path.abspath(args.out) + f".{step}.part"
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(args.rounds), "--result", part]
        t0 = time.perf_counter()
        try:
            p = subprocess.run(cmd, timeout=STEPS[step])            # its output goes where this process's goes, as it comes
            rec[step] = json.load(open(part)) if p.returncode == 0 and os.path.isfile(part) else dict(failed=p.returncode)
        except subprocess.TimeoutExpired:
            rec[step] = dict(failed="time limit", limit_s=STEPS[step])
        if os.path.isfile(part):
            os.remove(part)
        rec[step]["wall_s"] = round(time.perf_counter() - t0, 1)
        print(f"{step}: {json.dumps(rec[step])[:600]}", flush=True)
        if "failed" in rec[step]:
            print(f"{step} failed: the remaining steps are not started", flush=True)
            break
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)
    return 1 if any("failed" in v for v in rec.values() if isinstance(v, dict)) else 0


if __name__ == "__main__":
    sys.exit(main())
