"""Cost of temporal attention on long clips: the forward and the backward launch at ViT-B/16 dims (196 patches per frame, 8 heads
of 96) at a constant B * T = 256 frames -- 16 frames on the existing kernels through the existing entry points, 32 and 64 frames
on the matrix-core kernels (csrc/attention_temporal_long.inc) -- HIP events, the warm-up / repeat protocol of
tools/bench_kernels.py (3 + 20), achieved bytes/s against the algorithmic bytes (forward 4 * rows * D * 2 B: q, k, v in, o out;
backward 7 * rows * D * 2 B: q, k, v, dO in, dq, dk, dv out), shader clock and package power sampled as bench.py samples them.
--step adds the eager pre-train step of synthetic_model at 1.3B dims with 8 clips x 32 frames (the ViT rows of config B) and
temporal attention's share of it (12 blocks x (forward + backward) of the 32-frame row above).  One JSON object on stdout and in --out.

    python tools/bench_temporal_long.py [--step] [--steps 10] [--warmup 3] [--out profiles/temporal_long_cost.json]"""
import argparse
import dataclasses
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

N, HEADS, HD, FRAMES = 196, 8, 96, 256


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
    return s.elapsed_time(e) / iters * 1e-3


def kernel_rows(dev, sampler_cls):
    from youku_mplug_amd import ops
    N1, D = N + 1, HEADS * HD
    out = []
    for T in (16, 32, 64):
        B = FRAMES // T
        R = B * T * N1
        qkv = (torch.randn(R, 3 * D, device=dev) * 0.5).bfloat16()
        dout = (torch.randn(R, D, device=dev) * 0.5).bfloat16()
        o, dqkv = torch.empty(R, D, dtype=torch.bfloat16, device=dev), torch.empty_like(qkv)
        args = (B, T * N1, N, 1, N1, T, HEADS, HD, HD ** -0.5)
        plan = ops.temporal_attn_long_plan(B, N, T, HEADS, HD)["variant"] if T > ops.TEMPORAL_SHORT_MAX_T else "mpv_temporal_attn_fwd / _bwd"
        with sampler_cls(0) as sampler:
            tf = timeit(lambda: ops.temporal_attn_fwd(qkv, o, *args))
            tb = timeit(lambda: ops.temporal_attn_bwd(qkv, dout, dqkv, *args))
        tel = sampler.summary()
        by = B * T * N * D * 2                                          # one [token rows, D] bf16 operand
        row = dict(T=T, B=B, problems=B * N * HEADS, kernel=plan, fwd_us=round(tf * 1e6, 1), bwd_us=round(tb * 1e6, 1),
                   fwd_gbps=round(4 * by / tf / 1e9), bwd_gbps=round(7 * by / tb / 1e9), sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"],
                   clock_power_source=tel["clock_power_source"])
        print(f"T={T:2d} B={B:2d}  fwd {row['fwd_us']:8.1f} us ({row['fwd_gbps']:5d} GB/s)  bwd {row['bwd_us']:8.1f} us ({row['bwd_gbps']:5d} GB/s)  "
              f"{tel['sclk_mhz']} MHz {tel['power_w']} W  [{plan}]", file=sys.stderr, flush=True)
        out.append(row)
        del qkv, dout, o, dqkv
    return out


def step_row(dev, sampler_cls, steps, warmup, k32):
    from oracle.weights import CONFIG_B
    from youku_mplug_amd import engine as eng
    from youku_mplug_amd.pretrain import synthetic_model
    torch.manual_seed(1234)
    cfg = dataclasses.replace(CONFIG_B, num_frames=32)
    model = synthetic_model(cfg, device=dev)
    with torch.no_grad():                                               # as bench.py: the module default zeroes the temporal branch
        for blk in model.visual_encoder.blocks:
            blk.temporal_fc.weight.normal_(0, 0.015)
        model.visual_encoder.temporal_embed.normal_(0, 0.015)
    model.train()
    groups = eng.get_parameter_groups(model, 0.05, model.no_weight_decay(), visual_backbone_scale=True)
    engine, _, _, _ = eng.initialize(model=model, model_parameters=groups, config=dict(lr=1e-4, opt_betas=(0.9, 0.999), opt_eps=1e-6, clip_grad=3.0))
    B, T, L = FRAMES // 32, 32, 32
    video = torch.randn(B, 3, T, cfg.img_size, cfg.img_size, device=dev).to(torch.bfloat16)
    ids = torch.randint(0, cfg.vocab, (B, L), device=dev)
    mask = torch.ones(B, L, dtype=torch.long, device=dev)
    mask[:, L - L // 4:] = 0
    text = types.SimpleNamespace(input_ids=ids, attention_mask=mask)

    def step():
        loss, _ = engine(video, text)
        engine.backward(loss)
        engine.step()
        return loss

    for _ in range(warmup):
        loss = step()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    with sampler_cls(0) as sampler:
        marks[0].record()
        for i in range(steps):
            loss = step()
            marks[i + 1].record()
        torch.cuda.synchronize()
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    ms = per[len(per) // 2]
    tel = sampler.summary()
    temporal_ms = cfg.vit_depth * (k32["fwd_us"] + k32["bwd_us"]) * 1e-3
    assert torch.isfinite(loss).item()
    return dict(workload=f"pre-train step, eager, 1.3B dims, B={B} T={T} L={L} (last quarter padding), 1 GPU", steps=steps, ms_per_step=round(ms, 2),
                temporal_attn_ms=round(temporal_ms, 3), temporal_attn_share=round(temporal_ms / ms, 4), loss_last=loss.item(),
                peak_alloc_gib=round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 1), sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"],
                clock_power_source=tel["clock_power_source"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_long_cost.json"))
    a = ap.parse_args()
    import bench
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    dev = torch.device("cuda:0")
    _lib.check(_lib.lib().mpv_check_device(), "mpv_check_device")
    res = {"dims": dict(n_inner=N, heads=HEADS, head_dim=HD, frames=FRAMES), "protocol": "HIP events, 3 warm-up + 20 timed launches per figure",
           "algorithmic_bytes": "forward 4 * rows * D * 2, backward 7 * rows * D * 2 (rows = B * T * 196 token rows, D = 768)",
           "kernels": kernel_rows(dev, bench.ClockPowerSampler)}
    if a.step:
        res["step"] = step_row(dev, bench.ClockPowerSampler, a.steps, a.warmup, next(r for r in res["kernels"] if r["T"] == 32))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
