"""Cost of use_contrastive on the pre-train step: config B (1.3B dims, B = 32, 8 frames x 224^2, 32-token titles, bf16), eager
steps on one GPU, the contrastive head off and on ALTERNATED three times in one process (one model: the head's parameters exist in
both arms, `use_contrastive` is switched), 50 timed steps per arm after warm-up, HIP events, shader clock and package power sampled
as bench.py samples them.  One JSON object on stdout (and in --out when given).

    python tools/bench_contrastive.py [--steps 50] [--warmup 5] [--rounds 3] [--out profiles/contrastive_cost.json]"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    import youku_mplug_amd  # noqa: F401
    from oracle.weights import CONFIG_B
    from youku_mplug_amd import _lib, engine as eng
    from youku_mplug_amd.pretrain import synthetic_model
    dev = torch.device("cuda:0")
    _lib.check(_lib.lib().mpv_check_device(), "mpv_check_device")
    torch.manual_seed(1234)
    cfg = CONFIG_B
    model = synthetic_model(cfg, device=dev, use_contrastive=True)
    with torch.no_grad():                                            # as bench.py: the module default zeroes the temporal branch
        for blk in model.visual_encoder.blocks:
            blk.temporal_fc.weight.normal_(0, 0.015)
        model.visual_encoder.temporal_embed.normal_(0, 0.015)
    model.train()
    groups = eng.get_parameter_groups(model, 0.05, model.no_weight_decay(), visual_backbone_scale=True)
    engine, _, _, _ = eng.initialize(model=model, model_parameters=groups,
                                     config=dict(lr=1e-4, opt_betas=(0.9, 0.999), opt_eps=1e-6, clip_grad=3.0))
    B, T, L = 32, cfg.num_frames, 32
    video = torch.randn(B, 3, T, cfg.img_size, cfg.img_size, device=dev).to(torch.bfloat16)
    ids = torch.randint(0, cfg.vocab, (B, L), device=dev)
    mask = torch.ones(B, L, dtype=torch.long, device=dev)
    mask[:, L - L // 4:] = 0
    text = types.SimpleNamespace(input_ids=ids, attention_mask=mask)

    def step():
        lc, li = engine(video, text)
        engine.backward(lc + li)
        engine.step()
        return li

    arms = {"off": [], "on": []}
    telemetry = {"off": [], "on": []}
    last_ita = None
    for _ in range(args.rounds):
        for arm in ("off", "on"):
            model.use_contrastive = arm == "on"
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
            sampler = bench.ClockPowerSampler(0)
            with sampler:
                marks[0].record()
                for i in range(args.steps):
                    li = step()
                    marks[i + 1].record()
                torch.cuda.synchronize()
            per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
            arms[arm].append(per[len(per) // 2])
            telemetry[arm].append(sampler.summary())
            if arm == "on":
                last_ita = li.item()
    res = {"workload": "config B pre-train step, eager, B=32 T=8 L=32 (last quarter padding), 1 GPU",
           "steps_per_arm": args.steps, "rounds": args.rounds,
           "ms_per_step_off": arms["off"], "ms_per_step_on": arms["on"],
           "median_ms_off": sorted(arms["off"])[len(arms["off"]) // 2], "median_ms_on": sorted(arms["on"])[len(arms["on"]) // 2],
           "sclk_mhz_off": [t["sclk_mhz"] for t in telemetry["off"]], "sclk_mhz_on": [t["sclk_mhz"] for t in telemetry["on"]],
           "power_w_off": [t["power_w"] for t in telemetry["off"]], "power_w_on": [t["power_w"] for t in telemetry["on"]],
           "clock_power_source": telemetry["on"][0]["clock_power_source"], "loss_ita_last": last_ita}
    res["added_ms"] = round(res["median_ms_on"] - res["median_ms_off"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
