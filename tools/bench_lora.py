"""Cost of the decoder LoRA adapters.  One JSON object on stdout (and in --out when given):

  kernels   the six launches of a layer (forward: down, up_add; backward: wgrad dB, down dt, wgrad dA, up_add dx1) at the 1.3B
            (H = 2048) and 2.7B (H = 2560) shapes, R = 9216 rows (config B: 32 x (256 + 32)), rank --rank: median microseconds over
            --kernel_iters launches (HIP events) beside the byte floor -- the bytes a launch has to move (the long operand once; y read
            and written) -- and the bandwidth that time amounts to.
  step      the pre-train step (synthetic model, config B geometry, eager, 1 GPU) in three modes -- decoder frozen, frozen with
            adapters of rank --rank, and freeze_text_decoder: false -- ALTERNATED --rounds times in one process: median ms per step
            per round, shader clock and package power per round as bench.py samples them, and the peak allocation of each mode
            (above what was resident when its timed steps began, and the resident bytes its model + optimizer state added).

    python tools/bench_lora.py [--steps 20] [--warmup 3] [--rounds 3] [--rank 16] [--out profiles/lora.json]"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

BF = torch.bfloat16


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    marks[0].record()
    for i in range(iters):
        fn()
        marks[i + 1].record()
    torch.cuda.synchronize()
    per = sorted(marks[i].elapsed_time(marks[i + 1]) * 1e3 for i in range(iters))
    return per[len(per) // 2]


def bench_kernels(dev, rank, iters):
    from youku_mplug_amd import ops
    out = []
    R = 9216
    for name, H in (("1.3B", 2048), ("2.7B", 2560)):
        x1 = torch.randn((R, H), device=dev).to(BF)
        qkv = torch.randn((R, 3 * H), device=dev).to(BF)
        dx1 = torch.randn((R, H), device=dev).to(BF)
        A = (torch.randn((rank, H), device=dev) * 0.02).to(BF)
        Bm = (torch.randn((3 * H, rank), device=dev) * 0.02).to(BF)
        t = ops.lora_down(x1, A, R, H, rank, w_rank_major=True)
        dt = ops.lora_down(qkv, Bm, R, 3 * H, rank, w_rank_major=False)
        gA, gB = torch.empty_like(A), torch.empty_like(Bm)
        small = 2 * R * rank
        launches = [
            ("fwd down t = x1 A^T", lambda: ops.lora_down(x1, A, R, H, rank, w_rank_major=True, out=t), 2 * R * H + small),
            ("fwd up_add qkv += s t B^T", lambda: ops.lora_up_add(t, Bm, qkv, R, 3 * H, rank, w_rank_major=False, scale=1e-3), 4 * R * 3 * H + small),
            ("bwd wgrad dB = s t^T dqkv", lambda: ops.lora_wgrad(t, qkv, R, 3 * H, rank, g_rank_major=False, out=gB), 2 * R * 3 * H + small),
            ("bwd down dt = s dqkv B", lambda: ops.lora_down(qkv, Bm, R, 3 * H, rank, w_rank_major=False, out=dt), 2 * R * 3 * H + small),
            ("bwd wgrad dA = dt^T x1", lambda: ops.lora_wgrad(dt, x1, R, H, rank, g_rank_major=True, out=gA), 2 * R * H + small),
            ("bwd up_add dx1 += dt A", lambda: ops.lora_up_add(dt, A, dx1, R, H, rank, w_rank_major=True, scale=1e-3), 4 * R * H + small),
        ]
        total_us, total_bytes = 0.0, 0
        for what, fn, nbytes in launches:
            us = _time(fn, iters)
            total_us += us
            total_bytes += nbytes
            out.append(dict(model=name, R=R, H=H, rank=rank, launch=what, us=round(us, 2), floor_bytes=nbytes,
                            gb_per_s=round(nbytes / us / 1e3, 1)))
        out.append(dict(model=name, R=R, H=H, rank=rank, launch="layer total (six launches)", us=round(total_us, 2), floor_bytes=total_bytes,
                        gb_per_s=round(total_bytes / total_us / 1e3, 1)))
    return out


def build(cfg, dev, config):
    from youku_mplug_amd import engine as eng
    from youku_mplug_amd.gpt3 import GPT3Config
    from youku_mplug_amd.pretrain import DistributedGPT3_Pretrain
    vis = dict(img_size=cfg.img_size, patch_size=cfg.patch_size, depth=cfg.vit_depth, num_frames=cfg.num_frames, embed_dim=cfg.vit_dim,
               num_heads=cfg.vit_heads, mlp_ratio=cfg.vit_mlp_ratio, clip_model=True)
    txt = GPT3Config(vocab_size=cfg.vocab, hidden_size=cfg.hidden, ffn_hidden_size=cfg.ffn, num_hidden_layers=cfg.layers,
                     num_attention_heads=cfg.heads, max_position_embeddings=cfg.max_pos, layernorm_epsilon=cfg.gpt_ln_eps)
    before = torch.cuda.memory_allocated()
    model = DistributedGPT3_Pretrain({"num_learnable_token": cfg.num_queries, "_synthetic": True, **config}, visual_cfg=vis, text_cfg=txt, device=dev)
    with torch.no_grad():                                            # as bench.py: the module default zeroes the temporal branch
        for blk in model.visual_encoder.blocks:
            blk.temporal_fc.weight.normal_(0, 0.015)
        model.visual_encoder.temporal_embed.normal_(0, 0.015)
        if model.text_decoder.has_lora():                            # non-zero B: the arithmetic of a run in progress
            for lin in model.text_decoder._qkv_linears():
                lin.lora_B.normal_(0, 0.01)
    model.train()
    groups = eng.get_parameter_groups(model, 0.05, model.no_weight_decay(), visual_backbone_scale=True)
    engine, _, _, _ = eng.initialize(model=model, model_parameters=groups, config=dict(lr=1e-4, opt_betas=(0.9, 0.999), opt_eps=1e-6, clip_grad=3.0))
    trainable = sum(p.numel() for p in model.parameters() if p.requires_grad)
    return engine, trainable, torch.cuda.memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--kernel_iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    import youku_mplug_amd  # noqa: F401
    from oracle.weights import CONFIG_B
    from youku_mplug_amd import _lib
    dev = torch.device("cuda:0")
    _lib.check(_lib.lib().mpv_check_device(), "mpv_check_device")
    torch.manual_seed(1234)
    res = {"kernels": bench_kernels(dev, args.rank, args.kernel_iters)}
    cfg = CONFIG_B
    modes = {"frozen": {}, "lora": {"lora_rank": args.rank}, "trainable": {"freeze_text_decoder": False}}
    engines, info = {}, {}
    for name, config in modes.items():
        engines[name], n, resident = build(cfg, dev, config)
        info[name] = dict(trainable_parameters=n, resident_bytes=resident)
    B, T, L = 32, cfg.num_frames, 32
    video = torch.randn(B, 3, T, cfg.img_size, cfg.img_size, device=dev).to(BF)
    ids = torch.randint(0, cfg.vocab, (B, L), device=dev)
    mask = torch.ones(B, L, dtype=torch.long, device=dev)
    mask[:, L - L // 4:] = 0
    text = types.SimpleNamespace(input_ids=ids, attention_mask=mask)

    def step(engine):
        loss, _ = engine(video, text)
        engine.backward(loss)
        engine.step()

    ms = {m: [] for m in modes}
    tel = {m: [] for m in modes}
    peak = {m: 0 for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            for _ in range(args.warmup):
                step(engines[m])
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
            sampler = bench.ClockPowerSampler(0)
            with sampler:
                marks[0].record()
                for i in range(args.steps):
                    step(engines[m])
                    marks[i + 1].record()
                torch.cuda.synchronize()
            per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
            ms[m].append(round(per[len(per) // 2], 3))
            tel[m].append(sampler.summary())
            peak[m] = max(peak[m], torch.cuda.max_memory_allocated() - base)
    med = lambda v: sorted(v)[len(v) // 2]
    res["step"] = {"workload": "config B pre-train step, eager, B=32 T=8 L=32 (last quarter padding), 1 GPU", "rank": args.rank,
                   "steps_per_arm": args.steps, "rounds": args.rounds,
                   "modes": {m: dict(ms_per_step=ms[m], median_ms=med(ms[m]), sclk_mhz=[t["sclk_mhz"] for t in tel[m]],
                                     power_w=[t["power_w"] for t in tel[m]], peak_step_bytes=peak[m], **info[m]) for m in modes},
                   "clock_power_source": tel["frozen"][0]["clock_power_source"]}
    res["step"]["lora_added_ms"] = round(med(ms["lora"]) - med(ms["frozen"]), 3)
    res["step"]["trainable_added_ms"] = round(med(ms["trainable"]) - med(ms["frozen"]), 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
