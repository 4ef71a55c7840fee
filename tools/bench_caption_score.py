"""Cost of scoring given captions on one GPU, written to profiles/caption_score_cost.json.

(a) The attention alone at 1.3B dims (32 heads x 64): P = 264 prefix rows, 32 groups x 8 candidates, lengths drawn once from a seeded
    uniform 6..40 plus the prompt token: ops.attn_prefix_packed_fwd on the packed rows against ops.attn_prefix_fwd padded to the longest;
    the same at the uniform length 41; both again at head_dim 80 (32 heads x 80); then the category-scoring shape (8 groups x 45
    continuations of 5 rows, the uniform entry only) at both head dims.  HIP events, 3 warm-up + 20 timed launches per kernel, alternated
    launch by launch.
(b) End to end on the 1.3B decoder, the same candidates three ways, alternated --rounds times in one process: every (clip, candidate)
    pair as its own Q + L sequence (forward_lm: what _GenCls._scores does), the padded forward_continuation, and the packed pass
    (forward_continuation_packed); pairs/s and decoder rows of each.  Then the padded and the packed pass again at the uniform length
    41, where both run the same rows: the packed pass may be slower by no more than the larger run-to-run spread of the two.

Without --step this file is only a driver and does not touch the GPU: every measuring step is a child process under its own
`timeout -k 10`, the steps are chained (the first one that fails, faults or runs out of time ends the job, nothing is started behind
it) and their JSON lines are merged into the output file.  Clock and power are sampled as bench.py samples them.

    python tools/bench_caption_score.py [--out profiles/caption_score_cost.json] [--rounds 3]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = {"attention": 240, "end_to_end": 420}
GROUPS, PER_GROUP, LEN_LO, LEN_HI, UNIFORM = 32, 8, 6, 40, 41
CAT_GROUPS, CAT_PER_GROUP, CAT_LEN = 8, 45, 5        # the attention step's category-scoring rows
PAIR_CHUNK = 8            # clips per forward_lm call of the pair-by-pair way (its tape holds every layer of Q + L rows per pair)


def _lengths(uniform):
    import torch
    if uniform:
        return [UNIFORM] * (GROUPS * PER_GROUP)
    g = torch.Generator().manual_seed(0)
    return (torch.randint(LEN_LO, LEN_HI + 1, (GROUPS * PER_GROUP,), generator=g) + 1).tolist()        # + the prompt token


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


def attention_rows(dev, sampler_cls):
    import torch
    from bench_sampling import HEADS, HIDDEN
    from youku_mplug_amd import ops
    P = 264
    out = []
    g = torch.Generator().manual_seed(1)

    def uniform_entry(x, pq, o, n, per_group, Lc, hd):
        H = HEADS * hd
        st3 = (Lc * 3 * H, 3 * hd, 3 * H)
        pst = (P * 3 * H, 3 * hd, 3 * H)
        lay = ops.AttnLayout(st3, st3, st3, (Lc * H, hd, H))
        return lambda: ops.attn_prefix_fwd(x, x[:, hd:], x[:, 2 * hd:], pq[:, hd:], pq[:, 2 * hd:], o, lay, (pst, pst), n, per_group, HEADS, Lc, P, hd,
                                           scale=1.0 / math.sqrt(hd))

    for hd in (HIDDEN // HEADS, 80):                        # 64: the 1.3B decoder; 80: the 2.7B decoder's heads
        H = HEADS * hd
        for uniform in (False, True):
            lens = _lengths(uniform)
            layout = ops.PackedLayout(lens, [PER_GROUP] * GROUPS, device=dev)
            Lc, n = max(lens), len(lens)
            cq = (torch.randn(layout.rows, 3 * H, generator=g) * 1.5).to(torch.bfloat16).to(dev)
            pq = (torch.randn(GROUPS * P, 3 * H, generator=g) * 1.5).to(torch.bfloat16).to(dev)
            pad = torch.zeros((n, Lc, 3 * H), dtype=torch.bfloat16, device=dev)
            at = 0
            for c, ln in enumerate(lens):
                pad[c, :ln] = cq[at:at + ln]
                at += ln
            pad = pad.view(n * Lc, 3 * H)
            o1 = torch.empty((layout.rows, H), dtype=torch.bfloat16, device=dev)
            o2 = torch.empty((n * Lc, H), dtype=torch.bfloat16, device=dev)
            st = ((3 * H, 3 * hd),) * 3 + ((H, hd),)
            pst = (P * 3 * H, 3 * hd, 3 * H)
            sc = 1.0 / math.sqrt(hd)
            fns = {"packed": lambda: ops.attn_prefix_packed_fwd(cq, cq[:, hd:], cq[:, 2 * hd:], pq[:, hd:], pq[:, 2 * hd:], o1, st, (pst, pst), layout,
                                                                HEADS, P, hd, scale=sc),
                   "padded": uniform_entry(pad, pq, o2, n, PER_GROUP, Lc, hd)}
            with sampler_cls(0) as sampler:
                t = _timeit_alternated(fns)
            tel = sampler.summary()
            at, worst = 0, 0.0                                  # the two kernels agree on the real rows
            o2v = o2.view(n, Lc, H)
            for c, ln in enumerate(lens):
                worst = max(worst, (o1[at:at + ln].float() - o2v[c, :ln].float()).abs().max().item())
                at += ln
            row = dict(lengths="uniform 41" if uniform else f"uniform random {LEN_LO}..{LEN_HI} + 1 (seed 0)", prefix_len=P, groups=GROUPS, per_group=PER_GROUP,
                       heads=HEADS, head_dim=hd, packed_rows=layout.rows, padded_rows=n * Lc, rows_ratio=round(n * Lc / layout.rows, 3), packed=t["packed"],
                       padded=t["padded"], padded_over_packed=round(t["padded"]["median_us"] / t["packed"]["median_us"], 3),
                       max_abs_difference_on_real_rows=worst, sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"], clock_power_source=tel["clock_power_source"])
            print(f"attention hd {hd} {row['lengths']}: packed {t['packed']['median_us']} us ({layout.rows} rows), padded {t['padded']['median_us']} us "
                  f"({n * Lc} rows)", file=sys.stderr, flush=True)
            out.append(row)
    # category scoring, the shape the uniform entry was written for: many short continuations per clip (the uniform entry only)
    for hd in (HIDDEN // HEADS, 80):
        H = HEADS * hd
        x = (torch.randn(CAT_GROUPS * CAT_PER_GROUP * CAT_LEN, 3 * H, generator=g) * 1.5).to(torch.bfloat16).to(dev)
        pq = (torch.randn(CAT_GROUPS * P, 3 * H, generator=g) * 1.5).to(torch.bfloat16).to(dev)
        o = torch.empty((x.shape[0], H), dtype=torch.bfloat16, device=dev)
        with sampler_cls(0) as sampler:
            t = _timeit_alternated({"padded": uniform_entry(x, pq, o, CAT_GROUPS * CAT_PER_GROUP, CAT_PER_GROUP, CAT_LEN, hd)})
        tel = sampler.summary()
        row = dict(lengths=f"categories: uniform {CAT_LEN}", prefix_len=P, groups=CAT_GROUPS, per_group=CAT_PER_GROUP, heads=HEADS, head_dim=hd,
                   padded_rows=x.shape[0], padded=t["padded"], sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"], clock_power_source=tel["clock_power_source"])
        print(f"attention hd {hd} {row['lengths']}: padded {t['padded']['median_us']} us ({x.shape[0]} rows)", file=sys.stderr, flush=True)
        out.append(row)
    return out


def end_to_end_rows(dev, sampler_cls, rounds):
    import torch
    from bench_sampling import FFN, HEADS, HIDDEN, LAYERS, LN_EPS, MAX_POS, Q, VOCAB
    from youku_mplug_amd import ops
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    PROMPT = 9                                                # P = Q + PROMPT - 1 = 264
    cfg = GPT3Config(vocab_size=VOCAB, hidden_size=HIDDEN, ffn_hidden_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                     max_position_embeddings=MAX_POS, layernorm_epsilon=LN_EPS, eod_id=7)
    torch.manual_seed(0)
    gpt = DistributedGPT3(config=cfg, device=dev).eval()
    gen = torch.Generator().manual_seed(1)
    qf = (torch.randn(GROUPS, Q, HIDDEN, generator=gen) * 0.5).to(dev).to(torch.bfloat16)
    prompt = torch.randint(8, VOCAB, (GROUPS, PROMPT), generator=gen)
    out = []
    for uniform in (False, True):
        lens = _lengths(uniform)
        n, Lc = len(lens), max(lens)
        toks = [torch.randint(8, VOCAB, (ln,), generator=gen).tolist() for ln in lens]            # ln - 1 caption tokens + the terminator
        rows_in = [[int(prompt[c // PER_GROUP, -1])] + t[:-1] for c, t in enumerate(toks)]
        layout = ops.PackedLayout(lens, [PER_GROUP] * GROUPS, device=dev)
        p_ids = prompt[:, :-1].to(dev).contiguous()
        pk_in = torch.tensor([x for r in rows_in for x in r], dtype=torch.long, device=dev)
        pk_tg = torch.tensor([x for t in toks for x in t], dtype=torch.long, device=dev)
        pad_in = torch.tensor([r + [7] * (Lc - len(r)) for r in rows_in], dtype=torch.long, device=dev)
        loss_rows = torch.tensor([c * Lc + i for c, ln in enumerate(lens) for i in range(ln)], dtype=torch.long, device=dev)
        S = Q + PROMPT - 1 + Lc + 1                           # + the closing token's own row, which forward_lm runs and never scores
        full_ids = torch.cat([prompt[torch.arange(n) // PER_GROUP, :-1].to(dev), pad_in, torch.full((n, 1), 7, dtype=torch.long, device=dev)], dim=1)
        targets = torch.zeros((n, S), dtype=torch.long, device=dev)
        loss_mask = torch.zeros((n, S - 1), dtype=torch.long, device=dev)
        for c, ln in enumerate(lens):
            targets[c, Q + PROMPT - 1:Q + PROMPT - 1 + ln] = torch.tensor(toks[c], device=dev)
            loss_mask[c, Q + PROMPT - 1:Q + PROMPT - 1 + ln] = 1

        def pairs():
            res = []
            for g0 in range(0, GROUPS, PAIR_CHUNK):
                sl = slice(g0 * PER_GROUP, (g0 + PAIR_CHUNK) * PER_GROUP)
                qrep = qf[g0:g0 + PAIR_CHUNK].repeat_interleave(PER_GROUP, dim=0).reshape(-1, HIDDEN)
                o = gpt.forward_lm(qrep, full_ids[sl].contiguous(), targets[sl].contiguous(), loss_mask[sl].contiguous(), {})
                res.append(-(o["losses"] * loss_mask[sl]).sum(-1))
            return torch.cat(res)

        def padded():
            prefix = gpt.forward_prefix(qf.view(-1, HIDDEN), p_ids)
            return -gpt.forward_continuation(prefix, pad_in, PER_GROUP, loss_rows=loss_rows, labels=pk_tg)["losses"]

        def packed():
            prefix = gpt.forward_prefix(qf.view(-1, HIDDEN), p_ids)
            return gpt.forward_continuation_packed(prefix, pk_in, layout, labels=pk_tg)["token_logprob"]
        runs = {"padded": padded, "packed": packed} if uniform else {"pairs": pairs, "padded": padded, "packed": packed}
        rows = {"pairs": n * S, "padded": GROUPS * (Q + PROMPT - 1) + n * Lc, "packed": GROUPS * (Q + PROMPT - 1) + layout.rows}
        times = {k: [] for k in runs}
        with torch.no_grad(), sampler_cls(0) as sampler:
            first = {k: fn() for k, fn in runs.items()}
            torch.cuda.synchronize()
            for _ in range(rounds):
                for k, fn in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[k].append(time.perf_counter() - t0)
        tel = sampler.summary()
        seg = torch.tensor(layout.seg_start_host, device=dev)
        seq = torch.zeros(n, dtype=torch.float32, device=dev).index_add_(0, torch.unique_consecutive(seg, return_inverse=True)[1], first["packed"])
        agree = {"packed_vs_padded_max_abs_token": (first["packed"] - first["padded"]).abs().max().item()}
        if "pairs" in first:
            agree["packed_vs_pairs_max_abs_sequence"] = (seq - first["pairs"]).abs().max().item()
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        row = dict(lengths="uniform 41" if uniform else f"uniform random {LEN_LO}..{LEN_HI} + 1 (seed 0)", pairs=n, prefix_rows_per_clip=Q + PROMPT - 1,
                   decoder_rows={k: rows[k] for k in runs}, seconds={k: [round(x, 4) for x in v] for k, v in times.items()},
                   median_s={k: round(v, 4) for k, v in med.items()}, spread_s={k: round(v, 4) for k, v in spread.items()},
                   pairs_per_s={k: round(n / v, 1) for k, v in med.items()}, padded_over_packed_time=round(med["padded"] / med["packed"], 3),
                   padded_over_packed_continuation_rows=round(n * Lc / layout.rows, 3), agreement=agree,
                   sclk_mhz=tel["sclk_mhz"], power_w=tel["power_w"], clock_power_source=tel["clock_power_source"])
        if uniform:
            margin = max(spread["padded"], spread["packed"])
            row.update(margin_s=round(margin, 4), packed_not_slower=bool(med["packed"] - med["padded"] <= margin))
        print(f"end to end {row['lengths']}: " + ", ".join(f"{k} {med[k]:.4f} s ({rows[k]} rows)" for k in runs), file=sys.stderr, flush=True)
        out.append(row)
    return out


def run_step(step, rounds):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    dev = torch.device("cuda:0")
    _lib.check(_lib.lib().mpv_check_device(), "mpv_check_device")
    res = {"attention": lambda: attention_rows(dev, bench.ClockPowerSampler),
           "end_to_end": lambda: end_to_end_rows(dev, bench.ClockPowerSampler, rounds)}[step]()
    print("RESULT " + json.dumps({"device": torch.cuda.get_device_name(0), "result": res}), flush=True)


def _child(step, rounds):
    """one measuring step as a child process under its own time limit -> its result, or None (then the job ends)"""
    cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(rounds)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
    if p.returncode != 0 or line is None:
        print(f"step {step} ended with status {p.returncode}: nothing more is started", file=sys.stderr, flush=True)
        return None
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caption_score_cost.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None, help="(internal) run one measuring step in this process")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a.rounds)
    res = {"protocol": "one child process per step, each under its own timeout; attention: HIP events, 3 warm-up + 20 timed launches per kernel, "
           f"alternated launch by launch, median / min / max; end to end: wall clock, {a.rounds} alternated rounds in one process, median and max - min",
           "not_run": []}
    ok = True
    for step in ("attention", "end_to_end"):
        r = _child(step, a.rounds) if ok else None
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
