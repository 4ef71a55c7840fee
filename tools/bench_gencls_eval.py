"""Evaluation throughput of the ITM / category scoring heads at 1.3B dims on one GPU: (video, candidate) pairs per second of the
existing path (forward(..., train=False) = _GenCls._scores: every pair a full Q + max_length decoder sequence, the ViT and the
abstractor rerun per call) beside the shared-prefix path (encode_video once per video batch, then score_shared_prefix per call).
Random weights; 128 query tokens, max_length 80.

    python tools/bench_gencls_eval.py [--videos 4] [--iters 3] [--frames 8]

ITM geometry: titles of 20-40 tokens behind a 10-token shared question prefix, 8 and 64 titles per call (the reference evaluation
loop's chunk is 8).  Category geometry: 45 class names of 2-6 tokens behind a 12-token shared prompt.  Prints one table and one
JSON line."""
import argparse
import dataclasses
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _texts(vocab, n, L, shared, lo, hi, plen, g):
    ids = torch.randint(5, vocab, (n, L), generator=g)
    ids[:, :shared] = ids[0, :shared]
    mask = torch.zeros(n, L, dtype=torch.long)
    lens = torch.randint(shared + lo, shared + hi + 1, (n,), generator=g).clamp(max=L)
    for i in range(n):
        mask[i, :lens[i]] = 1
    return ids, mask, torch.full((n,), plen, dtype=torch.long)


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    args = ap.parse_args()
    from oracle.weights import CONFIG_B
    from youku_mplug_amd.downstream import synthetic_gencls_model
    dev = torch.device("cuda:0")
    cfg = dataclasses.replace(CONFIG_B, num_queries=128, num_frames=args.frames)
    g = torch.Generator().manual_seed(0)
    Bv, L = args.videos, 80
    video = torch.randn(Bv, 3, cfg.num_frames, cfg.img_size, cfg.img_size, generator=g).to(dev, torch.bfloat16)
    rows, res = [], {}
    for kind, t, shared, lo, hi, pshared in (("itm", 8, 10, 20, 40, 10), ("itm", 64, 10, 20, 40, 10), ("cls", 45, 12, 2, 6, 12)):
        torch.manual_seed(1)
        model = synthetic_gencls_model(cfg, kind, num_classes=2 if kind == "itm" else 45, device=dev).eval()
        ids, mask, plen = _texts(cfg.vocab, Bv * t, L, shared, lo, hi, shared, g)
        text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev), prompt_lengths=plen)
        np_ = Bv * t if kind == "itm" else Bv
        p_ids, p_mask, _ = _texts(cfg.vocab, np_, L, pshared, lo, hi, 0, g)
        ptext = types.SimpleNamespace(input_ids=p_ids.to(dev), attention_mask=p_mask.to(dev))
        with torch.no_grad():
            t_old = _time(lambda: model(video, text, ptext, train=False), args.iters)
            qf = model.encode_video(video)
            t_enc = _time(lambda: model.encode_video(video), args.iters)
            t_new = _time(lambda: model.score_shared_prefix(text, ptext, query_features=qf), args.iters)
        pairs = Bv * t
        name = f"{kind}_{t}"
        res[name] = dict(pairs=pairs, old_pairs_per_s=pairs / t_old, new_pairs_per_s=pairs / t_new, encode_ms=t_enc * 1e3,
                         old_ms=t_old * 1e3, new_ms=t_new * 1e3, speedup=t_old / t_new)
        rows.append(f"{name:>8} {pairs:6d} {t_old * 1e3:10.1f} {t_new * 1e3:10.1f} {t_enc * 1e3:10.1f} {pairs / t_old:11.1f} "
                    f"{pairs / t_new:11.1f} {t_old / t_new:7.2f}x")
        del model
        torch.cuda.empty_cache()
    print(f"{'geometry':>8} {'pairs':>6} {'_scores ms':>10} {'shared ms':>10} {'encode ms':>10} {'old pairs/s':>11} {'new pairs/s':>11} "
          f"{'speedup':>8}")
    print("\n".join(rows))
    print("(shared ms excludes encode_video, which runs once per video batch and is shown beside it)")
    print(json.dumps(dict(videos=Bv, frames=cfg.num_frames, queries=cfg.num_queries, max_length=L, results=res)))


if __name__ == "__main__":
    main()
