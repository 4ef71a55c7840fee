"""Query-max search on one GPU at the recipe's dims (E = 256, Q = 256): ops.maxsim_topk (k = 10) and ops.maxsim_rank beside the
existing way to the same answer -- mpv_maxsim_fwd into the [queries, gallery] matrix, then torch.topk -- for 1 k and 10 k clips x
1 k titles, both directions.  The two are ALTERNATED on one box (three alternations, HIP events, median of the rounds), in the
manner of tools/bench_retrieval_search.py.  Beside each measurement the floor: 2 nq ng Q E FLOPs at the bf16 MFMA peak, or the
gallery bytes once from HBM, whichever is larger.  Result: profiles/maxsim_search_cost.json."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import youku_mplug_amd  # noqa: E402,F401
from youku_mplug_amd import ops  # noqa: E402

MFMA_BF16_FLOPS = 2.5e15      # MI355X dense bf16 peak
HBM_BYTES_PER_S = 8.0e12


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def _unit(n, group, dim, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((n * group, dim), generator=g)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16).to(dev).view(n, group, dim)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--titles", type=int, default=1000)
    ap.add_argument("--Q", type=int, default=256)
    ap.add_argument("--E", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maxsim_search_cost.json"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    Q, E, K = a.Q, a.E, a.k
    rows = []
    for nc in a.clips:
        clips, titles = _unit(nc, Q, E, 1, dev), _unit(a.titles, 1, E, 2, dev)[:, 0]
        flat = clips.view(nc * Q, E)
        for direction in ("title->clip", "clip->title"):
            t2c = direction == "title->clip"
            q, g = (titles, clips) if t2c else (clips, titles)
            nq, ng = q.shape[0], g.shape[0]
            tgt = (torch.arange(nq, device=dev) % ng).view(nq, 1)

            def existing():
                m, _ = ops.maxsim_fwd(flat, titles, nc, Q, a.titles, E, trans=t2c)       # [nq, ng] either way
                return torch.topk(m, K, dim=1)
            fused = lambda: ops.maxsim_topk(q, g, K)
            fv, fi = fused()
            ev, ei = existing()
            agree = float((fi == ei).float().mean())
            t_f, t_e, t_r = [], [], []
            for _ in range(a.rounds):
                t_f.append(_time(fused, a.iters))
                t_e.append(_time(existing, a.iters))
                t_r.append(_time(lambda: ops.maxsim_rank(q, g, tgt), a.iters))
            tf_, te_, tr_ = (statistics.median(t) for t in (t_f, t_e, t_r))
            flops = 2.0 * nq * ng * Q * E
            gbytes = ng * (Q if t2c else 1) * E * 2
            floor = max(flops / MFMA_BF16_FLOPS, gbytes / HBM_BYTES_PER_S)
            row = dict(direction=direction, nq=nq, ng=ng, Q=Q, E=E, k=K, maxsim_topk_us=tf_ * 1e6, maxsim_rank_us=tr_ * 1e6,
                       maxsim_fwd_plus_torch_topk_us=te_ * 1e6, ratio_existing_over_fused=te_ / tf_, floor_us=floor * 1e6,
                       floor_is="mfma" if flops / MFMA_BF16_FLOPS >= gbytes / HBM_BYTES_PER_S else "gallery bytes",
                       matrix_bytes_not_written=nq * ng * 8, top_index_agreement=agree,
                       maxsim_topk_us_rounds=[t * 1e6 for t in t_f], existing_us_rounds=[t * 1e6 for t in t_e])
            rows.append(row)
            print(f"{direction} nq {nq:6d} ng {ng:6d}: maxsim_topk {tf_ * 1e6:10.1f} us  maxsim_rank {tr_ * 1e6:10.1f} us  "
                  f"maxsim_fwd + torch.topk {te_ * 1e6:10.1f} us  (x{te_ / tf_:.2f})  floor {floor * 1e6:8.1f} us ({row['floor_is']})",
                  flush=True)
    out = dict(device=torch.cuda.get_device_name(0), mfma_bf16_flops=MFMA_BF16_FLOPS, hbm_bytes_per_s=HBM_BYTES_PER_S, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
