"""What a per-row prior costs the fused searches, and what the bank pass of the inverted-softmax correction takes, on one GPU.

  (a) ops.sim_topk / sim_rank (and the _q8 forms) beside their *_prior twins at D = 256, k = 10 and the shapes of the existing search
      tables: 1 x 1e6, 64 x 1e6, 4096 x 1e5.  The plain and the prior entry alternate in one process, three rounds, timed with device
      events; reported: the median of each, the ratio of the medians, and the spread of the rounds ((max - min) / median) of both --
      a ratio inside that spread is no cost that this tool can see.  From bytes alone a prior adds 4 to a 512-byte row (0.8 %), or 4
      to 260 for codes (1.5 %).
  (b) ops.sim_bank_lse for nb in {1000, 10000} x ng in {1e5, 1e6} beside its two floors computed from the shapes -- the bytes (gallery
      and bank read once, lse written) at the measured HBM rate, the products at the bf16 MFMA peak -- and beside chunked torch fp32
      logsumexp(beta * bank @ g.T, 0).
  (c) RetrievalIndex.add of 32 rows into a fitted index (the bank pass over the 32 new rows) beside the same add into a plain index.

    python tools/bench_search_prior.py [--out profiles/search_prior.json] [--rounds 3] [--iters 5]

Prints one table and writes one JSON file.  No time is fixed in advance anywhere in here."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12          # measured streaming read rate of one MI355X (tools/bench_retrieval_search.py)
MFMA_BF16_FLOPS = 2.5e15          # dense bf16 MFMA peak of one MI355X
D, K, BETA = 256, 10, 20.0
SIM_SHAPES = [(1, 1000000), (64, 1000000), (4096, 100000)]
BANK_SHAPES = [(1000, 100000), (1000, 1000000), (10000, 100000), (10000, 1000000)]


def _time(fn, iters):
    """seconds per call, between two device events around `iters` calls (after one warm-up call)"""
    fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3 / iters


def _median(ts):
    return sorted(ts)[len(ts) // 2]


def _spread(ts):
    return (max(ts) - min(ts)) / _median(ts)


def _feats(n, seed, dev, chunk=1 << 20):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((n, D), dtype=torch.bfloat16, device=dev)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        out[lo:lo + m] = torch.nn.functional.normalize(torch.randn(m, D, generator=g, device=dev), dim=1).to(torch.bfloat16)
    return out


def _alternate(a, b, rounds, iters):
    ta, tb = [], []
    for _ in range(rounds):                                          # alternate: both sides see the same clocks and neighbours
        ta.append(_time(a, iters))
        tb.append(_time(b, iters))
    return ta, tb


def measure_prior(rounds, iters, dev):
    from youku_mplug_amd import ops
    rows = []
    for nq, ng in SIM_SHAPES:
        q, g = _feats(nq, 0, dev), _feats(ng, 1, dev)
        codes, scale = ops.quantize_rows_e4m3(g)
        gen = torch.Generator(device=dev).manual_seed(2)
        prior = 0.05 * torch.randn(ng, generator=gen, device=dev)
        prior[torch.rand(ng, generator=gen, device=dev) < 0.1] = float("-inf")
        tgt = torch.randint(0, ng, (nq, 1), device=dev)
        cases = (("sim_topk", "bf16", lambda: ops.sim_topk(q, g, K), lambda: ops.sim_topk_prior(q, g, prior, K)),
                 ("sim_rank", "bf16", lambda: ops.sim_rank(q, g, tgt), lambda: ops.sim_rank_prior(q, g, prior, tgt)),
                 ("sim_topk", "fp8", lambda: ops.sim_topk_q8(q, codes, scale, K), lambda: ops.sim_topk_prior_q8(q, codes, scale, prior, K)),
                 ("sim_rank", "fp8", lambda: ops.sim_rank_q8(q, codes, scale, tgt), lambda: ops.sim_rank_prior_q8(q, codes, scale, prior, tgt)))
        for entry, storage, plain, with_prior in cases:
            tp, tw = _alternate(plain, with_prior, rounds, iters)
            row_bytes = D * 2 if storage == "bf16" else D + 4
            r = dict(entry=entry, storage=storage, nq=nq, ng=ng, dim=D, plain_us=_median(tp) * 1e6, prior_us=_median(tw) * 1e6,
                     prior_over_plain=_median(tw) / _median(tp), plain_spread=_spread(tp), prior_spread=_spread(tw),
                     plain_us_rounds=[t * 1e6 for t in tp], prior_us_rounds=[t * 1e6 for t in tw],
                     bytes_ratio=(row_bytes + 4) / row_bytes, floor_stream_us=ng * (row_bytes + 4) / HBM_BYTES_PER_S * 1e6)
            rows.append(r)
            print(f"{entry:9s} {storage:4s} nq {nq:5d} ng {ng:8d}: plain {r['plain_us']:9.1f} us  prior {r['prior_us']:9.1f} us  "
                  f"prior/plain {r['prior_over_plain']:5.3f}  spread {r['plain_spread']:.3f} / {r['prior_spread']:.3f}  "
                  f"bytes {r['bytes_ratio']:.3f}", flush=True)
        del q, g, codes, scale, prior
    return rows


def _torch_lse(bank, g, beta, chunk=1 << 14):
    """chunked over the gallery so that the [nb, chunk] fp32 matrix stays small"""
    bf = bank.float()
    out = torch.empty(g.shape[0], dtype=torch.float32, device=g.device)
    for lo in range(0, g.shape[0], chunk):
        out[lo:lo + chunk] = torch.logsumexp(beta * (bf @ g[lo:lo + chunk].float().t()), dim=0)
    return out


def measure_bank(rounds, iters, dev):
    from youku_mplug_amd import ops
    rows = []
    for nb, ng in BANK_SHAPES:
        bank, g = _feats(nb, 3, dev), _feats(ng, 4, dev)
        tk, tt = _alternate(lambda: ops.sim_bank_lse(bank, g, BETA), lambda: _torch_lse(bank, g, BETA), rounds, max(1, iters // 2))
        err = (ops.sim_bank_lse(bank, g, BETA) - _torch_lse(bank, g, BETA)).abs().max().item()
        floor_bytes = (ng * D * 2 + nb * D * 2 + ng * 4) / HBM_BYTES_PER_S
        floor_mfma = 2.0 * nb * ng * D / MFMA_BF16_FLOPS
        floor = max(floor_bytes, floor_mfma)
        r = dict(nb=nb, ng=ng, dim=D, beta=BETA, kernel_us=_median(tk) * 1e6, torch_fp32_us=_median(tt) * 1e6,
                 kernel_spread=_spread(tk), torch_over_kernel=_median(tt) / _median(tk), floor_bytes_us=floor_bytes * 1e6,
                 floor_mfma_us=floor_mfma * 1e6, share_of_larger_floor=floor / _median(tk), max_abs_diff_to_torch_fp32=err,
                 kernel_us_rounds=[t * 1e6 for t in tk])
        rows.append(r)
        print(f"bank_lse nb {nb:6d} ng {ng:8d}: kernel {r['kernel_us']:10.1f} us  torch fp32 {r['torch_fp32_us']:10.1f} us  floors "
              f"{r['floor_bytes_us']:8.1f} (bytes) {r['floor_mfma_us']:8.1f} (mfma) us  share of the larger {r['share_of_larger_floor']:.3f}  "
              f"|diff| {err:.2e}", flush=True)
        del bank, g
    return rows


def measure_add(rounds, iters, dev):
    """RetrievalIndex.add of 32 rows into storage that does not grow: a plain index, and one fitted on 1000 / 10000 bank rows"""
    from youku_mplug_amd.retrieval import RetrievalIndex
    new = _feats(32, 5, dev)
    out = {}
    for name, nb in (("plain", 0), ("fitted_1000", 1000), ("fitted_10000", 10000)):
        index = RetrievalIndex(D, device=dev, capacity=100000 + 32 * (iters + 2) * (rounds + 1))
        index.add(_feats(100000, 6, dev))
        if nb:
            index.fit_normaliser(_feats(nb, 7, dev), BETA)
        out[name] = _median([_time(lambda: index.add(new), iters) for _ in range(rounds)]) * 1e6
    print("RetrievalIndex.add of 32 rows: " + ", ".join(f"{k} {v:.1f} us" for k, v in out.items()), flush=True)
    return dict(rows=32, dim=D, **{k + "_us": v for k, v in out.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_prior.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    import youku_mplug_amd  # noqa: F401
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters, prior=measure_prior(a.rounds, a.iters, dev),
                  bank=measure_bank(a.rounds, a.iters, dev), add=measure_add(a.rounds, a.iters, dev))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(dict(tool="bench_search_prior", out=a.out)))


if __name__ == "__main__":
    main()
