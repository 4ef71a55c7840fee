"""Searches over an FP8 (e4m3) gallery beside the bf16 searches on one GPU, at the shapes of the two existing search tables: sim at
1 x 1e6, 64 x 1e6 and 4096 x 1e5 rows (D = 256, k = 10; tools/bench_retrieval_search.py) and query-max title -> clip at 1k x 1k and
1k x 10k clips (Q = E = 256; tools/bench_maxsim_search.py).  The bf16 entry and the _q8 entry alternate in one process, three rounds,
median of the rounds; the bf16 gallery is the dequantised codes, so both sides compute the same results (checked, and recorded as
`identical`).  Beside each measurement: the stream floor of the codes (one byte per element at the HBM rate) and the bytes of both
indexes.  Then the time RetrievalIndex / MaxSimIndex.add spends quantising 32 clips x 256 rows.

    python tools/bench_index_fp8.py [--out profiles/index_fp8.json] [--rounds 3] [--iters 5]

Prints one table and writes one JSON file.  There is no threshold in here: the capacity is the feature, the times are a report."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12          # measured streaming read rate of one MI355X (tools/bench_retrieval_search.py)
D, K = 256, 10
SIM_SHAPES = [(1, 1000000), (64, 1000000), (4096, 100000)]
MAXSIM_SHAPES = [(1000, 1000), (1000, 10000)]          # titles x clips of Q = 256 rows


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def _median(ts):
    return sorted(ts)[len(ts) // 2]


def _feats(n, seed, dev, chunk=1 << 20):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((n, D), dtype=torch.bfloat16, device=dev)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        out[lo:lo + m] = torch.nn.functional.normalize(torch.randn(m, D, generator=g, device=dev), dim=1).to(torch.bfloat16)
    return out


def _dequantize(codes, scale, chunk=1 << 20):
    out = torch.empty(codes.shape, dtype=torch.bfloat16, device=codes.device)
    for lo in range(0, codes.shape[0], chunk):
        out[lo:lo + chunk] = (codes[lo:lo + chunk].view(torch.float8_e4m3fn).float() * scale[lo:lo + chunk, None]).to(torch.bfloat16)
    return out


def _row(kind, nq, ng, group, bf16, q8, rounds, iters):
    """alternate the bf16 and the _q8 call of one entry; -> dict of medians, rounds, floor and index bytes"""
    t_b, t_q = [], []
    for _ in range(rounds):                                          # alternate: both sides see the same clocks and neighbours
        t_b.append(_time(bf16, iters))
        t_q.append(_time(q8, iters))
    a, b = bf16(), q8()
    same = all(torch.equal(x, y) for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)))
    rows = ng * group
    r = dict(entry=kind, nq=nq, ng=ng, group=group, dim=D, bf16_us=_median(t_b) * 1e6, q8_us=_median(t_q) * 1e6,
             q8_over_bf16=_median(t_q) / _median(t_b), bf16_us_rounds=[t * 1e6 for t in t_b], q8_us_rounds=[t * 1e6 for t in t_q],
             floor_stream_q8_us=rows * D / HBM_BYTES_PER_S * 1e6, floor_stream_bf16_us=rows * D * 2 / HBM_BYTES_PER_S * 1e6,
             index_bytes_bf16=rows * D * 2, index_bytes_fp8=rows * D + rows * 4, identical=same)
    print(f"{kind:12s} nq {nq:5d} ng {ng:8d} x {group:3d}: bf16 {r['bf16_us']:9.1f} us  q8 {r['q8_us']:9.1f} us  q8/bf16 {r['q8_over_bf16']:5.2f}  "
          f"floor(1 B/el) {r['floor_stream_q8_us']:7.1f} us  index {r['index_bytes_bf16'] / 2 ** 20:8.1f} -> {r['index_bytes_fp8'] / 2 ** 20:8.1f} MiB  "
          f"identical {same}", flush=True)
    return r


def measure(rounds, iters, dev):
    from youku_mplug_amd import ops
    rows = []
    for nq, ng in SIM_SHAPES:
        q = _feats(nq, 0, dev)
        codes, scale = ops.quantize_rows_e4m3(_feats(ng, 1, dev))
        g = _dequantize(codes, scale)
        tgt = torch.randint(0, ng, (nq, 1), device=dev)
        rows.append(_row("sim_topk", nq, ng, 1, lambda: ops.sim_topk(q, g, K), lambda: ops.sim_topk_q8(q, codes, scale, K), rounds, iters))
        rows.append(_row("sim_rank", nq, ng, 1, lambda: ops.sim_rank(q, g, tgt), lambda: ops.sim_rank_q8(q, codes, scale, tgt), rounds, iters))
        del q, g, codes, scale
    for nq, ng in MAXSIM_SHAPES:
        q = _feats(nq, 2, dev)
        codes, scale = ops.quantize_rows_e4m3(_feats(ng * 256, 3, dev))
        g = _dequantize(codes, scale).view(ng, 256, D)
        codes, scale = codes.view(ng, 256, D), scale.view(ng, 256)
        tgt = torch.randint(0, ng, (nq, 1), device=dev)
        rows.append(_row("maxsim_topk", nq, ng, 256, lambda: ops.maxsim_topk(q, g, K), lambda: ops.maxsim_topk_q8(q, codes, scale, K),
                         rounds, iters))
        rows.append(_row("maxsim_rank", nq, ng, 256, lambda: ops.maxsim_rank(q, g, tgt), lambda: ops.maxsim_rank_q8(q, codes, scale, tgt),
                         rounds, iters))
        del q, g, codes, scale
    return rows


def measure_add(rounds, iters, dev):
    """MaxSimIndex.add of 32 clips x 256 rows into storage that does not grow: bf16 (a copy) and fp8 (quantise + two copies)"""
    from youku_mplug_amd.retrieval import MaxSimIndex
    clips = _feats(32 * 256, 4, dev).view(32, 256, D)
    out = {}
    for storage in ("bf16", "fp8"):
        index = MaxSimIndex(D, 256, device=dev, capacity=32 * (iters + 2) * (rounds + 1), storage=storage)
        out[storage] = _median([_time(lambda: index.add(clips), iters) for _ in range(rounds)]) * 1e6
    print(f"MaxSimIndex.add of 32 clips x 256 rows: bf16 {out['bf16']:.1f} us, fp8 {out['fp8']:.1f} us", flush=True)
    return dict(clips=32, rows_per_clip=256, dim=D, bf16_us=out["bf16"], fp8_us=out["fp8"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_fp8.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    import youku_mplug_amd  # noqa: F401
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters, shapes=measure(a.rounds, a.iters, dev),
                  add=measure_add(a.rounds, a.iters, dev))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(dict(tool="bench_index_fp8", out=a.out)))


if __name__ == "__main__":
    main()
