"""Retrieval search on one GPU: queries/s and gallery rows/s of ops.sim_topk (k = 10, D = 256) beside the torch formulation the
evaluation loop of downstream/run_retrieval_distributed_gpt3.py writes (fp32 copies of the features, `q @ g.T`, then a top-k of
every row; the matrix in query chunks where it would not fit), same process, alternated three times; the floors (gallery bytes at
the HBM rate, FLOPs at the dense bf16 peak); and the peak device memory of `evaluation` against `evaluation_on_device` at
V = T = 20000 synthetic features.

    python tools/bench_retrieval_search.py [--out profiles/retrieval_search.json] [--rounds 3] [--iters 5]

Prints one table and writes one JSON file."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "downstream"))

HBM_BYTES_PER_S = 6.3e12          # measured streaming read rate of one MI355X
BF16_FLOPS = 2.5e15               # dense bf16 MFMA peak (datasheet)
SHAPES = [(1, 1000000), (64, 1000000), (4096, 100000), (10000, 10000)]
D, K = 256, 10


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def _torch_topk(q, g, k, budget=1 << 31):
    """fp32 features, matmul, topk: the parent formulation; query chunks keep the fp32 matrix under `budget` bytes"""
    qf, gf = q.float(), g.float()
    step = max(1, min(q.shape[0], budget // (4 * g.shape[0])))
    out = [torch.topk(qf[i:i + step] @ gf.t(), min(k, g.shape[0]), dim=1) for i in range(0, q.shape[0], step)]
    return torch.cat([o.values for o in out]), torch.cat([o.indices for o in out])


def _feats(n, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, D, generator=g, device=dev), dim=1).to(torch.bfloat16)


class _Towers:
    def __init__(self, vf, tf):
        self.vf, self.tf = vf, tf

    def eval(self):
        return self

    def extract_text_feature(self, text):
        return self.tf[text.input_ids[:, 0]]

    def extract_vision_feature(self, video):
        return self.vf[video[:, 0].long()]


class _Split:
    def __init__(self, n, bs):
        self.text = [(t,) for t in range(n)]
        self.txt2vid = {t: t for t in range(n)}
        self.vid2txt = {t: [t] for t in range(n)}
        self.dataset, self.n, self.bs = self, n, bs

    def __iter__(self):
        for lo in range(0, self.n, self.bs):
            ids = torch.arange(lo, min(self.n, lo + self.bs))
            yield ids[:, None].float(), ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_search.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--eval_n", type=int, default=20000)
    a = ap.parse_args()
    import youku_mplug_amd  # noqa: F401
    import run_retrieval_distributed_gpt3 as entry
    from youku_mplug_amd import ops
    dev = torch.device("cuda:0")
    rows = []
    for nq, ng in SHAPES:
        q, g = _feats(nq, 0, dev), _feats(ng, 1, dev)
        tgt = torch.randint(0, ng, (nq, 1), device=dev)
        t_k, t_t, t_r = [], [], []
        for _ in range(a.rounds):                                   # alternate: both sides see the same clocks and neighbours
            t_k.append(_time(lambda: ops.sim_topk(q, g, K), a.iters))
            t_t.append(_time(lambda: _torch_topk(q, g, K), a.iters))
            t_r.append(_time(lambda: ops.sim_rank(q, g, tgt), a.iters))
        tk, tt, tr = sorted(t_k)[len(t_k) // 2], sorted(t_t)[len(t_t) // 2], sorted(t_r)[len(t_r) // 2]
        qtiles = (nq + 31) // 32
        floor_bytes = ng * D * 2 / HBM_BYTES_PER_S                  # every gallery row read once (query tiles share L2 / MALL)
        floor_flops = 2.0 * qtiles * 32 * ng * D / BF16_FLOPS       # the MFMA tile is 32 queries wide whatever nq is
        rows.append(dict(nq=nq, ng=ng, dim=D, k=K, sim_topk_us=tk * 1e6, sim_rank_us=tr * 1e6, torch_us=tt * 1e6,
                         speedup_topk=tt / tk, queries_per_s=nq / tk, gallery_rows_per_s=nq * ng / tk,
                         floor_stream_us=floor_bytes * 1e6, floor_mfma_us=floor_flops * 1e6,
                         sim_topk_us_rounds=[t * 1e6 for t in t_k], torch_us_rounds=[t * 1e6 for t in t_t]))
        print(f"nq {nq:6d} ng {ng:8d}: sim_topk {tk * 1e6:9.1f} us  sim_rank {tr * 1e6:9.1f} us  torch {tt * 1e6:9.1f} us  "
              f"x{tt / tk:5.2f}  floors: stream {floor_bytes * 1e6:7.1f} us, mfma {floor_flops * 1e6:7.1f} us", flush=True)
        del q, g
    # peak device memory of the two evaluation paths
    n = a.eval_n
    model, split, tok = _Towers(_feats(n, 2, dev), _feats(n, 3, dev)), _Split(n, 64), entry.SyntheticTokenizer()
    mem = {}
    for name, fn in (("evaluation", entry.evaluation), ("evaluation_on_device", entry.evaluation_on_device)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        fn(model, split, tok, dev, {"max_length": 8})
        torch.cuda.synchronize()
        mem[name] = dict(peak_bytes_over_baseline=torch.cuda.max_memory_allocated() - base, seconds=time.perf_counter() - t0)
        print(f"{name:22s} V = T = {n}: peak {mem[name]['peak_bytes_over_baseline'] / 2 ** 20:9.1f} MiB over the features, "
              f"{mem[name]['seconds']:.2f} s", flush=True)
    result = dict(device=torch.cuda.get_device_name(0), shapes=rows, eval_memory=dict(n=n, **mem))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(dict(tool="bench_retrieval_search", out=a.out)))


if __name__ == "__main__":
    main()
