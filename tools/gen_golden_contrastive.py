"""TEST INFRASTRUCTURE ONLY -- goldens of the pre-train model's contrastive head (use_contrastive, models/distributed_gpt3.py:
122-127, 168-212) from the reference's own DistributedGPT3_Pretrain, on CPU (needs the reference tree; see oracle/ref_loader.py).

    python tools/gen_golden_contrastive.py            # writes both files below
    python tools/gen_golden_contrastive.py --check    # regenerates in memory and compares with the committed files

tests/golden/contrastive_tiny.pt: CONFIG_TINY (Q = 32), B = 8, L = 10 ragged, eval mode, fp32 and bf16 runs recorded as
oracle.gen_golden.run_retrieval records them (both losses, every trainable tensor's gradient norm, 64-element and wide samples).
tests/golden/contrastive_tiny_world2.pt: the same model on two gloo ranks (two CPU processes), each with half of a global batch of
16: the reference's own data-parallel semantics (all-gather forward, gloo all-to-all sum backward, targets offset by rank * B).
Per rank its two losses; the rank-averaged gradients (what the data-parallel all-reduce / world leaves on every rank) as norms,
wide samples and the whole head tensors.  Weights (retrieval_spec: the pre-train keys + vision_proj / text_proj / temp) and inputs
are regenerated from their seeds.

One correction to the reference as it runs on CPU: the gloo branch of its all_gather backward (models/distributed_utils.py:
_AllGather.backward -> _AlltoAll, :347-352) scatters into torch.empty_like(grad) and so permutes the elements of a NON-contiguous
incoming gradient -- which the t2i product's `vision_feats_all.permute(0, 2, 1)` (models/distributed_gpt3.py:199) produces; at
world size 1 a transposed [2, 3] gradient comes back as [[0, 4, 3], [2, 1, 5]] instead of [[0, 2, 4], [1, 3, 5]].  The NCCL
branch the reference trains with (_Reduce_Scatter, inputs made contiguous) is exact.  `contiguous_gather_grads` hands that
backward contiguous gradients, so the goldens hold the reference's intended (NCCL) function; everything else runs unmodified."""
import contextlib
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import ref_loader  # noqa: E402
from oracle.gen_golden import GOLDEN_DIR, grad_sample, grad_wide, record_wide_grads  # noqa: E402
from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict, retrieval_spec  # noqa: E402

# weight seed 7: the smallest fp32 gap between the best and the second-best query token of any (clip, title) pair is 6.7e-3 here and
# 2.4e-3 in the two-rank batch (seed 3, for instance, has a 4e-5 near-tie: a bf16 path then picks the other token, and the gradient
# summed over every clip of that title lands on another query row).  The gaps are recorded as meta["min_top2_gap"].
META = dict(batch=8, text_len=10, weight_seed=7, input_seed=11, ragged=True, embed_dim=256, temp=0.07)
WORLD2 = dict(world=2, batch=16, text_len=10, weight_seed=7, input_seed=13, ragged=True)
HEAD_KEYS = ["vision_proj.weight", "vision_proj.bias", "text_proj.weight", "text_proj.bias", "temp"]


def build_reference_contrastive(cfg, seed, dtype=torch.float32, embed_dim=256, temp=0.07):
    """the reference DistributedGPT3_Pretrain with use_contrastive: True (ref_loader.build_reference_model fixes it to False)"""
    vt, mg, dg = ref_loader.import_reference()
    sd = make_state_dict(cfg, seed, spec_fn=lambda c: retrieval_spec(c, embed_dim))
    tmp = tempfile.mkdtemp(prefix="mpv_oracle_")
    for name, d in (("config.json", ref_loader._gpt_config_dict(cfg)), ("visual.json", ref_loader._visual_config_dict(cfg)),
                    ("text.json", ref_loader._gpt_config_dict(cfg))):
        with open(os.path.join(tmp, name), "w") as f:
            json.dump(d, f)
    config = {"visual_cfg": os.path.join(tmp, "visual.json"), "text_cfg": os.path.join(tmp, "text.json"), "text_decoder": tmp,
              "megatron_cfg": {"world_size": 1, "model_parallel_size": 1, "tensor_model_parallel_size": 1}, "freeze_vit": False,
              "freeze_text_decoder": True, "num_learnable_token": cfg.num_queries, "use_contrastive": True,
              "contrastive_embed_dim": embed_dim, "temp": temp}
    prefix = "text_decoder.dist_model."
    gpt_sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    old = mg.pre_load
    mg.pre_load = lambda *a, **k: gpt_sd
    try:
        with ref_loader._cpu_patches():
            model = dg.DistributedGPT3_Pretrain(config=config, tokenizer=None)
    finally:
        mg.pre_load = old
    model.load_state_dict(sd, strict=True)
    return model.to(dtype), sd


@contextlib.contextmanager
def contiguous_gather_grads():
    """models.distributed_gpt3.all_gather with every incoming gradient made contiguous (see the module docstring)"""
    _, _, dg = ref_loader.import_reference()

    class _Contiguous(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            return g.contiguous()

    orig = dg.all_gather
    dg.all_gather = lambda t, *a, **k: tuple(_Contiguous.apply(o) for o in orig(t, *a, **k))
    try:
        yield
    finally:
        dg.all_gather = orig


def _step(model, video, ids, mask, gaps=None):
    model.eval()
    feats = {}
    hooks = [getattr(model, n).register_forward_hook(lambda m, i, o, n=n: feats.__setitem__(n, o.detach().float()))
             for n in ("vision_proj", "text_proj")]
    lc, li = model(video, types.SimpleNamespace(input_ids=ids, attention_mask=mask))
    for h in hooks:
        h.remove()
    (lc + li).backward()
    if gaps is not None:        # fp32 gap between the two best query tokens, worst pair of this rank's clips x its titles
        v, t = torch.nn.functional.normalize(feats["vision_proj"], dim=-1), torch.nn.functional.normalize(feats["text_proj"], dim=-1)
        top = torch.einsum("bqe,ce->bcq", v, t).topk(2, dim=-1).values
        gaps.append(float((top[..., 0] - top[..., 1]).min()))
    return lc, li


def gen_tiny():
    cfg, m = CONFIG_TINY, META
    rec = {"meta": dict(case="contrastive_tiny", **m, torch=str(torch.__version__))}
    keep = {}
    for tag, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        model, _ = build_reference_contrastive(cfg, m["weight_seed"], dtype, m["embed_dim"], m["temp"])
        video, ids, mask = make_inputs(cfg, m["batch"], m["text_len"], seed=m["input_seed"], ragged=m["ragged"])
        gaps = []
        with ref_loader.single_rank_collectives(), contiguous_gather_grads():
            lc, li = _step(model, video.to(dtype), ids, mask, gaps if tag == "fp32" else None)
        if tag == "fp32":
            rec["meta"]["min_top2_gap"] = gaps[0]
        r = {"loss_caption": lc.detach().float().clone(), "loss_ita": li.detach().float().clone(), "grad_norm": {}, "grad_sample": {}}
        for n, p in model.named_parameters():
            if p.grad is not None:
                r["grad_norm"][n] = float(p.grad.float().norm())
                r["grad_sample"][n] = grad_sample(p.grad)
        record_wide_grads(model, r, keep, tag)
        rec[tag] = r
        print(f"[contrastive_tiny/{tag}] loss_caption={float(lc):.6f} loss_ita={float(li):.6f}", flush=True)
    return rec


def _world2_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, w = CONFIG_TINY, WORLD2
    model, _ = build_reference_contrastive(cfg, w["weight_seed"], torch.float32, META["embed_dim"], META["temp"])
    video, ids, mask = make_inputs(cfg, w["batch"], w["text_len"], seed=w["input_seed"], ragged=w["ragged"])
    bl = w["batch"] // world
    sl = slice(rank * bl, (rank + 1) * bl)
    with contiguous_gather_grads():
        lc, li = _step(model, video[sl], ids[sl], mask[sl])
    grads = {}
    for n, p in model.named_parameters():
        if p.grad is not None:
            g = p.grad.detach().float().clone()
            dist.all_reduce(g)
            grads[n] = (g / world).numpy()
    q.put((rank, float(lc.detach()), float(li.detach()), grads))
    dist.barrier()
    dist.destroy_process_group()


def gen_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + os.getpid() % 500
    procs = [ctx.Process(target=_world2_worker, args=(r, WORLD2["world"], port, q)) for r in range(WORLD2["world"])]
    for p in procs:
        p.start()
    res = dict((r[0], r[1:]) for r in (q.get(timeout=600) for _ in procs))
    for p in procs:
        p.join(timeout=60)
    grads = {n: torch.from_numpy(g) for n, g in res[0][2].items()}
    for n, g in res[1][2].items():
        assert torch.equal(grads[n], torch.from_numpy(g)), n
    rec = {"meta": dict(case="contrastive_tiny_world2", **WORLD2, embed_dim=META["embed_dim"], temp=META["temp"], torch=str(torch.__version__)),
           "loss_caption": [res[r][0] for r in range(WORLD2["world"])], "loss_ita": [res[r][1] for r in range(WORLD2["world"])],
           "grad_norm": {n: float(g.norm()) for n, g in grads.items()},
           "grad_wide": {n: grad_wide(g).to(torch.bfloat16) for n, g in grads.items()},
           "grad_head": {n: grads[n].clone() for n in HEAD_KEYS}}
    print(f"[contrastive_tiny_world2] loss_ita per rank {rec['loss_ita']}", flush=True)
    return rec


def main(argv):
    recs = {"contrastive_tiny": gen_tiny(), "contrastive_tiny_world2": gen_world2()}
    for name, rec in recs.items():
        path = os.path.join(GOLDEN_DIR, f"{name}.pt")
        if "--check" in argv:
            old = torch.load(path)
            assert _same(old, rec), f"{path}: regenerated record differs"
            print("matches", path)
        else:
            torch.save(rec, path)
            print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def _same(a, b):
    """records equal apart from the torch version string"""
    if isinstance(a, dict):
        return set(a) == set(b) and all(k == "torch" or _same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


if __name__ == "__main__":
    main(sys.argv[1:])
