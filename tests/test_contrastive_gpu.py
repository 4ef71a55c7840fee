"""The pre-train model's image-text contrastive head (use_contrastive, models/distributed_gpt3.py:122-127, 168-212) on the gfx950
kernels: the three entry points of csrc/contrastive.hip against fp32 torch, the model against the reference-module goldens
(tests/golden/contrastive_tiny*.pt, tools/gen_golden_contrastive.py), the head at config B's dims against an fp32 restatement,
graph capture, two ranks on one GPU, and the pre-train entry point.

The goldens' weight seed keeps every (clip, title) pair's best query token clear of the second best (tools/gen_golden_contrastive.py:
meta["min_top2_gap"]).  Near-ties of the max over query tokens can send a pair (i, j) to a different q in bf16 than in fp32, so the goldens gate gradient
norms and wide samples (tests/test_model_gpu.py: grad_devs), and the element-wise check of the head is made against an fp32
restatement that takes the HIP path's own argmax (`head_restatement`); the number of pairs whose argmax differs from fp32 is printed.
Gates are plain numbers (CONTRASTIVE_GATES), each <= ~2x the larger of the measured GPU value and the stand-in run of the same test
in tests/test_contrastive_cpu.py, both in the comments."""
import dataclasses
import json
import math
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# measured on an MI355X / on the stand-ins (worst case of the tests that use the gate)
CONTRASTIVE_GATES = {
    "loss_caption": 1.2e-4,     # relative: 4.6e-5 / 5.5e-5
    "loss_ita": 2e-3,           # relative: 9.3e-4 / 9.6e-4 (two ranks; one rank 3.7e-4 / 3.2e-4)
    "norm": 2.5e-2,             # worst |norm - ref| / ref over every trainable tensor: 1.1e-2 / 1.1e-2 (temp)
    "wide": 5e-2,               # worst relative L2 over the wide samples: 2.4e-2 / 2.3e-2
    "w2_norm": 6e-2,            # two ranks: worst |norm - ref| / ref over every trainable tensor: 1.6e-2 / 3.0e-2
    "w2_wide": 1.2e-1,          # two ranks: relative L2 of the wide samples / whole head tensors (WORLD2_KEYS): 5.1e-2 / 5.8e-2
    "head": 4e-2,               # relative L2 of head gradients / d image_query against the fp32 restatement with the HIP argmax:
}                               # 2.0e-2 / 1.5e-2 (vision_proj.bias)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _gate(what, measured, where=""):
    lim = CONTRASTIVE_GATES[what]
    print(f"    [gate contrastive] {what}: {measured:.3e} <= {lim:.1e} {where}")
    assert math.isfinite(measured) and measured <= lim, f"{what}: {measured:.3e} > {lim:.1e} {where}"


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def build_contrastive(cfg, dev, wseed, temp=0.07):
    from oracle.weights import make_state_dict, retrieval_spec
    from youku_mplug_amd.pretrain import synthetic_model
    model = synthetic_model(cfg, device=dev, use_contrastive=True, temp=temp)
    sd = make_state_dict(cfg, wseed, spec_fn=retrieval_spec)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    return model


def capture_itc_tapes(model):
    """record the tape of every contrastive forward of `model` (instance-level wrapper)"""
    tapes = []
    orig = model._contrastive_forward

    def spy(tape, ids, mask):
        orig(tape, ids, mask)
        tapes.append(tape)
    model._contrastive_forward = spy
    return tapes


def head_restatement(model, tape, rank=0):
    """fp32 torch restatement of the head from the HIP path's own image_query / pooled text state, routing the max through the HIP
    argmax.  World size 1 (the columns are this rank's own features).  -> dict(loss, grads of the head, d image_query,
    argmax disagreements with fp32)."""
    c = tape["itc"]
    B, E, Q = c["B"], c["E"], model.num_learnable_token
    assert c["WB"] == B
    f = lambda t: t.detach().float().cpu()
    iq = f(tape["image_query"]).requires_grad_(True)
    pooled = f(c["pooled"])
    Wv, bv, Wt, bt = (f(p).requires_grad_(True) for p in (model.vision_proj.weight, model.vision_proj.bias, model.text_proj.weight,
                                                          model.text_proj.bias))
    temp = f(model.temp).requires_grad_(True)
    v = F.normalize(iq @ Wv.t() + bv, dim=-1).view(B, Q, E)
    t = F.normalize(pooled @ Wt.t() + bt, dim=-1)
    s_q2t = torch.einsum("bqe,ce->bcq", v, t)                      # [clip, text, q]
    s_t2q = torch.einsum("be,cqe->bcq", t, v)                      # [text, clip, q]
    a1, a2 = c["arg1"].long().cpu(), c["arg2"].long().cpu()        # [clip, text] and (trans) [text, clip]
    sim_i2t = s_q2t.gather(-1, a1[..., None]).squeeze(-1) / temp
    sim_t2i = s_t2q.gather(-1, a2[..., None]).squeeze(-1) / temp
    tg = torch.arange(rank * B, rank * B + B)
    loss = (F.cross_entropy(sim_i2t, tg, label_smoothing=0.1) + F.cross_entropy(sim_t2i, tg, label_smoothing=0.1)) / 2
    loss.backward()
    flips = int((s_q2t.argmax(-1) != a1).sum() + (s_t2q.argmax(-1) != a2).sum())
    return dict(loss=loss.detach(), flips=flips, pairs=2 * B * B, diq=iq.grad, grads={"vision_proj.weight": Wv.grad, "vision_proj.bias": bv.grad,
                "text_proj.weight": Wt.grad, "text_proj.bias": bt.grad, "temp": temp.grad})


# ------------------------------------------------------------------------------------------------------------------ kernels
def _maxsim_ref(a, t, R, Q, C, E, alpha):
    s = torch.einsum("rqe,ce->rcq", a.float().cpu().view(R, Q, E), t.float().cpu().view(C, E))
    top2 = s.topk(min(2, Q), dim=-1).values
    gap = top2[..., 0] - top2[..., -1] if Q > 1 else torch.full((R, C), float("inf"))
    return s.max(-1).values * alpha, s.argmax(-1), gap


@pytest.mark.parametrize("R,Q,C,E", [(8, 32, 8, 256), (32, 128, 32, 256), (32, 128, 256, 256), (256, 128, 32, 256), (5, 40, 17, 24)])
@pytest.mark.parametrize("trans", [False, True])
def test_maxsim_fwd_vs_fp32(dev, R, Q, C, E, trans):
    from youku_mplug_amd import ops
    g = torch.Generator().manual_seed(R * 1000 + C + trans)
    a = F.normalize(torch.randn(R * Q, E, generator=g), dim=-1).to(torch.bfloat16)
    t = F.normalize(torch.randn(C, E, generator=g), dim=-1).to(torch.bfloat16)
    alpha = torch.tensor([1.0 / 0.07])
    sim, arg = ops.maxsim_fwd(a.to(dev), t.to(dev), R, Q, C, E, alpha_dev=alpha.to(dev), trans=trans)
    torch.cuda.synchronize()
    ref, refarg, gap = _maxsim_ref(a, t, R, Q, C, E, alpha.item())
    sim, arg = sim.cpu(), arg.cpu().long()
    if trans:
        sim, arg = sim.t(), arg.t()
    assert sim.shape == (R, C) and arg.shape == (R, C)
    err = (sim - ref).abs().max().item()
    assert err <= 2e-5 * (1 / 0.07), err                             # fp32 accumulation of bf16 products, scaled by alpha
    clear = gap > 1e-4
    assert torch.equal(arg[clear], refarg[clear]), int((arg[clear] != refarg[clear]).sum())
    assert ((arg >= 0) & (arg < Q)).all()


def test_maxsim_fwd_tie_goes_to_the_lowest_q(dev):
    from youku_mplug_amd import ops
    R, Q, C, E = 2, 128, 40, 64
    g = torch.Generator().manual_seed(3)
    t = F.normalize(torch.randn(C, E, generator=g), dim=-1).to(torch.bfloat16)
    a = (0.01 * torch.randn(R, Q, E, generator=g)).to(torch.bfloat16)
    # rows 17, 70 and 101 of clip 0 (one per wave's chunk) and rows 5, 6 of clip 1 are the same vector: exact ties
    best = torch.randn(E, generator=g).to(torch.bfloat16)
    for q in (101, 70, 17):
        a[0, q] = best
    a[1, 5] = a[1, 6] = best
    sim, arg = ops.maxsim_fwd(a.view(R * Q, E).to(dev), t.to(dev), R, Q, C, E)
    torch.cuda.synchronize()
    ref, _, _ = _maxsim_ref(a.view(R * Q, E), t, R, Q, C, E, 1.0)
    s = torch.einsum("qe,ce->cq", best.float()[None].expand(Q, E), t.float())[:, 0]
    win0 = ref[0] == s                                              # columns where the tied vector is the max
    assert win0.any()
    assert (arg.cpu()[0][win0] == 17).all()
    win1 = ref[1] == s
    assert win1.any() and (arg.cpu()[1][win1] == 5).all()
    again = ops.maxsim_fwd(a.view(R * Q, E).to(dev), t.to(dev), R, Q, C, E)
    assert torch.equal(again[0], sim) and torch.equal(again[1], arg)


@pytest.mark.parametrize("trans", [False, True])
def test_maxsim_route_is_exact(dev, trans):
    from youku_mplug_amd import ops
    R, Q, C = 24, 32, 16
    g = torch.Generator().manual_seed(5)
    arg = torch.randint(0, Q, (C, R) if trans else (R, C), generator=g, dtype=torch.int32)
    dsim = torch.randn(arg.shape, generator=g).to(torch.bfloat16)
    G = ops.maxsim_route(dsim.to(dev), arg.to(dev), R, Q, C, trans=trans).cpu()
    d, a = (dsim.t(), arg.t()) if trans else (dsim, arg)
    ref = torch.zeros(R, Q, C, dtype=torch.bfloat16)
    ref.scatter_(1, a.long()[:, None, :], d[:, None, :])
    assert torch.equal(G, ref.view(R * Q, C))


@pytest.mark.parametrize("rows,cols", [(8, 8), (32, 256), (3, 1000)])
def test_smoothed_ce_vs_torch(dev, rows, cols):
    from youku_mplug_amd import ops
    g = torch.Generator().manual_seed(rows + cols)
    raw = torch.randn(rows, cols, generator=g)
    target = torch.randint(0, cols, (rows,), generator=g)
    temp = torch.tensor(0.07, requires_grad=True)
    sim = raw / temp
    scale = 0.5 / rows
    losses, dsim, dts = ops.smoothed_ce(sim.detach().to(dev), target.to(dev), 0.1, scale, rows, cols)
    torch.cuda.synchronize()
    s = sim.detach().clone().requires_grad_(True)
    ref = F.cross_entropy(s, target, label_smoothing=0.1, reduction="none")
    (ref.sum() * scale).backward()
    assert torch.allclose(losses.cpu(), ref.detach(), rtol=1e-5, atol=1e-5)
    assert (dsim.float().cpu() - s.grad).abs().max().item() <= 1e-2 * s.grad.abs().max().item()
    (F.cross_entropy(raw / temp, target, label_smoothing=0.1, reduction="none").sum() * scale).backward()
    # dL/dtemp = -(1/temp) * sum(dsim * sim)
    mine = -(dts.cpu().sum() / 0.07)
    assert abs(mine.item() - temp.grad.item()) <= 1e-4 * abs(temp.grad.item()) + 1e-6, (mine.item(), temp.grad.item())


def test_soft_target_ce_unchanged(dev):
    """mpv_soft_target_ce (the retrieval head's loss, untouched by the contrastive kernels): deterministic to the bit and equal to its
    torch restatement on a fixed input."""
    from youku_mplug_amd import ops
    g = torch.Generator().manual_seed(11)
    sim = (torch.randn(16, 64, generator=g) * 10).to(dev)
    rid = torch.tensor([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3], device=dev)
    cid = torch.cat([rid, rid, rid, rid])
    a = ops.soft_target_ce(sim, rid, cid, 0.03, 16, 64)
    b = ops.soft_target_ce(sim, rid, cid, 0.03, 16, 64)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    t = (rid[:, None] == cid[None, :]).float()
    t = t / t.sum(1, keepdim=True)
    ref = -(torch.log_softmax(sim, 1) * t).sum(1)
    assert torch.allclose(a[0], ref, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------------ model
def test_contrastive_model_vs_reference_golden(dev):
    """DistributedGPT3_Pretrain with use_contrastive against the reference module (tests/golden/contrastive_tiny.pt): both losses,
    every trainable tensor's gradient (norm + wide sample), and the head element-wise against the fp32 restatement."""
    from oracle.weights import CONFIG_TINY, make_inputs
    from test_model_gpu import grad_devs
    g = torch.load(os.path.join(GOLD, "contrastive_tiny.pt"))
    m, f32, b16 = g["meta"], g["fp32"], g["bf16"]
    model = build_contrastive(CONFIG_TINY, dev, m["weight_seed"], m["temp"])
    model.eval()
    tapes = capture_itc_tapes(model)
    video, ids, mask = make_inputs(CONFIG_TINY, m["batch"], m["text_len"], seed=m["input_seed"], ragged=m["ragged"])
    text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    lc, li = model(video.to(dev).to(torch.bfloat16), text)
    assert lc.requires_grad and li.requires_grad
    for name, mine in (("loss_caption", lc), ("loss_ita", li)):
        ref = f32[name].item()
        _gate(name, abs(mine.item() - ref) / abs(ref), f"(reference bf16: {abs(b16[name].item() - ref) / abs(ref):.3e})")
    (lc + li).backward()
    _sync(dev)
    wn, ww = grad_devs(model, f32, b16, sample=False)
    _gate("norm", wn[0], f"at {wn[1]} (reference bf16 {wn[2]:.3e})")
    _gate("wide", ww[0], f"at {ww[1]} (reference bf16 {ww[2]:.3e})")
    r = head_restatement(model, tapes[0])
    print(f"    argmax differs from fp32 on {r['flips']} of {r['pairs']} pairs")
    assert abs(li.item() - r["loss"].item()) <= 1e-3 * abs(r["loss"].item())
    params = dict(model.named_parameters())
    for n, ref in r["grads"].items():
        _gate("head", rel(params[n].grad, ref), n)


def test_contrastive_head_at_config_b_dims(dev):
    """config B's head: B = 32, Q = 128, E = 256, vision width 768, text width 2048 (a one-layer tower on each side: the head does not
    see depth).  One step of the HIP path; the head's loss, gradients and d image_query against the fp32 restatement fed from the HIP
    path's own image_query and pooled text states."""
    from oracle.weights import CONFIG_B, make_inputs
    from youku_mplug_amd.pretrain import synthetic_model
    cfg = dataclasses.replace(CONFIG_B, img_size=64, num_frames=2, vit_depth=1, layers=1, vocab=2048, max_pos=256)
    torch.manual_seed(0)
    model = synthetic_model(cfg, device=dev, use_contrastive=True)
    with torch.no_grad():
        for p in (model.vision_proj.weight, model.text_proj.weight):
            p.normal_(0, 0.05)
        model.vision_proj.bias.normal_(0, 0.02)
        model.text_proj.bias.normal_(0, 0.02)
    model.eval()
    video, ids, mask = make_inputs(cfg, 32, 32, seed=21, ragged=True)
    with torch.no_grad():
        loss, tape = model._forward_pipeline(video.to(dev).to(torch.bfloat16), ids.to(dev), mask.to(dev))
        diq = model._contrastive_backward(tape, torch.ones((), device=dev))
    torch.cuda.synchronize()
    c = tape["itc"]
    assert c["B"] == 32 and c["WB"] == 32 and c["E"] == 256 and tape["image_query"].shape == (32 * 128, 768) and c["pooled"].shape == (32, 2048)
    r = head_restatement(model, tape)
    print(f"    argmax differs from fp32 on {r['flips']} of {r['pairs']} pairs")
    assert abs(tape["loss_ita"].item() - r["loss"].item()) <= 1e-3 * abs(r["loss"].item())
    params = dict(model.named_parameters())
    for n, ref in r["grads"].items():
        _gate("head", rel(params[n].grad, ref), n)
    _gate("head", rel(diq, r["diq"]), "d image_query")


def test_contrastive_graph_step_bit_identical_to_eager(dev):
    """engine.graph_step at world size 1 with the contrastive head on (dropout live in both decoder passes): three steps against the
    eager step from the same weights -- both losses and the final parameters bit-identical, loss_contrastive readable after replay."""
    from oracle.weights import CONFIG_TINY, make_inputs
    from youku_mplug_amd import engine as eng
    batches = []
    for i in range(3):
        video, ids, mask = make_inputs(CONFIG_TINY, 8, 12, seed=90 + i, ragged=True)
        batches.append((video.to(dev).to(torch.bfloat16), types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))))

    def run(graph):
        model = build_contrastive(CONFIG_TINY, dev, 4)
        model.train()
        groups = eng.get_parameter_groups(model, 0.05, model.no_weight_decay(), visual_backbone_scale=True)
        e, _, _, _ = eng.initialize(model=model, model_parameters=groups, config=dict(lr=2e-3, clip_grad=3.0))
        out = []
        for v, text in batches:
            if graph:
                total = e.graph_step(v, text)
                out.append((total.item(), model.loss_caption.item(), model.loss_contrastive.item()))
            else:
                lc, li = e(v, text)
                loss = lc + li
                e.backward(loss)
                e.step()
                out.append((loss.item(), lc.item(), li.item()))
        return out, e.flat.params.clone(), e

    la, pa, _ = run(False)
    lb, pb, eb = run(True)
    print("    eager", la, "\n    graph", lb)
    assert all(math.isfinite(x) and x > 0 for s in la for x in s) and len({s[2] for s in la}) > 1
    assert la == lb
    assert torch.equal(pa, pb)
    assert eb._graph is not None


# ------------------------------------------------------------------------------------------------------------------ two ranks
WORLD2_KEYS = ["vision_proj.weight", "vision_proj.bias", "text_proj.weight", "text_proj.bias", "temp", "learnable_queries",
               "attn_pool.attn.in_proj_weight", "visual_encoder.blocks.0.attn.qkv.weight", "visual_encoder.pos_embed"]


def world2_worker(rank, world, port, q, device, standins=False):
    """one rank of the two-rank run against contrastive_tiny_world2.pt: this rank's half of the global batch, (loss_caption +
    loss_ita).backward(), gradients all-reduced / world (what the data-parallel reducer leaves on every rank)"""
    import traceback
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
        import torch.distributed as dist
        if standins:
            torch.set_num_threads(2)
            import standin_contrastive

            class _MP:
                def setattr(self, obj, name, val):
                    setattr(obj, name, val)
            standin_contrastive.install(_MP())
        import youku_mplug_amd  # noqa: F401
        from oracle.weights import CONFIG_TINY, make_inputs
        dev = torch.device(device)
        if dev.type == "cuda":
            torch.cuda.set_device(dev)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        gold = torch.load(os.path.join(GOLD, "contrastive_tiny_world2.pt"))
        w = gold["meta"]
        model = build_contrastive(CONFIG_TINY, dev, w["weight_seed"], w["temp"])
        model.eval()
        video, ids, mask = make_inputs(CONFIG_TINY, w["batch"], w["text_len"], seed=w["input_seed"], ragged=w["ragged"])
        bl = w["batch"] // world
        sl = slice(rank * bl, (rank + 1) * bl)
        text = types.SimpleNamespace(input_ids=ids[sl].to(dev), attention_mask=mask[sl].to(dev))
        lc, li = model(video[sl].to(dev).to(torch.bfloat16), text)
        (lc + li).backward()
        _sync(dev)
        grads, norms = {}, {}
        for n, p in model.named_parameters():
            if p.grad is None:
                continue
            g = p.grad.float().clone()
            dist.all_reduce(g)
            g = (g / world).cpu()
            norms[n] = g.norm().item()
            if n in WORLD2_KEYS:
                grads[n] = g.numpy()
        q.put((rank, lc.item(), li.item(), norms, grads))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, "ERROR", traceback.format_exc()))
        raise


def run_world2(device, standins=False):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 39500 + os.getpid() % 2000
    procs = [ctx.Process(target=world2_worker, args=(r, 2, port, q, device, standins)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(300):
        try:
            r = q.get(timeout=2)
            res[r[0]] = r[1:]
        except Exception:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
        if len(res) == 2:
            break
    for p in procs:
        p.join(timeout=120 if len(res) == 2 else 5)
        if p.is_alive():
            p.kill()
    assert len(res) == 2 and all(v[0] != "ERROR" for v in res.values()), res
    return res


def check_world2(res):
    from oracle.gen_golden import WIDE_SAMPLE, wide_stride
    gold = torch.load(os.path.join(GOLD, "contrastive_tiny_world2.pt"))
    for r in range(2):
        for name, k in (("loss_caption", 0), ("loss_ita", 1)):
            ref = gold[name][r]
            _gate(name, abs(res[r][k] - ref) / abs(ref), f"rank {r}")
    assert res[0][1] != res[1][1]                                  # different rows, different local losses
    assert res[0][2] == res[1][2]                                  # replicas: the reduced gradients are the same on both ranks
    for n in res[0][3]:
        assert torch.equal(torch.from_numpy(res[0][3][n]), torch.from_numpy(res[1][3][n])), n
    assert set(res[0][2]) == set(gold["grad_norm"])
    worst = max((abs(res[0][2][n] - gold["grad_norm"][n]) / (gold["grad_norm"][n] + 1e-12), n) for n in gold["grad_norm"])
    _gate("w2_norm", worst[0], f"at {worst[1]}")
    for n, gnp in res[0][3].items():
        g = torch.from_numpy(gnp).reshape(-1)
        r = gold["grad_wide"][n].float()
        e = ((g[::wide_stride(g.numel())][:WIDE_SAMPLE] - r).norm() / (r.norm() + 1e-30)).item()
        if n in gold["grad_head"]:
            e = rel(torch.from_numpy(gnp), gold["grad_head"][n])
        _gate("w2_wide", e, f"two ranks, {n}")


def test_two_ranks_on_one_gpu_contrastive_vs_reference_golden(dev):
    """Two ranks with real kernels (both on this GPU, gloo on device tensors): features all-gathered in the forward, targets offset by
    rank * B, the gathered halves' gradients reduce-scattered back -- each rank's losses and the rank-averaged gradients against the
    reference module run the same way (tests/golden/contrastive_tiny_world2.pt); the replicas' gradients identical."""
    check_world2(run_world2("cuda:0"))


# ------------------------------------------------------------------------------------------------------------------ entry point
def write_contrastive_configs(d):
    from oracle.weights import CONFIG_TINY as s
    vis = dict(img_size=s.img_size, patch_size=s.patch_size, depth=s.vit_depth, num_frames=s.num_frames, embed_dim=s.vit_dim,
               num_heads=s.vit_heads, mlp_ratio=s.vit_mlp_ratio, drop_path=0, grad_ckpt=True, clip_model=True)
    txt = dict(vocab_size=s.vocab, hidden_size=s.hidden, ffn_hidden_size=s.ffn, num_hidden_layers=s.layers,
               num_attention_heads=s.heads, max_position_embeddings=s.max_pos, layernorm_epsilon=s.gpt_ln_eps)
    json.dump(vis, open(os.path.join(d, "vis.json"), "w"))
    json.dump(txt, open(os.path.join(d, "txt.json"), "w"))
    yml = f"""
text_decoder: 'nlp_gpt3_text-generation_1.3B/'
text_cfg: {d}/txt.json
visual_cfg: '{d}/vis.json'
_synthetic: true
batch_size: 8
num_workers: 0
max_length: 16
freeze_vit: false
freeze_text_decoder: true
num_learnable_token: {s.num_queries}
use_contrastive: true
temp: 0.07
embed_dim: 256
optimizer: {{lr: 1e-4, opt: "AdamW", weight_decay: 0.05, clip_grad: 3.0, opt_betas: [0.9, 0.999], opt_eps: 1e-6}}
schedular: {{epochs: 1, min_lr: 1e-6, warmup_epochs: -1, warmup_steps: 2, lr_sched_type: "cosine"}}
"""
    open(os.path.join(d, "pretrain.yaml"), "w").write(yml)
    return os.path.join(d, "pretrain.yaml")


def run_entry(cfg, out, seed, monkeypatch, graph="0"):
    """three --synthetic_steps steps of run_pretrain_distributed_gpt3.py; -> (epoch stats, engine, per-step log lines)"""
    sys.path.insert(0, ROOT)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(22000 + os.getpid() % 1000))
    monkeypatch.setenv("MPV_GRAPH", graph)
    import run_pretrain_distributed_gpt3 as entry
    from youku_mplug_amd import engine as eng
    args, config = entry.get_args(["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "3",
                                   "--seed", str(seed)])
    seen, per_step = {}, []
    orig_init, orig_train = eng.initialize, entry.train_one_epoch

    def spy(**kw):
        r = orig_init(**kw)
        seen["engine"] = r[0]
        return r

    def train(*a, **k):
        k["log"] = per_step.append
        return orig_train(*a, **k)
    monkeypatch.setattr(eng, "initialize", spy)
    monkeypatch.setattr(entry.mpv_engine, "initialize", spy)
    monkeypatch.setattr(entry, "train_one_epoch", train)
    stats = entry.main(args, config)
    return stats, seen.get("engine"), per_step


def test_entrypoint_contrastive_three_steps_checkpoint_and_graph(tmp_path, dev, monkeypatch):
    """run_pretrain_distributed_gpt3.py from a YAML with use_contrastive: true: loss_ita logged, finite and non-zero; the head's
    tensors in the DeepSpeed-layout checkpoint and back on resume; MPV_GRAPH=1 at N = 1 agrees with the eager loop."""
    cfg = write_contrastive_configs(str(tmp_path))
    out = str(tmp_path / "out0")
    stats, e, lines = run_entry(cfg, out, 5, monkeypatch)
    assert e.module.use_contrastive and math.isfinite(stats["loss_ita"]) and stats["loss_ita"] > 0
    assert math.isfinite(stats["loss"]) and stats["loss"] == pytest.approx(stats["loss_caption"] + stats["loss_ita"], rel=1e-6)
    assert any("loss_ita:" in ln for ln in lines)
    ck = torch.load(os.path.join(out, "checkpoint-0", "mp_rank_00_model_states.pt"), map_location="cpu")["module"]
    params = dict(e.module.named_parameters())
    for k in ("vision_proj.weight", "vision_proj.bias", "text_proj.weight", "text_proj.bias", "temp"):
        assert torch.equal(ck[k].cpu(), params[k].detach().cpu()), k
    # resume: nothing left to do, the weights (head included) are the checkpoint's
    _, e2, _ = run_entry(cfg, out, 5, monkeypatch)
    assert torch.equal(e2.flat.params, e.flat.params)
    assert torch.equal(e2.module.temp.detach(), e.module.temp.detach())
    # MPV_GRAPH=1 from the same seed in a fresh directory
    stats_g, eg, _ = run_entry(cfg, str(tmp_path / "out1"), 5, monkeypatch, graph="1")
    assert eg._graph is not None
    for k in ("loss", "loss_caption", "loss_ita"):
        assert stats_g[k] == stats[k], (k, stats_g[k], stats[k])
    assert torch.equal(eg.flat.params, e.flat.params)
