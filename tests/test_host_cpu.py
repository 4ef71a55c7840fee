"""CPU-side tests (no GPU): oracle vs the reference's own modules and the committed goldens,
state-dict drop-in layout, C-ABI export table, host logic (param groups, schedules, flat
buffers), and the world_size-2 gloo data-parallel path."""
import ctypes
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12)).item()


def test_cabi_exports_every_declared_symbol():
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    declared = set(re.findall(r"\b(mpv_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"mpv_gemm_epilogue", "mpv_attn_desc"}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/mpv.h but not exported"
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert _lib.lib().mpv_version() >= 100


def test_adamw_hyper_pack_matches_the_by_value_formula():
    """mpv_adamw_hyper_pack (host side of mpv_adamw_step_grouped_dev): lr[8], wd[8] and the two bias-correction factors computed as
    mpv_adamw_step_grouped computes them (double pow, one rounding to float) -- the reason the device-hyper step is bit-identical."""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    lrs, wds = [1e-4, 2.5e-5, 3e-3], [0.05, 0.0, 0.1]
    out = (ctypes.c_float * 18)()
    arr = ctypes.c_float * 3
    for step in (1, 7, 2000):
        _lib.check(_lib.lib().mpv_adamw_hyper_pack(arr(*lrs), arr(*wds), 3, 0.9, 0.999, step, out), "pack")
        f32 = lambda x: ctypes.c_float(x).value
        assert list(out[:3]) == [f32(x) for x in lrs] and list(out[8:11]) == [f32(x) for x in wds] and all(v == 0.0 for v in list(out[3:8]) + list(out[11:16]))
        b1, b2 = float(f32(0.9)), float(f32(0.999))
        assert out[16] == f32(1.0 / (1.0 - b1 ** step)) and out[17] == f32(1.0 / (1.0 - b2 ** step) ** 0.5)
    assert _lib.lib().mpv_adamw_hyper_pack(arr(*lrs), arr(*wds), 3, 0.9, 0.999, 0, out) != 0      # steps count from 1


def test_product_has_no_cpu_fallback():
    from youku_mplug_amd import _lib, ops
    with pytest.raises(_lib.MpvError):
        ops.gemm(torch.zeros(8, 8, dtype=torch.bfloat16), torch.zeros(8, 8, dtype=torch.bfloat16), 8, 8, 8)
    for f in os.listdir(os.path.join(ROOT, "youku-mplug_amd")):
        if f.endswith(".py"):
            src = open(os.path.join(ROOT, "youku-mplug_amd", f)).read()
            assert "import oracle" not in src and "from oracle" not in src, f"{f} imports the oracle"


def test_restatement_matches_goldens_tiny():
    """The travelling restatement reproduces the committed reference outputs (fp32, tight)."""
    from oracle import restate
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict
    g = torch.load(os.path.join(GOLD, "tiny.pt"))
    m = g["meta"]
    sd = {k: v.requires_grad_(True) for k, v in make_state_dict(CONFIG_TINY, m["weight_seed"]).items()}
    video, ids, mask = make_inputs(CONFIG_TINY, m["batch"], m["text_len"], seed=m["input_seed"], ragged=m["ragged"])
    r = restate.pretrain_forward(video, ids, mask, sd, CONFIG_TINY)
    assert abs(r["loss"].item() - g["fp32"]["loss"].item()) < 1e-5
    assert rel(r["logits"], g["fp32"]["logits"]) < 1e-5
    assert rel(r["losses"], g["fp32"]["losses"]) < 1e-5
    r["loss"].backward()
    for n, gn in g["fp32"]["grad_norm"].items():
        assert abs(sd[n].grad.norm().item() - gn) <= 1e-4 * gn + 1e-9, n


def test_restatement_matches_reference_modules_live():
    """The restatement against the reference's own DistributedGPT3_Pretrain (CONFIG_REF_MODULES: CONFIG_TINY's structure at narrow
    widths; weight seed 5, B=3, L=10 ragged): logits, last hidden state and every gradient, and the state-dict drop-in layout
    (tests/golden/ref_modules_small.pt, written from the reference modules by oracle/gen_golden.py)."""
    import dataclasses
    from oracle import restate
    from oracle.gen_golden import CONFIG_REF_MODULES as cfg
    from oracle.weights import make_inputs, make_state_dict
    gold = torch.load(os.path.join(GOLD, "ref_modules_small.pt"))
    assert gold["meta"]["config"] == dataclasses.asdict(cfg)
    g = gold["plain"]
    video, ids, mask = make_inputs(cfg, 3, 10, seed=g["input_seed"], ragged=True)
    sdd = {k: v.clone().requires_grad_(True) for k, v in make_state_dict(cfg, g["weight_seed"]).items()}
    r = restate.pretrain_forward(video, ids, mask, sdd, cfg)
    r["loss"].backward()
    assert rel(r["logits"], g["logits"]) < 1e-5 and rel(r["last_hidden_state"], g["last_hidden_state"]) < 1e-5
    assert len(g["grad"]) > 0
    for n, ref_grad in g["grad"].items():
        assert rel(sdd[n].grad, ref_grad) < 1e-4, n
    # state-dict drop-in: identical keys and shapes
    from youku_mplug_amd.pretrain import synthetic_model
    mine = synthetic_model(cfg, device="cpu").state_dict()
    ref = g["state_dict_shapes"]
    assert list(sorted(mine)) == list(sorted(ref))
    for k in ref:
        assert tuple(mine[k].shape) == tuple(ref[k]), k


def test_connect_ln_restatement_matches_reference_modules_live():
    """visual_cfg['connect_ln'] (models/distributed_gpt3.py:112-115,136): LayerNormWithForceFP32 behind visual_fc.  The restatement
    against the reference's own module built with the flag, and the product's state-dict layout against the reference's
    (tests/golden/ref_modules_small.pt, written from the reference modules by oracle/gen_golden.py)."""
    import dataclasses
    from oracle import restate
    from oracle.gen_golden import CONFIG_REF_MODULES
    from oracle.weights import make_inputs, make_state_dict
    gold = torch.load(os.path.join(GOLD, "ref_modules_small.pt"))
    assert gold["meta"]["config"] == dataclasses.asdict(CONFIG_REF_MODULES)
    g = gold["connect_ln"]
    cfg = dataclasses.replace(CONFIG_REF_MODULES, connect_ln=True)
    ref = g["state_dict_shapes"]
    assert "visual_norm.weight" in ref and g["visual_norm_type"] != "Identity"
    video, ids, mask = make_inputs(cfg, 3, 10, seed=g["input_seed"], ragged=True)
    sdd = {k: v.clone().requires_grad_(True) for k, v in make_state_dict(cfg, g["weight_seed"]).items()}
    r = restate.pretrain_forward(video, ids, mask, sdd, cfg)
    r["loss"].backward()
    assert rel(r["logits"], g["logits"]) < 1e-5 and rel(r["last_hidden_state"], g["last_hidden_state"]) < 1e-5
    for n in ("visual_norm.weight", "visual_norm.bias", "visual_fc.weight", "learnable_queries", "visual_encoder.blocks.0.attn.qkv.weight"):
        assert rel(sdd[n].grad, g["grad"][n]) < 1e-4, n
    from youku_mplug_amd.pretrain import synthetic_model
    mine = synthetic_model(cfg, device="cpu").state_dict()
    assert list(sorted(mine)) == list(sorted(ref))
    assert tuple(mine["visual_norm.weight"].shape) == tuple(ref["visual_norm.weight"])


def test_randaugment_restatement_vs_reference_module_through_cv2_shim():
    """oracle/augment.py against the reference's dataset/video_utils/randaugment_video.py, imported with oracle/cv2_shim.py standing
    in for opencv (not installed): the class-level draw logic (ops per clip, apply mask, level -> arguments), the numpy ops and the
    code around the cv2 calls are the reference's own; the cv2 calls themselves land in the oracle's restatement of opencv
    ("parity unpinned" at that boundary, see oracle/augment.py).  The reference's outputs are recorded in
    tests/golden/randaugment_digests.pt, written through the same shim by oracle/gen_golden.py, by their digest over dtype, shape and
    contents (oracle/gen_golden.py:array_digest): equal digests are equal dtype and equal arrays."""
    import numpy as np
    from oracle import augment as A
    from oracle.gen_golden import RANDAUG_LEVELS, RANDAUG_MS, RANDAUG_SEEDS, array_digest, randaug_frames
    g = torch.load(os.path.join(GOLD, "randaugment_digests.pt"))
    assert g["meta"]["augs"] == list(A.DEFAULT_AUGS)
    frames = randaug_frames()
    for M in RANDAUG_MS:
        for seed in RANDAUG_SEEDS:
            np.random.seed(seed)
            o = A.TemporalConsistentRandomAugment(N=2, M=M, augs=A.DEFAULT_AUGS)(frames)
            assert array_digest(o) == g["clips"][(M, seed)], (M, seed, o.dtype)
    for name in A.DEFAULT_AUGS:
        for level in RANDAUG_LEVELS:
            assert g["args"][(name, level)] == A.level_to_args(name, level), (name, level)
            got = A.FUNC[name](frames[1], *A.level_to_args(name, level))
            assert array_digest(got) == g["ops"][(name, level)], (name, level, got.dtype)
    # restated opencv pieces: properties that do not need opencv to check
    img = frames[0]
    assert np.array_equal(A.warp_affine_linear(img, np.float32([[1, 0, 0], [0, 1, 0]]), (128, 128, 128)), img)
    t = A.translate_x_func(img, 5, (128, 128, 128))
    assert np.array_equal(t[:, :-5], img[:, 5:]) and (t[:, -5:] == 128).all()
    t = A.translate_y_func(img, 3, (128, 128, 128))
    assert np.array_equal(t[:-3], img[3:]) and (t[-3:] == 128).all()
    r360 = A.warp_affine_linear(img, A.get_rotation_matrix_2d((28, 24), 360, 1), (0, 0, 0))
    assert np.abs(r360.astype(int) - img.astype(int)).max() <= 1
    flat = np.full((9, 9, 3), 77, dtype=np.uint8)
    assert np.array_equal(A.sharpness_func(flat, 0.64), flat) and np.array_equal(A.sharpness_func(flat, 0.0), flat)


def test_state_dict_layout_matches_spec():
    from oracle.weights import CONFIG_TINY, state_dict_spec
    from youku_mplug_amd.pretrain import synthetic_model
    sd = synthetic_model(CONFIG_TINY, device="cpu").state_dict()
    spec = {k: tuple(s) for k, s, _ in state_dict_spec(CONFIG_TINY)}
    assert set(sd) == set(spec)
    for k, s in spec.items():
        assert tuple(sd[k].shape) == s, k


def test_param_groups_and_schedule():
    from oracle import restate
    from oracle.weights import CONFIG_TINY
    from youku_mplug_amd import engine as eng
    from youku_mplug_amd.pretrain import synthetic_model
    model = synthetic_model(CONFIG_TINY, device="cpu")
    groups = eng.get_parameter_groups(model, 0.05, model.no_weight_decay(), visual_backbone_scale=True)
    by_param = {id(p): g for g in groups for p in g["params"]}
    for n, p in model.named_parameters():
        if not p.requires_grad:
            assert id(p) not in by_param
            continue
        gname, scale, decays = restate.param_group_of(n, p.shape)
        g = by_param[id(p)]
        assert g["name"] == gname and g["lr_scale"] == scale and (g["weight_decay"] > 0) == decays, n
    assert by_param[id(model.learnable_queries)]["name"] == "decay"
    assert by_param[id(model.visual_encoder.blocks[0].temporal_attn.q_bias)]["name"] == "no_decay"
    assert by_param[id(model.visual_encoder.pos_embed)]["name"] == "visual_encoder_no_decay"
    s = restate.cosine_schedule(1e-4, 1e-6, 100, 10)
    assert len(s) == 100 and s[0] == 0.0 and abs(s[9] - 1e-4) < 1e-12 and s[-1] > 1e-6 and s[10] == pytest.approx(1e-4)


def test_flat_params_views_and_stages():
    from oracle.weights import CONFIG_TINY
    from youku_mplug_amd import engine as eng
    from youku_mplug_amd.pretrain import synthetic_model
    model = synthetic_model(CONFIG_TINY, device="cpu")
    groups = eng.get_parameter_groups(model, 0.05, model.no_weight_decay(), visual_backbone_scale=True)
    group_of = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    stages = eng.default_stages(model)
    assert [s[0] for s in stages] == ["head", "block1", "block0", "stem"]
    flat = eng.FlatParams(stages, group_of)
    assert flat.numel % eng.TILE == 0
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), before[n])
        if p.requires_grad:
            assert p.data_ptr() % 16 == 0 and p.grad is not None and p.grad.shape == p.shape
            p.grad.fill_(1.0)
    used = sum(p.numel() for p in model.parameters() if p.requires_grad)
    assert flat.grads.float().sum().item() == used
    tg = flat.tile_group
    assert (tg != 255).sum().item() >= used // eng.TILE


def _dp_worker(rank, world, port, q, received):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import engine as eng
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.GELU(), torch.nn.Linear(32, 4))
    stages = [("s0", list(model[2].parameters())), ("s1", list(model[0].parameters()))]
    flat = eng.FlatParams(stages, dtype=torch.float32)
    red = eng.DPReducer(flat)
    g = torch.Generator().manual_seed(100)
    x = torch.randn(8, 16, generator=g)
    y = torch.randn(8, 4, generator=g)
    xs, ys = x[rank * 4:(rank + 1) * 4], y[rank * 4:(rank + 1) * 4]          # DistributedSampler-style shard
    loss = ((model(xs) - ys) ** 2).mean()
    grads = torch.autograd.grad(loss, [p for _, ps in stages for p in ps])
    for p, gr in zip([p for _, ps in stages for p in ps], grads):
        p.grad.copy_(gr)
    red.stage_ready("s0")                  # bucket 0 goes out while "backward" would still be running
    red.finish()
    avg = flat.grads / world
    q.put((rank, avg.clone()))
    received.wait(timeout=300)  # the parent takes the tensors over from this process: stay alive until it has them
    dist.barrier()
    dist.destroy_process_group()


def test_dp_gloo_world2_matches_single_process():
    """N>1 path on CPU: mean of per-rank gradients == gradient of the mean of per-rank losses."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q, received = ctx.Queue(), ctx.Event()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, received)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    received.set()
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.allclose(res[0], res[1])
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.GELU(), torch.nn.Linear(32, 4))
    g = torch.Generator().manual_seed(100)
    x = torch.randn(8, 16, generator=g)
    y = torch.randn(8, 4, generator=g)
    loss = 0.5 * (((model(x[:4]) - y[:4]) ** 2).mean() + ((model(x[4:]) - y[4:]) ** 2).mean())
    loss.backward()
    ref = torch.cat([torch.nn.functional.pad(p.grad.reshape(-1), (0, (-p.numel()) % 256)) for p in
                     list(model[2].parameters()) + list(model[0].parameters())])
    assert torch.allclose(res[0], ref, atol=1e-6)


# ------------------------------------------------------------------------------ retrieval (ITC, config 5)
def test_retrieval_restatement_matches_golden():
    from oracle import restate
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict, retrieval_spec
    g = torch.load(os.path.join(GOLD, "retrieval_tiny.pt"))
    m = g["meta"]
    sd = {k: v.requires_grad_(True) for k, v in make_state_dict(CONFIG_TINY, m["weight_seed"], spec_fn=retrieval_spec).items()}
    video, ids, mask = make_inputs(CONFIG_TINY, m["batch"], m["text_len"], seed=m["input_seed"], ragged=m["ragged"])
    r = restate.retrieval_forward(video, ids, mask, torch.tensor(m["idx"]), sd, CONFIG_TINY)
    assert abs(r["loss"].item() - g["fp32"]["loss"].item()) < 1e-5
    r["loss"].backward()
    for n, gn in g["fp32"]["grad_norm"].items():
        assert abs(sd[n].grad.norm().item() - gn) <= 1e-4 * gn + 1e-9, n


def test_retrieval_state_dict_layout():
    from oracle.weights import CONFIG_TINY, retrieval_spec
    from youku_mplug_amd.retrieval import synthetic_retrieval_model
    model = synthetic_retrieval_model(CONFIG_TINY, device="cpu")
    spec = {k: tuple(s) for k, s, _ in retrieval_spec(CONFIG_TINY)}
    sd = model.state_dict()
    assert set(sd) == set(spec)
    for k, s in spec.items():
        assert tuple(sd[k].shape) == s, k
    unused = {id(p) for p in model.unused_parameters()}
    assert id(model.learnable_queries) in unused and id(model.vision_proj.weight) not in unused


def _itc_worker(rank, world, port, q, received):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd.retrieval import gather_cat, reduce_scatter_sum
    g = torch.Generator().manual_seed(7)
    feats = torch.randn(world * 4, 8, generator=g)
    mine = feats[rank * 4:(rank + 1) * 4].clone()
    allf = gather_cat(mine)
    ids = gather_cat(torch.arange(4) + 4 * rank)
    # every rank forms d(all) = W_r * all ; the true d(mine) is the sum over ranks of their slice for `rank`
    w_r = torch.randn(world * 4, 8, generator=torch.Generator().manual_seed(100 + rank))
    d_mine = reduce_scatter_sum(w_r * allf)
    q.put((rank, allf.clone(), ids.clone(), d_mine.clone()))
    received.wait(timeout=300)  # the parent takes the tensors over from this process: stay alive until it has them
    dist.barrier()
    dist.destroy_process_group()


def test_itc_collectives_gloo_world2():
    """all-gather forward / reduce-scatter backward of the ITC features (models/distributed_utils.py:285-311)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q, received = ctx.Queue(), ctx.Event()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_itc_worker, args=(r, 2, port, q, received)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: (a, i, d) for r, a, i, d in (q.get(timeout=120) for _ in range(2))}
    received.set()
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g = torch.Generator().manual_seed(7)
    feats = torch.randn(8, 8, generator=g)
    for r in (0, 1):
        assert torch.equal(res[r][0], feats) and torch.equal(res[r][1], torch.arange(8))
    w = [torch.randn(8, 8, generator=torch.Generator().manual_seed(100 + r)) for r in (0, 1)]
    total = (w[0] + w[1]) * feats
    for r in (0, 1):
        assert torch.allclose(res[r][2], total[r * 4:(r + 1) * 4], atol=1e-6)


@pytest.mark.parametrize("kind", ["itm", "cls"])
def test_restatement_generation_cls_heads_vs_golden(kind):
    """oracle/restate.py:gencls_forward reproduces the reference modules' ITM / classification goldens
    (both losses, every gradient norm, the train=False scores) in fp32."""
    from oracle import restate
    from oracle.gen_golden import gencls_inputs
    from oracle.weights import CONFIG_TINY, cls_spec, make_state_dict
    g = torch.load(os.path.join(GOLD, f"{kind}_tiny.pt"))["fp32"]
    inp = gencls_inputs(CONFIG_TINY, kind)
    sd = make_state_dict(CONFIG_TINY, 3, spec_fn=lambda c: cls_spec(c, inp["num_classes"]))
    sd = {k: v.clone().requires_grad_(not k.startswith("text_decoder")) for k, v in sd.items()}
    out = restate.gencls_forward(inp["video"], inp["ids"], inp["mask"], inp["plen"].tolist(), inp["p_ids"], inp["p_mask"], inp["labels"],
                                 sd, CONFIG_TINY, negative_indices=inp["neg"], train=True, kind=kind)
    assert abs(out["loss_caption"].item() - g["loss_caption"].item()) < 1e-5
    assert abs(out["loss_cls"].item() - g["loss_cls"].item()) < 1e-5
    (out["loss_caption"] + out["loss_cls"]).backward()
    for n, gn in g["grad_norm"].items():
        assert abs(sd[n].grad.norm().item() - gn) <= 1e-4 * gn + 1e-9, n
    with torch.no_grad():
        ev = restate.gencls_forward(inp["video"], inp["e_ids"], inp["e_mask"], inp["e_plen"].tolist(), inp["e_pids"], inp["e_pmask"], None,
                                    {k: v.detach() for k, v in sd.items()}, CONFIG_TINY, train=False, kind=kind)
    assert (ev["generation_logits"] - g["generation_logits"]).abs().max().item() < 1e-4
    assert (ev["cls_logits"] - g["cls_logits"]).abs().max().item() < 1e-5


def test_restatement_eva_image_model_vs_golden():
    """oracle/restate.py:pretrain_image_forward (EVA encoder blocks) reproduces the reference module's golden in fp32."""
    from oracle import restate
    from oracle.weights import CONFIG_EVA_TINY, eva_spec, make_inputs, make_state_dict
    g = torch.load(os.path.join(GOLD, "eva_tiny.pt"))
    f, m = g["fp32"], g["meta"]
    sd = make_state_dict(CONFIG_EVA_TINY, m["weight_seed"], spec_fn=eva_spec)
    sd = {k: v.clone().requires_grad_(not k.startswith("text_decoder")) for k, v in sd.items()}
    video, ids, mask = make_inputs(CONFIG_EVA_TINY, m["batch"], m["text_len"], seed=m["input_seed"], ragged=True)
    out = restate.pretrain_image_forward(video[:, :, 0], ids, mask, sd, CONFIG_EVA_TINY, prompt_lengths=m["prompt_lengths"])
    assert abs(out["loss"].item() - f["loss"].item()) < 1e-5
    assert (out["logits"][:, :, ::8] - f["logits"]).abs().max().item() < 1e-4
    out["loss"].backward()
    for n, gn in f["grad_norm"].items():
        assert abs(sd[n].grad.norm().item() - gn) <= 1e-4 * gn + 1e-9, n


# ------------------------------------------------------------------------------ generation host logic
# The search loops are driven by oracle/gen_golden.py's StubLogits (deterministic logits as a function of a sequence's token prefix); the
# reference's own DistributedGPT3.beam_search / .sample (models/modeling_distributed_gpt3.py:1620-1873) driven by the same stub wrote
# tests/golden/search_stub.pt (oracle/gen_golden.py:run_search).  The search logic is discrete: it must agree token for token.
class _StubState:
    def __init__(self, stub, batch, max_len):
        self.stub, self.prefix, self.q = stub, None, 0

    def step(self, tokens, query_embeds=None):
        self.q += 0 if query_embeds is None else query_embeds.size(1)          # cached positions that are not token rows
        new = tokens.t().contiguous()
        self.prefix = new if self.prefix is None else torch.cat([self.prefix, new], dim=0)
        return torch.stack([self.stub.row(self.prefix[:, b].tolist()) for b in range(tokens.shape[0])])

    def reorder(self, idx, shared_prefix=0):
        n = shared_prefix - self.q
        assert n >= 0 and (self.prefix[:n] == self.prefix[:n, :1]).all(), "the promised shared prefix is not shared"
        self.prefix = self.prefix[:, idx]


def _torch_topk(logits, k, add):
    lp = torch.log_softmax(logits.float(), dim=-1) + (add.view(-1, 1) if add is not None else 0.0)
    v, i = torch.sort(lp, dim=-1, descending=True, stable=True)
    return v[:, :k], i[:, :k]


@pytest.mark.parametrize("Q", [0, 3])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_beam_search_host_logic_matches_reference(seed, Q):
    """generation.beam_search_loop == the reference's beam_search (same hypotheses bookkeeping, stop-token handling,
    done test, beam re-ordering, final ranking) when both are fed the same logits -- sequences and scores exact."""
    from oracle.gen_golden import BEAM_CASES, StubLogits
    from youku_mplug_amd import generation
    vocab, stub_seed, cfgd, tokens, _, _ = BEAM_CASES[(seed, Q)]
    stub = StubLogits(vocab=vocab, stop=7, seed=stub_seed)
    tokens = torch.tensor(tokens)
    qe = torch.zeros(1, Q, 4) if Q else None
    ref = torch.load(os.path.join(GOLD, "search_stub.pt"))["beam"][(seed, Q)]
    cfg = types.SimpleNamespace(**cfgd, top_k=1, top_p=0.0, vocab_size=stub.vocab)
    out = generation.beam_search_loop(cfg, lambda b, m: _StubState(stub, b, m), tokens.clone(), query_embeds=qe, beam_size=4,
                                      num_return_gen=3, prompt_length=3, topk_fn=_torch_topk)
    assert out.sequences.shape == ref["sequences"].shape
    assert torch.equal(out.sequences, ref["sequences"]), (out.sequences.tolist(), ref["sequences"].tolist())
    assert torch.allclose(out.scores, ref["scores"], atol=1e-5)


@pytest.mark.parametrize("Q", [0, 2])
def test_greedy_sample_host_logic_matches_reference(Q):
    """generation.sample_loop (top_k = 1) == the reference's sample(): ragged prompt lengths, teacher-forced prompt
    tokens until `started`, termination bookkeeping and the returned slice."""
    from oracle.gen_golden import SAMPLE_CASES, StubLogits
    from youku_mplug_amd import generation
    vocab, stub_seed, cfgd, tokens, lengths, _ = SAMPLE_CASES[Q]
    stub = StubLogits(vocab=vocab, stop=7, seed=stub_seed)
    tokens, lengths = torch.tensor(tokens), torch.tensor(lengths)
    qe = torch.zeros(3, Q, 4) if Q else None
    ref = torch.load(os.path.join(GOLD, "search_stub.pt"))["sample"][Q]
    cfg = types.SimpleNamespace(**cfgd, top_k=1, top_p=0.0, vocab_size=stub.vocab)
    import youku_mplug_amd.generation as G
    orig = G.sample_token
    G.sample_token = lambda logits, **kw: torch.argmax(logits, dim=-1)        # greedy without the device kernel
    try:
        out = generation.sample_loop(cfg, lambda b, m: _StubState(stub, b, m), tokens.clone(), query_embeds=qe, prompt_length=lengths.clone())
    finally:
        G.sample_token = orig
    assert torch.equal(out, ref), (out.tolist(), ref.tolist())


def test_video_transform_restatement_and_draws_vs_golden():
    """with the same python-random seed, VideoInputTransform draws the reference's crop
    boxes / flips (RandomResizedCrop.get_params + RandomHorizontalFlip call order) and oracle/video_ref.py's plain-torch
    restatement of crop -> interpolate -> .long() -> flip -> /255 -> normalise reproduces the reference transforms'
    golden outputs exactly (tests/golden/video_tiny.pt, generated from dataset/video_utils by oracle/gen_golden.py)."""
    import random
    from oracle.gen_golden import video_clip
    from oracle.video_ref import restate_video_transform
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd.video_input import CLIP_MEAN, CLIP_STD, VideoInputTransform
    g = torch.load(os.path.join(GOLD, "video_tiny.pt"))
    for (T, H, W, res, train, seed), ref in zip(g["meta"]["cases"], g["out"]):
        clip = video_clip(T, H, W, seed)
        tf = VideoInputTransform(res, train=train)
        random.seed(seed)
        if train:
            box = tf.get_params(H, W)
            flip = random.random() < 0.5
        else:
            box, flip = (0, 0, H, W), False
        out = restate_video_transform(clip, box, (res, res), tf.interpolation, flip, CLIP_MEAN, CLIP_STD)
        assert out.shape == ref.shape and torch.equal(out, ref), (T, H, W, res, train, seed, (out - ref).abs().max().item())


def test_gemm_row_band_plans():
    """Host-side planner of the 256x256 GEMM (csrc/gemm256.hip plan_bands): bands tile the rows exactly once in order,
    every band but the last is made of whole tiles, band tile rows are 256 / 192 / 160, and the shapes the planner exists
    for (a mostly empty last round of workgroups) come out with fewer modelled tile-rounds than the single launch."""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    f = _lib.lib().mpv_gemm_plan_bands
    out = (ctypes.c_int * 6)()
    rel = {256: 1.0, 192: 0.8, 160: 0.73}
    ncu = 256
    cases = [(50432, 768, 768), (50176, 768, 768), (50432, 768, 3072), (50432, 2304, 768), (50432, 3072, 768), (5120, 2048, 2048),
             (5120, 6144, 2048), (5120, 8192, 2048), (1024, 51200, 2048), (256, 256, 64), (300, 264, 320), (1, 256, 64), (70000, 1024, 64)]
    for (M, N, K) in cases:
        for pre, ext in ((0, 0), (1, 0), (0, 1)):
            n = f(M, N, K, ncu, pre, ext, out)
            bands = [(out[2 * i], out[2 * i + 1]) for i in range(n)]
            assert 1 <= n <= 3 and all(r in rel and t > 0 for r, t in bands), (M, N, K, bands)
            covered = 0
            for i, (r, t) in enumerate(bands):
                if i + 1 < n:
                    covered += r * t
                    assert covered < M
                else:
                    assert covered + r * (t - 1) < M <= covered + r * t, (M, N, K, bands)
            tn = (N + 255) // 256
            rounds = lambda r, t: -(-t * tn // ncu) * rel[r]
            assert sum(rounds(r, t) for r, t in bands) <= rounds(256, -(-M // 256)) + 1e-6, (M, N, K, bands)
    n = f(50432, 768, 3072, ncu, 0, 0, out)
    assert n == 3 and [out[0], out[2], out[4]] == [256, 192, 160]


def test_ctypes_struct_layouts_match_the_header(tmp_path):
    """The ctypes mirrors of the C-ABI structs (youku-mplug_amd/_lib.py) against include/mpv.h itself: a C program compiled with gcc prints
    sizeof and the offset of every field of mpv_gemm_epilogue / mpv_attn_desc / mpv_gpt_layer_weights / mpv_gpt_weights; size, field
    order and every offset must equal the ctypes layout.  (A field added to the header and forgotten in _lib.py -- or inserted in the
    middle -- would otherwise only show up on a GPU box, as wrong numbers.)"""
    import re
    import shutil
    import subprocess
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    pairs = [("mpv_gemm_epilogue", _lib.GemmEpilogue), ("mpv_attn_desc", _lib.AttnDesc), ("mpv_gpt_layer_weights", _lib.GptLayerWeights),
             ("mpv_gpt_weights", _lib.GptWeights), ("mpv_attn_plan_info", _lib.AttnPlanInfo)]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpv.h"', 'int main(void) {']
    for cname, ct in pairs:
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(","):
                names.append(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1])
        assert names == [f[0] for f in ct._fields_], (cname, names, [f[0] for f in ct._fields_])
        prog.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for n in names:
            prog.append(f'  printf(" %zu", offsetof({cname}, {n}));')
        prog.append('  printf("\\n");')
    prog += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    for line, (cname, ct) in zip(out, pairs):
        tok = line.split()
        assert tok[0] == cname
        assert int(tok[1]) == ctypes.sizeof(ct), (cname, tok[1], ctypes.sizeof(ct))
        assert [int(x) for x in tok[2:]] == [getattr(ct, f[0]).offset for f in ct._fields_], cname
