"""The contrastive head of the pre-train model (use_contrastive) without a GPU: the real host pipeline on the stand-ins of
tests/standin_contrastive.py (+ tests/standin_ops.py) against the reference-module goldens, on one process and on two gloo ranks;
the module contract (state dict, parameter groups, refusals) against the reference where it is available; and the golden generator
(tools/gen_golden_contrastive.py) against the committed goldens."""
import os
import subprocess
import sys

import pytest
import torch

import standin_contrastive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_available():
    from oracle.ref_loader import reference_available
    return reference_available()


def _on_cpu(monkeypatch):
    standin_contrastive.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()
    return torch.device("cpu")


def _model(**kw):
    from oracle.weights import CONFIG_TINY
    from youku_mplug_amd.pretrain import synthetic_model
    return synthetic_model(CONFIG_TINY, device="cpu", **kw)


def test_contrastive_pipeline_on_standins_vs_reference_golden(monkeypatch):
    """the GPU test's golden comparison (both losses, every gradient, the head element-wise) with the host pipeline on the stand-ins"""
    import test_contrastive_gpu as t
    t.test_contrastive_model_vs_reference_golden(_on_cpu(monkeypatch))


def test_contrastive_world2_gloo_on_standins_vs_reference_golden():
    """two gloo ranks (CPU processes) on the stand-ins against tests/golden/contrastive_tiny_world2.pt: all-gather in the forward,
    targets offset by rank * B, reduce-scatter of the gathered halves' gradients"""
    import test_contrastive_gpu as t
    t.check_world2(t.run_world2("cpu", standins=True))


def test_state_dict_matches_retrieval_spec_and_reference():
    from oracle.weights import CONFIG_TINY, retrieval_spec, state_dict_spec
    model = _model(use_contrastive=True, temp=0.05)
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert mine == {k: tuple(s) for k, s, _ in retrieval_spec(CONFIG_TINY)}
    assert model.temp.dtype == torch.bfloat16 and model.temp.dim() == 0 and model.temp.item() == pytest.approx(0.05, rel=1e-2)
    off = _model()
    assert not off.use_contrastive and {k: tuple(v.shape) for k, v in off.state_dict().items()} == {k: tuple(s) for k, s, _ in state_dict_spec(CONFIG_TINY)}
    if not _reference_available():
        return
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_golden_contrastive import build_reference_contrastive
    ref, _ = build_reference_contrastive(CONFIG_TINY, 0)
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == mine


def test_contrastive_embed_dim_key_and_yaml_embed_dim_ignored():
    from oracle.weights import CONFIG_TINY
    from youku_mplug_amd.gpt3 import GPT3Config
    from youku_mplug_amd.pretrain import DistributedGPT3_Pretrain
    s = CONFIG_TINY
    vis = dict(img_size=s.img_size, patch_size=s.patch_size, depth=s.vit_depth, num_frames=s.num_frames, embed_dim=s.vit_dim,
               num_heads=s.vit_heads, mlp_ratio=s.vit_mlp_ratio, clip_model=True)
    txt = GPT3Config(vocab_size=s.vocab, hidden_size=s.hidden, ffn_hidden_size=s.ffn, num_hidden_layers=s.layers,
                     num_attention_heads=s.heads, max_position_embeddings=s.max_pos, layernorm_epsilon=s.gpt_ln_eps)
    base = {"num_learnable_token": s.num_queries, "_synthetic": True, "use_contrastive": True, "embed_dim": 128}
    m = DistributedGPT3_Pretrain(base, visual_cfg=vis, text_cfg=txt, device="cpu")
    assert m.vision_proj.out_features == 256 and m.text_proj.out_features == 256
    m = DistributedGPT3_Pretrain(dict(base, contrastive_embed_dim=64), visual_cfg=vis, text_cfg=txt, device="cpu")
    assert m.vision_proj.weight.shape == (64, s.vit_dim) and m.text_proj.weight.shape == (64, s.hidden)


def test_parameter_groups_temp_decays_biases_do_not():
    """optim_factory.py:219-265 as restated by engine.get_parameter_groups: the 0-d temp lands in the DECAY group (len(shape) != 1, as
    in the reference), the projection biases in no-decay -- pinned, and compared with the reference's own function where available"""
    from youku_mplug_amd import engine as eng
    model = _model(use_contrastive=True)
    groups = eng.get_parameter_groups(model, 0.05, model.no_weight_decay(), visual_backbone_scale=True)
    where = {id(p): g["name"] for g in groups for p in g["params"]}
    assert where[id(model.temp)] == "decay"
    assert where[id(model.vision_proj.weight)] == where[id(model.text_proj.weight)] == "decay"
    assert where[id(model.vision_proj.bias)] == where[id(model.text_proj.bias)] == "no_decay"
    if not _reference_available():
        return
    from oracle import ref_loader
    ref_loader.import_reference()
    try:
        from optim import optim_factory
    except ImportError as e:
        pytest.skip(f"reference optim package not importable here: {e}")
    ref_groups = optim_factory.get_parameter_groups(model, 0.05, model.no_weight_decay())
    rw = {}
    for g in ref_groups:
        for p in g["params"]:
            rw[id(p)] = g["weight_decay"]
    for g in groups:
        for p in g["params"]:
            assert rw[id(p)] == g["weight_decay"]


def test_refusals_and_gencls_builds_no_head():
    from oracle.weights import CONFIG_TINY, CONFIG_EVA_TINY
    from youku_mplug_amd.downstream import synthetic_gencls_model
    from youku_mplug_amd.gpt3 import GPT3Config
    from youku_mplug_amd.pretrain import DistributedGPT3_Pretrain, DistributedGPT3_Pretrain_Image
    s = CONFIG_TINY
    vis = dict(img_size=s.img_size, patch_size=s.patch_size, depth=s.vit_depth, num_frames=s.num_frames, embed_dim=s.vit_dim,
               num_heads=s.vit_heads, mlp_ratio=s.vit_mlp_ratio, clip_model=True)
    txt = GPT3Config(vocab_size=s.vocab, hidden_size=s.hidden, ffn_hidden_size=s.ffn, num_hidden_layers=s.layers,
                     num_attention_heads=s.heads, max_position_embeddings=s.max_pos, layernorm_epsilon=s.gpt_ln_eps)
    with pytest.raises(NotImplementedError, match="freeze_text_decoder"):
        DistributedGPT3_Pretrain({"num_learnable_token": s.num_queries, "_synthetic": True, "use_contrastive": True,
                                  "freeze_text_decoder": False}, visual_cfg=vis, text_cfg=txt, device="cpu")
    e = CONFIG_EVA_TINY
    evis = dict(img_size=e.img_size, num_frames=1, embed_dim=e.vit_dim, num_heads=e.vit_heads, mlp_ratio=e.vit_mlp_ratio,
                depth=e.vit_depth, patch_size=e.patch_size)
    with pytest.raises(NotImplementedError, match="DistributedGPT3_Pretrain only"):
        DistributedGPT3_Pretrain_Image({"num_learnable_token": e.num_queries, "_synthetic": True, "use_eva_g": True,
                                        "use_contrastive": True}, visual_cfg=evis, text_cfg=txt, device="cpu")
    for kind in ("itm", "cls"):
        m = synthetic_gencls_model(CONFIG_TINY, kind, device="cpu")
        assert not m.use_contrastive and not hasattr(m, "vision_proj")
        from youku_mplug_amd import downstream
        cls = type(m)
        m2 = cls({"num_learnable_token": s.num_queries, "_synthetic": True, "use_contrastive": True},
                 visual_cfg=vis, text_cfg=txt, device="cpu")
        assert not m2.use_contrastive and not any(k.startswith(("vision_proj", "text_proj", "temp")) for k in m2.state_dict())
        assert downstream is not None


def test_contrastive_off_returns_a_detached_zero(monkeypatch):
    """the default model is unchanged: (loss_caption, zero) with the zero outside autograd, as before"""
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict
    import types
    _on_cpu(monkeypatch)
    model = _model()
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in make_state_dict(CONFIG_TINY, 0).items()})
    model.eval()
    video, ids, mask = make_inputs(CONFIG_TINY, 2, 8, seed=1, ragged=True)
    lc, li = model(video.to(torch.bfloat16), types.SimpleNamespace(input_ids=ids, attention_mask=mask))
    assert lc.requires_grad and not li.requires_grad and li.item() == 0.0 and li.dim() == 0


def test_generator_reproduces_committed_goldens():
    if not _reference_available():
        pytest.skip("reference tree not found")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_contrastive.py"), "--check"], capture_output=True,
                       text=True, timeout=900, cwd=ROOT, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("matches") == 2
