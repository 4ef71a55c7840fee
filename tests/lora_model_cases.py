"""Shared pieces of the LoRA model tests (tests/test_lora_model_gpu.py on the device, tests/test_lora_cpu.py on the stand-ins), TEST
INFRASTRUCTURE ONLY: the adapted tiny pre-train model with non-zero adapters, and its reference -- oracle.restate.pretrain_forward with
every layer's qkv weight replaced by the autograd expression W + s B A of leaf A, B (restate.gpt_layer uses the entry as given)."""
import types

import torch

RANK, ALPHA = 8, 12.0
SCALE = ALPHA / RANK
BASE_KEYS = ("visual_fc.weight", "visual_encoder.blocks.0.attn.qkv.weight")      # gradients that pass through the dx1 accumulation
QKV = "text_decoder.dist_model.language_model.encoder.layers.{}.self_attention.query_key_value."


def rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def pretrain_model(dev, *, lora=True, weight_seed=17, config=None):
    """-> (model, fp32 state dict it was loaded from): CONFIG_TINY, frozen decoder, adapters by the config keys"""
    from oracle.weights import CONFIG_TINY as cfg, make_state_dict
    from youku_mplug_amd.gpt3 import GPT3Config
    from youku_mplug_amd.pretrain import DistributedGPT3_Pretrain
    vis = dict(img_size=cfg.img_size, patch_size=cfg.patch_size, depth=cfg.vit_depth, num_frames=cfg.num_frames, embed_dim=cfg.vit_dim,
               num_heads=cfg.vit_heads, mlp_ratio=cfg.vit_mlp_ratio, clip_model=True)
    txt = GPT3Config(vocab_size=cfg.vocab, hidden_size=cfg.hidden, ffn_hidden_size=cfg.ffn, num_hidden_layers=cfg.layers,
                     num_attention_heads=cfg.heads, max_position_embeddings=cfg.max_pos, layernorm_epsilon=cfg.gpt_ln_eps)
    c = {"num_learnable_token": cfg.num_queries, "_synthetic": True}
    if lora:
        c.update(lora_rank=RANK, lora_alpha=ALPHA)
    c.update(config or {})
    model = DistributedGPT3_Pretrain(c, visual_cfg=vis, text_cfg=txt, device=dev)
    sd = make_state_dict(cfg, weight_seed)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)      # a BASE checkpoint, strict
    return model, sd


def set_adapters(decoder, seed=5, b_std=0.05):
    """seeded lora_A (std 0.02) and NON-ZERO lora_B on every layer"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for lin in decoder._qkv_linears():
            lin.lora_A.copy_((torch.randn(lin.lora_A.shape, generator=g) * 0.02).to(lin.lora_A.dtype))
            lin.lora_B.copy_((torch.randn(lin.lora_B.shape, generator=g) * b_std).to(lin.lora_B.dtype))


def inputs(dev, batch=3, text_len=10, seed=23):
    from oracle.weights import CONFIG_TINY, make_inputs
    video, ids, mask = make_inputs(CONFIG_TINY, batch, text_len, seed=seed, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    return video, ids, mask, video.to(dev).to(torch.bfloat16), text


def restated(model, sd, video, ids, mask, scale=SCALE):
    """-> (loss, {parameter name of the model: reference gradient}) of the fp32 restatement on the model's bf16 weights, adapters as
    W + s B A.  Names: the adapters' own, and BASE_KEYS."""
    from oracle import restate
    from oracle.weights import CONFIG_TINY as cfg
    sdr = {k: v.bfloat16().float() for k, v in sd.items()}
    for k in BASE_KEYS:
        sdr[k].requires_grad_(True)
    leaves = {}
    for i, lin in enumerate(model.text_decoder._qkv_linears()):
        A = lin.lora_A.detach().float().cpu().requires_grad_(True)
        B = lin.lora_B.detach().float().cpu().requires_grad_(True)
        leaves[QKV.format(i) + "lora_A"], leaves[QKV.format(i) + "lora_B"] = A, B
        sdr[QKV.format(i) + "weight"] = sdr[QKV.format(i) + "weight"] + scale * (B @ A)
    ref = restate.pretrain_forward(video.bfloat16().float(), ids, mask, sdr, cfg)
    ref["loss"].backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads.update({k: sdr[k].grad for k in BASE_KEYS})
    return ref["loss"].item(), grads, ref


def check_gradients(model, loss, ref_loss, ref_grads):
    """the gates of test_trainable_decoder_vs_restatement: loss 5e-3 relative, gradients 5e-2 relative L2"""
    assert abs(loss - ref_loss) <= 5e-3 * abs(ref_loss), (loss, ref_loss)
    params = dict(model.named_parameters())
    bad = []
    for k, gr in ref_grads.items():
        assert params[k].grad is not None and gr is not None, k
        e = rel_l2(params[k].grad, gr)
        print(f"    grad {k}: relative L2 {e:.3e}")
        if not e <= 5e-2:
            bad.append((k, e))
    assert not bad, bad
