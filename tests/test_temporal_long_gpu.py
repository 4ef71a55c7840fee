"""Temporal attention for clips of 17..64 frames (csrc/attention_temporal_long.inc, mpv_temporal_attn_long_fwd / _bwd) on the GPU:
the kernel against fp32 torch at the gates of tests/test_kernels_gpu.py::test_temporal_attention (out 1.5e-2, dq / dk / dv 3e-2,
max-abs error / max-abs reference), with every row the kernel does not own -- the cls rows between the sequences and 64 canary
rows behind the tensors -- compared bit for bit; the refusals; and the pre-train model end to end at 24 and 33 frames against
the fp32 restatement at the gates of tests/test_model_gpu.py and the README's whole-tensor relative-L2 gradient gate (3e-2)."""
import dataclasses
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL = 1.5e-2, 3e-2      # test_kernels_gpu.py::test_temporal_attention
CANARY = 64


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def close(a, b, tol, what=""):
    e = rel_err(a, b)
    print(f"    {what}: {e:.3e} <= {tol:.1e}")
    assert math.isfinite(e) and e <= tol, f"{what}: max-abs error / max-abs ref = {e:.3e} > {tol}"
    return e


def rn(*shape, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)


def bits(t):
    return t.contiguous().view(torch.int16)


def long_fwd(qkv, out, *a):
    from youku_mplug_amd import _lib, ops
    _lib.check(_lib.lib().mpv_temporal_attn_long_fwd(qkv.data_ptr(), out.data_ptr(), *a, ops._stream()), "mpv_temporal_attn_long_fwd")


def long_bwd(qkv, dout, dqkv, *a):
    from youku_mplug_amd import _lib, ops
    _lib.check(_lib.lib().mpv_temporal_attn_long_bwd(qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), *a, ops._stream()),
               "mpv_temporal_attn_long_bwd")


def run_kernel_case(dev, B, N, heads, hd, T, fwd, bwd, what):
    """The layout of test_temporal_attention: qkv [B*T*N1, 3D], sequence (b, n) has token t at row b*T*N1 + 1 + n + t*N1 (row
    b*T*N1 + t*N1 is a cls row no temporal problem owns).  qkv has exactly its rows (row T of the last sequence lies behind the
    allocation); out, dout and dqkv carry CANARY pre-filled rows more.  Returns the four errors."""
    D, N1 = heads * hd, N + 1
    R = B * T * N1
    scale = hd ** -0.5
    qkv = rn(R, 3 * D, dev=dev, seed=50)
    out_all = rn(R + CANARY, D, dev=dev, seed=52)                      # pre-fill: nothing the kernel skips may change
    out0 = out_all.clone()
    fwd(qkv, out_all, B, T * N1, N, 1, N1, T, heads, hd, scale)
    out = out_all[:R]
    x = qkv.view(B, T, N1, 3, heads, hd)[:, :, 1:]                    # [B,T,N,3,h,d]
    q, k, v = (x[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))  # [B,N,h,T,d]
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    ref = ((qr * scale) @ kr.transpose(-1, -2)).softmax(-1) @ vr
    errs = {"out": close(out.view(B, T, N1, heads, hd)[:, :, 1:].permute(0, 2, 3, 1, 4), ref, OUT_TOL, f"{what} out")}
    assert torch.equal(bits(out_all[R:]), bits(out0[R:])), f"{what}: forward wrote behind the last row"
    assert torch.equal(bits(out.view(B, T, N1, D)[:, :, 0]), bits(out0[:R].view(B, T, N1, D)[:, :, 0])), f"{what}: forward wrote a cls row"
    dout_all = rn(R + CANARY, D, dev=dev, seed=51)
    dout0 = dout_all.clone()
    dqkv_all = rn(R + CANARY, 3 * D, dev=dev, seed=53)
    dqkv0 = dqkv_all.clone()
    bwd(qkv, dout_all, dqkv_all, B, T * N1, N, 1, N1, T, heads, hd, scale)
    ref.backward(dout_all[:R].view(B, T, N1, heads, hd)[:, :, 1:].permute(0, 2, 3, 1, 4).float())
    g = dqkv_all[:R].view(B, T, N1, 3, heads, hd)[:, :, 1:]
    for i, (name, r) in enumerate((("dq", qr), ("dk", kr), ("dv", vr))):
        errs[name] = close(g[:, :, :, i].permute(0, 2, 3, 1, 4), r.grad, GRAD_TOL, f"{what} {name}")
    assert torch.equal(bits(dout_all), bits(dout0)), f"{what}: backward wrote dout"
    assert torch.equal(bits(dqkv_all[R:]), bits(dqkv0[R:])), f"{what}: backward wrote behind the last row"
    assert torch.equal(bits(dqkv_all[:R].view(B, T, N1, 3 * D)[:, :, 0]), bits(dqkv0[:R].view(B, T, N1, 3 * D)[:, :, 0])), \
        f"{what}: backward wrote a cls row"
    assert torch.isfinite(dqkv_all.float()).all()
    return errs


# one row into the second 16-block, inside the tile, the exact tile, one over the tile, inside the second tile pair, the maximum
@pytest.mark.parametrize("B,N,heads", [(2, 6, 2), (1, 5, 3)])         # (1, 5, 3): 15 problems, the last 4-wave workgroup is ragged
@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("T", [17, 24, 32, 33, 48, 64])
def test_long_kernel_vs_fp32_torch(dev, T, hd, B, N, heads):
    from youku_mplug_amd import ops
    assert T > ops.TEMPORAL_SHORT_MAX_T                                 # ops.temporal_attn_* take the new entry points here
    run_kernel_case(dev, B, N, heads, hd, T, ops.temporal_attn_fwd, ops.temporal_attn_bwd, f"T={T} hd={hd} B={B} N={N} h={heads}")


def test_long_kernel_true_dims_addressing(dev):
    """ViT-B/16 addressing: 196 patches + cls per frame, 8 heads of 96, one clip of 32 frames (1568 problems)."""
    from youku_mplug_amd import ops
    run_kernel_case(dev, 1, 196, 8, 96, 32, ops.temporal_attn_fwd, ops.temporal_attn_bwd, "true dims T=32")


@pytest.mark.parametrize("T", [8, 16])
def test_long_entry_points_compute_the_old_family_function(dev, T):
    """mpv_temporal_attn_long_* accept 1 <= T <= 64: at 8 and 16 frames, on the inputs of test_temporal_attention, they meet the
    same gates as the kernels that serve those lengths.  The printed ratio (new max error / old max error) is recorded in DESIGN
    section 15."""
    from youku_mplug_amd import ops
    new = run_kernel_case(dev, 2, 6, 2, 96, T, long_fwd, long_bwd, f"long entry T={T}")
    old = run_kernel_case(dev, 2, 6, 2, 96, T, ops.temporal_attn_fwd, ops.temporal_attn_bwd, f"short entry T={T}")
    for k in ("out", "dq", "dk", "dv"):
        print(f"    T={T} {k}: long / short max-error ratio {new[k] / max(old[k], 1e-12):.2f} ({new[k]:.3e} / {old[k]:.3e})")


def test_long_entry_points_refuse(dev):
    from youku_mplug_amd import _lib, ops
    lib = _lib.lib()
    B, N, heads, hd, T = 1, 2, 2, 96, 24
    D, N1 = heads * hd, N + 1
    R = B * T * N1
    qkv, dout = rn(R, 3 * D, dev=dev, seed=1), rn(R, D, dev=dev, seed=2)
    out, dqkv = rn(R, D, dev=dev, seed=3), rn(R, 3 * D, dev=dev, seed=4)
    out0, dqkv0 = out.clone(), dqkv.clone()
    st = ops._stream()

    def fwd(T=T, hd=hd, qkv_p=qkv.data_ptr(), out_p=out.data_ptr(), B=B):
        return lib.mpv_temporal_attn_long_fwd(qkv_p, out_p, B, T * N1, N, 1, N1, T, heads, hd, hd ** -0.5, st)

    def bwd(T=T, hd=hd, qkv_p=qkv.data_ptr(), dout_p=dout.data_ptr(), dqkv_p=dqkv.data_ptr(), B=B):
        return lib.mpv_temporal_attn_long_bwd(qkv_p, dout_p, dqkv_p, B, T * N1, N, 1, N1, T, heads, hd, hd ** -0.5, st)

    for kw in (dict(T=0), dict(T=65), dict(hd=88), dict(hd=112), dict(B=0), dict(qkv_p=None), dict(out_p=None)):
        assert fwd(**kw) != 0, kw
        assert b"mpv_temporal_attn_long_fwd" in lib.mpv_last_error(), (kw, lib.mpv_last_error())
    for kw in (dict(T=0), dict(T=65), dict(hd=88), dict(hd=112), dict(B=0), dict(qkv_p=None), dict(dout_p=None), dict(dqkv_p=None)):
        assert bwd(**kw) != 0, kw
        assert b"mpv_temporal_attn_long_bwd" in lib.mpv_last_error(), (kw, lib.mpv_last_error())
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(out0)) and torch.equal(bits(dqkv), bits(dqkv0)), "a refused call launched something"
    with pytest.raises(ValueError, match="64"):
        ops.temporal_attn_fwd(qkv, out, B, 65 * N1, N, 1, N1, 65, heads, hd, hd ** -0.5)
    with pytest.raises(ValueError, match="64"):
        ops.temporal_attn_bwd(qkv, dout, dqkv, B, 65 * N1, N, 1, N1, 65, heads, hd, hd ** -0.5)
    assert fwd() == 0 and bwd() == 0                                    # the same calls, unmodified, are accepted
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ the model, end to end
def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def check_model_against_restatement(model, sd, cfg, dev, what):
    """test_model_gpu.py::test_config_d_dims_vs_restatement with every trainable tensor: loss within 1e-2 relative, logits within
    2e-2, every gradient within the README's whole-tensor relative-L2 gate of 3e-2, against the fp32 restatement on the
    bf16-rounded weights."""
    from oracle import restate
    from oracle.weights import make_inputs
    video, ids, mask = make_inputs(cfg, 2, 12, seed=9, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    model.eval()
    out = model.forward_outputs(video.to(dev).to(torch.bfloat16), text)
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert any(n.startswith("visual_encoder.") for n in trainable), trainable[:5]
    sdr = {k: v.bfloat16().float() for k, v in sd.items()}
    for k in trainable:
        sdr[k].requires_grad_(True)
    ref = restate.pretrain_forward(video.bfloat16().float(), ids, mask, sdr, cfg)
    e_loss = abs(out.loss.item() - ref["loss"].item()) / abs(ref["loss"].item())
    e_logits = rel(out.logits, ref["logits"].detach())
    print(f"    [{what}] loss {e_loss:.3e} <= 1e-2, logits {e_logits:.3e} <= 2e-2")
    assert e_loss <= 1e-2, (out.loss.item(), ref["loss"].item())
    assert e_logits <= 2e-2
    ref["loss"].backward()
    loss, _ = model(video.to(dev).to(torch.bfloat16), text)
    loss.backward()
    torch.cuda.synchronize()
    worst = (0.0, "")
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None and sdr[n].grad is not None, n
        g, r = p.grad.float().cpu(), sdr[n].grad
        worst = max(worst, (((g - r).norm() / (r.norm() + 1e-30)).item(), n))
    print(f"    [{what}] worst whole-tensor relative-L2 gradient distance {worst[0]:.3e} at {worst[1]} <= 3e-2 ({len(trainable)} tensors)")
    assert worst[0] <= 3e-2, worst


def build(cfg, dev, wseed):
    from oracle.weights import make_state_dict
    from youku_mplug_amd.pretrain import synthetic_model
    model = synthetic_model(cfg, device=dev)
    sd = make_state_dict(cfg, wseed)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    return model, sd


@pytest.mark.parametrize("frames", [24, 33])
def test_long_clip_model_vs_restatement(dev, frames):
    from oracle.weights import CONFIG_TINY
    cfg = dataclasses.replace(CONFIG_TINY, num_frames=frames)
    model, sd = build(cfg, dev, 5)
    assert model.visual_encoder.temporal_embed.shape[1] == frames
    check_model_against_restatement(model, sd, cfg, dev, f"tiny, {frames} frames")


def test_checkpoint_with_a_shorter_clip_length(dev):
    """A 4-frame checkpoint loaded into the 24-frame model: temporal_embed goes through resize_temporal_embed (what every downstream
    --resume does), and the model then computes the restatement's function on the interpolated table."""
    from oracle.weights import CONFIG_TINY, make_state_dict
    from youku_mplug_amd.pretrain import synthetic_model
    from youku_mplug_amd.vision import resize_visual_embeds_in_state_dict
    cfg = dataclasses.replace(CONFIG_TINY, num_frames=24)
    sd = make_state_dict(cfg, 5)
    key = "visual_encoder.temporal_embed"
    short = make_state_dict(CONFIG_TINY, 6)[key]
    assert short.shape[1] == 4 and short.abs().max() > 0
    ckpt = {k: v.to(torch.bfloat16) for k, v in sd.items()}
    ckpt[key] = short.to(torch.bfloat16)
    model = synthetic_model(cfg, device=dev)
    ckpt = resize_visual_embeds_in_state_dict(ckpt, model)
    assert ckpt[key].shape == (1, 24, cfg.vit_dim)
    expect = torch.nn.functional.interpolate(short.to(torch.bfloat16).float().permute(0, 2, 1), 24, mode="linear").permute(0, 2, 1)
    assert torch.equal(ckpt[key].float(), expect.to(torch.bfloat16).float())
    model.load_state_dict(ckpt, strict=True)
    sd_ref = dict(sd)
    sd_ref[key] = ckpt[key].float()
    check_model_against_restatement(model, sd_ref, cfg, dev, "24 frames from a 4-frame checkpoint")


def test_32_frame_models_build_and_step(dev):
    """pretrain.synthetic_model(..., num_frames=32) takes a full training step (forward, backward, AdamW); the retrieval and the
    classification constructors build at 32 frames and run: the retrieval features against the restatement (the bound of
    test_model_gpu.py::test_retrieval_itc_vs_reference_golden), both downstream losses finite with gradients on the vision tower."""
    from oracle import restate
    from oracle.gen_golden import gencls_inputs
    from oracle.weights import CONFIG_TINY, cls_spec, make_inputs, make_state_dict, retrieval_spec
    from youku_mplug_amd import engine as eng
    from youku_mplug_amd.downstream import synthetic_gencls_model
    from youku_mplug_amd.pretrain import synthetic_model
    from youku_mplug_amd.retrieval import synthetic_retrieval_model
    cfg = dataclasses.replace(CONFIG_TINY, num_frames=32)
    # pre-train: one optimizer step
    model = synthetic_model(CONFIG_TINY, device=dev, num_frames=32)
    sd = make_state_dict(cfg, 3)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    video, ids, mask = make_inputs(cfg, 2, 8, seed=4, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    model.train()
    groups = eng.get_parameter_groups(model, 0.05, model.no_weight_decay(), visual_backbone_scale=True)
    e, _, _, _ = eng.initialize(model=model, model_parameters=groups, config=dict(lr=1e-4, clip_grad=3.0))
    before = model.visual_encoder.blocks[0].temporal_attn.qkv.weight.detach().float().clone()
    loss, _ = e(video.to(dev).to(torch.bfloat16), text)
    e.backward(loss)
    e.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    after = model.visual_encoder.blocks[0].temporal_attn.qkv.weight.detach().float()
    assert torch.isfinite(after).all() and not torch.equal(before, after), "the step did not move the temporal attention's weights"
    # retrieval (ITC)
    rmodel = synthetic_retrieval_model(CONFIG_TINY, device=dev, num_frames=32)
    rsd = make_state_dict(cfg, 5, spec_fn=retrieval_spec)
    rmodel.load_state_dict({k: v.to(torch.bfloat16) for k, v in rsd.items()}, strict=True)
    rmodel.eval()
    video, ids, mask = make_inputs(cfg, 8, 8, seed=6, ragged=True)      # (the similarity products take batches of 8)
    idx = torch.arange(8)
    text = types.SimpleNamespace(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    rloss = rmodel(video.to(dev).to(torch.bfloat16), text, idx.to(dev))
    rloss.backward()
    ref = restate.retrieval_forward(video, ids, mask, idx, {k: v.bfloat16().float() for k, v in rsd.items()}, cfg)
    vf = rmodel.extract_vision_feature(video.to(dev).to(torch.bfloat16))
    assert torch.isfinite(rloss).item() and rel(vf, ref["vision_feats"]) < 2e-2
    # classification head
    inp = gencls_inputs(cfg, "cls")
    cmodel = synthetic_gencls_model(CONFIG_TINY, "cls", num_classes=inp["num_classes"], device=dev, num_frames=32)
    csd = make_state_dict(cfg, 7, spec_fn=lambda c: cls_spec(c, inp["num_classes"]))
    cmodel.load_state_dict({k: v.to(torch.bfloat16) for k, v in csd.items()}, strict=True)
    cmodel.eval()
    d = lambda t: t.to(dev)
    text = types.SimpleNamespace(input_ids=d(inp["ids"]), attention_mask=d(inp["mask"]), prompt_lengths=inp["plen"])
    ptext = types.SimpleNamespace(input_ids=d(inp["p_ids"]), attention_mask=d(inp["p_mask"]))
    lc, lk = cmodel(d(inp["video"]).to(torch.bfloat16), text, ptext, d(inp["labels"]))
    (lc + lk).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(lc).item() and torch.isfinite(lk).item()
    g = cmodel.visual_encoder.blocks[0].temporal_attn.qkv.weight.grad
    assert g is not None and torch.isfinite(g.float()).all() and g.abs().max().item() > 0
