"""Decoder LoRA adapters through the HIP pipeline on CONFIG_TINY (H = 256, two layers), r = 8, alpha = 12, random non-zero lora_B:
gradients against the fp32 restatement with W + s B A, the zero-B identity, engine steps, and the merge."""
import math

import pytest
import torch

import lora_model_cases as M

pytestmark = pytest.mark.gpu


def test_gradients_vs_restatement(dev):
    """eval mode (dropout masks are not comparable across implementations): loss within 5e-3, every lora_A / lora_B gradient and the two
    base gradients that pass through the dx1 accumulation within 5e-2 relative L2 of autograd through the restatement"""
    model, sd = M.pretrain_model(dev)
    M.set_adapters(model.text_decoder)
    model.eval()
    assert not model.text_decoder.trainable and model.text_decoder.lora_live()
    video, ids, mask, vid, text = M.inputs(dev)
    loss, _ = model(vid, text)
    loss.backward()
    ref_loss, ref_grads, _ = M.restated(model, sd, video, ids, mask)
    M.check_gradients(model, loss.item(), ref_loss, ref_grads)


def test_zero_b_is_the_unadapted_model(dev):
    """lora_B = 0 (the initial state), dropout live: loss and every non-adapter gradient bit-equal to the un-adapted model's; dA is
    exactly zero, dB is not"""
    video, ids, mask, vid, text = M.inputs(dev)
    got = {}
    for lora in (False, True):
        model, _ = M.pretrain_model(dev, lora=lora)
        model.train()
        loss, _ = model(vid, text)
        loss.backward()
        got[lora] = (loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    (l0, g0), (l1, g1) = got[False], got[True]
    assert torch.equal(l0, l1)
    assert set(g0) == {k for k in g1 if "lora_" not in k}
    for k, g in g0.items():
        assert torch.equal(g, g1[k]), k
    adapters = [k for k in g1 if "lora_" in k]
    assert len(adapters) == 4
    for k in adapters:
        if k.endswith("lora_A"):
            assert not g1[k].float().any(), k
        else:
            assert g1[k].float().abs().max().item() > 0 and torch.isfinite(g1[k].float()).all(), k


def test_engine_steps_move_only_the_adapters(dev):
    from youku_mplug_amd import engine as eng
    model, _ = M.pretrain_model(dev)
    M.set_adapters(model.text_decoder)
    model.train()
    video, ids, mask, vid, text = M.inputs(dev)
    groups = eng.get_parameter_groups(model, 0.05, model.no_weight_decay(), visual_backbone_scale=True)
    e, _, _, _ = eng.initialize(model=model, model_parameters=groups, config=dict(lr=1e-3, clip_grad=3.0))
    dec = {k: p.detach().clone() for k, p in model.text_decoder.named_parameters()}
    flat = {id(p) for p, _, _ in e.flat.slots}
    assert all((id(p) in flat) == ("lora_" in k) for k, p in model.text_decoder.named_parameters())      # adapters, and only they, in the flat buffer
    losses = []
    for _ in range(6):
        l, _ = e(vid, text)
        e.backward(l)
        e.step()
        losses.append(l.item())
    assert all(math.isfinite(x) for x in losses), losses
    for k, p in model.text_decoder.named_parameters():
        if "lora_" in k:
            assert not torch.equal(p.detach(), dec[k]), f"{k} did not move"
        else:
            assert torch.equal(p.detach(), dec[k]), f"base tensor {k} changed"


def test_merge(dev):
    """merged loss within 5e-3 of the restatement; unmerge restores bit for bit; a fresh un-adapted model loaded from merged_state_dict()
    IS the merged model (logits and batched beam-search tokens bit-identical); FP8 decode weights are cleared by a merge"""
    from oracle.weights import CONFIG_TINY as cfg
    model, sd = M.pretrain_model(dev)
    gpt = model.text_decoder
    M.set_adapters(gpt)
    model.eval()
    video, ids, mask, vid, text = M.inputs(dev)
    ref_loss, _, _ = M.restated(model, sd, video, ids, mask)
    before = [lin.weight.detach().clone() for lin in gpt._qkv_linears()]
    with pytest.raises(RuntimeError, match="merge_lora"):
        gpt.quantize_decode_weights()
    gpt.merge_lora()
    assert not gpt.lora_live() and any(not torch.equal(w, lin.weight) for w, lin in zip(before, gpt._qkv_linears()))
    gpt.quantize_decode_weights()
    assert "_decode_weights_q8" in gpt.__dict__
    with torch.no_grad():
        out_m = model.forward_outputs(vid, text)
    assert abs(out_m.loss.item() - ref_loss) <= 5e-3 * abs(ref_loss), (out_m.loss.item(), ref_loss)
    qf = torch.randn((2, cfg.num_queries, cfg.hidden), generator=torch.Generator().manual_seed(3)).to(dev).to(torch.bfloat16) * 0.5
    prompt = ids[:2, :3].to(dev).contiguous()
    gpt.config.extra["tokens_to_generate"] = 6
    beams_m = gpt.beam_search_batched(prompt, query_embeds=qf, beam_size=3)
    gpt.unmerge_lora()
    assert "_decode_weights_q8" not in gpt.__dict__                         # stale codes of the merged weights are gone
    assert gpt.lora_live() and all(torch.equal(w, lin.weight) for w, lin in zip(before, gpt._qkv_linears()))
    merged_sd = gpt.merged_state_dict()
    assert all(torch.equal(w, lin.weight) for w, lin in zip(before, gpt._qkv_linears())) and not any("lora_" in k for k in merged_sd)
    fresh, _ = M.pretrain_model(dev, lora=False)
    fresh.eval()
    fresh.text_decoder.load_state_dict(merged_sd, strict=True)
    with torch.no_grad():
        out_f = fresh.forward_outputs(vid, text)
    assert torch.equal(out_f.logits, out_m.logits)
    fresh.text_decoder.config.extra["tokens_to_generate"] = 6
    beams_f = fresh.text_decoder.beam_search_batched(prompt, query_embeds=qf, beam_size=3)
    assert len(beams_f) == len(beams_m) == 2
    for a, b in zip(beams_f, beams_m):
        assert torch.equal(a.sequences, b.sequences) and a.sequences.shape[1] > prompt.shape[1]


def test_generate_and_score_captions_refuse_live_adapters(dev):
    import caption_score_cases as cs
    model, cfg, g, sd, video, ids, mask = cs.tiny_caption_model(dev)
    model.text_decoder.add_lora(M.RANK, M.ALPHA)
    M.set_adapters(model.text_decoder)
    term = g["meta"]["eod_id"]
    text = cs.text_of(ids, mask, [0, 1], dev)
    vid = video[[0, 1]].to(dev).to(torch.bfloat16)
    cands = cs.ragged_candidates(cfg, [2, 1], seed=21, avoid=term)
    with pytest.raises(RuntimeError, match="merge_lora"):
        model.generate(vid, text, termination_id=term)
    with pytest.raises(RuntimeError, match="merge_lora"):
        model.score_captions(vid, text, cands, termination_id=term)
    with model.text_decoder.lora_merged():
        res = model.score_captions(vid, text, cands, termination_id=term)
        model.generate(vid, text, termination_id=term)
    assert len(res) == 2 and model.text_decoder.lora_live()
