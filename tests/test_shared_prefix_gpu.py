"""Shared-prefix scoring of the ITM / category heads on the GPU (downstream._GenCls.score_shared_prefix: gpt3 forward_prefix +
forward_continuation on mpv_attn_prefix_fwd) against the reference-module goldens and against the existing train=False path."""
import dataclasses
import os
import types

import pytest
import torch

from test_model_gpu import GOLD, plain_gate, rel

pytestmark = pytest.mark.gpu
TOL = 1e-2


def _agree(mine, base, what, tol=TOL):
    """relative L2 <= tol, and the same argmax wherever the existing path's top two scores differ by more than that tolerance"""
    mine, base = mine.float().cpu(), base.float().cpu()
    e = ((mine - base).norm() / base.norm()).item()
    assert e <= tol, (what, e)
    top = base.topk(2, dim=-1).values
    clear = (top[:, 0] - top[:, 1]) > tol * base.abs().max()
    assert torch.equal(mine.argmax(-1)[clear], base.argmax(-1)[clear]), what
    return e


def _load(dev, kind, cfg, inp, seed):
    from oracle.weights import cls_spec, make_state_dict
    from youku_mplug_amd.downstream import synthetic_gencls_model
    model = synthetic_gencls_model(cfg, kind, num_classes=inp["num_classes"], device=dev)
    sd = make_state_dict(cfg, seed, spec_fn=lambda c: cls_spec(c, inp["num_classes"]))
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    return model.eval()


def _eval_inputs(dev, inp):
    d = lambda t: t.to(dev)
    video = d(inp["video"]).to(torch.bfloat16)
    etext = types.SimpleNamespace(input_ids=d(inp["e_ids"]), attention_mask=d(inp["e_mask"]), prompt_lengths=inp["e_plen"])
    eptext = types.SimpleNamespace(input_ids=d(inp["e_pids"]), attention_mask=d(inp["e_pmask"]))
    return video, etext, eptext


@pytest.mark.parametrize("kind", ["itm", "cls"])
def test_shared_prefix_scores_tiny_vs_reference_golden(dev, kind):
    from oracle.gen_golden import gencls_inputs
    from oracle.weights import CONFIG_TINY
    g = torch.load(os.path.join(GOLD, f"{kind}_tiny.pt"))
    inp = gencls_inputs(CONFIG_TINY, kind)
    model = _load(dev, kind, CONFIG_TINY, inp, g["meta"]["weight_seed"])
    video, etext, eptext = _eval_inputs(dev, inp)
    gen, cl = model.score_shared_prefix(etext, eptext, video=video)
    for name, mine in (("generation_logits", gen), ("cls_logits", cl)):
        plain_gate(f"{kind}_tiny", "score", rel(mine, g["fp32"][name]), rel(g["bf16"][name], g["fp32"][name]), name)
    gen0, cl0 = model(video, etext, eptext, train=False)
    _agree(gen, gen0, "generation")
    _agree(cl, cl0, "cls")


@pytest.mark.parametrize("kind", ["itm", "cls"])
def test_shared_prefix_scores_true_dims_vs_reference_golden(dev, kind):
    """1.3B decoder at full depth, ViT-B/16 x 16 frames (tests/golden/{itm,cls}_1p3b.pt), the gates of the existing path's test"""
    from oracle.gen_golden import FULL_GENCLS, full_gencls_cfg, gencls_inputs
    from test_parity_fullsize_gpu import FGATES
    g = torch.load(os.path.join(GOLD, f"{kind}_1p3b.pt"))
    cfg = full_gencls_cfg()
    inp = gencls_inputs(cfg, kind, **FULL_GENCLS)
    model = _load(dev, kind, cfg, inp, g["meta"]["weight_seed"])
    video, etext, eptext = _eval_inputs(dev, inp)
    qf = model.encode_video(video)
    gen, cl = model.score_shared_prefix(etext, eptext, query_features=qf)
    for name, mine in (("generation_logits", gen), ("cls_logits", cl)):
        ref = g["fp32"][name]
        e = (mine.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
        assert e <= FGATES[kind][name], (name, e)
    gen0, cl0 = model(video, etext, eptext, train=False)
    _agree(gen, gen0, "generation")
    # the cls_head output at true dims carries the bf16 noise of 24 layers on both paths: the existing path itself is gated at
    # FGATES[kind]["cls_logits"] against the fp32 reference (measured: 3.4e-2 between the two paths on the ITM probability)
    _agree(cl, cl0, "cls", tol=FGATES[kind]["cls_logits"])


def _shared_chunk(dev, cfg, kind, Bv, t, L, Lp, shared, seed):
    import test_shared_prefix_cpu as c
    video, text, ptext = c._chunk(cfg, kind, Bv, t, L, Lp, shared, seed)
    d = lambda x: x.to(dev)
    return d(video), types.SimpleNamespace(input_ids=d(text.input_ids), attention_mask=d(text.attention_mask),
                                           prompt_lengths=text.prompt_lengths), \
        types.SimpleNamespace(input_ids=d(ptext.input_ids), attention_mask=d(ptext.attention_mask))


@pytest.mark.parametrize("stream", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["itm", "cls"])
def test_shared_prefix_vs_scores_in_both_stream_modes(dev, monkeypatch, kind, stream):
    """a chunk whose texts share 6 tokens (and ragged tails) against _scores in the same residual-stream mode"""
    from oracle.gen_golden import gencls_inputs
    from oracle.weights import CONFIG_TINY
    from youku_mplug_amd import gpt3
    monkeypatch.setattr(gpt3, "FP32_STREAM", stream == "fp32")
    model = _load(dev, kind, CONFIG_TINY, gencls_inputs(CONFIG_TINY, kind), 5)
    t = 8 if kind == "itm" else model.num_classes
    video, text, ptext = _shared_chunk(dev, CONFIG_TINY, kind, 3, t, 20, 12, 6, seed=21)
    gen0, cl0 = model(video, text, ptext, train=False)
    gen, cl = model.score_shared_prefix(text, ptext, video=video)
    _agree(gen, gen0, "generation")
    _agree(cl, cl0, "cls")


def test_shared_prefix_on_a_head_dim_80_decoder(dev):
    """2.7B decoder dims (hidden 2560, 32 heads of 80), reduced depth, random weights, against _scores"""
    from oracle.weights import CONFIG_TINY
    from youku_mplug_amd.downstream import synthetic_gencls_model
    cfg = dataclasses.replace(CONFIG_TINY, hidden=2560, heads=32, ffn=4 * 2560, layers=2)
    torch.manual_seed(3)
    model = synthetic_gencls_model(cfg, "itm", num_classes=2, device=dev).eval()
    assert model.text_decoder.config.kv_channels == 80
    video, text, ptext = _shared_chunk(dev, cfg, "itm", 2, 8, 24, 12, 5, seed=4)
    gen0, cl0 = model(video, text, ptext, train=False)
    gen, cl = model.score_shared_prefix(text, ptext, video=video)
    _agree(gen, gen0, "generation")
    _agree(cl, cl0, "cls")
