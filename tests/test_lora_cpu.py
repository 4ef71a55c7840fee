"""Decoder LoRA adapters through the HOST pipelines on the CPU (device entry points on the stand-ins of tests/standin_ops.py and
tests/standin_lora.py): the gradient check of tests/test_lora_model_gpu.py in both residual-stream modes, the ITM and ITC models'
hidden_only / d_last_hidden passes, the state-dict rules, every refusal, two gloo ranks, and the caption entry point end to end."""
import json
import math
import os
import types

import pytest
import torch

import lora_model_cases as M
import standin_lora

BF = torch.bfloat16


def _on_cpu(monkeypatch):
    import test_w8_cpu as tw
    dev = tw._on_cpu(monkeypatch)
    standin_lora.install(monkeypatch)
    return dev


@pytest.mark.parametrize("fp32_stream", [True, False], ids=["fp32-stream", "bf16-stream"])
def test_gradients_vs_restatement_on_standins(monkeypatch, fp32_stream):
    from youku_mplug_amd import gpt3
    dev = _on_cpu(monkeypatch)
    monkeypatch.setattr(gpt3, "FP32_STREAM", fp32_stream)
    model, sd = M.pretrain_model(dev)
    M.set_adapters(model.text_decoder)
    model.eval()
    assert not model.text_decoder.trainable and model.text_decoder.lora_live()
    video, ids, mask, vid, text = M.inputs(dev)
    loss, _ = model(vid, text)
    loss.backward()
    ref_loss, ref_grads, _ = M.restated(model, sd, video, ids, mask)
    M.check_gradients(model, loss.item(), ref_loss, ref_grads)


def test_merge_on_standins(monkeypatch):
    import test_lora_model_gpu as t
    t.test_merge(_on_cpu(monkeypatch))


def test_generate_and_score_captions_refuse_live_adapters_on_standins(monkeypatch):
    import test_lora_model_gpu as t
    t.test_generate_and_score_captions_refuse_live_adapters(_on_cpu(monkeypatch))


def test_no_adapter_adds_no_call_and_no_tape_entry(monkeypatch):
    """without adapters the decoder makes not one LoRA call and its tape has no adapter entry"""
    from youku_mplug_amd import ops
    dev = _on_cpu(monkeypatch)
    calls = []
    for n in standin_lora.NAMES:
        monkeypatch.setattr(ops, n, lambda *a, _n=n, **k: calls.append(_n))
    model, _ = M.pretrain_model(dev, lora=False)
    model.eval()
    video, ids, mask, vid, text = M.inputs(dev)
    with torch.no_grad():                                              # the explicit pipeline, as forward_backward drives it
        loss, tape = model._forward_pipeline(vid, text.input_ids, text.attention_mask)
        assert all("t" not in ent and "x1" not in ent for ent in tape["gpt"]["layers"])
        model._backward_pipeline(tape, torch.ones((), dtype=torch.float32))
    assert not calls and not model.text_decoder.has_lora()


def _adapter_grads(model):
    return {k: p.grad for k, p in model.named_parameters() if "lora_" in k}


def test_itm_model_second_pass_accumulates(monkeypatch):
    """DistributedGPT3_Retrieval_Cls with adapters: the caption pass and the hidden_only prompt pass (pass_index 1, backward seeded by
    d_last_hidden) both reach the adapters -- finite, non-zero, and the step's gradient is the sum of the two passes'"""
    from oracle.gen_golden import gencls_inputs
    from oracle.weights import CONFIG_TINY, cls_spec, make_state_dict
    from youku_mplug_amd.downstream import synthetic_gencls_model
    dev = _on_cpu(monkeypatch)
    inp = gencls_inputs(CONFIG_TINY, "itm")
    model = synthetic_gencls_model(CONFIG_TINY, "itm", num_classes=inp["num_classes"], device=dev)
    sd = make_state_dict(CONFIG_TINY, 3, spec_fn=lambda c: cls_spec(c, inp["num_classes"]))
    model.load_state_dict({k: v.to(BF) for k, v in sd.items()}, strict=True)
    model.text_decoder.add_lora(M.RANK, M.ALPHA)
    M.set_adapters(model.text_decoder)
    model.eval()
    text = types.SimpleNamespace(input_ids=inp["ids"], attention_mask=inp["mask"], prompt_lengths=inp["plen"])
    ptext = types.SimpleNamespace(input_ids=inp["p_ids"], attention_mask=inp["p_mask"])
    video = inp["video"].to(BF)
    got = {}
    for name, wc, wk in (("both", 1.0, 1.0), ("caption", 1.0, 0.0), ("cls", 0.0, 1.0)):
        for p in model.parameters():
            p.grad = None
        lc, lk = model(video, text, ptext, inp["neg"], inp["labels"])
        (wc * lc + wk * lk).backward()
        got[name] = {k: g.float().clone() for k, g in _adapter_grads(model).items()}
    assert len(got["both"]) == 2 * CONFIG_TINY.layers
    for k, g in got["both"].items():
        assert torch.isfinite(g).all() and g.abs().max() > 0, k
        assert got["cls"][k].abs().max() > 0, f"{k}: the hidden_only pass gave the adapters nothing"
        s = got["caption"][k] + got["cls"][k]
        assert M.rel_l2(g, s) <= 2e-2, (k, M.rel_l2(g, s))


def test_itc_model_text_tower_reaches_the_adapters(monkeypatch):
    """DistributedGPT3_Retrieval with adapters: the text tower's hidden_only pass is kept and run backward from the pooled rows"""
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict, retrieval_spec
    from youku_mplug_amd.retrieval import DistributedGPT3_Retrieval, synthetic_retrieval_model
    dev = _on_cpu(monkeypatch)
    model = synthetic_retrieval_model(CONFIG_TINY, device=dev)
    sd = make_state_dict(CONFIG_TINY, 4, spec_fn=retrieval_spec)
    model.load_state_dict({k: v.to(BF) for k, v in sd.items()}, strict=True)
    model.eval()
    video, ids, mask = make_inputs(CONFIG_TINY, 8, 10, seed=31, ragged=True)
    text = types.SimpleNamespace(input_ids=ids, attention_mask=mask)
    idx = torch.arange(8)
    base = model(video.to(BF), text, idx)
    model.text_decoder.add_lora(M.RANK, M.ALPHA)                       # zero B: the loss is the un-adapted one
    loss0 = model(video.to(BF), text, idx)
    assert torch.equal(loss0.detach(), base.detach())
    M.set_adapters(model.text_decoder)
    loss = model(video.to(BF), text, idx)
    loss.backward()
    grads = _adapter_grads(model)
    assert len(grads) == 2 * CONFIG_TINY.layers
    for k, g in grads.items():
        assert g is not None and torch.isfinite(g.float()).all() and g.float().abs().max() > 0, k
    assert DistributedGPT3_Retrieval is type(model)


def test_state_dict_rules(monkeypatch):
    dev = _on_cpu(monkeypatch)
    model, sd = M.pretrain_model(dev)                                  # (a BASE checkpoint went in with strict=True)
    gpt = model.text_decoder
    M.set_adapters(gpt)
    keys = [k for k in model.state_dict() if "lora_" in k]
    assert len(keys) == 4 and all(k.endswith(("query_key_value.lora_A", "query_key_value.lora_B")) for k in keys)
    before = {k: model.state_dict()[k].clone() for k in keys}
    model.load_state_dict({k: v.to(BF) for k, v in sd.items()}, strict=True)
    assert all(torch.equal(model.state_dict()[k], before[k]) for k in keys), "a base load must leave the adapters as they are"
    short = {k: v.to(BF) for k, v in sd.items() if not k.endswith("visual_fc.weight")}
    with pytest.raises(RuntimeError, match="visual_fc.weight"):          # only the adapter keys may be missing
        model.load_state_dict(short, strict=True)
    lsd = gpt.lora_state_dict()
    assert lsd["lora_rank"] == M.RANK and lsd["lora_alpha"] == M.ALPHA and len(lsd) == 6
    other, _ = M.pretrain_model(dev)
    other.text_decoder.load_lora_state_dict(lsd)
    assert all(torch.equal(other.state_dict()[k], before[k]) for k in keys)
    wrong, _ = M.pretrain_model(dev, config=dict(lora_rank=16, lora_alpha=12.0))
    with pytest.raises(ValueError, match="rank"):
        wrong.text_decoder.load_lora_state_dict(lsd)
    with pytest.raises(ValueError, match="alpha"):
        other.text_decoder.load_lora_state_dict(dict(lsd, lora_alpha=8.0))
    bad = dict(lsd)
    k0 = next(k for k in lsd if k.endswith("lora_A"))
    bad[k0] = lsd[k0][:, :-8]
    with pytest.raises(ValueError, match="shape"):
        other.text_decoder.load_lora_state_dict(bad)
    msd = gpt.merged_state_dict()
    plain = {k for k in gpt.state_dict() if "lora_" not in k}
    assert set(msd) == plain and gpt.lora_live()
    changed = [k for k in msd if not torch.equal(msd[k], gpt.state_dict()[k])]
    assert changed and all(k.endswith("query_key_value.weight") for k in changed)


def test_refusals(monkeypatch):
    from oracle.weights import CONFIG_TINY as cfg
    from youku_mplug_amd import generation, ops
    from youku_mplug_amd.gpt3 import DistributedGPT3, GPT3Config
    dev = _on_cpu(monkeypatch)
    txt = GPT3Config(vocab_size=cfg.vocab, hidden_size=cfg.hidden, ffn_hidden_size=cfg.ffn, num_hidden_layers=cfg.layers,
                     num_attention_heads=cfg.heads, max_position_embeddings=cfg.max_pos, layernorm_epsilon=cfg.gpt_ln_eps)
    gpt = DistributedGPT3(config=txt, device=dev)
    with pytest.raises(RuntimeError, match="trainable"):                  # adapters on a trainable base
        gpt.add_lora(8)
    for p in gpt.parameters():
        p.requires_grad = False
    for rank in (0, 4, 12, 128):
        with pytest.raises(ValueError, match="rank"):
            gpt.add_lora(rank)
    with pytest.raises(RuntimeError, match="no adapters"):
        gpt.merge_lora()
    gpt.add_lora(8, 12)
    assert gpt._lora["scale"] == 1.5 and not gpt.trainable and gpt.lora_live()
    with pytest.raises(RuntimeError, match="already"):                    # a second add_lora
        gpt.add_lora(8)
    gpt.eval()
    ids = torch.zeros((2, 4), dtype=torch.long)
    prefix = gpt.forward_prefix(None, ids)                                  # forward_lm: applies the adapters
    live = "call merge_lora\\(\\) first"
    with pytest.raises(RuntimeError, match=live):
        gpt.forward_continuation(prefix, ids, 1, hidden_rows=torch.zeros(1, dtype=torch.long))
    with pytest.raises(RuntimeError, match=live):
        gpt.forward_continuation_packed(prefix, ids.view(-1), None, labels=ids.view(-1))
    with pytest.raises(RuntimeError, match=live):
        gpt.forward_shared_prefix_lm(torch.zeros((2 * 2, cfg.hidden), dtype=BF), ids, ids.view(-1), None, (None, None), {})
    with pytest.raises(RuntimeError, match=live):
        gpt.quantize_decode_weights()
    with pytest.raises(RuntimeError, match=live):
        gpt.decode_weights_q8()
    with pytest.raises(RuntimeError, match=live):
        generation.DecodeState(gpt, 2, 8)
    with pytest.raises(RuntimeError, match=live):
        generation.SharedPrefixDecodeState(gpt, 2, 8)
    with pytest.raises(RuntimeError, match=live):
        gpt.beam_search_batched(ids, beam_size=2)
    with gpt.lora_merged():
        state = generation.DecodeState(gpt, 2, 8)                           # made while merged ...
        assert not gpt.lora_live()
        with pytest.raises(RuntimeError, match="already merged"):
            gpt.merge_lora()
    with pytest.raises(RuntimeError, match=live):                           # ... and stepped after the unmerge
        state._call("mpv_gpt_decode_step")
    with pytest.raises(RuntimeError, match="not merged"):
        gpt.unmerge_lora()
    assert ops.LORA_RANKS == (8, 16, 32, 64)


def test_constructors_read_the_config(monkeypatch):
    from youku_mplug_amd.retrieval import DistributedGPT3_Retrieval
    dev = _on_cpu(monkeypatch)
    plain, _ = M.pretrain_model(dev, lora=False)
    assert not plain.text_decoder.has_lora() and not any("lora_" in k for k in plain.state_dict())
    model, _ = M.pretrain_model(dev, config=dict(lora_rank=16, lora_alpha=None))       # alpha defaults to the rank
    lo = model.text_decoder._lora
    assert lo["rank"] == 16 and lo["alpha"] == 16.0 and lo["scale"] == 1.0
    assert all(p.requires_grad for k, p in model.text_decoder.named_parameters() if "lora_" in k)
    assert not any(p.requires_grad for k, p in model.text_decoder.named_parameters() if "lora_" not in k)
    B = model.text_decoder._qkv_linears()[0].lora_B
    assert B.dtype == BF and tuple(B.shape) == (3 * 256, 16) and not B.float().any()
    with pytest.raises(ValueError, match="freeze_text_decoder"):
        M.pretrain_model(dev, config=dict(lora_rank=8, freeze_text_decoder=False))
    assert DistributedGPT3_Retrieval.__init__.__code__.co_names.count("add_lora") == 1


# ------------------------------------------------------------------------------------------------ two gloo ranks
def _dp_worker(rank, world, port, q, received):
    import torch.distributed as dist
    from test_engine_cpu import _MP, _stub_optimizer_kernels
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mp_ = _MP()
    standin_lora.install(mp_)
    _stub_optimizer_kernels(mp_)
    from youku_mplug_amd import engine as eng
    torch.manual_seed(1234 + rank)                                          # every rank draws its own lora_A
    model, _ = M.pretrain_model("cpu")
    model.eval()                                                            # the stand-ins do not model the hash dropout
    groups = eng.get_parameter_groups(model, 0.05, model.no_weight_decay(), visual_backbone_scale=True)
    engine, _, _, _ = eng.initialize(model=model, model_parameters=groups, config=dict(lr=1e-3, clip_grad=3.0))
    video, ids, mask, vid, text = M.inputs("cpu", batch=4, text_len=8, seed=9)
    sl = slice(rank * 2, rank * 2 + 2)
    start = {k: p.detach().clone() for k, p in model.named_parameters() if "lora_" in k}
    for _ in range(2):
        loss, _ = engine(vid[sl], types.SimpleNamespace(input_ids=text.input_ids[sl], attention_mask=text.attention_mask[sl]))
        engine.backward(loss)
        engine.step()
    end = {k: p.detach().clone() for k, p in model.named_parameters() if "lora_" in k}
    q.put((rank, start, end, loss.item()))
    received.wait(timeout=300)
    dist.barrier()
    dist.destroy_process_group()


def test_adapters_identical_across_two_gloo_ranks():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q, received = ctx.Queue(), ctx.Event()
    port = 29000 + os.getpid() % 3000
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, received)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(150):
        try:
            r = q.get(timeout=2)
            res[r[0]] = r[1:]
        except Exception:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
        if len(res) == 2:
            break
    received.set()
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert len(res) == 2
    (s0, e0, l0), (s1, e1, l1) = res[0], res[1]
    assert len(e0) == 4 and math.isfinite(l0) and math.isfinite(l1)
    for k in e0:
        assert torch.equal(s0[k], s1[k]), f"{k}: not broadcast at initialize()"
        assert torch.equal(e0[k], e1[k]), f"{k}: replicas diverged"
        assert not torch.equal(e0[k], s0[k]), f"{k}: did not move"


# ------------------------------------------------------------------------------------------------ the caption entry point
def _entry(monkeypatch, tmp_path):
    import test_entrypoint_gpu as t
    from test_engine_cpu import _stub_optimizer_kernels
    orig = t._write_configs

    def write(d, update_freq=1):
        path = orig(d, update_freq)
        cfg = json.load(open(os.path.join(d, "txt.json")))
        cfg.update(hidden_dropout=0.0, attention_dropout=0.0)              # the stand-ins do not model the hash dropout
        json.dump(cfg, open(os.path.join(d, "txt.json"), "w"))
        return path
    monkeypatch.setattr(t, "_write_configs", write)
    _stub_optimizer_kernels(monkeypatch)
    monkeypatch.setenv("MASTER_PORT", str(46000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    return entry, cfg


def test_caption_entrypoint_train_save_load_evaluate(tmp_path, monkeypatch):
    """--synthetic_steps 2 --lora_rank 8 --lora_save, then --evaluate_only twice on the run's checkpoint: once as saved (adapters
    inside), once with the adapter keys stripped (a BASE checkpoint) and the adapters from --lora_load -- the same captions.  The
    evaluation generates, so it runs inside lora_merged(): the adapters are live again behind it."""
    entry, cfg = _entry(monkeypatch, tmp_path)
    import finetune_common as ft
    seen = []
    build = ft.build_engine

    def spy(args, config, model_cls, s):
        r = build(args, config, model_cls, s)
        seen.append(getattr(s.model, "module", s.model))
        return r
    monkeypatch.setattr(ft, "build_engine", spy)
    adapters = str(tmp_path / "adapters.pt")
    common = ["--config", cfg, "--bf16", "--enable_deepspeed", "--seed", "7"]
    try:
        with pytest.raises(ValueError, match="lora_rank"):
            entry.get_args(common + ["--output_dir", str(tmp_path / "x"), "--lora_save", adapters])
        out = str(tmp_path / "train")
        args, config = entry.get_args(common + ["--output_dir", out, "--synthetic_steps", "2", "--lora_rank", "8", "--lora_alpha", "12",
                                                "--lora_save", adapters])
        assert config["lora_rank"] == 8 and config["lora_alpha"] == 12.0
        stats = entry.main(args, config)
        assert math.isfinite(stats["train_loss"])
        trained = seen[-1].text_decoder
        assert trained.lora_live() and any(lin.lora_B.float().abs().max() > 0 for lin in trained._qkv_linears()), "lora_B never moved"
        saved = torch.load(adapters)
        assert saved["lora_rank"] == 8 and saved["lora_alpha"] == 12.0 and len(saved) == 2 + 2 * len(trained._qkv_linears())
        ck = os.path.join(out, "checkpoint-0", "mp_rank_00_model_states.pt")
        state = torch.load(ck)
        assert sum("lora_" in k for k in state["module"]) == len(saved) - 2
        base = str(tmp_path / "base.pth")
        torch.save({"model": {k: v for k, v in state["module"].items() if "lora_" not in k}}, base)
        results = []
        for name, extra in (("with", ["--resume", ck]), ("loaded", ["--resume", base, "--lora_load", adapters])):
            o = str(tmp_path / name)
            a, c = entry.get_args(common + ["--output_dir", o, "--synthetic_steps", "1", "--evaluate_only", "--lora_rank", "8",
                                            "--lora_alpha", "12"] + extra)
            entry.main(a, c)
            gpt = seen[-1].text_decoder
            assert gpt.lora_live(), "the evaluation must leave the adapters live"
            for k, v in gpt.lora_state_dict().items():
                assert (v == saved[k]) if not torch.is_tensor(v) else torch.equal(v, saved[k]), k
            results.append(json.load(open(os.path.join(o, "result", "val_caption_result.json"))))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert results[0] and results[0] == results[1]
