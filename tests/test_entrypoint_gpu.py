"""GPU tests of the boundary pieces the training loop touches: the run_pretrain_distributed_gpt3.py entry point driven for
a few steps from a YAML config (tiny dims, synthetic clips), DistributedGPT3.forward(input_embeds=...), concurrent GEMMs on
two streams (per-stream workspace, no library-owned device state), ignored labels in the cross-entropy."""
import json
import math
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_configs(d, update_freq=1):
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
batch_size: 2
num_workers: 0
max_length: 16
freeze_vit: false
freeze_text_decoder: true
num_learnable_token: {s.num_queries}
use_contrastive: false
optimizer: {{lr: 1e-4, opt: "AdamW", weight_decay: 0.05, clip_grad: 3.0, opt_betas: [0.9, 0.999], opt_eps: 1e-6}}
schedular: {{epochs: 2, min_lr: 1e-6, warmup_epochs: -1, warmup_steps: 2, lr_sched_type: "cosine"}}
"""
    open(os.path.join(d, "pretrain.yaml"), "w").write(yml)
    return os.path.join(d, "pretrain.yaml")


def test_entrypoint_three_steps_from_yaml(tmp_path, dev):
    """The reference's per-step protocol against the native engine: schedule values land in param_groups (lr * lr_scale),
    the loss all-gather / NaN guard runs, _global_grad_norm and micro_steps are live, a DeepSpeed-layout checkpoint and a
    log line come out, and a second invocation auto-resumes from `latest`."""
    sys.path.insert(0, ROOT)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(24000 + os.getpid() % 2000))
    import run_pretrain_distributed_gpt3 as entry
    from youku_mplug_amd import engine as eng
    cfg = _write_configs(str(tmp_path))
    out = str(tmp_path / "out")
    args, config = entry.get_args(["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "3", "--seed", "7"])
    assert args.lr == 1e-4 and args.clip_grad == 3.0 and args.warmup_steps == 2 and args.epochs == 2 and args.max_length == 16
    seen = {}
    orig_init = eng.initialize

    def spy(**kw):
        r = orig_init(**kw)
        seen["engine"], seen["opt"] = r[0], r[1]
        return r
    eng.initialize, entry.mpv_engine.initialize = spy, spy
    try:
        stats = entry.main(args, config)
    finally:
        eng.initialize = entry.mpv_engine.initialize = orig_init
    e, opt = seen["engine"], seen["opt"]
    assert e.micro_steps == 3 and e.global_steps == 6 and opt.step_count == 6        # 2 epochs x 3 steps (micro_steps is reset per epoch)
    sched = eng.cosine_scheduler(1e-4, 1e-6, 2, 3, warmup_steps=2, sched_type="cosine")
    for g in opt.param_groups:
        assert g["lr"] == pytest.approx(sched[5] * g["lr_scale"])
    assert math.isfinite(stats["loss"]) and stats["grad_norm"] > 0 and stats["loss_ita"] == 0.0
    assert open(os.path.join(out, "latest")).read().strip() == "checkpoint-1"
    assert os.path.isfile(os.path.join(out, "checkpoint-1", "mp_rank_00_model_states.pt"))
    lines = open(os.path.join(out, "log.txt")).read().strip().splitlines()
    assert len(lines) == 2 and json.loads(lines[1])["epoch"] == 1
    # resume: nothing left to do, the loop is skipped and the weights are the checkpoint's
    args2, config2 = entry.get_args(["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "3"])
    eng.initialize, entry.mpv_engine.initialize = spy, spy
    try:
        entry.main(args2, config2)
    finally:
        eng.initialize = entry.mpv_engine.initialize = orig_init
    assert torch.equal(seen["engine"].flat.params, e.flat.params) and seen["opt"].step_count == 6


def test_entrypoint_graph_mode_matches_eager(tmp_path, dev, monkeypatch):
    """MPV_GRAPH=1: the entrypoint's loop drives engine.graph_step (one replayed HIP graph per step) -- same per-epoch statistics and
    bit-identical final parameters as the eager loop from the same seed."""
    sys.path.insert(0, ROOT)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(24000 + os.getpid() % 2000))
    import run_pretrain_distributed_gpt3 as entry
    from youku_mplug_amd import engine as eng
    cfg = _write_configs(str(tmp_path))
    got = {}
    orig_init = eng.initialize
    for mode in ("0", "1"):
        monkeypatch.setenv("MPV_GRAPH", mode)
        out = str(tmp_path / f"out{mode}")
        args, config = entry.get_args(["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "4", "--seed", "9"])
        seen = {}

        def spy(**kw):
            r = orig_init(**kw)
            seen["engine"] = r[0]
            return r
        eng.initialize, entry.mpv_engine.initialize = spy, spy
        try:
            stats = entry.main(args, config)
        finally:
            eng.initialize = entry.mpv_engine.initialize = orig_init
        got[mode] = (stats, seen["engine"].flat.params.clone(), seen["engine"])
    assert got["1"][2]._graph is not None and got["0"][2]._graph is None
    # (the gradient norm is a sum of atomically added partial sums: equal to rounding, not to the bit, between ANY two runs)
    assert got["0"][0]["loss"] == got["1"][0]["loss"] and got["0"][0]["grad_norm"] == pytest.approx(got["1"][0]["grad_norm"], rel=1e-5), (got["0"][0], got["1"][0])
    assert torch.equal(got["0"][1], got["1"][1])
    assert got["1"][2].global_steps == got["0"][2].global_steps == 8


def test_forward_input_embeds_matches_tokens_path(dev):
    """models/modeling_distributed_gpt3.py:1578-1618 / :652-657: input_embeds = word_embeddings(ids) (with the visual
    queries in front, as models/distributed_gpt3.py:155-166 builds them) gives the logits of the tokens + query_embeds call."""
    from oracle.weights import CONFIG_TINY
    from youku_mplug_amd.pretrain import synthetic_model
    torch.manual_seed(3)
    gpt = synthetic_model(CONFIG_TINY, device=dev).text_decoder.eval()
    B, L, Q, H = 2, 12, 5, CONFIG_TINY.hidden
    ids = torch.randint(0, CONFIG_TINY.vocab, (B, L), device=dev)
    query = (torch.randn(B, Q, H, device=dev) * 0.1).bfloat16()
    labels = torch.randint(0, CONFIG_TINY.vocab, (B, Q + L), device=dev)
    mask = torch.ones(B, Q + L - 1, dtype=torch.long, device=dev)
    with torch.no_grad():
        a = gpt(tokens=ids, query_embeds=query, labels=labels, loss_mask=mask)
        emb = gpt.dist_model.language_model.embedding.word_embeddings.weight[ids]
        b = gpt(input_embeds=torch.cat([query, emb], dim=1), labels=labels, loss_mask=mask)
        c = gpt(input_embeds=emb, query_embeds=query, labels=labels, loss_mask=mask)
    assert torch.equal(a.logits, b.logits) and torch.equal(a.logits, c.logits)
    assert a.loss.item() == b.loss.item()
    with pytest.raises(ValueError):
        gpt(labels=labels)


def test_gemm_two_streams_concurrently(dev):
    """mpv.h promises re-entrancy: split-K partials and tail-split arrival counters live in the caller's workspace, which the
    Python side keeps per (device, stream).  Two streams run different split-K / tail-split GEMMs at once, many times."""
    from youku_mplug_amd import ops
    g = torch.Generator().manual_seed(5)

    def rn(*s):
        return (torch.randn(*s, generator=g) * 0.5).bfloat16().to(dev)
    cases = [  # (M, N, K, ta, tb, hint): wgrad split-K on both kernels, a tail-split shape on the 128 kernel
        (768, 512, 6272, 1, 1, 256), (640, 384, 3136, 1, 1, 128), (5120, 2048, 2048, 0, 0, 128), (1000, 1160, 2304, 0, 1, 128)]
    data = []
    for M, N, K, ta, tb, hint in cases:
        a = rn(K, M) if ta else rn(M, K)
        b = rn(K, N) if tb else rn(N, K)
        ref = (a.float().t() if ta else a.float()) @ (b.float() if tb else b.float().t())
        data.append((M, N, K, ta, tb, hint, a, b, ref))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = {0: [], 1: []}
    for rep in range(10):
        for si, (st, order) in enumerate(((s1, data), (s2, data[::-1]))):
            with torch.cuda.stream(st):
                for M, N, K, ta, tb, hint, a, b, ref in order:
                    outs[si].append((ops.gemm(a, b, M, N, K, trans_a=bool(ta), trans_b=bool(tb), tile_hint=hint), ref))
    torch.cuda.synchronize()
    for si in (0, 1):
        for out, ref in outs[si]:
            err = ((out.float() - ref).abs().max() / ref.abs().max()).item()
            assert err < 1e-2, err
    assert len({k for k in ops._ws}) >= 2, "one workspace per stream"


def test_cross_entropy_ignores_out_of_range_labels(dev):
    from youku_mplug_amd import ops
    rows, V = 6, 512
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(rows, V, generator=g) * 2).bfloat16().to(dev)
    labels = torch.tensor([3, -100, 511, 512, 0, 100], device=dev)
    w = torch.full((rows,), 0.25, device=dev)
    dl = torch.empty_like(logits)
    losses, loss = ops.cross_entropy(logits.clone(), labels, w, rows, V, dlogits=dl)
    ok = (labels >= 0) & (labels < V)
    ref = torch.nn.functional.cross_entropy(logits.float()[ok], labels[ok], reduction="none")
    assert torch.allclose(losses[ok], ref, atol=2e-2)
    assert losses[~ok].abs().max().item() == 0.0 and dl[~ok].abs().max().item() == 0.0
    # in place (dlogits aliasing logits), as the training path calls it: same losses (the target logit is captured before the row is overwritten)
    buf = logits.clone()
    losses2, _ = ops.cross_entropy(buf, labels, w, rows, V, dlogits=buf)
    assert torch.equal(losses, losses2) and torch.equal(buf, dl)


def _write_retrieval_config(d, num_frames=None):
    _write_configs(d)
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
num_learnable_token: 32
temp: 0.07
contrastive_embed_dim: 64
{'num_frames: %d' % num_frames if num_frames else ''}
optimizer: {{lr: 1e-4, opt: "AdamW", weight_decay: 0.05, clip_grad: 3.0, opt_betas: [0.9, 0.999], opt_eps: 1e-8}}
schedular: {{epochs: 1, min_lr: 1e-7, warmup_epochs: -1, warmup_steps: 1, lr_sched_type: "cosine"}}
"""
    path = os.path.join(d, f"retrieval{num_frames or ''}.yaml")
    open(path, "w").write(yml)
    return path


def test_retrieval_entrypoint_train_eval_resume(tmp_path, dev):
    """downstream/run_retrieval_distributed_gpt3.py restated on this engine (reference :107-339, 402-420): two ITC training steps
    on synthetic (clip, title, idx) batches with padding='longest' titles, the evaluation loop + recall metrics on the synthetic
    val / test splits, a DeepSpeed-layout checkpoint and the log line; then `--evaluate_only --resume <checkpoint>` at ANOTHER frame
    count (temporal embeddings re-fitted) reproduces finite metrics."""
    sys.path.insert(0, os.path.join(ROOT, "downstream"))
    sys.path.insert(0, ROOT)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(24000 + os.getpid() % 2000))
    import run_retrieval_distributed_gpt3 as entry
    cfg = _write_retrieval_config(str(tmp_path))
    out = str(tmp_path / "out")
    args, config = entry.get_args(["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "2", "--seed", "3"])
    assert args.lr == 1e-4 and args.epochs == 1 and args.max_length == 16 and config["num_frames"] == 4
    stats = entry.main(args, config)
    assert math.isfinite(stats["train_loss"]) and stats["train_grad_norm"] > 0 and stats["train_text_len"] <= 16
    for split in ("val", "test"):
        for k in ("txt_r1", "txt_r10", "vid_r1", "vid_r10", "r_mean"):
            assert 0.0 <= stats[f"{split}_sim_{k}"] <= 100.0
    ck = os.path.join(out, "checkpoint-0", "mp_rank_00_model_states.pt")
    assert os.path.isfile(ck) and json.loads(open(os.path.join(out, "log.txt")).read().strip().splitlines()[-1])["epoch"] == 0
    cfg2 = _write_retrieval_config(str(tmp_path), num_frames=2)
    args2, config2 = entry.get_args(["--config", cfg2, "--output_dir", str(tmp_path / "out2"), "--bf16", "--enable_deepspeed", "--synthetic_steps", "1",
                                     "--evaluate_only", "--resume", ck])
    assert config2["num_frames"] == 2
    res = entry.main(args2, config2)
    assert set(res) == {"val", "test"} and all(0.0 <= v <= 100.0 for v in res["val"].values())


def _write_finetune_config(d, name, extra, batch_size=4, tokens_to_generate=None):
    _write_configs(d)
    if tokens_to_generate is not None:                       # short beam searches for the caption test
        cfg = json.load(open(os.path.join(d, "txt.json")))
        cfg["tokens_to_generate"] = tokens_to_generate
        json.dump(cfg, open(os.path.join(d, "txt.json"), "w"))
    yml = f"""
text_decoder: 'nlp_gpt3_text-generation_1.3B/'
text_cfg: {d}/txt.json
visual_cfg: '{d}/vis.json'
_synthetic: true
batch_size: {batch_size}
num_workers: 0
max_length: 24
freeze_vit: false
freeze_text_decoder: true
num_learnable_token: 32
{extra}
optimizer: {{lr: 1e-4, opt: "AdamW", weight_decay: 0.05, clip_grad: 3.0, opt_betas: [0.9, 0.999], opt_eps: 1e-8}}
schedular: {{epochs: 1, min_lr: 1e-7, warmup_epochs: -1, warmup_steps: 1, lr_sched_type: "cosine"}}
"""
    path = os.path.join(d, f"{name}.yaml")
    open(path, "w").write(yml)
    return path


def _finetune_entry(module_name):
    sys.path.insert(0, os.path.join(ROOT, "downstream"))
    sys.path.insert(0, ROOT)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(24000 + os.getpid() % 2000))
    import importlib
    return importlib.import_module(module_name)


def test_itm_entrypoint_train_eval(tmp_path, dev):
    """downstream/run_retrieval_distributed_gpt3_itm.py restated on this engine (reference :66-224, 228-286, 343-541): two ITM
    training steps (two derangements of negatives per step, generation + matching-head losses), the re-ranking evaluation (every clip
    against every title, generation and cls score matrices, recall both ways), checkpoint and log line; then `--evaluate_only
    --resume <checkpoint>`."""
    entry = _finetune_entry("run_retrieval_distributed_gpt3_itm")
    cfg = _write_finetune_config(str(tmp_path), "itm", "use_cls: true")
    out = str(tmp_path / "out")
    args, config = entry.get_args(["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "2", "--seed", "5",
                                   "--eval_freq", "1"])
    assert config["num_classes"] == 2 and args.max_length == 24
    stats = entry.main(args, config)
    assert math.isfinite(stats["train_loss"]) and stats["train_grad_norm"] > 0
    assert stats["train_loss_generation"] > 0 and stats["train_loss_cls"] > 0
    assert abs(stats["train_loss"] - stats["train_loss_generation"] - stats["train_loss_cls"]) < 1e-3 * stats["train_loss"]
    for split in ("val", "test"):
        for head in ("gen", "cls"):
            assert 0.0 <= stats[f"{split}_{head}_r_mean"] <= 100.0
    ck = os.path.join(out, "checkpoint-0", "mp_rank_00_model_states.pt")
    assert os.path.isfile(ck) and json.loads(open(os.path.join(out, "log.txt")).read().strip().splitlines()[-1])["epoch"] == 0
    args2, config2 = entry.get_args(["--config", cfg, "--output_dir", str(tmp_path / "out2"), "--bf16", "--enable_deepspeed", "--synthetic_steps", "1",
                                     "--evaluate_only", "--resume", ck])
    res = entry.main(args2, config2)
    # the checkpointed model scores the validation split as it did at the end of training
    assert res["val"]["gen_r_mean"] == pytest.approx(stats["val_gen_r_mean"], abs=1e-6)
    assert res["val"]["cls_r_mean"] == pytest.approx(stats["val_cls_r_mean"], abs=1e-6)


def test_itm_random_derangement_and_labels():
    """random_derangement (reference :42-53): permutations without fixed points, reproducible from `random`'s seed; a negative whose
    video id equals the anchor's is labelled a match (:112-116)."""
    import random
    entry = _finetune_entry("run_retrieval_distributed_gpt3_itm")
    random.seed(3)
    for n in (2, 3, 7, 24):
        v = entry.random_derangement(n)
        assert sorted(v) == list(range(n)) and all(v[i] != i for i in range(n))
    random.seed(11)
    a = entry.random_derangement(9)
    random.seed(11)
    assert entry.random_derangement(9) == a
    with pytest.raises(ValueError):
        entry.random_derangement(1)
    from finetune_common import SyntheticTextTokenizer
    random.seed(0)
    video = torch.zeros(3, 1)
    _, text, ptext, neg, labels = entry.make_training_batch(video, ["\u4e00\u4e01", "\u4e02", "\u4e03\u4e04\u4e05"], torch.tensor([7, 7, 9]),
                                                            SyntheticTextTokenizer(100), torch.device("cpu"), 24)
    ids = [7, 7, 9]
    assert labels.tolist() == [1, 1, 1] + [int(ids[i % 3] == ids[n]) for i, n in enumerate(neg)]
    assert text.input_ids.shape == (9, 24) and ptext.input_ids.shape == (9, 24) and text.prompt_lengths.shape == (9,)


def test_synthetic_tokenizer_pair_contract():
    """SyntheticTextTokenizer keeps DistributedGPT3Tokenizer's call contract (models/modeling_distributed_gpt3.py:209-317): bos +
    prompt + text + eos, prompt_lengths, padding to max_length, the prompt is cut before the target."""
    _finetune_entry("finetune_common")
    from finetune_common import SyntheticTextTokenizer
    tok = SyntheticTextTokenizer(1000)
    a, b = "\u4e00\u4e01\u4e02", "\u4e10\u4e11"
    e = tok([[a, b]], padding="max_length", max_length=10)
    assert e.input_ids.tolist() == [[1, 5, 6, 7, 21, 22, 0, 0, 0, 0]] and e.attention_mask.sum().item() == 7 and e.prompt_lengths.tolist() == [3]
    e = tok([[a * 4, b]], padding="max_length", max_length=10)             # 12 prompt tokens: cut to 10 - 2 - 2 = 6
    assert e.prompt_lengths.tolist() == [6] and e.attention_mask.sum().item() == 10 and e.input_ids[0, -3:].tolist() == [21, 22, 0]
    e = tok([a, b * 6], padding="longest", max_length=8)
    assert e.input_ids.shape == (2, 8) and e.attention_mask.sum(-1).tolist() == [5, 8]
    assert tok.decode(tok([a], max_length=8).input_ids[0]) == a


def test_cls_entrypoint_train_eval(tmp_path, dev):
    """downstream/run_cls_distributed_gpt3.py restated on this engine (reference :50-200, 203-263, 266-470): two training steps
    (generation loss on the class name + cls_head loss), top-1 / top-5 accuracy of both heads on val and test, checkpoint, log
    line; then `--evaluate_only --resume`."""
    entry = _finetune_entry("run_cls_distributed_gpt3")
    cfg = _write_finetune_config(str(tmp_path), "cls", "use_cls: true\nnum_classes: 6", batch_size=20)
    out = str(tmp_path / "out")
    args, config = entry.get_args(["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "2", "--seed", "6"])
    stats = entry.main(args, config)
    assert math.isfinite(stats["train_loss"]) and stats["train_loss_cls"] > 0 and stats["train_grad_norm"] > 0
    for split in ("val", "test"):
        for head in ("gen", "cls"):
            assert 0.0 <= stats[f"{split}_{head}_top1_accuracy"] <= stats[f"{split}_{head}_top5_accuracy"] <= 100.0
    ck = os.path.join(out, "checkpoint-0", "mp_rank_00_model_states.pt")
    args2, config2 = entry.get_args(["--config", cfg, "--output_dir", str(tmp_path / "out2"), "--bf16", "--enable_deepspeed", "--synthetic_steps", "1",
                                     "--evaluate_only", "--resume", ck])
    res = entry.main(args2, config2)
    assert res["epoch"] == -1 and res["val_cls_top5_accuracy"] == pytest.approx(stats["val_cls_top5_accuracy"], abs=1e-6)
    assert json.loads(open(os.path.join(str(tmp_path / "out2"), "log.txt")).read().strip().splitlines()[-1])["epoch"] == -1


def test_caption_entrypoint_train_generate(tmp_path, dev):
    """downstream/run_caption_distributed_gpt3.py restated on this engine (reference :66-205, 208-238, 301-500): two caption
    training steps, a checkpoint; then `--evaluate_only --resume`: beam-search captions of the validation clips, the per-rank and
    merged result files, and the metric line."""
    entry = _finetune_entry("run_caption_distributed_gpt3")
    cfg = _write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=6)
    out = str(tmp_path / "out")
    args, config = entry.get_args(["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "2", "--seed", "7"])
    stats = entry.main(args, config)
    assert math.isfinite(stats["train_loss_generation"]) and stats["train_grad_norm"] > 0
    ck = os.path.join(out, "checkpoint-0", "mp_rank_00_model_states.pt")
    out2 = str(tmp_path / "out2")
    args2, config2 = entry.get_args(["--config", cfg, "--output_dir", out2, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--evaluate_only",
                                     "--resume", ck])
    res = entry.main(args2, config2)
    merged = json.load(open(os.path.join(out2, "result", "val_caption_result.json")))
    assert len(merged) == 5 and all(set(r) == {"video_id", "pred_caption", "gold_caption"} and len(r["gold_caption"]) == 2 for r in merged)
    assert os.path.isfile(os.path.join(out2, "result", "val_caption_result_rank0.json"))
    assert all(0.0 <= res[f"val_{k}"] <= 1.0 for k in ("Bleu_1", "Bleu_4", "ROUGE_L")) and all(r["pred_caption"] for r in merged)


def test_caption_metrics_known_answers():
    """The built-in scorers against hand-computed values (pycocoevalcap's definitions): one clip, hypothesis 'a b c d' against
    references 'a b c e' and 'a b': BLEU-1 = 3/4, BLEU-2 = sqrt(3/4 * 2/3), ROUGE-L from LCS 3 (P = 3/4, R = max(3/4, 2/2))."""
    entry = _finetune_entry("run_caption_distributed_gpt3")
    pairs = [("a b c d".split(), ["a b c e".split(), "a b".split()])]
    b = entry.bleu_scores(pairs)
    assert b[0] == pytest.approx(0.75, rel=1e-6) and b[1] == pytest.approx(math.sqrt(0.75 * 2 / 3), rel=1e-6)
    assert b[2] == pytest.approx((0.75 * (2 / 3) * 0.5) ** (1 / 3), rel=1e-6)
    p, r, beta = 0.75, 1.0, 1.2
    assert entry.rouge_l(pairs) == pytest.approx((1 + beta ** 2) * p * r / (r + beta ** 2 * p), rel=1e-9)
    short = [("a b".split(), ["a b c d".split()])]                      # brevity penalty exp(1 - 4/2)
    assert entry.bleu_scores(short)[0] == pytest.approx(math.exp(-1.0), rel=1e-6)
    assert entry.normalize("ab\u4e00, \u4e01!") == "\u4e00 \u4e01"


def test_itm_eval_recall_metrics():
    """itm_eval (reference :296-339) against an independent count (rank of the true match = number of strictly larger scores in
    its row) on a random tie-free 40 x 40 similarity matrix with a boosted diagonal."""
    sys.path.insert(0, os.path.join(ROOT, "downstream"))
    sys.path.insert(0, ROOT)
    import numpy as np
    import run_retrieval_distributed_gpt3 as entry
    rng = np.random.default_rng(0)
    n = 40
    s = rng.standard_normal((n, n)) + 1.5 * np.eye(n)
    r = entry.itm_eval(s, s.T.copy(), {i: i for i in range(n)}, {i: [i] for i in range(n)})

    def recalls(m):
        ranks = np.array([(m[i] > m[i, i]).sum() for i in range(n)])
        return [100.0 * (ranks < k).mean() for k in (1, 5, 10)]
    t, v = recalls(s), recalls(s.T)
    assert [r["txt_r1"], r["txt_r5"], r["txt_r10"]] == pytest.approx(t) and [r["vid_r1"], r["vid_r5"], r["vid_r10"]] == pytest.approx(v)
    assert r["r_mean"] == pytest.approx((sum(t) / 3 + sum(v) / 3) / 2) and 0 < r["txt_r1"] < 100


def test_bench_contract_line_forced_distributed_path():
    """bench.py as the driver runs it (a subprocess, one JSON line on stdout), with MPV_BENCH_FORCE_DIST=1 so that the N > 1 code path
    -- RCCL communicator on the high-priority stream, parameter broadcast, bucketed all-reduce in the backward, fences with barriers,
    max-over-ranks timing, the post-run roofline steps on every rank -- executes on this one GPU: exactly one line, the contract's keys,
    value = global batch x steps / time, roofline with a live HIP-event measurement."""
    import subprocess
    env = dict(os.environ, MPV_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(25000 + os.getpid() % 2000))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=600, env=env, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in rec, k
    assert rec["n_gpus"] == 1 and rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "samples/s" and rec["higher_is_better"] is True
    assert rec["scaling"] == "weak" and rec["vs_baseline"] is None and rec["dtype"] == "bf16" and rec["data"] == "synthetic" and rec["cpu_baseline"] is None
    assert "workload" in rec["config"] and rec["config"]["global_batch"] == 32 and rec["config"]["parallelism"] == "dp1"
    assert rec["value"] == pytest.approx(32 * 3 / (rec["ms_per_step"] * 3e-3), rel=1e-3)
    roof = rec["roofline"]
    assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s" and roof["peak"] == 2500.0
    assert 0.2 < roof["frac"] < 1.0 and roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], abs=1e-3)
    # `frac` is the STEP-level fraction: executed FLOPs of the step / the contract's step time / peak; the GEMM family is gemm_frac
    assert roof["achieved"] == pytest.approx(roof["step_algorithmic_tflop"] / (rec["ms_per_step"] * 1e-3), rel=2e-3)
    assert roof["frac"] < roof["gemm_frac"] < 1.0 and roof["gemm_frac"] == pytest.approx(roof["gemm_achieved"] / roof["peak"], abs=1e-3)
    for k in ("sclk_mhz", "power_w", "clock_power_samples", "clock_power_source"):
        assert k in roof, k
    if roof["clock_power_source"] is not None:      # a box whose SMI answers: plausible MI355X figures, sampled during the timed region
        assert roof["clock_power_samples"] >= 1 and 500 < roof["sclk_mhz"] < 3000 and 100 < roof["power_w"] < 2000
    assert 30.0 < rec["ms_per_step"] < 400.0


def test_bench_plain_run_is_lean():
    """bench.py without --full, exactly as the driver runs it: the contract's line with the --full measurements null, and at most
    30 s of the whole process's wall time spent outside its warm-up and timed steps."""
    import subprocess
    import time
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MPV_BENCH_FORCE_DIST", "MPV_BENCH_BY_SHAPE", "MPV_GRAPH"):
        env.pop(k, None)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, env=env, stdin=subprocess.DEVNULL)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert rec["metric"] == "video-text samples/sec/node, mPLUG-Video 1.3B pretrain step" and rec["unit"] == "samples/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "bf16" and rec["data"] == "synthetic" and rec["step_mode"] == "eager"
    assert rec["value"] == pytest.approx(32 * 3 / (rec["ms_per_step"] * 3e-3), rel=1e-3) and 30.0 < rec["ms_per_step"] < 400.0
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and rec["host"]["idle_queue_launch_ms"] is None
    outside = wall - (3 + 1) * rec["ms_per_step"] * 1e-3
    assert outside < 30.0, f"{outside:.1f} s outside the steps"


def test_bench_two_ranks_on_one_gpu():
    """bench.py launched as the driver launches it for N = 2 (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment, `--gpus 2`), both
    ranks on this box's one GPU over gloo on device tensors (`--_test-one-gpu`: RCCL refuses two ranks per device; the line is stamped TEST):
    the N > 1 flow on REAL kernels -- process group, parameter broadcast, the memory guard's eager step, engine.graph_self_check on two ranks
    (must pass bit for bit), the measured mode choice, fenced timed region with MAX over ranks, roofline steps on every rank, exactly one
    JSON line from rank 0 and nothing on rank 1's stdout."""
    import subprocess
    import tempfile
    port = 27000 + os.getpid() % 2000
    procs = []
    # (the flow is what is under test: reduced dims -- two processes time-slicing one GPU with 260 MB of gradients per step staged through the
    # host took minutes at the 1.3B dims)
    worker = tempfile.NamedTemporaryFile("w", suffix="_bench_two_ranks.py", delete=False)
    worker.write("import sys\nsys.path.insert(0, %r)\nimport bench\nS = bench.Shapes\n"
                 "S.img_size, S.patch_size, S.vit_dim, S.vit_depth, S.vit_heads, S.num_queries = 64, 16, 192, 2, 2, 32\n"
                 "S.hidden, S.layers, S.heads, S.ffn, S.vocab, S.max_pos = 256, 2, 4, 1024, 1024, 256\n"
                 "sys.argv = ['bench.py', '--gpus', '2', '--steps', '3', '--warmup', '1', '--batch', '4', '--frames', '4', '--text-len', '8', '--full', '--no-cpu-baseline', '--_test-one-gpu']\n"
                 "bench.main()\n" % ROOT)
    worker.close()
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.pop("MPV_BENCH_FORCE_DIST", None)
        procs.append(subprocess.Popen([sys.executable, worker.name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env,
                                      stdin=subprocess.DEVNULL))
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, o, e))
    for r, (rc, o, e) in enumerate(outs):
        assert rc == 0, (r, e[-2500:])
    assert outs[1][1].strip() == "", outs[1][1][:300]
    lines = [ln for ln in outs[0][1].splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["global_batch"] == 8 and rec["config"]["parallelism"] == "dp2" and rec["data"].startswith("TEST")
    assert rec["host"]["graph_self_check"] == {"passed": True, "detail": "bit-identical"}, rec["host"]
    assert set(rec["host"]["mode_probe_ms_per_step"]) == {"graph", "eager"} and rec["step_mode"] in ("graph", "eager")
    assert rec["value"] == pytest.approx(8 * 3 / (rec["ms_per_step"] * 3e-3), rel=1e-2)
    os.unlink(worker.name)
    assert rec["roofline"] is not None and rec["roofline"]["launches_per_step"] > 0 and rec["cpu_baseline"] is None
    assert math.isfinite(rec["config"]["final_loss"])


def _entry_two_rank_gpu_worker(rank, world, port, d, graph, zero, q):
    import traceback
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                          MPV_GRAPH="1" if graph else "0")
        sys.path.insert(0, ROOT)
        import youku_mplug_amd  # noqa: F401
        from youku_mplug_amd import engine as eng
        orig_pg = eng.init_process_group_for_dp
        eng.init_process_group_for_dp = lambda backend=None, **kw: orig_pg("gloo", **kw)      # RCCL refuses two ranks on one device
        seen = {}
        orig_init = eng.initialize

        def spy(**kw):
            r = orig_init(**kw)
            seen["engine"] = r[0]
            return r
        eng.initialize = spy
        import run_pretrain_distributed_gpt3 as entry
        entry.mpv_engine.initialize = spy
        entry.mpv_engine.init_process_group_for_dp = eng.init_process_group_for_dp
        logs = []
        out = os.path.join(d, f"out_g{int(graph)}_z{zero}")
        args, config = entry.get_args(["--config", os.path.join(d, "pretrain.yaml"), "--output_dir", out, "--bf16", "--enable_deepspeed",
                                       "--synthetic_steps", "3", "--seed", "7", "--zero_stage", str(zero)])
        stats = entry.main(args, config)
        e = seen["engine"]
        torch.cuda.synchronize()
        q.put((rank, e.flat.params.float().cpu().numpy(), e.zero_shards, {k: v for k, v in stats.items() if isinstance(v, (int, float))},
               bool(getattr(e, "_graph_dp_ok", False)), sorted(os.listdir(os.path.join(out, "checkpoint-1")))))
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, "ERROR", traceback.format_exc()))
        raise


@pytest.mark.parametrize("graph,zero", [(False, 1), (True, 0)])
def test_entrypoint_two_ranks_on_one_gpu(tmp_path, graph, zero):
    """run_pretrain_distributed_gpt3.py as TWO ranks on real kernels (both on this box's GPU; the test worker swaps the communicator's backend
    for gloo, nothing in the product changes): (False, 1) the command line's default ZeRO stage 1 -- ranks end with identical parameters, one
    zero_pp_rank_<r> optimizer file each; (True, 0) MPV_GRAPH=1 -- the segmented replay is used only after engine.graph_self_check has passed on
    both ranks, and the run ends with identical parameters on both."""
    import torch.multiprocessing as mp
    d = str(tmp_path)
    _write_configs(d)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 41000 + os.getpid() % 2000 + (3 if graph else 0)
    procs = [ctx.Process(target=_entry_two_rank_gpu_worker, args=(r, 2, port, d, graph, zero, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(200):
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
    assert len(res) == 2 and not any(isinstance(v[0], str) for v in res.values()), res
    import numpy as np
    assert np.array_equal(res[0][0], res[1][0]), "ranks must end with identical parameters"
    assert np.isfinite(res[0][0]).all() and abs(res[0][0]).sum() > 0
    files = res[0][4]
    if zero == 1:
        assert res[0][1] is not None and len(res[0][1]) == 2
        assert files == ["mp_rank_00_model_states.pt", "zero_pp_rank_0_mp_rank_00_optim_states.pt", "zero_pp_rank_1_mp_rank_00_optim_states.pt"], files
    else:
        assert files == ["mp_rank_00_model_states.pt", "mp_rank_00_optim_states.pt"], files
    if graph:
        assert res[0][3] and res[1][3], "MPV_GRAPH=1 on two ranks: the start-up self-check must have passed on both"

