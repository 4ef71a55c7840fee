"""Decode against a per-clip shared prefix KV cache, on CPU: the torch reference of the new attention against its fp64 definition,
generation.SharedPrefixDecodeState on the stand-ins (tests/standin_decode_shared.py) against DecodeState, its memory formula,
DistributedGPT3_Caption.generate(kv_cache="shared_prefix") and --eval_shared_kv on the stand-ins, the C-ABI mirror of
mpv_attn_decode_shared_desc and what the library refuses before it would launch."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import standin_decode_shared as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


# ------------------------------------------------------------------------------------------------ the reference of the GPU test
@pytest.mark.parametrize("case", sd.SWEEP, ids=lambda c: "-".join(map(str, c)))
def test_fp32_reference_matches_the_fp64_definition(case):
    """the fp32 torch softmax over the concatenated keys (the stand-in, and the reference of tests/test_decode_shared_gpu.py) against
    the element-by-element fp64 definition, on the kernel sweep's shapes: 1e-6 (fp32 rounding of ~300 products is 1e-7)"""
    c = sd.make_case(*case, seed=3)
    args = [c[n] for n in ("q", "k", "v", "pk", "pv", "lay", "prefix_lay", "n_seq", "group_size", "heads", "prefix_len", "own_len", "hd", "scale")]
    got, want = sd.attn_decode_shared_ref(*args), sd.reference_fp64(*args)
    assert got.shape == want.shape == (c["n_seq"], c["heads"], c["hd"])
    assert rel(got, want) <= 1e-6
    sd.run_case(sd.attn_decode_shared_fwd, c)                                    # the op form: the same values in bf16, strided into o
    assert torch.equal(c["o"].view(c["n_seq"], c["heads"], c["hd"]), got.to(torch.bfloat16))


def test_standin_refuses_what_the_kernel_refuses():
    c = sd.make_case(64, 1, 1, 2, 3, 1)
    for bad in (dict(hd=96), dict(group_size=0), dict(own_len=0), dict(own_len=2049), dict(prefix_len=0)):
        with pytest.raises(ValueError):
            sd.run_case(sd.attn_decode_shared_fwd, {**c, **bad})


# ------------------------------------------------------------------------------------------------ the state on the stand-ins
def _tiny_decoder(dev):
    from oracle.weights import CONFIG_TINY, make_state_dict
    from youku_mplug_amd.pretrain import synthetic_model
    cfg = CONFIG_TINY
    model = synthetic_model(cfg, device=dev)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in make_state_dict(cfg, 6).items()}, strict=True)
    model.eval()
    return cfg, model.text_decoder


def run_state_case(dev, make_ref, make_shared):
    """B = 2 clips x K = 3, Q = 8 query slots, a prompt of 3: prefill, two steps, then three steps after in-group re-orders.
    -> the list of (reference logits, shared logits, second shared logits) per call, and the states"""
    cfg, gpt = _tiny_decoder(dev)
    B, K, Q, P, H = 2, 3, 8, 3, cfg.hidden
    g = torch.Generator().manual_seed(21)
    qe = (torch.randn(B, Q, H, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    prompt = torch.randint(0, cfg.vocab, (B, P), generator=g).to(dev)
    ref, sh, sh2 = make_ref(gpt, B * K, Q + P + 6), make_shared(gpt, B * K, Q + P + 6), make_shared(gpt, B * K, Q + P + 6)
    out = [(ref.prefill_fan_out(prompt, qe, K), sh.prefill_fan_out(prompt, qe, K), sh2.prefill_fan_out(prompt, qe, K))]
    for t in range(2):
        tok = torch.randint(0, cfg.vocab, (B * K, 1), generator=g).to(dev)
        out.append((ref.step(tok), sh.step(tok), sh2.step(tok)))
    for perm in ([0, 0, 1, 5, 3, 3], [2, 1, 1, 4, 4, 3], [1, 2, 0, 3, 5, 4]):                    # sources stay inside their group of K
        perm = torch.tensor(perm, device=dev)
        ref.reorder(perm, shared_prefix=Q + P)
        sh.reorder(perm, shared_prefix=Q + P)
        sh2.reorder(perm)
        tok = torch.randint(0, cfg.vocab, (B * K, 1), generator=g).to(dev)
        out.append((ref.step(tok), sh.step(tok), sh2.step(tok)))
    return out, ref, sh, (cfg, B, K, Q, P)


def test_shared_state_matches_decode_state_on_standins(monkeypatch):
    from youku_mplug_amd.generation import DecodeState, SharedPrefixDecodeState
    sd.install(monkeypatch)
    out, ref, sh, (cfg, B, K, Q, P) = run_state_case(torch.device("cpu"), DecodeState, SharedPrefixDecodeState)
    assert len(out) == 6
    for i, (a, b, b2) in enumerate(out):
        assert a.shape == b.shape == (B * K, cfg.vocab) and b.dtype == torch.bfloat16
        assert rel(b, a) <= 1e-2, (i, rel(b, a))                                  # the project's KV-cache gate
        assert torch.equal(b, b2), i
    assert sh.pos == ref.pos == Q + P + 5 and sh.t == 5
    # kv_bytes: the formula, and smaller than a cache per sequence
    nl, H3, S = cfg.layers, 3 * cfg.hidden, 6
    assert sh.kv_bytes() == nl * (B * (Q + P) + 2 * B * K * S) * H3 * 2
    assert ref.kv_bytes() == nl * 2 * B * K * (Q + P + S) * H3 * 2 and sh.kv_bytes() < ref.kv_bytes()
    # no twin before a re-order moves rows (sampling never re-orders); the prefix is stored once
    _, gpt = _tiny_decoder(torch.device("cpu"))
    fresh = SharedPrefixDecodeState(gpt, B * K, Q + P + S)
    assert fresh.kv_bytes() == 0
    fresh.prefill_fan_out(torch.zeros((B, P), dtype=torch.long), torch.zeros((B, Q, cfg.hidden), dtype=torch.bfloat16), K)
    fresh.reorder(torch.arange(B * K), shared_prefix=Q + P)                        # nothing generated yet: nothing to move
    assert fresh.twin is None and fresh.kv_bytes() == nl * (B * (Q + P) + B * K * S) * H3 * 2
    assert fresh.prefix.cache.shape == (nl, B * (Q + P), H3) and fresh.suffix.shape == (nl, B * K * S, H3)
    with pytest.raises(ValueError):
        fresh.reorder(torch.arange(B * K), shared_prefix=Q + P - 1)                # the prefix is shared by construction
    with pytest.raises(ValueError):
        fresh.step(torch.zeros((B * K, 2), dtype=torch.long))
    with pytest.raises(ValueError):
        fresh.step(torch.zeros((B * K, 1), dtype=torch.long), torch.zeros((B * K, 1, cfg.hidden)))


# ------------------------------------------------------------------------------------------------ generate and the entry point
def _on_cpu(monkeypatch):
    import standin_beam
    import standin_sampling
    import test_pipeline_cpu as tp
    from youku_mplug_amd import ops
    dev = tp._on_cpu(monkeypatch)
    sd.install(monkeypatch)
    monkeypatch.setattr(ops, "beam_advance", standin_beam.beam_advance)
    monkeypatch.setattr(ops, "sample_advance", standin_sampling.sample_advance)
    return dev


def test_caption_generate_shared_prefix_on_standins(monkeypatch):
    """generate(batched=True) and generate(do_sample=True, num_samples=3) with kv_cache="shared_prefix" in the setup of
    test_caption_generate_batched_on_standins (ragged prompts: two groups): the list length, shapes, dtypes and order of the
    per_sequence twin, the prompts kept, every state a SharedPrefixDecodeState; a bad value raises."""
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict
    from youku_mplug_amd import generation
    from youku_mplug_amd.downstream import synthetic_gencls_model
    dev = _on_cpu(monkeypatch)
    m = torch.load(os.path.join(GOLD, "caption_tiny.pt"))["meta"]
    model = synthetic_gencls_model(CONFIG_TINY, "caption", device=dev)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in make_state_dict(CONFIG_TINY, m["weight_seed"]).items()}, strict=True)
    model.text_decoder.config.extra.update(tokens_to_generate=m["tokens_to_generate"], eod_id=m["eod_id"])
    video, ids, mask = make_inputs(CONFIG_TINY, m["batch"], m["text_len"], seed=m["input_seed"], ragged=False)
    mask[1, 4:] = 0
    text = types.SimpleNamespace(input_ids=ids, attention_mask=mask)
    video = video.to(torch.bfloat16)
    made = []
    orig_init = generation.SharedPrefixDecodeState.__init__

    def spy(self, *a, **kw):
        made.append(self)
        orig_init(self, *a, **kw)
    monkeypatch.setattr(generation.SharedPrefixDecodeState, "__init__", spy)
    for kw in (dict(batched=True), dict(do_sample=True, num_samples=3, seed=5, temperature=1.2, top_p=0.9)):
        twin = model.generate(video, text, termination_id=m["eod_id"], **kw)
        assert not made                                                            # keyword absent: today's state
        explicit = model.generate(video, text, termination_id=m["eod_id"], kv_cache="per_sequence", **kw)
        assert not made and all(torch.equal(a, b) for a, b in zip(twin, explicit))
        res = model.generate(video, text, termination_id=m["eod_id"], kv_cache="shared_prefix", **kw)
        assert len(made) == 2                                                      # one search per prompt length
        assert all(s.prefix is not None and s.kv_bytes() > 0 for s in made)
        if "do_sample" in kw:
            assert all(s.twin is None for s in made)                               # sampling never allocates a twin
        made.clear()
        assert isinstance(res, list) and len(res) == len(twin) == m["batch"]
        for i, (r, p) in enumerate(zip(res, twin)):
            assert r.shape == p.shape and r.dtype == p.dtype and r.device == p.device
            n_prompt = int(mask[i].sum()) - 1
            assert (r[:, :n_prompt] == ids[i, :n_prompt]).all(), i                 # clip i's own prompt: input order is kept
        with pytest.raises(ValueError):
            model.generate(video, text, termination_id=m["eod_id"], kv_cache="paged", **kw)
    with pytest.raises(ValueError):
        model.generate(video, text, termination_id=m["eod_id"], kv_cache="shared_prefix")          # the per-clip search
    gpt = model.text_decoder
    for call in (lambda: gpt.beam_search_batched(ids[:1, :3], kv="paged"), lambda: gpt.sample_batched(ids[:1, :3], kv="paged"),
                 lambda: gpt.generate(ids[:1, :3], sampler="device", kv="paged"), lambda: gpt.generate(ids[:1, :3], kv="shared_prefix")):
        with pytest.raises(ValueError):
            call()


def test_sampling_with_ragged_prompts_shares_the_shortest_prompt(monkeypatch):
    """sample_batched(kv="shared_prefix") with ragged prompt lengths: the shared prefix is Q + min_prompt, the teacher-forced
    positions behind it go into the suffix, and the tokens equal those of kv="per_sequence" on the stand-ins' near-identical logits
    (greedy: top_k = 1 removes the draw)."""
    from youku_mplug_amd import generation
    dev = _on_cpu(monkeypatch)
    cfg, gpt = _tiny_decoder(dev)
    gpt.config.extra.update(tokens_to_generate=4, eod_id=cfg.vocab - 1)
    g = torch.Generator().manual_seed(2)
    Q = 8
    qe = (torch.randn(2, Q, cfg.hidden, generator=g) * 0.5).to(torch.bfloat16)
    ids = torch.randint(0, cfg.vocab - 1, (2, 5), generator=g)
    made = []
    orig_init = generation.SharedPrefixDecodeState.__init__
    monkeypatch.setattr(generation.SharedPrefixDecodeState, "__init__", lambda self, *a, **kw: (made.append(self), orig_init(self, *a, **kw))[1])
    kw = dict(query_embeds=qe, num_samples=2, top_k=1, prompt_length=torch.tensor([5, 3]))
    a = gpt.sample_batched(ids, **kw)
    b = gpt.sample_batched(ids, kv="shared_prefix", **kw)
    assert len(made) == 1 and made[0].P == Q + 3 and made[0].fan == 2 and made[0].twin is None
    assert a.shape == b.shape and (b[:2, :5] == ids[0]).all() and (b[2:, :3] == ids[1, :3]).all()
    assert torch.equal(a, b)


def test_caption_entrypoint_shared_kv_flag_on_standins(tmp_path, monkeypatch):
    """downstream/run_caption_distributed_gpt3.py --evaluate_only: --eval_shared_kv defaults off and reaches model.generate as
    kv_cache="shared_prefix" in the --eval_batched_beam and the --eval_sample call; the result file keeps its format."""
    import test_entrypoint_gpu as t
    from test_engine_cpu import _stub_optimizer_kernels
    from youku_mplug_amd import downstream
    orig = t._write_configs

    def write(d, update_freq=1):
        path = orig(d, update_freq)
        cfg = json.load(open(os.path.join(d, "txt.json")))
        cfg.update(hidden_dropout=0.0, attention_dropout=0.0)
        json.dump(cfg, open(os.path.join(d, "txt.json"), "w"))
        return path
    monkeypatch.setattr(t, "_write_configs", write)
    _stub_optimizer_kernels(monkeypatch)
    monkeypatch.setenv("MASTER_PORT", str(42000 + os.getpid() % 2000))
    _on_cpu(monkeypatch)
    seen = []
    gen = downstream.DistributedGPT3_Caption.generate

    def spy(self, image, text, *a, **kw):
        seen.append((kw.get("batched", False), kw.get("do_sample", False), kw.get("kv_cache")))
        return gen(self, image, text, *a, **kw)
    monkeypatch.setattr(downstream.DistributedGPT3_Caption, "generate", spy)
    entry = t._finetune_entry("run_caption_distributed_gpt3")
    cfg = t._write_finetune_config(str(tmp_path), "caption", 'prompt: ""', tokens_to_generate=4)
    try:
        out = str(tmp_path / "shared")
        base = ["--config", cfg, "--output_dir", out, "--bf16", "--enable_deepspeed", "--synthetic_steps", "1", "--seed", "7", "--evaluate_only",
                "--eval_batched_beam", "--eval_sample", "2"]
        assert entry.get_args(base)[0].eval_shared_kv is False
        args, config = entry.get_args(base + ["--eval_shared_kv"])
        assert args.eval_shared_kv is True
        entry.main(args, config)
        assert seen and set(seen) == {(True, False, "shared_prefix"), (False, True, "shared_prefix")}, seen
        merged = json.load(open(os.path.join(out, "result", "val_caption_result.json")))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    assert len(merged) == 5
    for rec in merged:
        assert set(rec) == {"video_id", "pred_caption", "gold_caption", "sampled_captions"}
        assert isinstance(rec["pred_caption"], str) and len(rec["sampled_captions"]) == 2


# ------------------------------------------------------------------------------------------------ C ABI
def test_attn_decode_shared_desc_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    body = re.search(r"typedef struct mpv_attn_decode_shared_desc \{(.*?)\} mpv_attn_decode_shared_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    ct = _lib.AttnDecodeSharedDesc
    assert names == [f[0] for f in ct._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpv.h"', 'int main(void) {',
            '  printf("%zu", sizeof(mpv_attn_decode_shared_desc));'] + \
           [f'  printf(" %zu", offsetof(mpv_attn_decode_shared_desc, {n}));' for n in names] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    tok = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert tok[0] == ctypes.sizeof(ct)
    assert tok[1:] == [getattr(ct, f[0]).offset for f in ct._fields_]
    for sym in ("mpv_attn_decode_shared_fwd", "mpv_gpt_decode_step_shared", "mpv_gpt_decode_shared_workspace_size"):
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym)


def _desc(**over):
    """a well-formed descriptor over addresses that are never dereferenced on the host: 2 groups x 5 sequences, 4 heads of 64"""
    from youku_mplug_amd import _lib
    H, S, P = 256, 8, 11
    d = _lib.AttnDecodeSharedDesc()
    d.q, d.k, d.v, d.pk, d.pv, d.o = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    d.q_ss = d.k_ss = d.v_ss = S * 3 * H
    d.pk_gs = d.pv_gs = P * 3 * H
    d.q_hs = d.k_hs = d.v_hs = d.pk_hs = d.pv_hs = 3 * 64
    d.k_rs = d.v_rs = d.pk_rs = d.pv_rs = 3 * H
    d.o_ss, d.o_hs = H, 64
    d.n_seq, d.group_size, d.n_groups, d.heads, d.prefix_len, d.own_len, d.head_dim, d.scale = 10, 5, 2, 4, P, 3, 64, 0.125
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("over", [dict(head_dim=96), dict(group_size=0), dict(own_len=0), dict(own_len=2049), dict(prefix_len=0),
                                  dict(n_groups=3), dict(n_groups=1), dict(k_rs=3 * 256 + 4), dict(pv_gs=11 * 768 + 2), dict(o_ss=258),
                                  dict(q=0x10008), dict(pk=0), dict(scale=0.0), dict(n_seq=0)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_library_refuses_bad_descriptors_before_any_launch(over):
    """every refusal is a negative code from host-side checks: no device is needed (and none is touched) to get it"""
    from youku_mplug_amd import _lib
    rc = _lib.lib().mpv_attn_decode_shared_fwd(ctypes.byref(_desc(**over)), None)
    assert rc < 0, (over, rc)
    assert b"mpv_attn_decode_shared_fwd" in _lib.lib().mpv_last_error()
