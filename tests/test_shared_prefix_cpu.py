"""Shared-prefix scoring of the ITM / category heads (downstream._GenCls.score_shared_prefix) on CPU: the split rule, the host
pipeline on the torch stand-ins (tests/standin_ops.py + tests/standin_prefix.py) against the existing _scores path, the C-ABI
mirror of mpv_attn_prefix_desc, and the ISA budget of the new kernel."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import standin_prefix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _split(ids, first, last, gs, Q=4):
    from youku_mplug_amd.downstream import shared_prefix_split
    return shared_prefix_split(torch.as_tensor(ids), torch.as_tensor(first), torch.as_tensor(last), gs, Q)


# ------------------------------------------------------------------------------------------------ split rule
def test_split_takes_the_common_prefix_of_a_chunk():
    ids = [[5, 6, 7, 8, 1, 0], [5, 6, 7, 9, 2, 0]]
    assert _split(ids, [6, 6], [-1, -1], 2) == (4 + 3, 1)        # nothing read: t = 3, one row left for the continuations


def test_split_is_capped_at_the_first_scored_or_pooled_row():
    ids = [[5, 6, 7, 8, 1, 0], [5, 6, 7, 8, 2, 0]]
    assert _split(ids, [2, 3], [4, 3], 2) == (4 + 2, 3)          # common 4, first output at token 2; last at 4 -> rows 6..8


def test_split_trims_trailing_padding():
    ids = [[5, 1, 2, 0, 0, 0, 0, 0], [5, 3, 0, 0, 0, 0, 0, 0]]
    P, Lc = _split(ids, [1, 0], [2, 1], 2)
    assert (P, Lc) == (4 + 0, 3)                                 # rows after the last output (token 2) are dropped


def test_split_uses_the_smallest_prefix_over_groups():
    ids = [[5, 6, 7, 1], [5, 6, 7, 2], [5, 9, 7, 1], [5, 8, 7, 2]]
    assert _split(ids, [3, 3, 3, 3], [3, 3, 3, 3], 2) == (4 + 1, 3)   # group 0 shares 3 tokens, group 1 only 1


def test_split_with_nothing_shared_beyond_the_video():
    ids = [[1, 6, 7], [2, 6, 7]]
    assert _split(ids, [0, 1], [2, 2], 2) == (4, 3)              # P = Q


def test_split_single_continuation_row_and_group_size_one():
    ids = [[5, 6, 7, 8], [9, 6, 7, 8]]
    assert _split(ids, [3, 3], [3, 3], 1) == (4 + 3, 1)          # each row is its own group: Lc = 1


# ------------------------------------------------------------------------------------------------ host pipeline on the stand-ins
def _model(monkeypatch, kind, cfg=None):
    from oracle.weights import CONFIG_TINY, cls_spec, make_state_dict
    from youku_mplug_amd.downstream import synthetic_gencls_model
    standin_prefix.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    cfg = cfg or CONFIG_TINY
    C = 2 if kind == "itm" else 3
    model = synthetic_gencls_model(cfg, kind, num_classes=C, device="cpu")
    sd = make_state_dict(cfg, 7, spec_fn=lambda c: cls_spec(c, C))
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    return model.eval(), cfg, C


def _chunk(cfg, kind, Bv, t, L, Lp, shared, seed):
    """t candidates per video; the first `shared` tokens of every text (and prompt) are common to the chunk, ragged lengths"""
    g = torch.Generator().manual_seed(seed)

    def rows(n, length):
        ids = torch.randint(0, cfg.vocab, (n, length), generator=g)
        ids[:, :shared] = ids[0, :shared]
        mask = torch.ones(n, length, dtype=torch.long)
        lens = torch.randint(shared + 2, length + 1, (n,), generator=g)
        for b in range(n):
            mask[b, lens[b]:] = 0
        return ids, mask
    ids, mask = rows(Bv * t, L)
    p_ids, p_mask = rows(Bv * t if kind == "itm" else Bv, Lp)
    plen = torch.randint(shared, shared + 2, (Bv * t,), generator=g)
    video = torch.randn(Bv, 3, cfg.num_frames, cfg.img_size, cfg.img_size, generator=g).to(torch.bfloat16)
    return video, types.SimpleNamespace(input_ids=ids, attention_mask=mask, prompt_lengths=plen), \
        types.SimpleNamespace(input_ids=p_ids, attention_mask=p_mask)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.mark.parametrize("kind", ["itm", "cls"])
@pytest.mark.parametrize("shared", [0, 3])
def test_shared_prefix_pipeline_matches_scores_on_standins(monkeypatch, kind, shared):
    model, cfg, C = _model(monkeypatch, kind)
    t = 4 if kind == "itm" else C
    video, text, ptext = _chunk(cfg, kind, 2, t, 10, 8, shared, seed=3 + shared)
    gen0, cls0 = model._scores(video, text, ptext)
    gen1, cls1 = model.score_shared_prefix(text, ptext, video=video)
    qf = model.encode_video(video)
    gen2, cls2 = model.score_shared_prefix(text, ptext, query_features=qf)
    assert gen1.shape == gen0.shape and cls1.shape == cls0.shape
    # shared = 0: the same rows through the same stand-ins.  shared > 0: the prefix rows come from a pass of their own, whose
    # stand-in matmuls have other shapes (fp32 summation order of the host BLAS); bf16 roundings carry that to ~1e-5 of the scores
    # and ~1e-3 of the ITM probability
    tg, tc = (1e-5, 1e-5) if shared == 0 else (1e-4, 3e-3)
    assert _rel(gen1, gen0) <= tg and _rel(cls1, cls0) <= tc, (_rel(gen1, gen0), _rel(cls1, cls0))
    assert torch.equal(gen1, gen2) and torch.equal(cls1, cls2)


def test_shared_prefix_runs_only_the_continuation_rows(monkeypatch):
    """The continuation pass sees P = Q + shared tokens and only the rows up to the chunk's last scored position; the LM head
    runs on the scored rows only."""
    model, cfg, C = _model(monkeypatch, "itm")
    video, text, ptext = _chunk(cfg, "itm", 2, 4, 12, 8, 3, seed=9)
    seen = []
    from youku_mplug_amd import ops
    orig_attn, orig_gemm = ops.attn_prefix_fwd, ops.gemm

    def attn(*a, **k):
        seen.append(("attn", a[-4], a[-3], a[-2]))       # heads, cont_len, prefix_len
        return orig_attn(*a, **k)

    def gemm(a, b, M, N, K, **k):
        if N == cfg.vocab:
            seen.append(("lm_head", M))
        return orig_gemm(a, b, M, N, K, **k)
    monkeypatch.setattr(ops, "attn_prefix_fwd", attn)
    monkeypatch.setattr(ops, "gemm", gemm)
    model.score_shared_prefix(text, ptext, video=video)
    Q = model.num_learnable_token
    gen_calls = [s for s in seen if s[0] == "attn"][:cfg.layers]
    assert all(s[3] == Q + 3 for s in gen_calls)
    _, loss_mask = model._gen_targets(text.input_ids, text.attention_mask, text.prompt_lengths, Q)
    last = int(loss_mask.nonzero()[:, 1].max())
    assert all(s[2] == last + 1 - (Q + 3) for s in gen_calls)
    assert ("lm_head", int(loss_mask.sum())) in seen


# ------------------------------------------------------------------------------------------------ C ABI and ISA
def test_attn_prefix_desc_layout_matches_the_header(tmp_path):
    from youku_mplug_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = open(os.path.join(ROOT, "include", "mpv.h")).read()
    body = re.search(r"typedef struct mpv_attn_prefix_desc \{(.*?)\} mpv_attn_prefix_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    ct = _lib.AttnPrefixDesc
    assert names == [f[0] for f in ct._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpv.h"', 'int main(void) {',
            '  printf("%zu", sizeof(mpv_attn_prefix_desc));'] + [f'  printf(" %zu", offsetof(mpv_attn_prefix_desc, {n}));' for n in names] + \
           ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    tok = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert tok[0] == ctypes.sizeof(ct)
    assert tok[1:] == [getattr(ct, f[0]).offset for f in ct._fields_]
    assert "mpv_attn_prefix_fwd" in _lib.EXPORTS


def test_prefix_attention_kernel_budget():
    """Two 256-thread workgroups per CU: no scratch, at most 256 VGPRs (launch_bounds(256, 2)), 52 KiB of LDS (two buffers of
    64-row K and V chunks at a 208-byte pitch)."""
    import test_isa_cpu as isa
    if not os.path.isfile(os.path.join(isa.LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    ks = {}
    import tempfile
    d = tempfile.mkdtemp()
    for i, blob in enumerate(isa._code_objects()):
        f = os.path.join(d, f"co_{i}.elf")
        open(f, "wb").write(blob)
        txt = subprocess.run([os.path.join(isa.LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
        for blk in txt.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "attn_prefix_fwd_kernel" in name:
                g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                ks[name] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), lds=g("group_segment_fixed_size"),
                                scratch=g("private_segment_fixed_size"))
    shutil.rmtree(d, ignore_errors=True)
    assert len(ks) == 4, ks                        # head_dim 64 and 80, each with the uniform and the packed row map
    for n, k in ks.items():
        assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= 256 and k["lds"] == 4 * 64 * 208, (n, k)


# ------------------------------------------------------------------------------------------------ entry points on the stand-ins
def _entry_on_standins(tmp_path, monkeypatch, capsys, test_name, port):
    """the GPU entry-point test of tests/test_shared_prefix_entrypoint_gpu.py on CPU / gloo through the stand-ins"""
    import json
    import test_entrypoint_gpu as t
    import test_shared_prefix_entrypoint_gpu as e
    from test_engine_cpu import _stub_optimizer_kernels
    orig = t._write_configs

    def write(d, update_freq=1):
        path = orig(d, update_freq)
        cfg = json.load(open(os.path.join(d, "txt.json")))
        cfg.update(hidden_dropout=0.0, attention_dropout=0.0)          # the stand-ins do not model the hash dropout
        json.dump(cfg, open(os.path.join(d, "txt.json"), "w"))
        return path
    monkeypatch.setattr(t, "_write_configs", write)
    standin_prefix.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    _stub_optimizer_kernels(monkeypatch)
    monkeypatch.setenv("MASTER_PORT", str(port + os.getpid() % 2000))
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()
    try:
        getattr(e, test_name)(tmp_path, torch.device("cpu"), monkeypatch, capsys)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_itm_entrypoint_shared_prefix_on_standins(tmp_path, monkeypatch, capsys):
    _entry_on_standins(tmp_path, monkeypatch, capsys, "test_itm_entrypoint_evaluates_through_the_shared_prefix", 36000)


def test_cls_entrypoint_shared_prefix_on_standins(tmp_path, monkeypatch, capsys):
    _entry_on_standins(tmp_path, monkeypatch, capsys, "test_cls_entrypoint_evaluates_through_the_shared_prefix", 38000)
