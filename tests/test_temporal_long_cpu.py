"""Temporal attention for clips of 17..64 frames, checked without a GPU: the launch plan of the new family
(mpv_temporal_attn_long_plan_describe: instance, block, LDS from csrc/attention_layout.h, capped grid, refusals), the untouched
refusal of the old family, the register / scratch budget of the four new kernels, the fp32 restatement
at 24 frames against the reference's own modules, and the host pipeline at 24 frames on the torch stand-ins."""
import ctypes as C
import dataclasses
import importlib.util
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "youku-mplug_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
GRID_CAP = 16384          # csrc/attention.hip: TEMPORAL_GRID_CAP
WAVES = 4                 # csrc/attention_layout.h: TEMPORAL_MFMA_WAVES
VGPR_BUDGET = 256         # two waves per SIMD = 8 waves per CU


def _binding():
    spec = importlib.util.spec_from_file_location("mpv_lib_binding_long", os.path.join(ROOT, "youku-mplug_amd", "_lib.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _layout_header_values():
    """temporal_mfma_lds(bwd, tt) as csrc/attention_layout.h computes it: the header compiled into a host program.  None when
    this machine has no C++ compiler (the plan is then still held to the variant's limit, which is the same function)."""
    cxx = next((c for c in (os.path.join(LLVM, "clang++"), shutil.which("g++"), shutil.which("c++"), shutil.which("clang++")) if c and os.path.isfile(c)), None)
    if cxx is None:
        return None
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "lay.cpp"), os.path.join(d, "lay")
        open(src, "w").write('#define __host__\n#define __device__\n#include <cstdio>\n#include "attention_layout.h"\n'
                             "int main() { for (int b = 0; b < 2; ++b) for (int tt = 32; tt <= 64; tt += 32)\n"
                             '  std::printf("%d %d %d %d\\n", b, tt, attn_layout::temporal_mfma_lds(b != 0, tt), attn_layout::temporal_mfma_wave_lds(b != 0, tt)); }\n')
        subprocess.run([cxx, "-std=c++17", "-I", CSRC, src, "-o", exe], check=True, capture_output=True, timeout=120)
        out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    return {(int(b), int(tt)): (int(v), int(w)) for b, tt, v, w in (l.split() for l in out.strip().splitlines())}


def test_long_plan_describe():
    lib_mod = _binding()
    lib, info = lib_mod.lib(), lib_mod.AttnPlanInfo()
    header = _layout_header_values()
    for T in (17, 32, 33, 64):
        for hd in (64, 96):
            for bwd in (0, 1):
                for n_outer, n_inner, heads in ((2, 6, 2), (1, 5, 3), (32, 196, 8)):
                    assert lib.mpv_temporal_attn_long_plan_describe(n_outer, n_inner, T, heads, hd, bwd, C.byref(info)) == 0, lib.mpv_last_error()
                    tt = 32 if T <= 32 else 64
                    name = info.variant.decode()
                    assert name == f"temporal_attn_mfma_kernel<{'true' if bwd else 'false'}, {tt}>", name
                    assert info.block % 64 == 0 and info.block == 64 * WAVES
                    nprob = n_outer * n_inner * heads
                    assert info.grid_y == 1 and info.grid_x == min(-(-nprob // WAVES), GRID_CAP) <= GRID_CAP
                    assert 0 < info.lds_bytes == info.lds_limit <= 160 * 1024
                    if header is not None:
                        assert info.lds_bytes == header[(bwd, tt)][0] == WAVES * header[(bwd, tt)][1]
                    # at least 8 waves per CU by LDS (and whole 4-wave workgroups of them)
                    assert (160 * 1024 // info.lds_bytes) * WAVES >= 8, (name, info.lds_bytes)
    # T <= 16 is accepted by the new entry points too (the 32-token instance)
    assert lib.mpv_temporal_attn_long_plan_describe(2, 6, 1, 2, 96, 0, C.byref(info)) == 0 and info.variant.decode().endswith(", 32>")
    for n_outer, n_inner, T, heads, hd in ((2, 6, 0, 2, 96), (2, 6, 65, 2, 96), (2, 6, 24, 2, 88), (2, 6, 24, 2, 112), (2, 6, 24, 2, 8),
                                           (0, 6, 24, 2, 96), (2, 0, 24, 2, 96), (2, 6, 24, 0, 96)):
        for bwd in (0, 1):
            assert lib.mpv_temporal_attn_long_plan_describe(n_outer, n_inner, T, heads, hd, bwd, C.byref(info)) != 0, (n_outer, n_inner, T, heads, hd)
            assert b"mpv_temporal_attn_long_plan_describe" in lib.mpv_last_error()
    assert lib.mpv_temporal_attn_long_plan_describe(2, 6, 24, 2, 96, 0, None) != 0
    assert b"mpv_temporal_attn_long_plan_describe" in lib.mpv_last_error()
    # null operands are refused before anything else is looked at (host only: no device is touched)
    assert lib.mpv_temporal_attn_long_fwd(None, None, 2, 24 * 7, 6, 1, 7, 24, 2, 96, 0.1, None) != 0
    assert b"mpv_temporal_attn_long_fwd" in lib.mpv_last_error()
    assert lib.mpv_temporal_attn_long_bwd(None, None, None, 2, 24 * 7, 6, 1, 7, 24, 2, 96, 0.1, None) != 0
    assert b"mpv_temporal_attn_long_bwd" in lib.mpv_last_error()


def test_old_family_still_refuses_long_clips():
    lib_mod = _binding()
    lib, info = lib_mod.lib(), lib_mod.AttnPlanInfo()
    assert lib.mpv_temporal_attn_plan_describe(2, 6, 16, 2, 96, 0, C.byref(info)) == 0
    assert info.variant.decode() == "temporal_attn_b16_kernel<false, 16, 96>"
    for T in (17, 32, 64):
        assert lib.mpv_temporal_attn_plan_describe(2, 6, T, 2, 96, 0, C.byref(info)) != 0
        assert b"mpv_temporal_attn_plan_describe" in lib.mpv_last_error() and b"[1,16]" in lib.mpv_last_error()


def test_ops_dispatch_by_clip_length(monkeypatch):
    """ops.temporal_attn_fwd / _bwd: the old entry points up to 16 frames, the new ones for 17..64, ValueError above -- before any
    launch (the library is replaced by a recorder here)."""
    from youku_mplug_amd import _lib, ops
    calls = []

    class Recorder:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a[-5])) or 0      # (entry point, T)

    monkeypatch.setattr(_lib, "lib", lambda: Recorder())
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    t = torch.zeros(8, dtype=torch.bfloat16)
    for T in (1, 8, 16, 17, 32, 64):
        ops.temporal_attn_fwd(t, t, 1, 1, 1, 0, 1, T, 1, 96, 0.1)
        ops.temporal_attn_bwd(t, t, t, 1, 1, 1, 0, 1, T, 1, 96, 0.1)
    short, long_ = ("mpv_temporal_attn_fwd", "mpv_temporal_attn_bwd"), ("mpv_temporal_attn_long_fwd", "mpv_temporal_attn_long_bwd")
    assert calls == [(n, T) for T in (1, 8, 16) for n in short] + [(n, T) for T in (17, 32, 64) for n in long_], calls
    for fn, args in ((ops.temporal_attn_fwd, (t, t)), (ops.temporal_attn_bwd, (t, t, t))):
        with pytest.raises(ValueError, match="at most 64 frames"):
            fn(*args, 1, 1, 1, 0, 1, 65, 1, 96, 0.1)
    assert len(calls) == 12


def test_new_kernels_fit_their_budget():
    """The four instances in the gfx950 code object: no scratch, and within the registers of two waves per SIMD (DESIGN.md
    section 15: 8 waves per CU), read the way tests/test_isa_cpu.py reads them."""
    import test_isa_cpu as isa
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not present")
    import tempfile
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for i, blob in enumerate(isa._code_objects()):
            f = os.path.join(d, f"co_{i}.elf")
            open(f, "wb").write(blob)
            txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout
            for blk in txt.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                if "temporal_attn_mfma_kernel" in name:
                    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                    found[name] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), scratch=g("private_segment_fixed_size"),
                                       lds=g("group_segment_fixed_size"))
    want = {f"25temporal_attn_mfma_kernelILb{b}ELi{tt}EE" for b in (0, 1) for tt in (32, 64)}
    assert len(found) == 4 and all(any(w in n for n in found) for w in want), sorted(found)
    for n, k in found.items():
        assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= VGPR_BUDGET and k["lds"] == 0, (n, k)      # (LDS is dynamic: the plan's)
    fwd32 = next(k for n, k in found.items() if "ILb0ELi32EE" in n)
    assert fwd32["vgpr"] + fwd32["agpr"] <= 128, fwd32          # the 32-token forward keeps four waves per SIMD


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _reference_available():
    from oracle.ref_loader import reference_available
    return reference_available()


@pytest.mark.skipif(not _reference_available(), reason="reference tree not found")
def test_restatement_at_24_frames_matches_reference_modules_live():
    """The yardstick of the GPU model tests at a frame count no golden covers: oracle.restate against the reference's own
    DistributedGPT3_Pretrain, fp32, at CONFIG_REF_MODULES' narrow widths with 24 frames -- loss, logits, last hidden state and
    every gradient (the bounds of tests/test_host_cpu.py::test_restatement_matches_reference_modules_live)."""
    from oracle import restate
    from oracle.gen_golden import CONFIG_REF_MODULES
    from oracle.ref_loader import build_reference_model, reference_forward
    from oracle.weights import make_inputs, make_state_dict
    cfg = dataclasses.replace(CONFIG_REF_MODULES, num_frames=24)
    model, sd = build_reference_model(cfg, 5)
    video, ids, mask = make_inputs(cfg, 3, 10, seed=11, ragged=True)
    loss, out, _ = reference_forward(model, video, ids, mask)
    loss.backward()
    sdd = {k: v.clone().requires_grad_(True) for k, v in make_state_dict(cfg, 5).items()}
    r = restate.pretrain_forward(video, ids, mask, sdd, cfg)
    r["loss"].backward()
    assert abs(r["loss"].item() - loss.item()) < 1e-5 * abs(loss.item())
    assert rel(r["logits"], out.logits.detach()) < 1e-5 and rel(r["last_hidden_state"], out.last_hidden_state.detach()) < 1e-5
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert any("temporal_attn" in n for n in grads) and "visual_encoder.temporal_embed" in grads
    for n, g in grads.items():
        assert rel(sdd[n].grad, g) < 1e-4, n


def test_host_pipeline_at_24_frames_on_standins(monkeypatch):
    """vision.py / pretrain.py at 24 frames on the stand-ins of tests/standin_ops.py (which take any T) against the fp32
    restatement on the bf16-rounded weights: loss within 1e-2 relative and logits within 2e-2 (the forward gates of the GPU
    model tests), and every trainable tensor's gradient within the README's whole-tensor relative-L2 gate of 3e-2, as on the GPU."""
    import standin_ops
    from oracle import restate
    from oracle.weights import CONFIG_TINY, make_inputs, make_state_dict
    from youku_mplug_amd.pretrain import synthetic_model
    standin_ops.install(monkeypatch)
    cfg = dataclasses.replace(CONFIG_TINY, num_frames=24)
    model = synthetic_model(cfg, device="cpu")
    sd = make_state_dict(cfg, 5)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    assert model.visual_encoder.temporal_embed.shape == (1, 24, cfg.vit_dim)
    video, ids, mask = make_inputs(cfg, 2, 12, seed=9, ragged=True)
    text = types.SimpleNamespace(input_ids=ids, attention_mask=mask)
    model.eval()
    out = model.forward_outputs(video.to(torch.bfloat16), text)
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    sdr = {k: v.bfloat16().float() for k, v in sd.items()}
    for k in trainable:
        sdr[k].requires_grad_(True)
    ref = restate.pretrain_forward(video.bfloat16().float(), ids, mask, sdr, cfg)
    assert abs(out.loss.item() - ref["loss"].item()) <= 1e-2 * abs(ref["loss"].item())
    assert rel(out.logits, ref["logits"].detach()) <= 2e-2
    ref["loss"].backward()
    loss, _ = model(video.to(torch.bfloat16), text)
    loss.backward()
    worst = (0.0, "")
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and sdr[n].grad is not None, n
            worst = max(worst, (((p.grad.float() - sdr[n].grad).norm() / (sdr[n].grad.norm() + 1e-30)).item(), n))
    print(f"    worst whole-tensor relative-L2 gradient distance on the stand-ins at 24 frames: {worst[0]:.3e} at {worst[1]}")
    assert worst[0] <= 3e-2, worst
