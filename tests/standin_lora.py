"""Torch stand-ins for the LoRA entry points (youku-mplug_amd/ops.py: lora_down / lora_up_add / lora_wgrad), TEST INFRASTRUCTURE ONLY,
in the manner of tests/standin_ops.py: the contract of include/mpv.h restated with plain indexing on host tensors -- bf16 storage, an fp32
accumulator holding the correctly rounded sum (formed in fp64), ONE bf16 rounding per output element, nothing touched outside
[R, r] / [R, N] / the g layout.  install(monkeypatch) layers them on standin_ops.install so that the host pipelines run their adapter
paths on the CPU."""
import torch

import standin_ops as so

BF = torch.bfloat16


def _ld(t, ld):
    return int(ld) if ld is not None else int(t.stride(0))


def _w(w, ldw, n, r, rank_major):
    """fp32 [n, r]: w(c, j)"""
    return so._rd(w, torch.arange(r), ldw, n).t() if rank_major else so._rd(w, torch.arange(n), ldw, r)


def _f32(scale):
    return float(torch.tensor(float(scale), dtype=torch.float32).item())


def lora_down(x, w, R, C, r, *, w_rank_major, scale=1.0, out=None, ldx=None, ldw=None, ldt=None):
    if out is None:
        out = torch.empty((R, r), dtype=BF, device=x.device)
    X, W = so._rd(x, torch.arange(R), _ld(x, ldx), C), _w(w, _ld(w, ldw), C, r, w_rank_major)
    acc = (X.double() @ W.double()).float()
    so._wr(out, torch.arange(R), _ld(out, ldt), acc * _f32(scale))
    return out


def lora_up_add(t, w, y, R, N, r, *, w_rank_major, scale=1.0, ldt=None, ldw=None, ldy=None):
    T, W = so._rd(t, torch.arange(R), _ld(t, ldt), r), _w(w, _ld(w, ldw), N, r, w_rank_major)
    acc = (T.double() @ W.double().t()).float()
    rows = torch.arange(R)
    so._wr(y, rows, _ld(y, ldy), so._rd(y, rows, _ld(y, ldy), N) + acc * _f32(scale))
    return y


def lora_wgrad(t, x, R, C, r, *, g_rank_major, scale=1.0, out=None, ldt=None, ldx=None, ldg=None):
    if out is None:
        out = torch.empty((r, C) if g_rank_major else (C, r), dtype=BF, device=x.device)
    T, X = so._rd(t, torch.arange(R), _ld(t, ldt), r), so._rd(x, torch.arange(R), _ld(x, ldx), C)
    g = (X.double().t() @ T.double()).float() * _f32(scale)              # [C, r]
    if g_rank_major:
        so._wr(out, torch.arange(r), _ld(out, ldg), g.t())
    else:
        so._wr(out, torch.arange(C), _ld(out, ldg), g)
    return out


NAMES = ["lora_down", "lora_up_add", "lora_wgrad"]


def install(monkeypatch):
    """standin_ops.install plus the three LoRA stand-ins"""
    so.install(monkeypatch)
    from youku_mplug_amd import ops
    g = globals()
    for n in NAMES:
        monkeypatch.setattr(ops, n, g[n])
