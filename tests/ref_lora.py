"""Plain fp64 reference of the LoRA products (csrc/lora.hip: mpv_lora_down / mpv_lora_up_add / mpv_lora_wgrad) as include/mpv.h documents
them, TEST INFRASTRUCTURE ONLY.  It looks neither at tests/standin_lora.py nor at the kernels' source.  tests/test_lora_refs_cpu.py
checks it against an independent einsum formulation; tests/test_lora_kernels_gpu.py compares the HIP kernels with it element by element.

Every output comes with its SCALE per element: the sum of the absolute terms that enter it,
    down:    |scale| sum_c |x||w|
    up_add:  |y_old| + |scale| sum_j |t||w|
    wgrad:   |scale| sum_i |t||x|
The gates of tests/lora_cases.py are rtol |ref| + coefficient x scale.  Each output is ONE bf16 rounding of an fp32 sum, so it is compared
with the fp64 value directly.

Operands are the 2-D [rows, ld] buffers the kernel is given.  w(c, j) = w[j, c] when rank_major (lora_A, [r, in]) and w[c, j] otherwise
(lora_B, [out, r]).  `scale` is taken as the float the C ABI passes."""
import torch

from ref_loss_optim import F64, close_elementwise, f32

TINY = 1e-300


def w_matrix(w, n, r, rank_major):
    """-> fp64 [n, r]: w(c, j)"""
    return w[:r, :n].to(F64).t() if rank_major else w[:n, :r].to(F64)


def down_ref(x, w, R, C, r, rank_major, scale):
    """-> (t [R, r], scale [R, r]) fp64"""
    s = f32(scale)
    X, W = x[:R, :C].to(F64), w_matrix(w, C, r, rank_major)
    return s * (X @ W), abs(s) * (X.abs() @ W.abs())


def up_add_ref(t, w, y_old, R, N, r, rank_major, scale):
    """-> (y [R, N], scale [R, N]) fp64; y_old: the prior contents of y"""
    s = f32(scale)
    T, W, Y = t[:R, :r].to(F64), w_matrix(w, N, r, rank_major), y_old[:R, :N].to(F64)
    return Y + s * (T @ W.t()), Y.abs() + abs(s) * (T.abs() @ W.abs().t())


def wgrad_ref(t, x, R, C, r, scale):
    """-> (g [C, r], scale [C, r]) fp64, g(c, j) whatever layout the kernel writes"""
    s = f32(scale)
    T, X = t[:R, :r].to(F64), x[:R, :C].to(F64)
    return s * (X.t() @ T), abs(s) * (X.abs().t() @ T.abs())


def close_scaled(got, ref, scale, gate, what):
    """|got - ref| <= rtol |ref| + coef * scale per element; the printed residual is the measured coefficient"""
    rtol, coef = gate
    g = got.detach().to(F64).cpu()
    assert tuple(g.shape) == tuple(ref.shape), f"{what}: shape {tuple(g.shape)} vs reference {tuple(ref.shape)}"
    s = scale.clamp_min(TINY)
    close_elementwise(g / s, ref / s, rtol, coef, what)
