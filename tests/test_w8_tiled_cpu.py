"""The many-row FP8 product on the host (include/mpv.h, "FP8 decoder weights": mpv_gemm_w8_tiled): the row limits of header and
binding, the export and the host-side refusals of the entry, and the exact-arithmetic cases of tests/test_w8_tiled_gpu.py on a
stand-in (at a reduced K where the GPU test's K is 8192)."""
import ctypes
import os
import re

import pytest
import torch

import standin_w8 as sw
import w8_cases as wc

BF = torch.bfloat16


def gemm_w8_tiled(a, codes, scale, M, N, K, *, use_workspace=True, **kw):
    """ops.gemm_w8_tiled on host tensors: the contract is mpv_gemm_w8's, so the stand-in is too"""
    return sw.gemm_w8(a, codes, scale, M, N, K, **kw)


def test_header_and_binding_agree_on_the_row_limits():
    from youku_mplug_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mpv.h")).read()
    assert int(re.search(r"#define MPV_W8_TILED_MAX_ROWS (\d+)", text).group(1)) == _lib.W8_TILED_MAX_ROWS
    assert int(re.search(r"#define MPV_W8_MAX_ROWS (\d+)", text).group(1)) == _lib.W8_MAX_ROWS == 96
    assert _lib.W8_MAX_ROWS < _lib.W8_TILED_MAX_ROWS <= 512


def test_library_exports_the_tiled_entry_and_refuses_on_the_host():
    """every refusal is a negative code from host-side checks: no device is needed (and none is touched) to get it -- with and
    without a workspace"""
    from youku_mplug_amd import _lib
    lib = _lib.lib()
    assert "mpv_gemm_w8_tiled" in _lib.EXPORTS and hasattr(lib, "mpv_gemm_w8_tiled")
    A, W, S, Cc, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x60000                      # never dereferenced on the host
    good = dict(A=A, W=W, S=S, C=Cc, M=160, N=64, K=128, lda=128, ldw=128, ldc=64)

    def call(ep=None, ws=(None, 0), **over):
        a = dict(good, **over)
        return lib.mpv_gemm_w8_tiled(a["A"], a["W"], a["S"], a["C"], a["M"], a["N"], a["K"], a["lda"], a["ldw"], a["ldc"],
                                     None if ep is None else ctypes.byref(ep), ws[0], ws[1], None)
    for ws in ((None, 0), (WS, 1 << 20)):
        for over, code in ((dict(M=0), -1), (dict(M=513), -1), (dict(K=120), -1), (dict(N=60), -1), (dict(K=0), -1), (dict(lda=64), -1),
                           (dict(ldc=56), -1), (dict(A=None), -5), (dict(W=None), -5), (dict(S=None), -5), (dict(C=None), -5),
                           (dict(A=A + 8), -2), (dict(ldw=136), -2)):
            assert call(ws=ws, **over) == code, over
            assert b"mpv_gemm_w8_tiled" in lib.mpv_last_error()
        for field, value in (("out_f32", 1), ("accumulate", 1), ("act", 1), ("act", 3), ("act_bwd", 2), ("a_group", 2), ("k_group", 2),
                             ("preact_out", 0x50000), ("act_bwd_z", 0x50000), ("dropout_p", 0.1), ("alpha", 2.0), ("alpha_dev", 0x50000),
                             ("colsum_out", 0x50000), ("row_tap_out", 0x50000), ("tile_hint", 128), ("split_hint", 2), ("colscale_cols", 8),
                             ("keep_output", 1), ("preact_deriv", 1)):
            ep = _lib.GemmEpilogue()
            setattr(ep, field, value)
            assert call(ep, ws=ws) == -5, field
        ep = _lib.GemmEpilogue()
        ep.ldr = 72                                                                     # a residual pitch without a residual
        assert call(ep, ws=ws) == -5


@pytest.mark.parametrize("M,N,K", [(97, 64, 1024), (160, 64, 1024), (512, 64, 1024), (101, 40, 1040), (512, 4096, 384), (160, 6144, 272),
                                   (500, 8200, 144), (500, 2048, 272)],
                         ids=lambda v: str(v))
def test_standin_on_the_exact_cases(M, N, K):
    """the stand-in's fp32 product of the exact construction IS the fp64 result (so its bf16 rounding is what the GPU test expects),
    and the partial sums stay exact: below 2^24 in units of the products' common 2^-5"""
    a, codes, scale, want = wc.exact_case(M, N, K)
    got = gemm_w8_tiled(a, codes, scale, M, N, K)
    assert torch.equal(got.float(), want.to(BF).float())
    unscaled = want / scale.double()[None]
    assert unscaled.abs().max() < 2.0 ** 18 and torch.equal(unscaled * 32, (unscaled * 32).round())
    with pytest.raises(ValueError):
        gemm_w8_tiled(a, codes, scale, 513, N, K)
    with pytest.raises(ValueError):
        gemm_w8_tiled(a, codes, scale, M, N, K, out_f32=1)
