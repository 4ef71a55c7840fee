"""Torch stand-ins of the FP8 decoder-weight path (include/mpv.h, "FP8 decoder weights": mpv_quantize_rows_e4m3, mpv_gemm_w8,
mpv_gpt_decode_step_q8 / _shared_q8) on host tensors.  The quantiser restates the contract with torch's float8_e4m3fn conversion
and is the reference of the kernel's GPU test; the product and the steps are those of tests/standin_ops.py /
tests/standin_decode_shared.py on the dequantised weights -- deq(code) * scale is a bf16 number, so that IS the function the FP8
entries compute.  install() adds them to the stand-ins of those modules."""
import copy

import torch

import standin_decode_shared as sds
import standin_ops as so

BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def scale_exponent(amax):
    """fp32 amax [N] -> int32 e [N]: the smallest e with amax <= 448 * 2^e (448 = 0.875 * 2^9), 0 for a zero row, never below -126"""
    f, x = torch.frexp(amax)
    e = torch.where(f <= 0.875, x - 9, x - 8)
    return torch.where(amax > 0, e, torch.zeros_like(e)).clamp(min=-126)


def quantize_rows_e4m3(w, N=None, K=None, ldw=None):
    """ops.quantize_rows_e4m3: w [N, K] bf16 (a 2-D view carries its own row pitch) -> (codes uint8 [N, K], scale fp32 [N])"""
    N = w.shape[0] if N is None else N
    K = w.shape[1] if K is None else K
    if N < 1 or K < 1 or K % 16:
        raise ValueError("mpv_quantize_rows_e4m3: K must be a positive multiple of 16")
    rows = (w if w.dim() == 2 else so._flat(w).as_strided((N, K), (ldw or K, 1)))[:N, :K].float()
    scale = torch.ldexp(torch.ones(N, device=w.device), scale_exponent(rows.abs().amax(dim=1)))
    codes = (rows / scale[:, None]).to(F8).view(torch.uint8).contiguous()             # the division is exact: a power of two
    return codes, scale.float()


def dequantize(codes, scale):
    """bf16 deq(code) * scale (exact)"""
    return (codes.view(F8).float() * scale[:, None]).to(BF)


def gemm_w8(a, codes, scale, M, N, K, *, out=None, lda=None, ldw=None, ldc=None, bias=None, act=0, residual=None, ldr=0, cmap=so.IDENT,
            out_rows=None, **other):
    """ops.gemm_w8: refuses what the library refuses (ValueError here); the product is standin_ops.gemm on the dequantised weight"""
    if not 1 <= M <= 512 or N < 8 or N % 8 or K < 16 or K % 16:
        raise ValueError("mpv_gemm_w8: unsupported shape")
    if act not in (so.ACT_NONE, so.ACT_GELU_TANH) or any(other.values()):
        raise ValueError("mpv_gemm_w8: unsupported epilogue")
    w = dequantize(so._flat(codes).as_strided((N, K), (ldw or K, 1)), scale)
    return so.gemm(a, w, M, N, K, out=out, lda=lda, ldc=ldc, bias=bias, act=act, residual=residual, ldr=ldr, cmap=cmap, out_rows=out_rows)


def _dequantised_decoder(gpt, q8):
    """a copy of the decoder with q8's dequantised tensors loaded (kept on q8: one copy per quantisation)"""
    twin = getattr(q8, "_standin_twin", None)
    if twin is None:
        twin = copy.deepcopy(gpt)
        twin.clear_decode_weights()
        names = {id(p): n for n, p in gpt.named_parameters()}
        twin.load_state_dict({names[id(p)]: t for p, t in zip(q8.sources, q8.dequantized())}, strict=False)
        q8._standin_twin = twin
    return twin


def decode_step(self, tokens, query_embeds=None):
    """mpv_gpt_decode_step / mpv_gpt_decode_step_q8 behind generation.DecodeState.step"""
    if self.q8 is None:
        return so.decode_step(self, tokens, query_embeds)
    real, self.gpt = self.gpt, _dequantised_decoder(self.gpt, self.q8)
    try:
        return so.decode_step(self, tokens, query_embeds)
    finally:
        self.gpt = real


def shared_step(self, tokens):
    """mpv_gpt_decode_step_shared / _shared_q8 behind generation.SharedPrefixDecodeState._shared_step"""
    st = self.prefix
    if st.q8 is None:
        return sds.shared_step(self, tokens)
    real, st.gpt = st.gpt, _dequantised_decoder(st.gpt, st.q8)
    try:
        return sds.shared_step(self, tokens)
    finally:
        st.gpt = real


def install(monkeypatch):
    """standin_decode_shared.install (which includes standin_ops.install) plus the quantiser, the product and the FP8-aware steps"""
    sds.install(monkeypatch)
    from youku_mplug_amd import generation, ops
    monkeypatch.setattr(ops, "quantize_rows_e4m3", quantize_rows_e4m3)
    monkeypatch.setattr(ops, "gemm_w8", gemm_w8)
    monkeypatch.setattr(generation.DecodeState, "step", decode_step)
    monkeypatch.setattr(generation.SharedPrefixDecodeState, "_shared_step", shared_step)
