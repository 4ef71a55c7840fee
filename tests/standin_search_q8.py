"""Torch stand-ins for the searches over an FP8 gallery (include/mpv.h, "Searches over an FP8 gallery": mpv_sim_*_q8,
mpv_maxsim_*_q8), TEST INFRASTRUCTURE ONLY.  The contract says what they are: the bf16 searches on the bf16 gallery
deq(code) * g_scale -- so each stand-in is the existing search stand-in (standin_search / standin_maxsim_search) called on
standin_w8.dequantize(codes, scale), after the refusals the ops add (codes uint8, one fp32 scale per row, no grouped queries).
`install(monkeypatch)` installs standin_maxsim_search (and with it standin_search and standin_ops), the quantiser of standin_w8,
and these on top."""
import torch

import standin_maxsim_search
import standin_search
import standin_w8


def dequantize(codes, g_scale):
    """bf16 deq(code) * scale of codes [.., dim] and scales [..] (exact for power-of-two scales)"""
    return standin_w8.dequantize(codes.reshape(-1, codes.shape[-1]), g_scale.reshape(-1)).view(codes.shape)


def _gallery(what, codes, g_scale, dims):
    from youku_mplug_amd._lib import MpvError
    if not torch.is_tensor(codes) or codes.dtype != torch.uint8:
        raise MpvError(f"{what}: gallery must be torch.uint8 (got {getattr(codes, 'dtype', type(codes))})")
    if codes.dim() not in dims or codes.shape[0] == 0:
        raise MpvError(f"{what}: bad gallery shape {tuple(codes.shape)}")
    if not torch.is_tensor(g_scale) or g_scale.dtype != torch.float32 or tuple(g_scale.shape) != tuple(codes.shape[:-1]):
        raise MpvError(f"{what}: g_scale must be float32 of shape {tuple(codes.shape[:-1])}")
    return dequantize(codes, g_scale)


def _single_row_queries(what, q):
    from youku_mplug_amd._lib import MpvError
    if torch.is_tensor(q) and q.dim() == 3 and q.shape[1] > 1:
        raise MpvError(f"{what}: q_group ({q.shape[1]}) must be 1 over a gallery of codes")


def sim_topk_q8(q, codes, g_scale, k, scale=None, slices=0):
    return standin_search.sim_topk(q, _gallery("sim_topk_q8", codes, g_scale, (2,)), k, scale=scale, slices=slices)


def sim_rank_q8(q, codes, g_scale, target, slices=0):
    return standin_search.sim_rank(q, _gallery("sim_rank_q8", codes, g_scale, (2,)), target, slices=slices)


def maxsim_topk_q8(q, codes, g_scale, k, scale=None, slices=0):
    _single_row_queries("maxsim_topk_q8", q)
    return standin_maxsim_search.maxsim_topk(q, _gallery("maxsim_topk_q8", codes, g_scale, (2, 3)), k, scale=scale, slices=slices)


def maxsim_rank_q8(q, codes, g_scale, target, slices=0):
    _single_row_queries("maxsim_rank_q8", q)
    return standin_maxsim_search.maxsim_rank(q, _gallery("maxsim_rank_q8", codes, g_scale, (2, 3)), target, slices=slices)


NAMES = ["sim_topk_q8", "sim_rank_q8", "maxsim_topk_q8", "maxsim_rank_q8"]


def install(monkeypatch):
    standin_maxsim_search.install(monkeypatch)
    from youku_mplug_amd import ops
    monkeypatch.setattr(ops, "quantize_rows_e4m3", standin_w8.quantize_rows_e4m3)
    g = globals()
    for n in NAMES:
        monkeypatch.setattr(ops, n, g[n])
