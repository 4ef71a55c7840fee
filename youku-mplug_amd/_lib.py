"""ctypes binding of libmpv_hip.so (the C ABI declared in include/mpv.h).

The product path has NO CPU / PyTorch fallback: if the library is missing or a call fails
this module raises.  Build with `python __graft_entry__.py` (or `make -C youku-mplug_amd/csrc`).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPV_LIB_PATH") or os.path.join(_HERE, "libmpv_hip.so")   # override: instrumented measurement builds only

c_void_p, c_int, c_int64, c_float, c_uint64, c_size_t = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint64, C.c_size_t


class GemmEpilogue(C.Structure):
    _fields_ = [
        ("a_group", c_int), ("a_stride", c_int), ("a_offset", c_int),
        ("c_group", c_int), ("c_stride", c_int), ("c_offset", c_int),
        ("k_group", c_int), ("k_stride", c_int), ("k_offset", c_int),
        ("bias", c_void_p), ("act", c_int), ("preact_out", c_void_p),
        ("residual", c_void_p), ("ldr", c_int64),
        ("act_bwd_z", c_void_p), ("ldz", c_int64), ("act_bwd", c_int),
        ("dropout_p", c_float), ("seed", c_uint64), ("offset", c_uint64),
        ("alpha_dev", c_void_p), ("alpha", c_float), ("out_f32", c_int), ("accumulate", c_int),
        ("colsum_out", c_void_p), ("tile_hint", c_int), ("row_tap_out", c_void_p), ("row_tap_group", c_int), ("split_hint", c_int), ("gm_hint", c_int), ("preact_deriv", c_int), ("keep_output", c_int),
        ("colscale", c_float), ("colscale_cols", c_int),
    ]


class AttnDesc(C.Structure):
    _fields_ = [
        ("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("o", c_void_p), ("lse", c_void_p),
        ("q_bs", c_int64), ("q_hs", c_int64), ("q_rs", c_int64),
        ("k_bs", c_int64), ("k_hs", c_int64), ("k_rs", c_int64),
        ("v_bs", c_int64), ("v_hs", c_int64), ("v_rs", c_int64),
        ("o_bs", c_int64), ("o_hs", c_int64), ("o_rs", c_int64),
        ("batch", c_int), ("heads", c_int), ("sq", c_int), ("sk", c_int), ("head_dim", c_int),
        ("causal", c_int), ("scale", c_float), ("scale_q_bf16", c_int),
        ("dropout_p", c_float), ("seed", c_uint64), ("offset", c_uint64),
    ]


class AttnPlanInfo(C.Structure):
    _fields_ = [("variant", C.c_char_p), ("grid_x", C.c_uint), ("grid_y", C.c_uint), ("block", c_int), ("lds_bytes", c_int),
                ("lds_limit", c_int)]


class AttnPrefixDesc(C.Structure):
    _fields_ = [
        ("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("pk", c_void_p), ("pv", c_void_p), ("o", c_void_p),
        ("q_cs", c_int64), ("q_hs", c_int64), ("q_rs", c_int64),
        ("k_cs", c_int64), ("k_hs", c_int64), ("k_rs", c_int64),
        ("v_cs", c_int64), ("v_hs", c_int64), ("v_rs", c_int64),
        ("pk_gs", c_int64), ("pk_hs", c_int64), ("pk_rs", c_int64),
        ("pv_gs", c_int64), ("pv_hs", c_int64), ("pv_rs", c_int64),
        ("o_cs", c_int64), ("o_hs", c_int64), ("o_rs", c_int64),
        ("n_cont", c_int), ("group_size", c_int), ("n_groups", c_int), ("heads", c_int), ("cont_len", c_int),
        ("prefix_len", c_int), ("head_dim", c_int), ("scale", c_float),
    ]


class AttnPrefixPackedDesc(C.Structure):
    _fields_ = [
        ("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("pk", c_void_p), ("pv", c_void_p), ("o", c_void_p),
        ("seg_start", c_void_p), ("group_row", c_void_p),
        ("q_rs", c_int64), ("q_hs", c_int64), ("k_rs", c_int64), ("k_hs", c_int64), ("v_rs", c_int64), ("v_hs", c_int64),
        ("o_rs", c_int64), ("o_hs", c_int64),
        ("pk_gs", c_int64), ("pk_hs", c_int64), ("pk_rs", c_int64),
        ("pv_gs", c_int64), ("pv_hs", c_int64), ("pv_rs", c_int64),
        ("rows", c_int), ("n_groups", c_int), ("heads", c_int), ("prefix_len", c_int), ("head_dim", c_int), ("max_group_rows", c_int),
        ("scale", c_float),
    ]


class AttnPrefixPackedBwdDesc(C.Structure):
    _fields_ = [
        ("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("o", c_void_p), ("dO", c_void_p), ("pk", c_void_p), ("pv", c_void_p),
        ("lse", c_void_p), ("delta", c_void_p), ("dq", c_void_p), ("dk", c_void_p), ("dv", c_void_p), ("dpk", c_void_p), ("dpv", c_void_p),
        ("seg_start", c_void_p), ("group_row", c_void_p),
        ("q_rs", c_int64), ("q_hs", c_int64), ("k_rs", c_int64), ("k_hs", c_int64), ("v_rs", c_int64), ("v_hs", c_int64),
        ("o_rs", c_int64), ("o_hs", c_int64),
        ("pk_gs", c_int64), ("pk_hs", c_int64), ("pk_rs", c_int64),
        ("pv_gs", c_int64), ("pv_hs", c_int64), ("pv_rs", c_int64),
        ("rows", c_int), ("n_groups", c_int), ("heads", c_int), ("prefix_len", c_int), ("head_dim", c_int), ("max_group_rows", c_int),
        ("accumulate_prefix", c_int), ("scale", c_float),
    ]


class AttnDecodeSharedDesc(C.Structure):
    _fields_ = [
        ("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("pk", c_void_p), ("pv", c_void_p), ("o", c_void_p),
        ("q_ss", c_int64), ("q_hs", c_int64),
        ("k_ss", c_int64), ("k_hs", c_int64), ("k_rs", c_int64),
        ("v_ss", c_int64), ("v_hs", c_int64), ("v_rs", c_int64),
        ("pk_gs", c_int64), ("pk_hs", c_int64), ("pk_rs", c_int64),
        ("pv_gs", c_int64), ("pv_hs", c_int64), ("pv_rs", c_int64),
        ("o_ss", c_int64), ("o_hs", c_int64),
        ("n_seq", c_int), ("group_size", c_int), ("n_groups", c_int), ("heads", c_int), ("prefix_len", c_int),
        ("own_len", c_int), ("head_dim", c_int), ("scale", c_float),
    ]


class SimSearchDesc(C.Structure):
    _fields_ = [
        ("queries", c_void_p), ("gallery", c_void_p), ("q_rs", c_int64), ("g_rs", c_int64), ("nq", c_int64), ("ng", c_int64),
        ("dim", c_int), ("k", c_int), ("slices", c_int), ("scale", c_float),
    ]


class SimBankDesc(C.Structure):
    _fields_ = [
        ("bank", c_void_p), ("gallery", c_void_p), ("b_rs", c_int64), ("g_rs", c_int64), ("nb", c_int64), ("ng", c_int64),
        ("dim", c_int), ("beta", c_float),
    ]


class MaxSimSearchDesc(C.Structure):
    _fields_ = [
        ("queries", c_void_p), ("gallery", c_void_p), ("q_rs", c_int64), ("g_rs", c_int64), ("nq", c_int64), ("ng", c_int64),
        ("q_group", c_int), ("g_group", c_int), ("dim", c_int), ("k", c_int), ("slices", c_int), ("scale", c_float),
    ]


class BeamAdvanceDesc(C.Structure):
    _fields_ = [(n, c_void_p) for n in ("cand_val", "cand_idx", "tokens_in", "tokens_out", "scores", "hyp_score", "hyp_order", "hyp_tokens",
                                        "hyp_count", "hyp_next", "worst", "done", "src_row", "next_tok")] + \
               [(n, c_int) for n in ("batch", "beams", "row_len", "vocab", "pos", "cur_len", "first")] + [("stop_token", c_int64)]


class BeamAdvanceGroupsDesc(C.Structure):
    _fields_ = [(n, c_void_p) for n in ("cand_val", "cand_idx", "tokens_in", "tokens_out", "scores", "hyp_score", "hyp_order", "hyp_tokens",
                                        "hyp_count", "hyp_next", "worst", "done", "src_row", "next_tok")] + \
               [(n, c_int) for n in ("batch", "beams", "row_len", "vocab", "pos", "cur_len", "first", "groups")] + \
               [("diversity_penalty", c_float), ("stop_token", c_int64)]


class SampleAdvanceDesc(C.Structure):
    _fields_ = [(n, c_void_p) for n in ("logits", "stream_id", "u_override", "prompt_len", "tokens", "done", "next_tok", "n_done", "out_kept",
                                        "out_mass", "out_token")] + \
               [("ld", c_int64), ("seed", c_uint64), ("termination_id", c_int64)] + \
               [(n, c_int) for n in ("rows", "vocab", "row_len", "pos", "top_k", "vocab_size", "termination_mode")] + \
               [("temperature", c_float), ("top_p", c_float)]


class LogitsConstrainDesc(C.Structure):
    _fields_ = [(n, c_void_p) for n in ("logits", "tokens", "prompt_len", "eos_ids", "banned_ids")] + \
               [("ld", c_int64), ("prompt_len_all", c_int64)] + \
               [(n, c_int) for n in ("rows", "vocab", "row_len", "pos", "n_eos", "n_banned", "ngram", "min_new_tokens", "include_prompt")] + \
               [("penalty", c_float), ("ban_value", c_float)]


class LogitsGuideDesc(C.Structure):
    _fields_ = [("cond", c_void_p), ("uncond", c_void_p), ("ld_c", c_int64), ("ld_u", c_int64), ("rows", c_int), ("vocab", c_int),
                ("scale_m1", c_float), ("plaus_log", c_float), ("ban_value", c_float)]


class LogitsTrieDesc(C.Structure):
    _fields_ = [(n, c_void_p) for n in ("logits", "tokens", "prompt_len", "eos_ids", "child_begin", "child_tok", "child_node", "terminal", "node_out")] + \
               [("ld", c_int64), ("prompt_len_all", c_int64)] + \
               [(n, c_int) for n in ("rows", "vocab", "row_len", "pos", "n_eos", "n_nodes", "n_edges")] + [("ban_value", c_float)]


class SampleScoreDesc(C.Structure):
    _fields_ = [(n, c_void_p) for n in ("logits", "tokens", "prompt_len", "done", "live", "token_logprob", "sum_logprob", "count")] + \
               [("ld", c_int64)] + [(n, c_int) for n in ("rows", "vocab", "row_len", "pos")]


class CaptionOverlapDesc(C.Structure):
    _fields_ = [(n, c_void_p) for n in ("tok_a", "tok_b", "start_a", "start_b", "begin_a", "begin_b", "pair_begin", "len_a", "len_b", "counts",
                                        "host_start_a", "host_start_b", "host_begin_a", "host_begin_b", "host_pair_begin")] + \
               [("ld_a", c_int64), ("ld_b", c_int64), ("term", c_int64)] + \
               [(n, c_int) for n in ("rows_a", "rows_b", "width_a", "width_b", "groups")]


CAPTION_OVERLAP_MAX_LEN = 255   # include/mpv.h MPV_CAPTION_OVERLAP_MAX_LEN


class CaptionCiderDesc(C.Structure):
    _fields_ = [(n, c_void_p) for n in ("tok_a", "tok_b", "start_a", "start_b", "begin_a", "begin_b", "pair_begin", "table_keys", "table_idf",
                                        "pair", "score", "host_start_a", "host_start_b", "host_begin_a", "host_begin_b", "host_pair_begin")] + \
               [("ld_a", c_int64), ("ld_b", c_int64), ("term", c_int64), ("table_capacity", c_int64)] + \
               [("log_ref_len", C.c_double), ("sigma", C.c_double)] + \
               [(n, c_int) for n in ("rows_a", "rows_b", "width_a", "width_b", "groups")]


CAPTION_CIDER_ORDERS = 4        # include/mpv.h MPV_CAPTION_CIDER_ORDERS

_RM = [c_int, c_int, c_int]
_SIGS = {
    "mpv_version": (c_int, []),
    "mpv_last_error": (C.c_char_p, []),
    "mpv_check_device": (c_int, []),
    "mpv_check_arch_name": (c_int, [C.c_char_p]),
    "mpv_gemm_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int, c_int]),
    "mpv_gemm_plan_bands": (c_int, [c_int64, c_int64, c_int64, c_int, c_int, c_int, C.POINTER(c_int)]),
    "mpv_gemm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                              c_int, c_int, C.POINTER(GemmEpilogue), c_void_p, c_size_t, c_void_p]),
    "mpv_layernorm_fwd": (c_int, [c_void_p] * 6 + [c_int64] * 4 + [c_float] + _RM + _RM + [c_void_p]),
    "mpv_layernorm_bwd_workspace_size": (c_size_t, [c_int64]),
    "mpv_layernorm_bwd": (c_int, [c_void_p] * 8 + [c_float, c_uint64, c_uint64, c_void_p, c_void_p, c_int] +
                          [c_int64] * 4 + _RM + _RM + [c_void_p, c_size_t, c_void_p]),
    "mpv_ln_stream_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int64] * 5 +
                          [c_float] + _RM + _RM + _RM + [c_void_p]),
    "mpv_ln_stream_fwd_drop": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int64] * 5 +
                               [c_float] + _RM + _RM + _RM + [c_float, c_uint64, c_uint64, c_void_p]),
    "mpv_ln_stream_bwd": (c_int, [c_void_p] * 8 + [c_float, c_uint64, c_uint64] + [c_int64] * 4 + _RM + _RM + [c_void_p]),
    "mpv_attn_fwd": (c_int, [C.POINTER(AttnDesc), c_void_p]),
    "mpv_attn_bwd": (c_int, [C.POINTER(AttnDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mpv_attn_plan_describe": (c_int, [C.POINTER(AttnDesc), c_int, C.POINTER(AttnPlanInfo)]),
    "mpv_temporal_attn_plan_describe": (c_int, [c_int] * 6 + [C.POINTER(AttnPlanInfo)]),
    "mpv_attn_prefix_fwd": (c_int, [C.POINTER(AttnPrefixDesc), c_void_p]),
    "mpv_attn_prefix_packed_fwd": (c_int, [C.POINTER(AttnPrefixPackedDesc), c_void_p]),
    "mpv_attn_prefix_packed_fwd_lse": (c_int, [C.POINTER(AttnPrefixPackedDesc), c_void_p, c_void_p]),
    "mpv_attn_prefix_packed_bwd": (c_int, [C.POINTER(AttnPrefixPackedBwdDesc), c_void_p]),
    "mpv_attn_prefix_packed_layout": (c_int, [C.POINTER(C.c_int32), c_int, C.POINTER(C.c_int32), c_int, C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32), C.POINTER(c_int), C.POINTER(c_int)]),
    "mpv_attn_decode_shared_fwd": (c_int, [C.POINTER(AttnDecodeSharedDesc), c_void_p]),
    "mpv_temporal_attn_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int64, c_int, c_int, c_int,
                                      c_float, c_void_p]),
    "mpv_temporal_attn_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int64, c_int,
                                      c_int, c_int, c_float, c_void_p]),
    "mpv_temporal_attn_long_plan_describe": (c_int, [c_int] * 6 + [C.POINTER(AttnPlanInfo)]),
    "mpv_temporal_attn_long_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int64, c_int, c_int, c_int,
                                           c_float, c_void_p]),
    "mpv_temporal_attn_long_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int64, c_int64, c_int,
                                           c_int, c_int, c_float, c_void_p]),
    "mpv_im2col_patches": (c_int, [c_void_p, c_void_p] + [c_int] * 7 + [c_void_p]),
    "mpv_vit_embed_assemble_fwd": (c_int, [c_void_p] * 5 + [c_int] * 4 + [c_void_p]),
    "mpv_vit_embed_assemble_bwd": (c_int, [c_void_p] * 5 + [c_int] * 4 + [c_void_p]),
    "mpv_vit_cls_merge_fwd": (c_int, [c_void_p] * 3 + [c_int] * 4 + [c_void_p]),
    "mpv_vit_cls_merge_bwd": (c_int, [c_void_p] * 2 + [c_int] * 4 + [c_void_p]),
    "mpv_vit_cls_fix_fwd": (c_int, [c_void_p] * 3 + [c_int] * 4 + [c_void_p]),
    "mpv_vit_cls_merge_bwd_inplace": (c_int, [c_void_p] * 2 + [c_int] * 4 + [c_void_p]),
    "mpv_copy_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64] + _RM + _RM + [c_void_p]),
    "mpv_colsum_workspace_size": (c_size_t, [c_int64]),
    "mpv_colsum": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64] + _RM + [c_int, c_void_p, c_size_t, c_void_p]),
    "mpv_add": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mpv_accum_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "mpv_store_words": (c_int, [c_void_p, C.POINTER(C.c_uint32), c_int, c_void_p]),
    "mpv_f32_to_bf16": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "mpv_copy_segments": (c_int, [C.POINTER(c_void_p), C.POINTER(c_void_p), C.POINTER(c_int64), c_int, c_void_p]),
    "mpv_vit_compose_bwd_finish": (c_int, [c_void_p] * 6 + [c_int, c_void_p]),
    "mpv_vit_compose_bias_batched": (c_int, [C.POINTER(c_void_p)] * 4 + [c_int, c_int, c_void_p]),
    "mpv_vit_compose_bwd_finish_batched": (c_int, [C.POINTER(c_void_p)] * 6 + [c_int, c_int, c_void_p]),
    "mpv_gemm_bf16_batched": (c_int, [C.POINTER(c_void_p)] * 3 + [c_int] + [c_int64] * 6 + [c_int, c_int, c_void_p]),
    "mpv_caption_targets": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mpv_layernorm_bwd_partial_rows": (c_int, [c_int64]),
    "mpv_layernorm_dparam_finish": (c_int, [C.POINTER(c_void_p), C.POINTER(c_int), C.POINTER(c_void_p), C.POINTER(c_void_p),
                                            C.POINTER(c_int), c_int, c_int64, c_void_p]),
    "mpv_gpt_embed_fwd": (c_int, [c_void_p] * 5 + [c_int] * 4 + [c_float, c_uint64, c_uint64, c_void_p]),
    "mpv_gpt_embed_rows_fwd": (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_void_p]),
    "mpv_gpt_embed_bwd": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_float, c_uint64, c_uint64, c_void_p]),
    "mpv_gpt_embed_bwd_full": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_uint64, c_uint64, c_void_p]),
    "mpv_cross_entropy": (c_int, [c_void_p] * 6 + [c_int64] * 3 + [c_void_p]),
    "mpv_l2norm_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_void_p]),
    "mpv_l2norm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "mpv_gather_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p]),
    "mpv_video_resized_crop_normalize": (c_int, [c_void_p] + [c_int] * 11 + [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "mpv_video_resized_crop_u8": (c_int, [c_void_p] + [c_int] * 11 + [c_void_p, c_void_p]),
    "mpv_video_aug_pointwise": (c_int, [c_void_p, c_int, c_int, c_int, c_int, C.c_double, c_void_p, c_void_p]),
    "mpv_video_aug_sharpness": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, C.c_double, c_void_p]),
    "mpv_video_aug_warp_affine": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint8), c_void_p]),
    "mpv_video_u8_normalize": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "mpv_scatter_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p]),
    "mpv_gather_rows_ld": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p]),
    "mpv_logprob_topk_workspace_size": (c_size_t, [c_int64, c_int]),
    "mpv_logprob_topk": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_beam_advance": (c_int, [C.POINTER(BeamAdvanceDesc), c_void_p]),
    "mpv_beam_advance_groups": (c_int, [C.POINTER(BeamAdvanceGroupsDesc), c_void_p]),
    "mpv_sample_advance": (c_int, [C.POINTER(SampleAdvanceDesc), c_void_p]),
    "mpv_logits_constrain": (c_int, [C.POINTER(LogitsConstrainDesc), c_void_p]),
    "mpv_sample_score": (c_int, [C.POINTER(SampleScoreDesc), c_void_p]),
    "mpv_sample_advance_ragged": (c_int, [C.POINTER(SampleAdvanceDesc), c_void_p]),
    "mpv_logits_constrain_ragged": (c_int, [C.POINTER(LogitsConstrainDesc), c_void_p]),
    "mpv_sample_score_ragged": (c_int, [C.POINTER(SampleScoreDesc), c_void_p]),
    "mpv_soft_target_ce": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "mpv_maxsim_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p]),
    "mpv_maxsim_route": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p]),
    "mpv_smoothed_ce": (c_int, [c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "mpv_sim_topk_workspace_size": (c_size_t, [C.POINTER(SimSearchDesc)]),
    "mpv_sim_topk": (c_int, [C.POINTER(SimSearchDesc), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_sim_rank_workspace_size": (c_size_t, [C.POINTER(SimSearchDesc), c_int]),
    "mpv_sim_rank": (c_int, [C.POINTER(SimSearchDesc), c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_maxsim_topk_workspace_size": (c_size_t, [C.POINTER(MaxSimSearchDesc)]),
    "mpv_maxsim_topk": (c_int, [C.POINTER(MaxSimSearchDesc), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_maxsim_rank_workspace_size": (c_size_t, [C.POINTER(MaxSimSearchDesc), c_int]),
    "mpv_maxsim_rank": (c_int, [C.POINTER(MaxSimSearchDesc), c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    # the searches over e4m3 codes: the same descriptors plus g_scale (fp32 per gallery row)
    "mpv_sim_topk_q8_workspace_size": (c_size_t, [C.POINTER(SimSearchDesc), c_void_p]),
    "mpv_sim_topk_q8": (c_int, [C.POINTER(SimSearchDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_sim_rank_q8_workspace_size": (c_size_t, [C.POINTER(SimSearchDesc), c_void_p, c_int]),
    "mpv_sim_rank_q8": (c_int, [C.POINTER(SimSearchDesc), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_maxsim_topk_q8_workspace_size": (c_size_t, [C.POINTER(MaxSimSearchDesc), c_void_p]),
    "mpv_maxsim_topk_q8": (c_int, [C.POINTER(MaxSimSearchDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_maxsim_rank_q8_workspace_size": (c_size_t, [C.POINTER(MaxSimSearchDesc), c_void_p, c_int]),
    "mpv_maxsim_rank_q8": (c_int, [C.POINTER(MaxSimSearchDesc), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    # searches with per-row priors, and the bank pass of the inverted-softmax correction
    "mpv_sim_topk_prior_workspace_size": (c_size_t, [C.POINTER(SimSearchDesc), c_void_p]),
    "mpv_sim_topk_prior": (c_int, [C.POINTER(SimSearchDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_sim_rank_prior_workspace_size": (c_size_t, [C.POINTER(SimSearchDesc), c_void_p, c_int]),
    "mpv_sim_rank_prior": (c_int, [C.POINTER(SimSearchDesc), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_sim_topk_prior_q8_workspace_size": (c_size_t, [C.POINTER(SimSearchDesc), c_void_p, c_void_p]),
    "mpv_sim_topk_prior_q8": (c_int, [C.POINTER(SimSearchDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_sim_rank_prior_q8_workspace_size": (c_size_t, [C.POINTER(SimSearchDesc), c_void_p, c_void_p, c_int]),
    "mpv_sim_rank_prior_q8": (c_int, [C.POINTER(SimSearchDesc), c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "mpv_sim_bank_lse_workspace_size": (c_size_t, [C.POINTER(SimBankDesc)]),
    "mpv_sim_bank_lse": (c_int, [C.POINTER(SimBankDesc), c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_sim_bank_lse_q8_workspace_size": (c_size_t, [C.POINTER(SimBankDesc), c_void_p]),
    "mpv_sim_bank_lse_q8": (c_int, [C.POINTER(SimBankDesc), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_grad_sumsq_workspace_size": (c_size_t, []),
    "mpv_grad_sumsq": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mpv_adamw_step": (c_int, [c_void_p] * 5 + [c_int64] + [c_float] * 5 + [c_int, c_float, c_void_p, c_float, c_void_p]),
    "mpv_adamw_hyper_pack": (c_int, [C.POINTER(c_float), C.POINTER(c_float), c_int, c_float, c_float, c_int, C.POINTER(c_float)]),
    "mpv_adamw_step_grouped_dev": (c_int, [c_void_p] * 5 + [c_int64, c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_void_p,
                                           c_float, c_void_p]),
    "mpv_adamw_step_grouped": (c_int, [c_void_p] * 5 + [c_int64, c_void_p, C.POINTER(c_float), C.POINTER(c_float), c_int,
                                       c_float, c_float, c_float, c_int, c_float, c_void_p, c_float, c_void_p]),
}
class GptLayerWeights(C.Structure):
    _fields_ = [(n, c_void_p) for n in ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "dense_w", "dense_b", "ln2_w", "ln2_b", "fc1_w", "fc1_b",
                                        "fc2_w", "fc2_b")]


class GptWeights(C.Structure):
    _fields_ = [("layers", c_int), ("hidden", c_int), ("heads", c_int), ("ffn", c_int), ("vocab", c_int), ("ln_eps", c_float),
                ("layer", C.POINTER(GptLayerWeights)), ("wte", c_void_p), ("wpe", c_void_p), ("lnf_w", c_void_p), ("lnf_b", c_void_p),
                ("max_positions", c_int)]


class GptLayerWeightsQ8(C.Structure):
    _fields_ = [(n, c_void_p) for n in ("qkv_q", "qkv_s", "dense_q", "dense_s", "fc1_q", "fc1_s", "fc2_q", "fc2_s")]


class GptWeightsQ8(C.Structure):
    _fields_ = [("layers", c_int), ("layer", C.POINTER(GptLayerWeightsQ8)), ("wte_q", c_void_p), ("wte_s", c_void_p)]


W8_MAX_ROWS = 96       # include/mpv.h MPV_W8_MAX_ROWS
W8_TILED_MAX_ROWS = 512  # include/mpv.h MPV_W8_TILED_MAX_ROWS

_SIGS.update({
    "mpv_gpt_decode_workspace_size": (c_size_t, [C.POINTER(GptWeights), c_int, c_int]),
    "mpv_gpt_decode_step": (c_int, [C.POINTER(GptWeights), C.POINTER(c_void_p), c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                    c_void_p, c_size_t, c_void_p, c_void_p]),
    "mpv_kv_reorder": (c_int, [C.POINTER(c_void_p), C.POINTER(c_void_p), c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "mpv_gpt_decode_shared_workspace_size": (c_size_t, [C.POINTER(GptWeights), c_int]),
    "mpv_gpt_decode_step_shared": (c_int, [C.POINTER(GptWeights), C.POINTER(c_void_p), C.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int,
                                           c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mpv_quantize_rows_e4m3": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "mpv_gemm_w8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                            C.POINTER(GemmEpilogue), c_void_p]),
    "mpv_gemm_w8_tiled": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                  C.POINTER(GemmEpilogue), c_void_p, c_size_t, c_void_p]),
    "mpv_gpt_embed_w8_fwd": (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_void_p]),
    "mpv_gpt_decode_step_q8": (c_int, [C.POINTER(GptWeights), C.POINTER(GptWeightsQ8), C.POINTER(c_void_p), c_int, c_int, c_int, c_void_p,
                                       c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mpv_gpt_decode_step_shared_q8": (c_int, [C.POINTER(GptWeights), C.POINTER(GptWeightsQ8), C.POINTER(c_void_p), C.POINTER(c_void_p), c_int,
                                              c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mpv_attn_decode_shared_ragged_fwd": (c_int, [C.POINTER(AttnDecodeSharedDesc), c_void_p, c_void_p]),
    "mpv_gpt_embed_rows_w8_fwd": (c_int, [c_void_p] * 6 + [c_int] * 3 + [c_void_p]),
    "mpv_gpt_decode_step_shared_ragged": (c_int, [C.POINTER(GptWeights), C.POINTER(c_void_p), C.POINTER(c_void_p), c_int, c_int, c_int,
                                                  c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mpv_gpt_decode_step_shared_ragged_q8": (c_int, [C.POINTER(GptWeights), C.POINTER(GptWeightsQ8), C.POINTER(c_void_p), C.POINTER(c_void_p),
                                                     c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                                     c_void_p, c_void_p]),
    "mpv_gpt_prefill_ragged": (c_int, [C.POINTER(GptWeights), C.POINTER(c_void_p), c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                       c_void_p, c_size_t, c_void_p, c_void_p]),
    "mpv_gpt_prefill_ragged_q8": (c_int, [C.POINTER(GptWeights), C.POINTER(GptWeightsQ8), C.POINTER(c_void_p), c_int, c_int, c_void_p, c_int,
                                          c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mpv_attn_decode_shared_steps_fwd": (c_int, [C.POINTER(AttnDecodeSharedDesc), c_void_p, c_void_p, c_void_p]),
    "mpv_gpt_decode_shared_steps_workspace_size": (c_size_t, [C.POINTER(GptWeights), c_int]),
    "mpv_gpt_decode_step_shared_steps": (c_int, [C.POINTER(GptWeights), C.POINTER(c_void_p), C.POINTER(c_void_p), c_int, c_int, c_int,
                                                 c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mpv_gpt_decode_step_shared_steps_q8": (c_int, [C.POINTER(GptWeights), C.POINTER(GptWeightsQ8), C.POINTER(c_void_p), C.POINTER(c_void_p),
                                                    c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                                    c_void_p, c_void_p]),
    "mpv_sample_advance_steps": (c_int, [C.POINTER(SampleAdvanceDesc), c_void_p, c_void_p]),
    "mpv_logits_constrain_steps": (c_int, [C.POINTER(LogitsConstrainDesc), c_void_p, c_void_p]),
    "mpv_sample_score_steps": (c_int, [C.POINTER(SampleScoreDesc), c_void_p, c_void_p]),
    "mpv_beam_advance_steps": (c_int, [C.POINTER(BeamAdvanceGroupsDesc), c_void_p, c_void_p, c_void_p]),
    "mpv_kv_suffix_reorder_steps": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "mpv_logits_guide": (c_int, [C.POINTER(LogitsGuideDesc), c_void_p]),
    "mpv_logits_trie_mask": (c_int, [C.POINTER(LogitsTrieDesc), c_void_p]),
    "mpv_logits_trie_mask_ragged": (c_int, [C.POINTER(LogitsTrieDesc), c_void_p]),
    "mpv_logits_trie_mask_steps": (c_int, [C.POINTER(LogitsTrieDesc), c_void_p, c_void_p]),
    "mpv_caption_overlap": (c_int, [C.POINTER(CaptionOverlapDesc), c_void_p]),
    "mpv_caption_cider_workspace_size": (c_size_t, [C.POINTER(CaptionCiderDesc)]),
    "mpv_caption_cider": (c_int, [C.POINTER(CaptionCiderDesc), c_void_p, c_size_t, c_void_p]),
    "mpv_cider_table_fill": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64]),
    "mpv_cider_table_lookup": (c_int64, [c_void_p, c_int64, c_uint64]),
    # LoRA products (csrc/lora.hip)
    "mpv_lora_down": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_int64, c_int, c_float, c_void_p]),
    "mpv_lora_up_add": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_int64, c_int, c_float, c_void_p]),
    "mpv_lora_wgrad_workspace_size": (c_size_t, [c_int64, c_int64, c_int]),
    "mpv_lora_wgrad": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int64, c_int64, c_int, c_float,
                               c_void_p, c_size_t, c_void_p]),
})

EXPORTS = tuple(_SIGS)

_lib = None


class MpvError(RuntimeError):
    pass


def lib():
    """The loaded library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise MpvError(f"{LIB_PATH} not found: the HIP kernels are not built. "
                           "Run `python __graft_entry__.py` (build()) first; there is no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)      # AttributeError if a declared symbol is missing
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


n_calls = 0      # C-ABI calls checked so far (engine.graph_step: "has this graph segment captured anything yet?")


def check(rc: int, what: str = ""):
    global n_calls
    n_calls += 1
    if rc != 0:
        raise MpvError(f"{what} failed ({rc}): {lib().mpv_last_error().decode()}")
