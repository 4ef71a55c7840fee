"""Frozen GPT-3 causal LM (Megatron-style decoder) on the gfx950 kernels.

Mirrors models/modeling_distributed_gpt3.py: GPT3Config :459-547, GPT3Embedding :598-666,
GPT3ParallelAttention :820-938 (+ GPT3CoreAttention :689-817), GPT3ParallelMLP :550-595,
GPT3ParallelTransformerLayer :982-1089, GPT3ParallelTransformer :1092-1186, GPT3Model
:1272-1366, DistributedGPT3 :1522-1618 -- same attribute paths and state-dict keys
(text_decoder.dist_model.language_model.{embedding,encoder}...), TP=1/PP=1.

Rows are kept batch-major [B*S, H] (the reference's [s,b,h] transpose :653 is a pure
permutation of rows; every op here is row-wise or addressed by strides).  The decoder is
frozen in the pre-train recipe (models/distributed_gpt3.py:91-93), so backward computes
dgrad only -- no weight gradients through 24 layers (the reference computes and discards
them).  Dropout (hidden 0.1, attention-prob 0.1) is live in train() mode even though the
weights are frozen and is regenerated from (seed, offset) in backward.
"""
from __future__ import annotations

import json
import math
import os
from typing import Optional

import torch
from torch import nn

from . import ops
from .vision import grad_of
from .ops import ACT_GELU_TANH
from .vision import Linear, _param


SEED_PASS_STRIDE = 0x51ED2705      # seed of decoder pass k of a step = step_seed + k * SEED_PASS_STRIDE

class GPT3Config:
    """Field names of configs/models/config_gpt3_*.json; every GPT3Config default (:463-496) overridable."""

    def __init__(self, vocab_size=25600, hidden_size=768, ffn_hidden_size=None, num_hidden_layers=12, num_attention_heads=12,
                 max_position_embeddings=2048, layernorm_epsilon=1e-12, hidden_dropout=0.1, attention_dropout=0.1,
                 init_method_std=0.02, bias_gelu_fusion=True, apply_query_key_layer_scaling=True, **kw):
        self.vocab_size, self.hidden_size = vocab_size, hidden_size
        self.ffn_hidden_size = ffn_hidden_size or 4 * hidden_size
        self.num_hidden_layers, self.num_attention_heads = num_hidden_layers, num_attention_heads
        self.max_position_embeddings = max_position_embeddings
        self.layernorm_epsilon = layernorm_epsilon
        self.hidden_dropout, self.attention_dropout = hidden_dropout, attention_dropout
        self.init_method_std = init_method_std
        self.bias_gelu_fusion = bias_gelu_fusion
        self.apply_query_key_layer_scaling = apply_query_key_layer_scaling
        self.kv_channels = hidden_size // num_attention_heads
        self.extra = kw

    @classmethod
    def from_json_file(cls, path):
        with open(path) as f:
            return cls(**json.load(f))

    @classmethod
    def from_pretrained(cls, model_dir):
        import os
        return cls.from_json_file(os.path.join(model_dir, "config.json"))


class _LN(nn.Module):
    def __init__(self, dim, eps, device=None):
        super().__init__()
        self.eps = eps
        self.weight = _param(dim, const=1.0, device=device)
        self.bias = _param(dim, const=0.0, device=device)


class _WordEmbeddings(nn.Module):
    """mpu.VocabParallelEmbedding at TP=1 (:619).  Callable like the reference's
    (models/distributed_gpt3.py:155) -- the gather runs on the HIP embedding kernel."""

    def __init__(self, vocab, hidden, std, device=None):
        super().__init__()
        self.weight = _param(vocab, hidden, std=std, device=device)
        self._zero_pos = None

    def forward(self, ids: torch.Tensor):
        B, L = ids.shape
        H = self.weight.shape[1]
        if self._zero_pos is None or self._zero_pos.shape[0] < L:
            self._zero_pos = torch.zeros((L, H), dtype=torch.bfloat16, device=self.weight.device)
        return ops.gpt_embed_fwd(None, ids.contiguous(), self.weight, self._zero_pos, B, 0, L, H).view(B, L, H)


class GPT3Embedding(nn.Module):
    def __init__(self, cfg: GPT3Config, device=None):
        super().__init__()
        self.word_embeddings = _WordEmbeddings(cfg.vocab_size, cfg.hidden_size, cfg.init_method_std, device)
        self.position_embeddings = nn.Module()
        self.position_embeddings.weight = _param(cfg.max_position_embeddings, cfg.hidden_size, std=cfg.init_method_std, device=device)


class GPT3ParallelAttention(nn.Module):
    def __init__(self, cfg, layer_number, std, out_std, device=None):
        super().__init__()
        self.layer_number = max(1, layer_number)
        H = cfg.hidden_size
        self.query_key_value = Linear(H, 3 * H, std=std, device=device)     # rows head-major [h0:q,k,v | h1:q,k,v ...] (:895-902)
        self.dense = Linear(H, H, std=out_std, device=device)


class GPT3ParallelMLP(nn.Module):
    def __init__(self, cfg, std, out_std, device=None):
        super().__init__()
        self.dense_h_to_4h = Linear(cfg.hidden_size, cfg.ffn_hidden_size, std=std, device=device)
        self.dense_4h_to_h = Linear(cfg.ffn_hidden_size, cfg.hidden_size, std=out_std, device=device)


class GPT3ParallelTransformerLayer(nn.Module):
    def __init__(self, cfg, layer_number, std, out_std, device=None):
        super().__init__()
        self.layer_number = layer_number
        self.input_layernorm = _LN(cfg.hidden_size, cfg.layernorm_epsilon, device)
        self.self_attention = GPT3ParallelAttention(cfg, layer_number, std, out_std, device)
        self.post_attention_layernorm = _LN(cfg.hidden_size, cfg.layernorm_epsilon, device)
        self.mlp = GPT3ParallelMLP(cfg, std, out_std, device)


class GPT3ParallelTransformer(nn.Module):
    def __init__(self, cfg, device=None):
        super().__init__()
        std = cfg.init_method_std
        out_std = std / math.sqrt(2.0 * cfg.num_hidden_layers)
        self.layers = nn.ModuleList([GPT3ParallelTransformerLayer(cfg, i + 1, std, out_std, device)
                                     for i in range(cfg.num_hidden_layers)])
        self.final_layernorm = _LN(cfg.hidden_size, cfg.layernorm_epsilon, device)


class GPT3TransformerLanguageModel(nn.Module):
    def __init__(self, cfg, device=None):
        super().__init__()
        self.embedding = GPT3Embedding(cfg, device)
        self.encoder = GPT3ParallelTransformer(cfg, device)


class GPT3Model(nn.Module):
    def __init__(self, cfg: GPT3Config, device=None):
        super().__init__()
        self.config = cfg
        self.language_model = GPT3TransformerLanguageModel(cfg, device)

    def word_embeddings_weight(self):
        return self.language_model.embedding.word_embeddings.weight


_SITE_EMBED, _SITE_ATTN, _SITE_DROP1, _SITE_DROP2 = 0, 1, 2, 3

# The residual stream of the decoder is kept in fp32 (ops.ln_stream_fwd: the add of a sublayer's output happens inside the
# LayerNorm that follows it, in fp32, instead of in the GEMM's bf16 residual epilogue).  The reference adds in bf16
# (models/modeling_distributed_gpt3.py:1059-1078); 48 such roundings are what put a 24-layer bf16 run 1.2e-2 from the fp32
# function in the logits (tools/parity_bisect.py: 0.87e-2 with the fp32 stream).  MPV_DECODER_STREAM=bf16 (measurement knob)
# restores the bf16 stream with the residual adds in the GEMM epilogues.
FP32_STREAM = os.environ.get("MPV_DECODER_STREAM", "fp32") != "bf16"
# Round 4: in the fp32-stream form the dropout of a sublayer's output (bias_dropout_add, models/modeling_distributed_gpt3.py:953-979) is
# applied by the LayerNorm that adds it into the stream (mpv_ln_stream_fwd_drop: same element index, threshold and bf16 rounding, so the
# step is bit-identical) instead of by the sublayer GEMM's epilogue.  MPV_DROPOUT_IN_LN=0 (measurement knob) keeps it in the GEMM.
DROPOUT_IN_LN = os.environ.get("MPV_DROPOUT_IN_LN", "1") != "0"


def _offset(layer: int, site: int) -> int:
    return (layer * 4 + site) << 36


_LORA_SUFFIXES = ("query_key_value.lora_A", "query_key_value.lora_B")


def _lora_keys_may_be_missing(module, incompatible_keys):
    """load_state_dict post-hook of an adapted decoder: a base checkpoint has no adapter keys, and that is not an error"""
    incompatible_keys.missing_keys[:] = [k for k in incompatible_keys.missing_keys if not k.endswith(_LORA_SUFFIXES)]


class DistributedGPT3(nn.Module):
    """Drop-in for models/modeling_distributed_gpt3.py:1522 at TP=1 (checkpoint loading of
    `<model_dir>/model/mp_rank_00_model_states.pt['module']` :431-441 is kept)."""

    def __init__(self, model_dir=None, rank=0, path_load_tag="model", config: Optional[GPT3Config] = None, device=None,
                 load_state_dict=True, **kwargs):
        super().__init__()
        import os
        self.config = config if config is not None else GPT3Config.from_pretrained(model_dir)
        assert self.config.kv_channels in (64, 80, 96), "fused attention kernels are built for head_dim 64/80/96"
        self.dist_model = GPT3Model(self.config, device=device)
        if config is None and load_state_dict and model_dir is not None:
            path = os.path.join(model_dir, str(path_load_tag), "mp_rank_00_model_states.pt")
            if os.path.isfile(path):
                sd = torch.load(path, map_location="cpu")["module"]
                self.dist_model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()})
        self.inference_params = None
        self.step_seed = 0        # bumped by the engine every step -> fresh dropout masks
        self.seed_dev = None      # engine.enable_device_step_state(): int64[4] device tensor, seed of decoder pass k of this step

    # -------------------------------------------------------------- FP8 weights of the decode steps (generation.DecodeWeightsQ8)
    def quantize_decode_weights(self):
        """Quantises the layer products' weights and the tied embedding to e4m3 codes with per-row power-of-two scales, on the
        device, once, and keeps the result on the decoder (decode_weights="fp8" does this on first use, and again when a source
        parameter has been written to since).  -> the generation.DecodeWeightsQ8."""
        self._refuse_live_lora("quantize_decode_weights")
        self._decode_weights_q8 = _generation.DecodeWeightsQ8(self)
        return self._decode_weights_q8

    def clear_decode_weights(self):
        """Drops the FP8 copy (the attribute too)."""
        if "_decode_weights_q8" in self.__dict__:
            del self._decode_weights_q8

    def decode_weights_q8(self):
        """The current FP8 copy: quantised now if there is none or a source parameter's _version has moved."""
        q8 = self.__dict__.get("_decode_weights_q8")
        return self.quantize_decode_weights() if q8 is None or q8.stale() else q8

    def dequantized_state_dict(self) -> dict:
        """The bf16 tensors deq(code) * scale of the FP8 copy under the parameters' own state-dict keys (the quantised tensors only:
        load with strict=False).  The unchanged bf16 stack with these loaded computes what decode_weights="fp8" computes -- for
        tests, and for measuring the quality cost of the quantisation through any existing path."""
        q8 = self.decode_weights_q8()
        names = {id(p): n for n, p in self.named_parameters()}
        return {names[id(p)]: t for p, t in zip(q8.sources, q8.dequantized())}

    @property
    def trainable(self) -> bool:
        """freeze_text_decoder: false (models/distributed_gpt3.py:91-93): the decoder's own (BASE) parameters receive gradients.
        LoRA adapters do not count: an adapted frozen decoder stays on the frozen (dgrad-only, fp32-stream) path."""
        return any(p.requires_grad for n, p in self.named_parameters() if not n.endswith(_LORA_SUFFIXES))

    # -------------------------------------------------------------- LoRA adapters on the fused q/k/v projection
    def _qkv_linears(self):
        return [layer.self_attention.query_key_value for layer in self.dist_model.language_model.encoder.layers]

    def add_lora(self, rank: int, alpha: Optional[float] = None):
        """Gives every layer's self_attention.query_key_value two trainable bf16 parameters, lora_A [rank, H] (std 0.02) and lora_B
        [3H, rank] (zeros): qkv = x W^T + b + s (x A^T) B^T with s = alpha / rank (alpha defaults to rank).  The base stays frozen."""
        if rank not in ops.LORA_RANKS:
            raise ValueError(f"add_lora: rank {rank} is not one of {ops.LORA_RANKS}")
        if self.__dict__.get("_lora") is not None:
            raise RuntimeError("add_lora: this decoder already has adapters")
        if self.trainable:
            raise RuntimeError("add_lora: adapters go on a FROZEN decoder (freeze_text_decoder: true); this one's base parameters are trainable")
        alpha = float(rank if alpha is None else alpha)
        H = self.config.hidden_size
        for lin in self._qkv_linears():
            dev = lin.weight.device
            lin.lora_A = _param(rank, H, std=0.02, device=dev)
            lin.lora_B = _param(3 * H, rank, const=0.0, device=dev)
        self._lora = dict(rank=int(rank), alpha=alpha, scale=alpha / rank, merged=False, saved=None)
        # a BASE checkpoint loads with strict=True: only the adapter keys may be missing, and they stay as they are
        self.register_load_state_dict_post_hook(_lora_keys_may_be_missing)
        return self

    def has_lora(self) -> bool:
        return self.__dict__.get("_lora") is not None

    def lora_live(self) -> bool:
        """adapters present and not merged: forward_lm / backward_lm apply them; every other entry refuses"""
        lo = self.__dict__.get("_lora")
        return lo is not None and not lo["merged"]

    def _refuse_live_lora(self, what: str):
        if self.lora_live():
            raise RuntimeError(f"{what} runs its own layer loop, which does not know the LoRA adapters: call merge_lora() first "
                               "(or run it inside `with decoder.lora_merged():`)")

    def _drop_weight_copies(self):
        """the in-place merge writes the qkv weights through the kernels, which moves no tensor version: drop what is derived from them"""
        cache = self.__dict__.get("_wt_cache")
        if cache is not None:
            for lin in self._qkv_linears():
                cache.pop(id(lin.weight), None)
        self.clear_decode_weights()

    @torch.no_grad()
    def merge_lora(self):
        """W <- bf16(W + s B A) in place on every layer (ops.lora_up_add with t = B, w = A, y = W); keeps a bf16 copy of the original
        weights and switches the adapters off.  Documented limit: the merge rounds W + dW to bf16, so what the delta contributes below
        half a bf16 step of W is lost in the merged model (and only there)."""
        lo = self.__dict__.get("_lora")
        if lo is None:
            raise RuntimeError("merge_lora: this decoder has no adapters")
        if lo["merged"]:
            raise RuntimeError("merge_lora: the adapters are already merged")
        H, r = self.config.hidden_size, lo["rank"]
        saved = []
        for lin in self._qkv_linears():
            saved.append(lin.weight.detach().clone())
            ops.lora_up_add(lin.lora_B.detach(), lin.lora_A.detach(), lin.weight.detach(), 3 * H, H, r, w_rank_major=True, scale=lo["scale"])
        lo.update(merged=True, saved=saved)
        self._drop_weight_copies()

    @torch.no_grad()
    def unmerge_lora(self):
        """restores the copy merge_lora kept, bit for bit, and switches the adapters back on"""
        lo = self.__dict__.get("_lora")
        if lo is None or not lo["merged"]:
            raise RuntimeError("unmerge_lora: the adapters are not merged")
        for lin, w in zip(self._qkv_linears(), lo["saved"]):
            lin.weight.detach().copy_(w)
        lo.update(merged=False, saved=None)
        self._drop_weight_copies()

    def lora_merged(self):
        """context manager: merge_lora() on entry (unless already merged, which it then leaves alone), unmerge_lora() on exit.
        Without adapters it does nothing."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            mine = self.lora_live()
            if mine:
                self.merge_lora()
            try:
                yield self
            finally:
                if mine:
                    self.unmerge_lora()
        return cm()

    def merged_state_dict(self) -> dict:
        """The state dict of the MERGED model under base names only (no adapter keys): loaded into an un-adapted stack it is the
        merged model."""
        with self.lora_merged():
            return {k: v.detach().clone() for k, v in self.state_dict().items() if not k.endswith(_LORA_SUFFIXES)}

    def lora_state_dict(self) -> dict:
        """the adapters alone (state-dict keys of this module) plus their rank and alpha"""
        lo = self.__dict__.get("_lora")
        if lo is None:
            raise RuntimeError("lora_state_dict: this decoder has no adapters")
        sd = {k: v.detach().clone() for k, v in self.state_dict().items() if k.endswith(_LORA_SUFFIXES)}
        sd["lora_rank"], sd["lora_alpha"] = lo["rank"], lo["alpha"]
        return sd

    @torch.no_grad()
    def load_lora_state_dict(self, sd: dict):
        lo = self.__dict__.get("_lora")
        if lo is None:
            raise RuntimeError("load_lora_state_dict: this decoder has no adapters (add_lora first)")
        if lo["merged"]:
            raise RuntimeError("load_lora_state_dict: the adapters are merged: unmerge_lora() first")
        if int(sd["lora_rank"]) != lo["rank"] or float(sd["lora_alpha"]) != lo["alpha"]:
            raise ValueError(f"load_lora_state_dict: file has rank {sd['lora_rank']} / alpha {sd['lora_alpha']}, the model "
                             f"rank {lo['rank']} / alpha {lo['alpha']}")
        own = {k: v for k, v in self.state_dict().items() if k.endswith(_LORA_SUFFIXES)}
        given = {k: v for k, v in sd.items() if k not in ("lora_rank", "lora_alpha")}
        if set(own) != set(given):
            raise ValueError(f"load_lora_state_dict: keys differ: missing {sorted(set(own) - set(given))[:3]}, "
                             f"unexpected {sorted(set(given) - set(own))[:3]}")
        for k, v in given.items():
            if tuple(v.shape) != tuple(own[k].shape):
                raise ValueError(f"load_lora_state_dict: {k} has shape {tuple(v.shape)}, the model {tuple(own[k].shape)}")
        for k, v in given.items():
            own[k].copy_(v.to(own[k].dtype))

    def _lora_forward(self, lin, x1, qkv, R):
        """qkv += s (x1 A^T) B^T behind the frozen product; -> t = bf16(x1 A^T) [R, r] for the tape"""
        lo = self._lora
        H, r = self.config.hidden_size, lo["rank"]
        t = ops.lora_down(x1, lin.lora_A, R, H, r, w_rank_major=True)
        ops.lora_up_add(t, lin.lora_B, qkv, R, 3 * H, r, w_rank_major=False, scale=lo["scale"])
        return t

    def _lora_backward(self, lin, s, dqkv, R, accumulate):
        """dB = s t^T dqkv -> grad_of(lora_B); dt = s dqkv B; dA = dt^T x1 -> grad_of(lora_A).  -> dt (the caller adds dt A to dx1).
        accumulate: a later decoder pass of the same step adds to what the first one wrote."""
        lo = self._lora
        H, r = self.config.hidden_size, lo["rank"]
        gB, gA = grad_of(lin.lora_B), grad_of(lin.lora_A)
        dB = ops.lora_wgrad(s["t"], dqkv, R, 3 * H, r, g_rank_major=False, scale=lo["scale"], out=None if accumulate else gB)
        dt = ops.lora_down(dqkv, lin.lora_B, R, 3 * H, r, w_rank_major=False, scale=lo["scale"])
        dA = ops.lora_wgrad(dt, s["x1"], R, H, r, g_rank_major=True, out=None if accumulate else gA)
        if accumulate:
            ops.add(gB, dB, out=gB)
            ops.add(gA, dA, out=gA)
        return dt

    # -------------------------------------------------------------- explicit forward / backward
    def forward_lm(self, query_features: Optional[torch.Tensor], ids: torch.Tensor, labels: Optional[torch.Tensor],
                   loss_mask: Optional[torch.Tensor], tape: dict, want_logits: bool = False, hidden_only: bool = False,
                   pass_index: int = 0, loss_window: Optional[tuple] = None, window_targets: Optional[tuple] = None):
        """query_features [B*Q, H] (or None), ids [B,L] int64, labels [B,S] int64, loss_mask [B,S-1].
        Returns dict(loss fp32 scalar, losses [B,S-1] fp32, logits?, last_hidden_state [B,S,H]).
        loss_window = (start, length): the caller's promise that loss_mask is zero outside positions
        [start, start + length) of every sequence (pre-training: the Q query slots in front are always masked,
        models/distributed_gpt3.py:142-159).  The tied LM head, the CE and the LM head's dgrad then run on those
        B * length rows only -- the reference evaluates all B * S rows of [S, V] logits and multiplies 80 % of the
        per-token losses by zero; the loss and every gradient are unchanged (those rows' dlogits are exactly 0).
        window_targets = (labels int64 [B * length], weights fp32 [B * length]) of the window rows, already on the device
        (ops.caption_targets): labels / loss_mask are then not consulted and no per-token `losses` tensor is assembled (the
        training step only needs the scalar) -- it takes a dozen small framework launches off every step."""
        cfg = self.config
        lm = self.dist_model.language_model
        B, L = ids.shape
        H, np_, hn, V = cfg.hidden_size, cfg.num_attention_heads, cfg.kv_channels, cfg.vocab_size
        Q = 0 if query_features is None else query_features.shape[0] // B
        S, R = Q + L, B * (Q + L)
        train = self.training
        p_h = cfg.hidden_dropout if train else 0.0
        p_a = cfg.attention_dropout if train else 0.0
        seed = self.step_seed + SEED_PASS_STRIDE * pass_index     # a second decoder pass of one step draws its own dropout masks
        if self.seed_dev is not None:       # the same value, read by the kernels from device memory (include/mpv.h: MPV_SEED_FROM_DEVICE)
            assert pass_index < self.seed_dev.numel()
            seed = (self.seed_dev.data_ptr() + 8 * pass_index) | (1 << 63)
        ids_dev = ids.contiguous() if L > 0 else torch.zeros(1, dtype=torch.long, device=ids.device)   # never dereferenced when L == 0
        h = ops.gpt_embed_fwd(query_features, ids_dev, lm.embedding.word_embeddings.weight,
                              lm.embedding.position_embeddings.weight, B, Q, L, H, dropout_p=p_h, seed=seed,
                              offset=_offset(0, _SITE_EMBED))
        st3 = (S * 3 * H, 3 * hn, 3 * H)
        lay = ops.AttnLayout(st3, st3, st3, (S * H, hn, H))
        scale = 1.0 / math.sqrt(hn)       # alpha=1/(sqrt(hn)*l) then *l inside the softmax (:718-727,757-762): net 1/sqrt(hn)
        window = None
        if loss_window is not None and not want_logits and not hidden_only:
            w0, wl = int(loss_window[0]), int(loss_window[1])
            if 0 <= w0 and w0 + wl <= S and 0 < wl < S:
                window = (w0, wl)
        nl = len(lm.encoder.layers)
        layers = []
        train_dec = self.trainable and not want_logits      # (autograd.Function.forward runs with grad mode off: not a usable signal)
        lora = self.lora_live()
        if train_dec:
            # a trainable decoder runs the reference's own bf16 residual stream (the LayerNorm backward with parameter gradients reads
            # bf16 rows) on all rows of every layer, and keeps what the weight gradients need: the inputs of the four products
            h, xf, mf, rf = self._layers_bf16_stream(h, lay, scale, window, layers, seed, p_h, p_a, B, S, R, H, np_, hn, keep_inputs=True)
        elif FP32_STREAM:
            # stream = the residual stream (bf16 straight out of the embedding, fp32 from the first add on); `pending` = the last
            # sublayer output (bias + dropout applied by its GEMM) that the next LayerNorm adds into the stream in fp32
            stream, pending, pmap = h, None, ops.IDENT
            pend_off = 0                   # dropout site of `pending` (applied by the LayerNorm that adds it: DROPOUT_IN_LN)
            p_g = 0.0 if DROPOUT_IN_LN else p_h      # dropout probability the sublayer GEMMs apply themselves
            p_l = p_h if DROPOUT_IN_LN else 0.0      # ... and the one the adding LayerNorm applies
            smap = ops.IDENT               # rows of `stream` the current layer works on (the loss window in the top layer)
            for li, layer in enumerate(lm.encoder.layers):
                ln = li + 1
                att, mlp = layer.self_attention, layer.mlp
                l1 = layer.input_layernorm
                x1, nxt, m1, r1 = ops.ln_stream_fwd(stream, pending, l1.weight, l1.bias, l1.eps, R, H, amap=pmap,
                                                    add_dropout_p=p_l, seed=seed, offset=pend_off)
                stream = nxt if nxt is not None else stream
                h_in = stream                                                   # x of LayerNorm 1 (for its backward)
                qkv = ops.gemm(x1, att.query_key_value.weight, R, 3 * H, H, bias=att.query_key_value.bias, keep_output=True)
                t_lora = self._lora_forward(att.query_key_value, x1, qkv, R) if lora else None
                ctx = torch.empty((R, H), dtype=torch.bfloat16, device=h.device)
                lse = ops.attn_fwd(qkv, qkv[:, hn:], qkv[:, 2 * hn:], ctx, lay, B, np_, S, S, hn, causal=True, scale=scale,
                                   dropout_p=p_a, seed=seed, offset=_offset(ln, _SITE_ATTN))
                top = window is not None and li == nl - 1
                # Top layer under a loss window: nothing downstream reads its hidden states outside the window (they feed only the
                # LM head, which runs on the window), and everything after the attention is row-wise -- the projection, LN2, the MLP
                # and their residual adds run on the B * wl window rows (a row map on the [B*S, H] stream; the sublayer outputs are
                # compact).  K/V of all rows are still needed by the window's queries, so LN1, qkv and the attention stay whole.
                tm = (window[1], S, window[0]) if top else ops.IDENT
                Rl = B * window[1] if top else R
                a1 = ops.gemm(ctx, att.dense.weight, Rl, H, H, bias=att.dense.bias, dropout_p=p_g, seed=seed,
                              offset=_offset(ln, _SITE_DROP1), amap=tm)                            # compact [Rl, H]
                l2 = layer.post_attention_layernorm
                x2, h1, m2, r2 = ops.ln_stream_fwd(stream, a1, l2.weight, l2.bias, l2.eps, Rl, H, hmap=tm, h_rows=R,
                                                   add_dropout_p=p_l, seed=seed, offset=_offset(ln, _SITE_DROP1))
                F4 = mlp.dense_h_to_4h.out_features
                z = torch.empty((Rl, F4), dtype=torch.bfloat16, device=h.device)
                g = ops.gemm(x2, mlp.dense_h_to_4h.weight, Rl, F4, H, bias=mlp.dense_h_to_4h.bias, act=ACT_GELU_TANH, preact_out=z, preact_deriv=True)
                pending = ops.gemm(g, mlp.dense_4h_to_h.weight, Rl, H, F4, bias=mlp.dense_4h_to_h.bias, dropout_p=p_g, seed=seed,
                                   offset=_offset(ln, _SITE_DROP2))
                pend_off = _offset(ln, _SITE_DROP2)                                # compact [Rl, H]
                ent = dict(h=h_in, s1=(m1, r1), qkv=qkv, ctx=ctx, lse=lse, h1=h1, s2=(m2, r2), z=z)
                if top:
                    ent["rows"] = tm
                if lora:
                    ent.update(x1=x1, t=t_lora)
                layers.append(ent)
                stream, smap = h1, tm
            fl = lm.encoder.final_layernorm
            Rf = B * window[1] if window is not None else R
            xf, h, mf, rf = ops.ln_stream_fwd(stream, pending, fl.weight, fl.bias, fl.eps, Rf, H, hmap=smap, h_rows=R,
                                              add_dropout_p=p_l, seed=seed, offset=pend_off)
        else:
            h, xf, mf, rf = self._layers_bf16_stream(h, lay, scale, window, layers, seed, p_h, p_a, B, S, R, H, np_, hn)
        if hidden_only:     # only last_hidden_state is consumed (models/distributed_gpt3.py:958, 583-584, 1149-1150)
            tape.update(B=B, Q=Q, L=L, S=S, layers=layers, h_last=h, sf=(mf, rf), dlogits=None, lm_window=None, lay=lay, scale=scale,
                        seed=seed, p_h=p_h, p_a=p_a)
            return dict(last_hidden_state=xf.view(B, S, H))
        # masked mean of per-token CE over positions 0..S-2 (:1615-1617)
        if window is not None and window_targets is not None:
            Rw = B * window[1]
            logits = ops.gemm(xf, lm.embedding.word_embeddings.weight, Rw, V, H)       # xf is already the window's rows
            _, loss = ops.cross_entropy(logits, window_targets[0], window_targets[1], Rw, V, dlogits=logits)
            tape.update(B=B, Q=Q, L=L, S=S, layers=layers, h_last=h, sf=(mf, rf), dlogits=logits, lm_window=window, lay=lay, scale=scale,
                        seed=seed, p_h=p_h, p_a=p_a, xf=xf if train_dec else None, ids=ids_dev if train_dec else None)
            return dict(loss=loss, losses=None, last_hidden_state=None)
        lmf = loss_mask.to(torch.float32)
        denom = lmf.sum()
        w = torch.zeros((B, S), dtype=torch.float32, device=h.device)
        w[:, :S - 1] = lmf / denom
        if window is not None:
            w0, wl = window
            Rw = B * wl
            logits = ops.gemm(xf, lm.embedding.word_embeddings.weight, Rw, V, H)       # xf is already the window's rows
            losses_w, loss = ops.cross_entropy(logits, labels[:, w0:w0 + wl].contiguous().view(-1),
                                               w[:, w0:w0 + wl].contiguous().view(-1), Rw, V, dlogits=logits)
            losses = torch.zeros((B, S), dtype=torch.float32, device=h.device)
            losses[:, w0:w0 + wl] = losses_w.view(B, wl)
            keep_logits = None
        else:
            logits = ops.gemm(xf, lm.embedding.word_embeddings.weight, R, V, H)          # tied LM head (:1348-1350)
            keep_logits = logits.clone() if want_logits else None
            losses, loss = ops.cross_entropy(logits, labels.contiguous().view(-1), w.view(-1), R, V, dlogits=logits)
        tape.update(B=B, Q=Q, L=L, S=S, layers=layers, h_last=h, sf=(mf, rf), dlogits=logits, lm_window=window, lay=lay, scale=scale,
                    seed=seed, p_h=p_h, p_a=p_a, xf=xf if train_dec else None, ids=ids_dev if train_dec else None)
        # under a loss window the top layer and the final LayerNorm exist on the window rows only: no full last_hidden_state
        out = dict(loss=loss, losses=losses.view(B, S)[:, :S - 1], last_hidden_state=xf.view(B, S, H) if window is None else None)
        if want_logits:
            out["logits"] = keep_logits.view(B, S, V)
        return out

    @torch.no_grad()
    def forward_prefix(self, query_features: Optional[torch.Tensor], ids: torch.Tensor) -> dict:
        """Prefix pass of shared-prefix scoring: forward_lm over the n_groups prefix sequences (query features + the shared
        tokens, ids [n_groups, t]).  -> the tape forward_continuation reads: every layer's packed qkv rows [n_groups * P, 3H]
        (both residual-stream modes keep them)."""
        assert not self.training, "shared-prefix scoring is an evaluation path (no dropout)"
        tape = {}
        self.forward_lm(query_features, ids, None, None, tape, hidden_only=True)
        return dict(B=tape["B"], P=tape["S"], qkv=[ent["qkv"] for ent in tape["layers"]])

    @torch.no_grad()
    def forward_continuation(self, prefix: dict, ids: torch.Tensor, group_size: int, *, loss_rows: Optional[torch.Tensor] = None,
                             labels: Optional[torch.Tensor] = None, hidden_rows: Optional[torch.Tensor] = None) -> dict:
        """Continuation pass: ids [n_cont, Lc] continue the prefixes of forward_prefix, continuation c that of group
        c // group_size, at absolute positions P .. P + Lc - 1.  Per layer the kernel sequence of forward_lm on the continuation
        rows only (in whichever residual-stream mode forward_lm runs), with the attention against [prefix | own causal] keys
        (ops.attn_prefix_fwd).  Outputs, on the rows asked for (row r = c * Lc + i of the flattened continuations):
        loss_rows + labels -> losses fp32 [len(loss_rows)], the per-token CE of the tied LM head run on those rows only;
        hidden_rows -> hidden bf16 [len(hidden_rows), H], the final LayerNorm's output there."""
        assert not self.training, "shared-prefix scoring is an evaluation path (no dropout)"
        self._refuse_live_lora("forward_continuation")
        cfg = self.config
        lm = self.dist_model.language_model
        n, Lc = ids.shape
        P, ng = prefix["P"], prefix["B"]
        assert Lc > 0 and ng == (n + group_size - 1) // group_size
        H, np_, hn, V = cfg.hidden_size, cfg.num_attention_heads, cfg.kv_channels, cfg.vocab_size
        R = n * Lc
        wpe = lm.embedding.position_embeddings.weight
        if P + Lc > wpe.shape[0]:
            raise ops._lib.MpvError(f"sequence of {P + Lc} positions exceeds max_position_embeddings = {wpe.shape[0]}")
        h = ops.gpt_embed_fwd(None, ids.contiguous(), lm.embedding.word_embeddings.weight, wpe[P:], n, 0, Lc, H)   # positions from P
        st3 = (Lc * 3 * H, 3 * hn, 3 * H)
        lay = ops.AttnLayout(st3, st3, st3, (Lc * H, hn, H))
        pst = (P * 3 * H, 3 * hn, 3 * H)
        scale = 1.0 / math.sqrt(hn)

        def attention(qkv, li):
            ctx = torch.empty((R, H), dtype=torch.bfloat16, device=h.device)
            pq = prefix["qkv"][li]
            ops.attn_prefix_fwd(qkv, qkv[:, hn:], qkv[:, 2 * hn:], pq[:, hn:], pq[:, 2 * hn:], ctx, lay, (pst, pst), n, group_size, np_, Lc,
                                P, hn, scale=scale)
            return ctx

        xf = self._continuation_layers(h, R, attention)
        out = {}
        if loss_rows is not None and loss_rows.numel() > 0:
            nr = loss_rows.numel()
            xs = ops.gather_rows(xf, loss_rows.contiguous(), nr, H)
            logits = ops.gemm(xs, lm.embedding.word_embeddings.weight, nr, V, H)      # tied LM head (:1348-1350), scored rows only
            ones = torch.ones(nr, dtype=torch.float32, device=xf.device)
            out["losses"], _ = ops.cross_entropy(logits, labels.contiguous().view(-1), ones, nr, V)
        elif loss_rows is not None:
            out["losses"] = torch.zeros(0, dtype=torch.float32, device=xf.device)
        if hidden_rows is not None:
            out["hidden"] = ops.gather_rows(xf, hidden_rows.contiguous(), hidden_rows.numel(), H)
        return out

    def _continuation_layers(self, h, R, attention):
        """The layer stack of a continuation pass on the R embedded rows h (forward_continuation: [n_cont * Lc, H]; forward_continuation_
        packed: the packed rows), in whichever residual-stream mode forward_lm runs; attention(qkv, li) -> ctx [R, H] is the pass's
        own attention against [prefix | own causal] keys.  -> the final LayerNorm's output [R, H]."""
        cfg = self.config
        lm = self.dist_model.language_model
        H = cfg.hidden_size
        if FP32_STREAM:
            stream, pending = h, None
            for li, layer in enumerate(lm.encoder.layers):
                att, mlp = layer.self_attention, layer.mlp
                l1, l2 = layer.input_layernorm, layer.post_attention_layernorm
                x1, nxt, _, _ = ops.ln_stream_fwd(stream, pending, l1.weight, l1.bias, l1.eps, R, H)
                stream = nxt if nxt is not None else stream
                qkv = ops.gemm(x1, att.query_key_value.weight, R, 3 * H, H, bias=att.query_key_value.bias, keep_output=True)
                a1 = ops.gemm(attention(qkv, li), att.dense.weight, R, H, H, bias=att.dense.bias)
                x2, stream, _, _ = ops.ln_stream_fwd(stream, a1, l2.weight, l2.bias, l2.eps, R, H)
                F4 = mlp.dense_h_to_4h.out_features
                g = ops.gemm(x2, mlp.dense_h_to_4h.weight, R, F4, H, bias=mlp.dense_h_to_4h.bias, act=ACT_GELU_TANH)
                pending = ops.gemm(g, mlp.dense_4h_to_h.weight, R, H, F4, bias=mlp.dense_4h_to_h.bias)
            fl = lm.encoder.final_layernorm
            xf, _, _, _ = ops.ln_stream_fwd(stream, pending, fl.weight, fl.bias, fl.eps, R, H)
        else:
            for li, layer in enumerate(lm.encoder.layers):
                att, mlp = layer.self_attention, layer.mlp
                l1, l2 = layer.input_layernorm, layer.post_attention_layernorm
                x1, _, _ = ops.layernorm_fwd(h, l1.weight, l1.bias, l1.eps, R, H, want_stats=False)
                qkv = ops.gemm(x1, att.query_key_value.weight, R, 3 * H, H, bias=att.query_key_value.bias, keep_output=True)
                h1 = ops.gemm(attention(qkv, li), att.dense.weight, R, H, H, bias=att.dense.bias, residual=h)
                x2, _, _ = ops.layernorm_fwd(h1, l2.weight, l2.bias, l2.eps, R, H, want_stats=False)
                F4 = mlp.dense_h_to_4h.out_features
                g = ops.gemm(x2, mlp.dense_h_to_4h.weight, R, F4, H, bias=mlp.dense_h_to_4h.bias, act=ACT_GELU_TANH)
                h = ops.gemm(g, mlp.dense_4h_to_h.weight, R, H, F4, bias=mlp.dense_4h_to_h.bias, residual=h1)
            fl = lm.encoder.final_layernorm
            xf, _, _ = ops.layernorm_fwd(h, fl.weight, fl.bias, fl.eps, R, H, want_stats=False)
        return xf

    @torch.no_grad()
    def forward_continuation_packed(self, prefix: dict, ids: torch.Tensor, layout, *, labels: torch.Tensor) -> dict:
        """The packed twin of forward_continuation: ids int64 [rows] are the rows of ragged continuations laid end to end as `layout`
        (an ops.PackedLayout with its device arrays) says -- continuation c has layout.cont_len[c] rows, group g (the prefix sequence g
        of forward_prefix) layout.conts_per_group[g] consecutive continuations -- so no padding row exists anywhere in the pass.
        Packed row r sits at absolute position P + (r - seg_start[r]).  Per layer the kernel sequence of forward_continuation on
        [rows, H], with the attention of ops.attn_prefix_packed_fwd; the tied LM head runs on ALL rows (every packed row is a scored
        row) and labels int64 [rows] are their targets.  -> dict(token_logprob fp32 [rows]): log softmax(logits[r])[labels[r]], the
        negated per-row loss of mpv_cross_entropy."""
        assert not self.training, "shared-prefix scoring is an evaluation path (no dropout)"
        self._refuse_live_lora("forward_continuation_packed")
        cfg = self.config
        lm = self.dist_model.language_model
        P, ng = prefix["P"], prefix["B"]
        R = layout.rows
        assert ids.numel() == R and labels.numel() == R and layout.n_groups == ng, \
            f"{ids.numel()} ids / {labels.numel()} labels for {R} packed rows; {layout.n_groups} groups for {ng} prefixes"
        H, np_, hn, V = cfg.hidden_size, cfg.num_attention_heads, cfg.kv_channels, cfg.vocab_size
        wpe = lm.embedding.position_embeddings.weight
        pos_host = [P + i for i in layout.pos_in_cont]
        pos = (torch.arange(R, dtype=torch.int32, device=ids.device) - layout.seg_start) + P
        h = ops.gpt_embed_rows_fwd(ids.contiguous(), pos, pos_host, lm.embedding.word_embeddings.weight, wpe, R, H)   # checks pos_host
        st = ((3 * H, 3 * hn),) * 3 + ((H, hn),)
        pst = (P * 3 * H, 3 * hn, 3 * H)
        scale = 1.0 / math.sqrt(hn)

        def attention(qkv, li):
            ctx = torch.empty((R, H), dtype=torch.bfloat16, device=h.device)
            pq = prefix["qkv"][li]
            ops.attn_prefix_packed_fwd(qkv, qkv[:, hn:], qkv[:, 2 * hn:], pq[:, hn:], pq[:, 2 * hn:], ctx, st, (pst, pst), layout, np_, P,
                                       hn, scale=scale)
            return ctx

        xf = self._continuation_layers(h, R, attention)
        logits = ops.gemm(xf, lm.embedding.word_embeddings.weight, R, V, H)      # tied LM head (:1348-1350), every packed row
        ones = torch.ones(R, dtype=torch.float32, device=xf.device)
        losses, _ = ops.cross_entropy(logits, labels.contiguous().view(-1), ones, R, V)
        return dict(token_logprob=-losses)

    # -------------------------------------------------------------- training on a shared prefix
    def _shared_prefix_lm_check(self, P: int, longest: int):
        """forward_shared_prefix_lm's refusals, before any launch (forward_scst makes them before its rollout)"""
        cfg = self.config
        self._refuse_live_lora("forward_shared_prefix_lm")
        if self.trainable:
            raise NotImplementedError("the shared-prefix training pass computes no decoder weight gradients: it needs freeze_text_decoder: true")
        if not FP32_STREAM:
            raise NotImplementedError("the shared-prefix training pass runs the fp32 residual stream only (MPV_DECODER_STREAM=bf16 is set)")
        if cfg.kv_channels not in (64, 80):
            raise NotImplementedError(f"the packed shared-prefix attention is built for head_dim 64 / 80 (got {cfg.kv_channels})")
        n_pos = self.dist_model.language_model.embedding.position_embeddings.weight.shape[0]
        if P + longest > n_pos:
            raise ops._lib.MpvError(f"sequence of {P + longest} positions exceeds max_position_embeddings = {n_pos}")

    def forward_shared_prefix_lm(self, query_features: torch.Tensor, prefix_ids: torch.Tensor, cont_ids: torch.Tensor, layout,
                                 window_targets: tuple, tape: dict):
        """The training pass of forward_lm for sequences that share a prefix per group, each prefix computed ONCE: query_features
        [B*Q, H] and prefix_ids int64 [B, pl-1] (pl-1 may be 0) are the B prefixes [Q query slots | prompt[:-1]] of P = Q + pl - 1 rows;
        cont_ids int64 [Rc] are the rows of the ragged continuations laid end to end as `layout` (an ops.PackedLayout with its device
        arrays; group g continues prefix g), packed row r at position P + (r - seg_start[r]).  ONE token stream of Rp + Rc rows, Rp = B P:
        LayerNorms and the four products of a layer run once on all rows, only the attention is two launches -- ops.attn_fwd (causal)
        on the prefix block, ops.attn_prefix_packed_fwd_lse on the continuation rows against that layer's prefix K / V.  The loss
        window is the continuation rows: the top layer's row-wise part, the final LayerNorm, the tied LM head and the CE run on those
        Rc rows (row map (Rc, R, Rp)); window_targets = (labels int64 [Rc], weights fp32 [Rc]) as in forward_lm.
        Frozen decoder, fp32 residual stream, head_dim 64 / 80 (anything else raises before any launch).  The pass applies NO decoder
        dropout, neither hidden nor attention, whatever the module's mode: the packed attention has none, and one prefix cannot carry
        the N independent masks of its N continuations.  -> dict(loss); backward_shared_prefix_lm(tape, grad_loss)."""
        self._refuse_live_lora("forward_shared_prefix_lm")
        cfg = self.config
        lm = self.dist_model.language_model
        H, np_, hn, V = cfg.hidden_size, cfg.num_attention_heads, cfg.kv_channels, cfg.vocab_size
        B, Lp = prefix_ids.shape
        Q = query_features.shape[0] // B
        P, Rc = Q + Lp, layout.rows
        Rp = B * P
        R = Rp + Rc
        assert Q >= 1 and layout.n_groups == B and cont_ids.numel() == Rc and window_targets[0].numel() == Rc, \
            f"{layout.n_groups} groups for {B} prefixes; {cont_ids.numel()} ids / {window_targets[0].numel()} labels for {Rc} packed rows"
        self._shared_prefix_lm_check(P, max(layout.cont_len))
        wte, wpe = lm.embedding.word_embeddings.weight, lm.embedding.position_embeddings.weight
        ids_dev = prefix_ids.contiguous() if Lp > 0 else torch.zeros(1, dtype=torch.long, device=prefix_ids.device)
        pos_host = [P + i for i in layout.pos_in_cont]
        pos = (torch.arange(Rc, dtype=torch.int32, device=cont_ids.device) - layout.seg_start) + P
        h = torch.cat([ops.gpt_embed_fwd(query_features, ids_dev, wte, wpe, B, Q, Lp, H),
                       ops.gpt_embed_rows_fwd(cont_ids.contiguous(), pos, pos_host, wte, wpe, Rc, H)])
        st3 = (P * 3 * H, 3 * hn, 3 * H)
        lay = ops.AttnLayout(st3, st3, st3, (P * H, hn, H))
        st = ((3 * H, 3 * hn),) * 3 + ((H, hn),)
        scale = 1.0 / math.sqrt(hn)
        tm = (Rc, R, Rp)                                      # the continuation rows of the [R, H] stream
        nl = len(lm.encoder.layers)
        layers = []
        stream, pending = h, None
        for li, layer in enumerate(lm.encoder.layers):
            att, mlp = layer.self_attention, layer.mlp
            l1, l2 = layer.input_layernorm, layer.post_attention_layernorm
            x1, nxt, m1, r1 = ops.ln_stream_fwd(stream, pending, l1.weight, l1.bias, l1.eps, R, H)
            stream = nxt if nxt is not None else stream
            h_in = stream
            qkv = ops.gemm(x1, att.query_key_value.weight, R, 3 * H, H, bias=att.query_key_value.bias, keep_output=True)
            ctx = torch.empty((R, H), dtype=torch.bfloat16, device=h.device)
            lse = ops.attn_fwd(qkv, qkv[:, hn:], qkv[:, 2 * hn:], ctx, lay, B, np_, P, P, hn, causal=True, scale=scale)
            qc = qkv[Rp:]
            lse_c = ops.attn_prefix_packed_fwd_lse(qc, qc[:, hn:], qc[:, 2 * hn:], qkv[:, hn:], qkv[:, 2 * hn:], ctx[Rp:], st, (st3, st3),
                                                   layout, np_, P, hn, scale=scale)
            top = li == nl - 1
            rm = tm if top else ops.IDENT
            Rl = Rc if top else R
            a1 = ops.gemm(ctx, att.dense.weight, Rl, H, H, bias=att.dense.bias, amap=rm)
            x2, h1, m2, r2 = ops.ln_stream_fwd(stream, a1, l2.weight, l2.bias, l2.eps, Rl, H, hmap=rm, h_rows=R)
            F4 = mlp.dense_h_to_4h.out_features
            z = torch.empty((Rl, F4), dtype=torch.bfloat16, device=h.device)
            g = ops.gemm(x2, mlp.dense_h_to_4h.weight, Rl, F4, H, bias=mlp.dense_h_to_4h.bias, act=ACT_GELU_TANH, preact_out=z, preact_deriv=True)
            pending = ops.gemm(g, mlp.dense_4h_to_h.weight, Rl, H, F4, bias=mlp.dense_4h_to_h.bias)
            layers.append(dict(h=h_in, s1=(m1, r1), qkv=qkv, ctx=ctx, lse=lse, lse_c=lse_c, h1=h1, s2=(m2, r2), z=z, rows=tm if top else None))
            stream = h1
        fl = lm.encoder.final_layernorm
        xf, h_last, mf, rf = ops.ln_stream_fwd(stream, pending, fl.weight, fl.bias, fl.eps, Rc, H, hmap=tm, h_rows=R)
        logits = ops.gemm(xf, wte, Rc, V, H)                      # tied LM head on the continuation rows
        _, loss = ops.cross_entropy(logits, window_targets[0], window_targets[1], Rc, V, dlogits=logits)
        tape.update(B=B, Q=Q, L=Lp, P=P, Rp=Rp, Rc=Rc, layers=layers, h_last=h_last, sf=(mf, rf), dlogits=logits, lay=lay, st=st, scale=scale,
                    layout=layout)
        return dict(loss=loss)

    def backward_shared_prefix_lm(self, tape: dict, grad_loss: Optional[torch.Tensor] = None):
        """-> d(query_features) [B*Q, H] of forward_shared_prefix_lm (dgrad only: the decoder is frozen).  Per layer from the top: the
        row-wise kernels of backward_lm's frozen branch on all rows (the top layer's on the continuation rows: the prefix rows' incoming
        gradient is exactly zero there, their only gradient arrives through K and V); ops.attn_bwd on the prefix block writes dqkv[:Rp];
        ops.attn_prefix_packed_bwd (accumulate_prefix) writes dqkv[Rp:] and adds the continuations' share into the K / V parts of
        dqkv[:Rp]; then the qkv dgrad and LayerNorm 1 on all rows."""
        cfg = self.config
        lm = self.dist_model.language_model
        H, np_, hn, V = cfg.hidden_size, cfg.num_attention_heads, cfg.kv_channels, cfg.vocab_size
        B, Q, Lp, P, Rp, Rc = tape["B"], tape["Q"], tape["L"], tape["P"], tape["Rp"], tape["Rc"]
        R = Rp + Rc
        lay, st, scale, layout = tape["lay"], tape["st"], tape["scale"], tape["layout"]
        st3 = lay.k
        tm = (Rc, R, Rp)
        fl = lm.encoder.final_layernorm
        dxf = self._dgrad(tape["dlogits"], lm.embedding.word_embeddings.weight, Rc, H, V, alpha_dev=grad_loss)
        tape["dlogits"] = None
        dh = torch.empty((R, H), dtype=torch.bfloat16, device=dxf.device)      # only the continuation rows are read (top layer)
        self._ln_bwd(dxf, tape["h_last"], fl.weight, *tape["sf"], Rc, H, dx=dh, xmap=tm)
        for li in range(len(lm.encoder.layers) - 1, -1, -1):
            layer, s = lm.encoder.layers[li], tape["layers"][li]
            att, mlp = layer.self_attention, layer.mlp
            F4 = mlp.dense_h_to_4h.out_features
            if s["rows"] is not None:
                dz = self._dgrad(dh, mlp.dense_4h_to_h.weight, Rc, F4, H, act_bwd_z=s["z"], act_bwd=ACT_GELU_TANH, z_is_deriv=True, amap=tm)
                dx2 = self._dgrad(dz, mlp.dense_h_to_4h.weight, Rc, H, F4)
                dh1, dctx = self._window_zero_pair(R, H, tm, dh.device)       # the prefix rows stay exact zeros
                self._ln_bwd(dx2, s["h1"], layer.post_attention_layernorm.weight, *s["s2"], Rc, H, dres=dh, dx=dh1, xmap=tm)
                self._dgrad(dh1, att.dense.weight, Rc, H, H, amap=tm, cmap=tm, out=dctx)
            else:
                dz = self._dgrad(dh, mlp.dense_4h_to_h.weight, R, F4, H, act_bwd_z=s["z"], act_bwd=ACT_GELU_TANH, z_is_deriv=True)
                dx2 = self._dgrad(dz, mlp.dense_h_to_4h.weight, R, H, F4)
                dh1 = self._ln_bwd(dx2, s["h1"], layer.post_attention_layernorm.weight, *s["s2"], R, H, dres=dh)
                dctx = self._dgrad(dh1, att.dense.weight, R, H, H)
            qkv = s["qkv"]
            dqkv = torch.empty_like(qkv)
            ops.attn_bwd(qkv, qkv[:, hn:], qkv[:, 2 * hn:], s["ctx"], s["lse"], dctx, dqkv, dqkv[:, hn:], dqkv[:, 2 * hn:], lay,
                         B, np_, P, P, hn, causal=True, scale=scale)
            qc, dqc = qkv[Rp:], dqkv[Rp:]
            ops.attn_prefix_packed_bwd(qc, qc[:, hn:], qc[:, 2 * hn:], qkv[:, hn:], qkv[:, 2 * hn:], s["ctx"][Rp:], s["lse_c"], dctx[Rp:],
                                       dqc, dqc[:, hn:], dqc[:, 2 * hn:], dqkv[:, hn:], dqkv[:, 2 * hn:], st, (st3, st3), layout, np_, P, hn,
                                       scale=scale, accumulate_prefix=True)
            dx1 = self._dgrad(dqkv, att.query_key_value.weight, R, H, 3 * H)
            dh = self._ln_bwd(dx1, s["h"], layer.input_layernorm.weight, *s["s1"], R, H, dres=dh1)
            tape["layers"][li] = None
        return ops.gpt_embed_bwd(dh[:Rp], B, Q, Lp, H)           # the prefix block's rows: the front of forward_lm

    def _layers_bf16_stream(self, h, lay, scale, window, layers, seed, p_h, p_a, B, S, R, H, np_, hn, keep_inputs=False):
        """The layer stack with the reference's bf16 residual stream (residual adds in the GEMM epilogues): MPV_DECODER_STREAM=bf16,
        and always for a trainable decoder (keep_inputs: x1 / x2 / gelu(z) stay on the tape for the weight gradients, and the top layer
        is not trimmed to the loss window)."""
        lm = self.dist_model.language_model
        nl = len(lm.encoder.layers)
        trim_top = window is not None and not keep_inputs
        lora = self.lora_live()
        for li, layer in enumerate(lm.encoder.layers):
            ln = li + 1
            att, mlp = layer.self_attention, layer.mlp
            x1, m1, r1 = ops.layernorm_fwd(h, layer.input_layernorm.weight, layer.input_layernorm.bias, layer.input_layernorm.eps, R, H)
            qkv = ops.gemm(x1, att.query_key_value.weight, R, 3 * H, H, bias=att.query_key_value.bias, keep_output=True)
            t_lora = self._lora_forward(att.query_key_value, x1, qkv, R) if lora else None
            ctx = torch.empty((R, H), dtype=torch.bfloat16, device=h.device)
            lse = ops.attn_fwd(qkv, qkv[:, hn:], qkv[:, 2 * hn:], ctx, lay, B, np_, S, S, hn, causal=True, scale=scale,
                               dropout_p=p_a, seed=seed, offset=_offset(ln, _SITE_ATTN))
            if trim_top and li == nl - 1:
                # Top layer under a loss window: nothing downstream reads its hidden states outside the window (they feed only
                # the LM head, which runs on the window), and everything after the attention is row-wise -- the projection,
                # LN2, the MLP and their residual adds run on the B * wl window rows (a row map on the [B*S, H] stream; the
                # MLP's own tensors are compact).  K/V of all rows are still needed by the window's queries, so LN1, qkv and
                # the attention stay whole.  The reference evaluates all S rows and discards them (models/
                # modeling_distributed_gpt3.py:1340-1366 + distributed_gpt3.py:142-159); loss and gradients are unchanged.
                tm = (window[1], S, window[0])
                Rw = B * window[1]
                h1 = torch.empty((R, H), dtype=torch.bfloat16, device=h.device)
                ops.gemm(ctx, att.dense.weight, Rw, H, H, bias=att.dense.bias, residual=h, dropout_p=p_h, seed=seed,
                         offset=_offset(ln, _SITE_DROP1), amap=tm, cmap=tm, out=h1)
                x2, m2, r2 = ops.layernorm_fwd(h1, layer.post_attention_layernorm.weight, layer.post_attention_layernorm.bias,
                                               layer.post_attention_layernorm.eps, Rw, H, xmap=tm)
                F4 = mlp.dense_h_to_4h.out_features
                z = torch.empty((Rw, F4), dtype=torch.bfloat16, device=h.device)
                g = ops.gemm(x2, mlp.dense_h_to_4h.weight, Rw, F4, H, bias=mlp.dense_h_to_4h.bias, act=ACT_GELU_TANH, preact_out=z, preact_deriv=True)
                h2 = torch.empty((R, H), dtype=torch.bfloat16, device=h.device)
                ops.gemm(g, mlp.dense_4h_to_h.weight, Rw, H, F4, bias=mlp.dense_4h_to_h.bias, residual=h1, dropout_p=p_h,
                         seed=seed, offset=_offset(ln, _SITE_DROP2), cmap=tm, out=h2)
                layers.append(dict(h=h, s1=(m1, r1), qkv=qkv, ctx=ctx, lse=lse, h1=h1, s2=(m2, r2), z=z, rows=tm))
                if lora:
                    layers[-1].update(x1=x1, t=t_lora)
                h = h2
                continue
            h1 = ops.gemm(ctx, att.dense.weight, R, H, H, bias=att.dense.bias, residual=h, dropout_p=p_h, seed=seed,
                          offset=_offset(ln, _SITE_DROP1))
            x2, m2, r2 = ops.layernorm_fwd(h1, layer.post_attention_layernorm.weight, layer.post_attention_layernorm.bias,
                                           layer.post_attention_layernorm.eps, R, H)
            F4 = mlp.dense_h_to_4h.out_features
            z = torch.empty((R, F4), dtype=torch.bfloat16, device=h.device)
            g = ops.gemm(x2, mlp.dense_h_to_4h.weight, R, F4, H, bias=mlp.dense_h_to_4h.bias, act=ACT_GELU_TANH, preact_out=z, preact_deriv=True)
            h2 = ops.gemm(g, mlp.dense_4h_to_h.weight, R, H, F4, bias=mlp.dense_4h_to_h.bias, residual=h1, dropout_p=p_h,
                          seed=seed, offset=_offset(ln, _SITE_DROP2))
            ent = dict(h=h, s1=(m1, r1), qkv=qkv, ctx=ctx, lse=lse, h1=h1, s2=(m2, r2), z=z)
            if keep_inputs:
                ent.update(x1=x1, x2=x2, g=g)
            if lora:
                ent.update(x1=x1, t=t_lora)
            layers.append(ent)
            h = h2
        fl = lm.encoder.final_layernorm
        if window is not None:       # final LayerNorm on the window rows of the stream -> compact [B * wl, H]
            xf, mf, rf = ops.layernorm_fwd(h, fl.weight, fl.bias, fl.eps, B * window[1], H, xmap=(window[1], S, window[0]))
        else:
            xf, mf, rf = ops.layernorm_fwd(h, fl.weight, fl.bias, fl.eps, R, H)
        return h, xf, mf, rf

    def _window_zero_pair(self, R, H, rows, device):
        key = (R, H, tuple(rows), str(device), torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0)
        ent = self.__dict__.setdefault("_wz_cache", {}).get(key)
        if ent is None:
            self._wz_cache.clear()
            ent = self._wz_cache[key] = (torch.zeros((R, H), dtype=torch.bfloat16, device=device),
                                         torch.zeros((R, H), dtype=torch.bfloat16, device=device))
        return ent

    def _dgrad(self, dy, weight, R, n_in, n_out, **kw):
        """dX[R, n_in] = dY[R, n_out] W[n_out, n_in].  A frozen weight (the recipes' freeze_text_decoder: true) is
        kept in a second, transposed copy so the pass runs as the k-contiguous (forward-type, LDS-DMA) GEMM, which is
        measurably faster than the reduction-slow operand path; a trainable weight takes the ordinary dgrad kernel."""
        if weight.requires_grad:
            return ops.gemm(dy, weight, R, n_in, n_out, trans_b=True, **kw)
        cache = self.__dict__.setdefault("_wt_cache", {})
        key = id(weight)
        ent = cache.get(key)
        if ent is None or ent[0] != weight._version or ent[1] != weight.data_ptr():
            ent = (weight._version, weight.data_ptr(), weight.detach().t().contiguous())
            cache[key] = ent
        return ops.gemm(dy, ent[2], R, n_in, n_out, **kw)

    @staticmethod
    def _ln_bwd(dy, x, gamma, mean, rstd, rows, cols, **kw):
        """LayerNorm backward of the frozen decoder: x is the fp32 residual stream (ops.ln_stream_bwd), or bf16 -- the embedding
        output in front of layer 0, and everything under MPV_DECODER_STREAM=bf16."""
        if x.dtype == torch.float32:
            return ops.ln_stream_bwd(dy, x, gamma, mean, rstd, rows, cols, **kw)
        return ops.layernorm_bwd(dy, x, gamma, mean, rstd, rows, cols, **kw)

    def backward_lm(self, tape: dict, grad_loss: Optional[torch.Tensor] = None, d_last_hidden: Optional[torch.Tensor] = None,
                    accumulate_lora: bool = False):
        """-> d(query_features) [B*Q, H] (dgrad only: the decoder is frozen).  The seed is the loss (grad_loss scales the
        stored dlogits) and/or d_last_hidden [B*S, H], the gradient of the final-layernorm output.
        A tape recorded with live LoRA adapters also writes their gradients into grad_of(lora_A / lora_B), overwriting them as the
        decoder's other weight gradients do; accumulate_lora: this is a LATER decoder pass of the same step and adds to them."""
        cfg = self.config
        lm = self.dist_model.language_model
        B, Q, L, S = tape["B"], tape["Q"], tape["L"], tape["S"]
        H, np_, hn, V = cfg.hidden_size, cfg.num_attention_heads, cfg.kv_channels, cfg.vocab_size
        R = B * S
        p_h, p_a, seed, lay, scale = tape["p_h"], tape["p_a"], tape["seed"], tape["lay"], tape["scale"]
        nl = len(lm.encoder.layers)
        fl = lm.encoder.final_layernorm
        tm = None
        td = tape.get("xf") is not None       # trainable decoder (forward_lm kept the GEMM inputs): weight gradients below
        wte = lm.embedding.word_embeddings.weight
        if td and tape["dlogits"] is not None:
            # tied LM head (:1348-1350): dWte = grad_loss * dlogits^T xf over the rows the head ran on (the loss window, or all rows);
            # the lookup half of the word-embedding gradient is added at the end (embedding front)
            rows_lm = B * tape["lm_window"][1] if tape.get("lm_window") is not None else R
            ops.gemm(tape["dlogits"], tape["xf"], V, H, rows_lm, trans_a=True, trans_b=True, alpha_dev=grad_loss, out=grad_of(wte))
        if tape["dlogits"] is not None and tape.get("lm_window") is not None:
            # LM head dgrad on the loss window only (few output tiles, K = V: split along K inside mpv_gemm_bf16): dxf is the
            # compact [B * wl, H] gradient of the final LayerNorm's window rows; the final LayerNorm and the top layer's
            # row-wise part run backward on those rows through the row map tm (forward_lm)
            assert d_last_hidden is None, "a loss window leaves no full last_hidden_state to receive a gradient"
            w0, wl = tape["lm_window"]
            tm = (wl, S, w0)
            dxf = self._dgrad(tape["dlogits"], lm.embedding.word_embeddings.weight, B * wl, H, V, alpha_dev=grad_loss)
            tape["dlogits"] = None
        elif tape["dlogits"] is not None:
            dxf = self._dgrad(tape["dlogits"], lm.embedding.word_embeddings.weight, R, H, V, alpha_dev=grad_loss,
                              residual=d_last_hidden)
            tape["dlogits"] = None
        else:
            dxf = d_last_hidden
        drop = p_h > 0.0
        dh_m = torch.empty((R, H), dtype=torch.bfloat16, device=dxf.device) if drop else None
        lnp = lambda ln_mod: dict(dgamma=grad_of(ln_mod.weight), dbeta=grad_of(ln_mod.bias)) if td else {}
        if tm is not None and td:
            # trainable decoder: every layer runs on all rows; the rows outside the window carry an exactly-zero gradient
            dh = torch.zeros((R, H), dtype=torch.bfloat16, device=dxf.device)
            if dh_m is not None:
                dh_m.zero_()
            self._ln_bwd(dxf, tape["h_last"], fl.weight, *tape["sf"], B * tm[0], H, dx=dh, dx_drop=dh_m, dropout_p=p_h, seed=seed,
                              offset=_offset(nl, _SITE_DROP2), xmap=tm, **lnp(fl))
        elif tm is not None:      # window rows of the [B*S, H] stream (the other rows of dh / dh_m are never read)
            dh = torch.empty((R, H), dtype=torch.bfloat16, device=dxf.device)
            self._ln_bwd(dxf, tape["h_last"], fl.weight, *tape["sf"], B * tm[0], H, dx=dh, dx_drop=dh_m, dropout_p=p_h, seed=seed,
                              offset=_offset(nl, _SITE_DROP2), xmap=tm)
        elif td:
            dh = self._ln_bwd(dxf, tape["h_last"], fl.weight, *tape["sf"], R, H, dx_drop=dh_m, dropout_p=p_h, seed=seed,
                                   offset=_offset(nl, _SITE_DROP2), **lnp(fl))
        else:
            dh = self._ln_bwd(dxf, tape["h_last"], fl.weight, *tape["sf"], R, H, dx_drop=dh_m, dropout_p=p_h, seed=seed,
                                   offset=_offset(nl, _SITE_DROP2))
        for li in range(nl - 1, -1, -1):
            layer, s = lm.encoder.layers[li], tape["layers"][li]
            ln = li + 1
            att, mlp = layer.self_attention, layer.mlp
            F4 = mlp.dense_h_to_4h.out_features
            do = dh_m if drop else dh
            if s.get("rows") is not None:
                # top layer under a loss window (forward_lm): MLP, LN2 and the projection backward on the window rows; the
                # gradients of the other rows are exact zeros (dh1 feeds LN1's residual gradient, dctx the attention backward)
                rm = s["rows"]
                Rw = B * rm[0]
                dz = self._dgrad(do, mlp.dense_4h_to_h.weight, Rw, F4, H, act_bwd_z=s["z"], act_bwd=ACT_GELU_TANH, z_is_deriv=True, amap=rm)
                dx2 = self._dgrad(dz, mlp.dense_h_to_4h.weight, Rw, H, F4)
                # the rows outside the window stay exact zeros: two buffers cleared once and kept across steps (only window rows
                # are ever written), instead of two activation-sized clears per step
                dh1, dctx = self._window_zero_pair(R, H, rm, dh.device)
                dh1_m = torch.empty((R, H), dtype=torch.bfloat16, device=dh.device) if drop else None
                self._ln_bwd(dx2, s["h1"], layer.post_attention_layernorm.weight, *s["s2"], Rw, H, dres=dh, dx=dh1, dx_drop=dh1_m,
                                  dropout_p=p_h, seed=seed, offset=_offset(ln, _SITE_DROP1), xmap=rm)
                da = dh1_m if drop else dh1
                self._dgrad(da, att.dense.weight, Rw, H, H, amap=rm, cmap=rm, out=dctx)
            else:
                dz = self._dgrad(do, mlp.dense_4h_to_h.weight, R, F4, H, act_bwd_z=s["z"], act_bwd=ACT_GELU_TANH, z_is_deriv=True)
                if td:      # dense_4h_to_h: dW = do^T gelu(z), db = colsum(do); dense_h_to_4h: dW = dz^T x2, db = colsum(dz)
                    ops.gemm(do, s["g"], H, F4, R, trans_a=True, trans_b=True, out=grad_of(mlp.dense_4h_to_h.weight))
                    ops.colsum(do, R, H, out=grad_of(mlp.dense_4h_to_h.bias))
                    ops.gemm(dz, s["x2"], F4, H, R, trans_a=True, trans_b=True, out=grad_of(mlp.dense_h_to_4h.weight))
                    ops.colsum(dz, R, F4, out=grad_of(mlp.dense_h_to_4h.bias))
                dx2 = self._dgrad(dz, mlp.dense_h_to_4h.weight, R, H, F4)
                dh1_m = torch.empty((R, H), dtype=torch.bfloat16, device=dh.device) if drop else None
                dh1 = self._ln_bwd(dx2, s["h1"], layer.post_attention_layernorm.weight, *s["s2"], R, H, dres=dh, dx_drop=dh1_m,
                                        dropout_p=p_h, seed=seed, offset=_offset(ln, _SITE_DROP1), **lnp(layer.post_attention_layernorm))
                da = dh1_m if drop else dh1
                if td:      # attention output projection: dW = da^T ctx
                    ops.gemm(da, s["ctx"], H, H, R, trans_a=True, trans_b=True, out=grad_of(att.dense.weight))
                    ops.colsum(da, R, H, out=grad_of(att.dense.bias))
                dctx = self._dgrad(da, att.dense.weight, R, H, H)
            qkv = s["qkv"]
            dqkv = torch.empty_like(qkv)
            ops.attn_bwd(qkv, qkv[:, hn:], qkv[:, 2 * hn:], s["ctx"], s["lse"], dctx, dqkv, dqkv[:, hn:], dqkv[:, 2 * hn:], lay,
                         B, np_, S, S, hn, causal=True, scale=scale, dropout_p=p_a, seed=seed, offset=_offset(ln, _SITE_ATTN))
            if td:      # fused q/k/v projection: dW = dqkv^T x1
                ops.gemm(dqkv, s["x1"], 3 * H, H, R, trans_a=True, trans_b=True, out=grad_of(att.query_key_value.weight))
                ops.colsum(dqkv, R, 3 * H, out=grad_of(att.query_key_value.bias))
            dt_lora = self._lora_backward(att.query_key_value, s, dqkv, R, accumulate_lora) if s.get("t") is not None else None
            dx1 = self._dgrad(dqkv, att.query_key_value.weight, R, H, 3 * H)
            if dt_lora is not None:      # the adapter's share of dx1: dx1 += dt A
                ops.lora_up_add(dt_lora, att.query_key_value.lora_A, dx1, R, H, self._lora["rank"], w_rank_major=True)
            prev_off = _offset(li, _SITE_DROP2) if li > 0 else 0
            want_mask = drop and li > 0
            dh_m = torch.empty((R, H), dtype=torch.bfloat16, device=dh.device) if want_mask else None
            dh = self._ln_bwd(dx1, s["h"], layer.input_layernorm.weight, *s["s1"], R, H, dres=dh1, dx_drop=dh_m,
                                   dropout_p=p_h if want_mask else 0.0, seed=seed, offset=prev_off, **lnp(layer.input_layernorm))
            tape["layers"][li] = None
        if td:
            # embedding front (GPT3Embedding, :640-666): h0 = dropout(x + wpe[s]) with x = the query features (s < Q) or wte[ids].
            # de = mask * dh on every row; dWpe[s] = sum over the batch of de[b, s]; the word-embedding rows get de through the
            # lookup -- a one-hot product so that repeated tokens add up: dWte += onehot(ids)^T de[text rows] (on top of the LM head's half)
            de = ops.gpt_embed_bwd_full(dh, R, H, dropout_p=p_h, seed=seed, offset=_offset(0, _SITE_EMBED))
            wpe = lm.embedding.position_embeddings.weight
            gpe = grad_of(wpe)
            gpe.zero_()
            ops.colsum(de, B, S * H, out=gpe.view(-1)[:S * H])
            if L > 0:
                onehot = torch.zeros((B * L, V), dtype=torch.bfloat16, device=dh.device)
                onehot.scatter_(1, tape["ids"].reshape(-1, 1), 1.0)
                de_text = ops.copy_rows(de, torch.empty((B * L, H), dtype=torch.bfloat16, device=dh.device), B * L, H, smap=(L, S, Q))
                ops.gemm(onehot, de_text, V, H, B * L, trans_a=True, trans_b=True, accumulate=True, out=grad_of(wte))
        if Q == 0:
            return None
        return ops.gpt_embed_bwd(dh, B, Q, L, H, dropout_p=p_h, seed=seed, offset=_offset(0, _SITE_EMBED))

    # -------------------------------------------------------------- reference-shaped API
    def forward(self, tokens=None, input_embeds=None, query_embeds=None, attention_mask=None, position_ids=None, labels=None,
                prompt_length=None, loss_mask=None, is_pair=(False,)):
        """models/modeling_distributed_gpt3.py:1578-1618 signature (no-grad / evaluation use).  The
        training path goes through DistributedGPT3_Pretrain, which drives forward_lm/backward_lm."""
        if tokens is None:
            # models/modeling_distributed_gpt3.py:652-657: without ids the word embeddings ARE input_embeds [B, L, H]
            # (query_embeds, if any, in front): the whole sequence enters as embedding rows, no token lookups
            if input_embeds is None:
                raise ValueError("DistributedGPT3.forward needs `tokens` or `input_embeds`")
            emb = input_embeds if query_embeds is None else torch.cat([query_embeds, input_embeds], dim=1)
            B = emb.shape[0]
            qf = emb.to(torch.bfloat16).reshape(-1, emb.shape[-1]).contiguous()
            tokens = torch.zeros((B, 0), dtype=torch.long, device=emb.device)
            L = 0
        else:
            B, L = tokens.shape
            qf = None
            if query_embeds is not None:
                qf = query_embeds.to(torch.bfloat16).reshape(-1, query_embeds.shape[-1]).contiguous()
        Q = 0 if qf is None else qf.shape[0] // B
        if labels is None:
            labels = torch.zeros((B, Q + L), dtype=torch.long, device=tokens.device)
        if loss_mask is None:
            loss_mask = attention_mask[:, 1:].contiguous() if attention_mask is not None else \
                torch.ones((B, Q + L - 1), dtype=torch.long, device=tokens.device)
        out = self.forward_lm(qf, tokens, labels, loss_mask, {}, want_logits=True)

        class _Out(dict):
            __getattr__ = dict.__getitem__
        return _Out(logits=out["logits"], loss=out["loss"], losses=out["losses"], last_hidden_state=out["last_hidden_state"])


from . import generation as _generation  # noqa: E402  (sample / beam_search / generate, models/modeling_distributed_gpt3.py:1620-1880)

_generation.install(DistributedGPT3)
