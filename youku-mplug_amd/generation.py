"""KV-cache generation on the gfx950 kernels -- the inference half of models/modeling_distributed_gpt3.py
(InferenceParams :1444-1473, sample :1398-1441 / :1620-1735, beam_search :1737-1873, BeamHypotheses :1908-1960)
and DistributedGPT3_Caption.generate (models/distributed_gpt3.py:790-809).

Layout: one cache per layer, cache[l] = [beams, max_len, 3H] bf16 in the decoder's own head-interleaved q|k|v row
format -- the qkv GEMM of every new position writes its row straight into the cache through the GEMM's C row map, and
the fused attention reads K/V from it with (batch, head, row) strides; nothing is transposed or copied (the reference
keeps [max_s, b, np, hn] K and V tensors and copies into them, :905-915).  A step processes the n new positions of
every sequence (prefill: the visual prefix + prompt; afterwards one token), attends causally over the cached rows and
runs the LM head on the last position only.  Beam re-ordering (swap_key_value_dict) is one strided row gather per
layer into the twin buffer.  The search logic of the per-clip loops stays on the host, as in the reference; the lockstep
search over a batch of clips (beam_search_batched_loop) keeps it on the device (ops.beam_advance / ops.beam_advance_groups: one kernel,
csrc/beam_search.hip), and so does sampled generation in lockstep (sample_batched_loop: ops.sample_advance, csrc/sampling.hip; with
return_scores ops.sample_score, csrc/sample_score.hip, records every drawn token's log-probability).  The lockstep loops can also keep
the positions all sequences of a clip share (visual prefix + prompt) once per clip: SharedPrefixDecodeState (kv="shared_prefix";
mpv_gpt_decode_step_shared, csrc/decode_shared_attention.hip), and with it the lockstep beam search takes clips whose prompts differ in
length in ONE search (prompt_length = a sequence: mpv_gpt_prefill_ragged, mpv_gpt_decode_step_shared_ragged), and so does the lockstep
sampling loop (mixed_prompts=True: a left-aligned table and a token column per row, ops.sample_advance_ragged / logits_constrain_ragged /
sample_score_ragged); sample_inflight_loop refills a finished clip's rows with the next clip of the data set while the others go on
(InflightDecodeState: mpv_gpt_decode_step_shared_steps, a suffix position per clip; ops.sample_advance_steps / logits_constrain_steps /
sample_score_steps, a step per row).  decode_weights="fp8" (default "bf16") runs the steps of any of these
loops on e4m3 codes of the decoder's weights (DecodeWeightsQ8; mpv_gpt_decode_step_q8 / _shared_q8, csrc/gemm_w8.hip).
LogitsConstraints(allowed_phrases=PhraseTrie) makes the lockstep and in-flight loops produce members of a closed set of phrases only:
one more launch per step keeps the tokens that continue a row along the trie (ops.logits_trie_mask*, csrc/logits_trie.hip).
Guidance (classifier-free guidance / contrastive decoding) runs a second branch behind a null video's query features in the same state
(guided_state_fn: 2R rows, no loop change) and one launch per step rewrites the conditional logits (ops.logits_guide, csrc/logits_guide.hip).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from types import SimpleNamespace
from typing import Callable, List, Optional

import torch

from . import _lib, ops


class BeamHypotheses:
    """models/modeling_distributed_gpt3.py:1908-1960 (length_penalty 1.0, early_stopping False as constructed at :1763)."""

    def __init__(self, num_beams: int, length_penalty: float = 1.0, early_stopping: bool = False):
        self.length_penalty, self.early_stopping, self.num_beams = length_penalty, early_stopping, num_beams
        self.beams: List[tuple] = []
        self.worst_score = 1e9

    def __len__(self):
        return len(self.beams)

    def add(self, hyp: torch.Tensor, sum_logprobs: float, beam_indices=None):
        score = sum_logprobs / (hyp.shape[-1] ** self.length_penalty)                      # :1936
        if len(self) < self.num_beams or score > self.worst_score:
            self.beams.append((score, hyp, beam_indices))
            if len(self) > self.num_beams:
                order = sorted([(s, i) for i, (s, _, _) in enumerate(self.beams)])
                del self.beams[order[0][1]]
                self.worst_score = order[1][0]
            else:
                self.worst_score = min(score, self.worst_score)

    def is_done(self, best_sum_logprobs: float, cur_len: int) -> bool:
        if len(self) < self.num_beams:
            return False
        if self.early_stopping:
            return True
        return self.worst_score >= best_sum_logprobs / cur_len ** self.length_penalty        # :1958-1960


WEIGHT_MODES = ("bf16", "fp8")


def _check_weight_mode(weights):
    if weights not in WEIGHT_MODES:
        raise ValueError(f"decode_weights must be one of {WEIGHT_MODES} (got {weights!r})")


def _is_scalar(x) -> bool:
    """the arguments that are "one number, or one per clip / row": None, an int and a 0-dim tensor are scalars"""
    return x is None or not hasattr(x, "__len__") or (torch.is_tensor(x) and x.dim() == 0)


def _int_list(x):
    """a sequence or tensor of numbers -> them as a list of ints (a tensor on the device is read); a scalar -> None"""
    return None if _is_scalar(x) else [int(v) for v in (x.tolist() if torch.is_tensor(x) else x)]


class DecodeWeightsQ8:
    """Weight-only FP8 copy of a frozen decoder for the decode steps (include/mpv.h, "FP8 decoder weights"): e4m3fn codes and one
    power-of-two fp32 scale per output row of every layer's qkv / dense / fc1 / fc2 weight and of the tied embedding (the LM head),
    quantised on the device, once (DistributedGPT3.quantize_decode_weights).  The bf16 parameters stay where they are -- this is an
    extra 0.5 x of the quantised tensors.  deq(code) * scale is a bf16 number, so the FP8 steps compute exactly the function of
    the bf16 decoder with dequantized() loaded.  The rounding to e4m3 itself is about 2.7 % relative L2 noise per product (computed
    on the CPU for Gaussian rows; the bf16 gates of this project are 1e-2).  What it costs in caption quality on a trained
    checkpoint has NOT been measured -- no checkpoint exists here; running the unchanged bf16 stack with
    DistributedGPT3.dequantized_state_dict() loaded measures exactly that cost.
    Every source parameter's _version (and storage address) is recorded: stale() is True once any of them has been written to, or
    moved, since."""

    SITES = (("qkv", lambda l: l.self_attention.query_key_value), ("dense", lambda l: l.self_attention.dense),
             ("fc1", lambda l: l.mlp.dense_h_to_4h), ("fc2", lambda l: l.mlp.dense_4h_to_h))

    def __init__(self, gpt):
        lm = gpt.dist_model.language_model
        self.sources = [site(layer).weight for layer in lm.encoder.layers for _, site in self.SITES] + [lm.embedding.word_embeddings.weight]
        for p in self.sources:
            if p.dtype != torch.bfloat16 or p.dim() != 2 or not p.is_contiguous():
                raise ValueError("quantize_decode_weights takes contiguous 2-D bf16 weights")
        self.tensors = [ops.quantize_rows_e4m3(p.detach()) for p in self.sources]       # (codes uint8 [N, K], scale fp32 [N]) per source
        self.versions = [(p._version, p.data_ptr()) for p in self.sources]

    def stale(self) -> bool:
        return any((p._version, p.data_ptr()) != v for p, v in zip(self.sources, self.versions))

    def table(self):
        """-> (_lib.GptWeightsQ8, what it points into): the C table of the step entries"""
        nl = len(self.tensors) // len(self.SITES)
        layers = (_lib.GptLayerWeightsQ8 * nl)()
        for i in range(nl):
            for j, (name, _) in enumerate(self.SITES):
                codes, scale = self.tensors[i * len(self.SITES) + j]
                setattr(layers[i], name + "_q", codes.data_ptr())
                setattr(layers[i], name + "_s", scale.data_ptr())
        return _lib.GptWeightsQ8(nl, layers, self.tensors[-1][0].data_ptr(), self.tensors[-1][1].data_ptr()), layers

    def dequantized(self):
        """-> the bf16 tensors deq(code) * scale, in the order of self.sources"""
        return [(codes.view(torch.float8_e4m3fn).float() * scale[:, None]).to(torch.bfloat16) for codes, scale in self.tensors]

    def nbytes(self) -> int:
        return sum(c.numel() + 4 * s.numel() for c, s in self.tensors)


class DecodeState:
    """Per-generation KV caches of a DistributedGPT3 (the InferenceParams of :1444-1473).  A step is ONE call into the
    C ABI (mpv_gpt_decode_step issues every launch of the incremental forward; the step is launch-bound otherwise)."""

    def __init__(self, gpt, batch: int, max_len: int, weights: str = "bf16"):
        _check_weight_mode(weights)
        gpt._refuse_live_lora("a decode state (the C decode drivers)")
        cfg = gpt.config
        self.gpt, self.batch, self.max_len = gpt, batch, max_len
        self.q8 = None                        # weights="fp8": the decoder's DecodeWeightsQ8 (re-quantised if a weight has moved)
        if weights == "fp8":
            self.q8 = gpt.decode_weights_q8()
            self._q8, self._q8_layers = self.q8.table()
        self.H, self.np_, self.hn, self.V = cfg.hidden_size, cfg.num_attention_heads, cfg.kv_channels, cfg.vocab_size
        assert self.V % 8 == 0, "vocab_size must be a multiple of 8"
        lm = gpt.dist_model.language_model
        dev = lm.embedding.word_embeddings.weight.device
        self.nl = nl = len(lm.encoder.layers)
        self.cache = torch.zeros((nl, batch * max_len, 3 * self.H), dtype=torch.bfloat16, device=dev)
        self.twin = None                      # allocated on the first beam re-order
        self.pos = 0                          # rows cached so far (per sequence)
        # weight table (device pointers; the parameters outlive the state)
        self._layers = (_lib.GptLayerWeights * nl)()
        for i, layer in enumerate(lm.encoder.layers):
            att, mlp, w = layer.self_attention, layer.mlp, self._layers[i]
            w.ln1_w, w.ln1_b = layer.input_layernorm.weight.data_ptr(), layer.input_layernorm.bias.data_ptr()
            w.qkv_w, w.qkv_b = att.query_key_value.weight.data_ptr(), att.query_key_value.bias.data_ptr()
            w.dense_w, w.dense_b = att.dense.weight.data_ptr(), att.dense.bias.data_ptr()
            w.ln2_w, w.ln2_b = layer.post_attention_layernorm.weight.data_ptr(), layer.post_attention_layernorm.bias.data_ptr()
            w.fc1_w, w.fc1_b = mlp.dense_h_to_4h.weight.data_ptr(), mlp.dense_h_to_4h.bias.data_ptr()
            w.fc2_w, w.fc2_b = mlp.dense_4h_to_h.weight.data_ptr(), mlp.dense_4h_to_h.bias.data_ptr()
        fl = lm.encoder.final_layernorm
        self._w = _lib.GptWeights(nl, self.H, self.np_, lm.encoder.layers[0].mlp.dense_h_to_4h.out_features, self.V,
                                  float(fl.eps), self._layers, lm.embedding.word_embeddings.weight.data_ptr(),
                                  lm.embedding.position_embeddings.weight.data_ptr(), fl.weight.data_ptr(), fl.bias.data_ptr(),
                                  int(lm.embedding.position_embeddings.weight.shape[0]))
        self._ptrs = lambda t: (C.c_void_p * nl)(*[t[i].data_ptr() for i in range(nl)])
        self._cache_ptrs = self._ptrs(self.cache)
        self._twin_ptrs = None

    # ------------------------------------------------------------------ one incremental forward
    def step(self, tokens: Optional[torch.Tensor], query_embeds: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tokens [B, n_tok] int64, query_embeds [B, Q, H] for the first call.  Appends Q + n_tok positions per
        sequence and returns the logits of the last one: [B, V] bf16."""
        B = self.batch
        qf, Q = self._query_rows(query_embeds)
        if query_embeds is not None and self.twin is not None:
            self._twin_shared = 0                    # a new visual prefix: the twin's copy of the shared positions is stale (reorder re-gathers from 0)
        L = 0 if tokens is None else tokens.shape[1]
        ids = tokens.contiguous() if L else None
        ws, logits = self._scratch("mpv_gpt_decode_workspace_size", B, Q + L)
        self._call("mpv_gpt_decode_step", self._cache_ptrs, B, self.max_len, self.pos, ops._p(qf), Q, ops._p(ids), L, ws.data_ptr(), ws.numel(),
                   logits.data_ptr(), ops._stream())
        self.pos += Q + L
        return logits

    def _call(self, name: str, *tail):
        """The seam to the C step entries, also for the states built on a DecodeState: name(&weights, *tail), or, when the state holds
        an FP8 table, name_q8(&weights, &fp8 table, *tail) -- every step entry of include/mpv.h has both forms with the same tail."""
        self.gpt._refuse_live_lora(name)      # (a state made while the adapters were merged, stepped after an unmerge)
        head = (C.byref(self._w),)
        if self.q8 is not None:
            name, head = name + "_q8", head + (C.byref(self._q8),)
        ops.check(getattr(_lib.lib(), name)(*head, *tail), name)

    def _scratch(self, size_entry: str, rows: int, *more):
        """-> (the workspace size_entry(&weights, rows, *more) asks for, logits [rows, V] bf16 to be written) for one _call"""
        dev = self.cache.device
        ws = ops.workspace(getattr(_lib.lib(), size_entry)(C.byref(self._w), rows, *more), dev)
        return ws, torch.empty((rows, self.V), dtype=torch.bfloat16, device=dev)

    def _query_rows(self, query_embeds):
        """query_embeds [batch, Q, H] or None -> (the contiguous bf16 rows [batch * Q, H] or None, Q)"""
        qf = None if query_embeds is None else query_embeds.reshape(-1, self.H).to(torch.bfloat16).contiguous()
        return qf, 0 if qf is None else qf.shape[0] // self.batch

    def _ensure_twin(self):
        if self.twin is None:
            self.twin = torch.empty_like(self.cache)
            self._twin_ptrs = self._ptrs(self.twin)
            self._layer_base = torch.arange(self.nl, device=self.cache.device, dtype=torch.int64)[:, None] * self.batch
            self._twin_shared = 0                    # leading positions known to be identical in cache AND twin

    def prefill_fan_out(self, tokens: Optional[torch.Tensor], query_embeds: Optional[torch.Tensor], fan: int) -> torch.Tensor:
        """Prefill ONCE per clip, then fan out: tokens [G, n_tok] / query_embeds [G, Q, H] with G = batch // fan clips are run as
        one step of batch G (they fill the cache rows of sequences 0 .. G-1), then sequence j of the `batch` sequences takes the
        cached rows of clip j // fan -- one gather_rows_ld per copy of the cache (into the twin with index j // fan, and back, so
        that both copies hold the prefix).  That is the first gather of the shared_prefix bookkeeping: a later
        reorder(idx, shared_prefix=n) with n <= the prefilled length moves generated rows only.
        -> logits [batch, V]: row j is clip j // fan's.  (beam_search_loop instead repeats the clip `fan` times and prefills
        identical rows `fan` times.)"""
        assert self.pos == 0 and fan >= 1 and self.batch % fan == 0, (self.pos, self.batch, fan)
        full, G = self.batch, self.batch // fan
        assert (tokens is None or tokens.shape[0] == G) and (query_embeds is None or query_embeds.shape[0] == G)
        self.batch = G                               # a step over the first G sequences' cache rows
        try:
            logits = self.step(tokens, query_embeds)
        finally:
            self.batch = full
        self._ensure_twin()
        dev = self.cache.device
        seq = torch.arange(full, device=dev, dtype=torch.int64)
        pitch, cols = self.max_len * 3 * self.H, self.pos * 3 * self.H
        for idx, src, dst in (((self._layer_base + (seq // fan)[None]).reshape(-1), self.cache, self.twin),
                              ((self._layer_base + seq[None]).reshape(-1), self.twin, self.cache)):
            ops.gather_rows_ld(src.view(-1), idx.contiguous(), dst.view(-1), self.nl * full, cols, pitch, pitch)
        self._twin_shared = self.pos                 # both copies hold the prefilled positions of every sequence
        return logits.repeat_interleave(fan, dim=0)

    def reorder(self, batch_idx: torch.Tensor, shared_prefix: int = 0):
        """swap_key_value_dict(:1459-1473): sequence j continues from the cache of sequence batch_idx[j].  The layers
        are one allocation, so the whole re-order is a single strided row gather over (layer, sequence) rows.
        `shared_prefix`: the caller's promise that the first `shared_prefix` cached positions of sequence j and of sequence
        batch_idx[j] are the same for every j -- beam search over one clip: the visual prefix and the prompt are the same in
        every sequence (264 of ~290 positions at the caption shapes); beam search over a batch of clips: they are identical
        within each group of K consecutive sequences, and batch_idx never leaves the group (ops.beam_advance's src_row).  Once
        both copies of the cache hold them they are not moved again: the gather starts at that position (round 4: 122 -> 9 us
        per step)."""
        self._ensure_twin()
        B, nl = self.batch, self.nl
        shared_prefix = min(int(shared_prefix), self.pos)
        lo = shared_prefix if shared_prefix <= self._twin_shared else 0
        idx = (self._layer_base + batch_idx.to(torch.int64)[None]).reshape(-1)
        pitch = self.max_len * 3 * self.H
        if self.pos > lo:
            off = lo * 3 * self.H
            ops.gather_rows_ld(self.cache.view(-1)[off:], idx, self.twin.view(-1)[off:], nl * B, (self.pos - lo) * 3 * self.H, pitch, pitch)
        self._twin_shared = shared_prefix            # after a gather from 0 the twin holds them too; the source did already
        self.cache, self.twin = self.twin, self.cache
        self._cache_ptrs, self._twin_ptrs = self._twin_ptrs, self._cache_ptrs

    def kv_bytes(self) -> int:
        """bytes of the cache and twin allocations"""
        return sum(t.numel() * t.element_size() for t in (self.cache, self.twin) if t is not None)


class _PrefixSuffixCaches:
    """What SharedPrefixDecodeState and InflightDecodeState have in common: `prefix`, a DecodeState of one sequence per clip whose
    cache [nl, clips * P, 3H] IS the prefix cache (it also carries the weight tables); `suffix` [nl, batch * S, 3H] for the positions
    the batch = clips * fan sequences generate, with its pointer table; and the ONE call of the three shared-prefix step entries."""
    prefix = suffix = twin = None

    def _attach_suffix(self, prefix: "DecodeState", fan: int, P: int, S: int):
        self.prefix, self.fan, self.P, self.S = prefix, fan, P, S
        self.nl, self.H = prefix.nl, prefix.H
        self.suffix = torch.zeros((prefix.nl, self.batch * S, 3 * prefix.H), dtype=torch.bfloat16, device=prefix.cache.device)
        self._suffix_ptrs = prefix._ptrs(self.suffix)

    def _layer_rows(self, per_layer: int) -> torch.Tensor:
        """int64 [nl, 1]: the first of layer l's `per_layer` rows when all layers' rows are numbered through (a gather / scatter index base)"""
        return torch.arange(self.nl, device=self.suffix.device, dtype=torch.int64)[:, None] * per_layer

    def _step_call(self, tokens: torch.Tensor, group_t: Optional[torch.Tensor] = None, max_t: Optional[int] = None) -> torch.Tensor:
        """tokens [batch, 1] int64 -> logits [batch, V] bf16 through ONE step entry, chosen by what the state and the caller hold:
        (group_t, max_t) given -- a suffix position per clip (int32 [clips] on the device, negative: idle) and the largest of them:
        mpv_gpt_decode_step_shared_steps; else a group_prefix_len (a prefix length per clip): mpv_gpt_decode_step_shared_ragged at the
        suffix position self.t; else mpv_gpt_decode_step_shared at self.t.  With prefix lengths both prefix_stride and max_prefix_len
        are P: the pitch of a clip's prefix rows is the longest prefix."""
        st = self.prefix
        steps = group_t is not None
        ws, logits = st._scratch("mpv_gpt_decode_shared_steps_workspace_size" if steps else "mpv_gpt_decode_shared_workspace_size", self.batch)
        caches = (st._cache_ptrs, self._suffix_ptrs, self.batch // self.fan, self.fan, self.P)
        io = (tokens.data_ptr(), ws.data_ptr(), ws.numel(), logits.data_ptr(), ops._stream())
        if steps:
            st._call("mpv_gpt_decode_step_shared_steps", *caches, self.group_prefix_len.data_ptr(), self.P, self.S, group_t.data_ptr(), max_t, *io)
        elif self.group_prefix_len is not None:
            st._call("mpv_gpt_decode_step_shared_ragged", *caches, self.group_prefix_len.data_ptr(), self.P, self.S, self.t, *io)
        else:
            st._call("mpv_gpt_decode_step_shared", *caches, self.S, self.t, *io)
        return logits

    def kv_bytes(self) -> int:
        """bytes of the prefix, suffix and twin allocations that exist"""
        return sum(t.numel() * t.element_size() for t in (None if self.prefix is None else self.prefix.cache, self.suffix, self.twin)
                   if t is not None)


class SharedPrefixDecodeState(_PrefixSuffixCaches):
    """DecodeState for the lockstep loops with the prefix every sequence of a clip shares stored ONCE per clip: a prefix cache
    [nl, G * P, 3H] (P = Q + prompt positions; it is the cache of a DecodeState of batch G and max_len P, filled by the ordinary
    prefill) and a suffix cache [nl, batch * S, 3H] (S = max_len - P) for the positions the sequences generate.  A step is ONE
    call into the C ABI (mpv_gpt_decode_step_shared): its attention reads a clip's prefix once per head for all of the clip's
    sequences (mpv_attn_decode_shared_fwd).  A re-order gathers suffix rows only; the prefix is never copied or moved.
    Resident KV: nl * (G * P + (1 or 2) * batch * S) * 3H * 2 bytes (the twin exists once a re-order has moved rows) against
    nl * 2 * batch * (P + S) * 3H * 2 of DecodeState.
    prefill_fan_out(..., prompt_len=[G lengths]) makes the state ragged: the prompts are right-padded to one width, P = Q + the
    longest prompt is the pitch of a clip's prefix rows, and a device array group_prefix_len = Q + prompt_len says how many of them
    are real (mpv_gpt_prefill_ragged, mpv_gpt_decode_step_shared_ragged: clip g's sequences sit at position group_prefix_len[g] + t).
    The pad rows behind a clip's prompt are written by the prefill and never read."""

    def __init__(self, gpt, batch: int, max_len: int, weights: str = "bf16"):
        _check_weight_mode(weights)
        gpt._refuse_live_lora("a shared-prefix decode state (the C decode drivers)")
        self.gpt, self.batch, self.max_len, self.weights = gpt, batch, max_len, weights
        self.fan = self.P = self.S = 0       # set, with prefix (the DecodeState of the prefill) and suffix, by prefill_fan_out
        self.t = 0                            # suffix rows cached so far (per sequence)
        self.group_prefix_len = None          # ragged: int32 [G] on the device, Q + prompt_len

    @property
    def pos(self) -> int:
        return self.P + self.t

    def prefill_fan_out(self, tokens: Optional[torch.Tensor], query_embeds: Optional[torch.Tensor], fan: int,
                        prompt_len: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tokens [G, n_tok] / query_embeds [G, Q, H], G = batch // fan: the prefill runs once per clip into the prefix cache and
        nothing is copied.  -> logits [batch, V]: row j is clip j // fan's.
        prompt_len (G lengths, 1 <= prompt_len[g] <= n_tok; default None: every prompt is n_tok long): clip g's prompt is
        tokens[g, :prompt_len[g]], the rest of its row padding; the logits are those of each clip's own last prompt row."""
        assert self.prefix is None and fan >= 1 and self.batch % fan == 0, (self.batch, fan)
        G = self.batch // fan
        assert (tokens is None or tokens.shape[0] == G) and (query_embeds is None or query_embeds.shape[0] == G)
        P = (0 if query_embeds is None else query_embeds.shape[1]) + (0 if tokens is None else tokens.shape[1])
        if not 0 < P < self.max_len:
            raise ValueError(f"a shared prefix of {P} positions leaves no room in max_len {self.max_len}")
        self.prefix = DecodeState(self.gpt, G, P, self.weights)
        if prompt_len is None:
            logits = self.prefix.step(tokens, query_embeds)
        else:
            logits = self._ragged_prefill(tokens, query_embeds, prompt_len)
        self._attach_suffix(self.prefix, fan, P, self.max_len - P)
        return logits.repeat_interleave(fan, dim=0)

    def _ragged_prefill(self, tokens, query_embeds, prompt_len) -> torch.Tensor:
        st = self.prefix
        G, dev = st.batch, st.cache.device
        if tokens is None or tokens.dim() != 2:
            raise ValueError("prefill_fan_out(prompt_len=...) needs the right-padded prompts: tokens [G, n_tok]")
        L = tokens.shape[1]
        lens = _int_list(prompt_len)                 # host values: the caller's
        if lens is None or len(lens) != G or min(lens) < 1 or max(lens) > L:
            raise ValueError(f"prompt_len must hold {G} lengths in [1, {L}] (got {lens})")
        qf, Q = st._query_rows(query_embeds)
        plen = torch.as_tensor(lens, dtype=torch.int64).to(dev)
        self.group_prefix_len = (plen + Q).to(torch.int32)
        last_row = (plen + (Q - 1)).contiguous()
        ids = tokens.contiguous()
        ws, logits = st._scratch("mpv_gpt_decode_workspace_size", G, Q + L)
        st._call("mpv_gpt_prefill_ragged", st._cache_ptrs, G, st.max_len, ops._p(qf), Q, ids.data_ptr(), L, last_row.data_ptr(), ws.data_ptr(),
                 ws.numel(), logits.data_ptr(), ops._stream())
        st.pos += Q + L
        return logits

    def step(self, tokens: torch.Tensor, query_embeds: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tokens [batch, 1] int64 -> the logits of the new position: [batch, V] bf16"""
        if self.prefix is None:
            raise ValueError("SharedPrefixDecodeState.step: prefill_fan_out comes first")
        if query_embeds is not None or tokens is None or tokens.dim() != 2 or tokens.shape[1] != 1:
            raise ValueError("SharedPrefixDecodeState.step takes ONE token per sequence and no query_embeds after the prefill")
        if tokens.shape[0] != self.batch:
            raise ValueError(f"SharedPrefixDecodeState.step: {tokens.shape[0]} rows for {self.batch} sequences")
        if self.t >= self.S:
            raise ValueError(f"SharedPrefixDecodeState.step: the suffix cache of {self.S} positions is full")
        logits = self._shared_step(tokens.contiguous())
        self.t += 1
        return logits

    def _shared_step(self, tokens: torch.Tensor) -> torch.Tensor:
        return self._step_call(tokens)

    def reorder(self, batch_idx: torch.Tensor, shared_prefix: Optional[int] = None):
        """sequence j continues from the suffix rows of sequence batch_idx[j] (which must belong to the same clip): one strided
        row gather of the t cached suffix rows over (layer, sequence) into the twin.  `shared_prefix` (default: the prefilled
        length) must cover the prefilled positions -- they are shared by construction."""
        if self.prefix is None:
            raise ValueError("SharedPrefixDecodeState.reorder: prefill_fan_out comes first")
        if shared_prefix is not None and int(shared_prefix) < self.P:
            raise ValueError(f"shared_prefix {int(shared_prefix)} is smaller than the {self.P} prefilled positions, which are stored once per clip")
        if self.t == 0:
            return                                   # nothing generated yet: nothing to move
        if self.twin is None:
            self.twin = torch.empty_like(self.suffix)
            self._twin_ptrs = self.prefix._ptrs(self.twin)
            self._layer_base = self._layer_rows(self.batch)
        idx = (self._layer_base + batch_idx.to(torch.int64)[None]).reshape(-1)
        pitch = self.S * 3 * self.H
        ops.gather_rows_ld(self.suffix.view(-1), idx, self.twin.view(-1), self.nl * self.batch, self.t * 3 * self.H, pitch, pitch)
        self.suffix, self.twin = self.twin, self.suffix
        self._suffix_ptrs, self._twin_ptrs = self._twin_ptrs, self._suffix_ptrs


class InflightDecodeState(_PrefixSuffixCaches):
    """The shared-prefix state of sample_inflight_loop: `slots` clips x `fan` sequences stay resident and a finished clip's slot is
    given to the next clip while the others go on.  The prefix cache is [nl, slots * P, 3H] with P = Q + the longest prompt of the
    whole call (it is the cache of a DecodeState of batch `slots`, which also carries the weight tables), group_prefix_len int32
    [slots] says how many of a slot's rows are real, and the suffix cache is [nl, slots * fan * S, 3H]; samples never swap caches, so
    there is no twin.  install() prefills new clips on a small staging state (mpv_gpt_prefill_ragged) and copies their prefix rows
    into their slots with ONE scatter over all layers; step() is ONE call into the C ABI (mpv_gpt_decode_step_shared_steps) with a
    suffix position per slot, idle slots included."""

    def __init__(self, gpt, slots: int, fan: int, prefix_rows: int, suffix_rows: int, weights: str = "bf16"):
        _check_weight_mode(weights)
        if slots < 1 or fan < 1 or prefix_rows < 1 or suffix_rows < 1:
            raise ValueError(f"InflightDecodeState: slots {slots}, fan {fan}, prefix rows {prefix_rows} and suffix rows {suffix_rows} must be positive")
        self.gpt, self.slots, self.weights = gpt, int(slots), weights
        self.batch = self.slots * int(fan)
        self._attach_suffix(DecodeState(gpt, self.slots, int(prefix_rows), weights), int(fan), int(prefix_rows), int(suffix_rows))
        self.group_prefix_len = torch.ones(self.slots, dtype=torch.int32, device=self.suffix.device)   # a free slot: one (zero) prefix row, never used
        self._layer_base = self._layer_rows(self.slots)
        self.prefills = self.steps = 0            # launches issued so far (the loop's report)

    def install(self, slot_ids, tokens: torch.Tensor, query_embeds: Optional[torch.Tensor], prompt_len) -> torch.Tensor:
        """prefills k new clips -- tokens [k, L] right-padded, query_embeds [k, Q, H], prompt_len k lengths in [1, L], Q + L == the
        state's prefix rows -- into the slots slot_ids (k distinct slot numbers) -> their prefill logits [k, V]"""
        slot_ids = [int(s) for s in slot_ids]
        k = len(slot_ids)
        Q = 0 if query_embeds is None else query_embeds.shape[1]
        if k < 1 or tokens.shape[0] != k or len(set(slot_ids)) != k or min(slot_ids) < 0 or max(slot_ids) >= self.slots:
            raise ValueError(f"install: {k} distinct slots in [0, {self.slots}) for {tokens.shape[0]} clips (got {slot_ids})")
        if Q + tokens.shape[1] != self.P:
            raise ValueError(f"install: {Q} query slots + {tokens.shape[1]} prompt columns are not the state's {self.P} prefix rows")
        staging = SharedPrefixDecodeState(self.gpt, k, self.P + 1, self.weights)
        logits = staging.prefill_fan_out(tokens, query_embeds, 1, prompt_len=prompt_len)
        dev = self.suffix.device
        idx = (self._layer_base + torch.as_tensor(slot_ids, dtype=torch.int64).to(dev)[None]).reshape(-1).contiguous()
        row = self.P * 3 * self.H                 # a clip's prefix rows of one layer are one "row" of the scatter
        ops.scatter_rows(staging.prefix.cache.view(-1), idx, self.prefix.cache.view(-1), self.nl * k, row, row)
        self.group_prefix_len[torch.as_tensor(slot_ids, dtype=torch.long).to(dev)] = staging.group_prefix_len
        self.prefills += 1
        return logits

    def step(self, tokens: torch.Tensor, group_t: torch.Tensor, max_t: int) -> torch.Tensor:
        """tokens [slots * fan, 1] int64, group_t int32 [slots] on the device (slot g's suffix position; negative: idle), max_t the
        largest of them (host) -> logits [slots * fan, V] bf16; an idle slot's rows are unspecified"""
        if tokens is None or tokens.dim() != 2 or tokens.shape != (self.batch, 1):
            raise ValueError(f"InflightDecodeState.step takes ONE token for each of the {self.batch} sequences")
        if group_t.dtype != torch.int32 or group_t.numel() != self.slots or not group_t.is_contiguous():
            raise ValueError(f"InflightDecodeState.step: group_t must be a contiguous int32 tensor of {self.slots} positions")
        if not 0 <= int(max_t) < self.S:
            raise ValueError(f"InflightDecodeState.step: suffix position {int(max_t)} does not fit the suffix cache of {self.S} positions")
        self.steps += 1
        return self._steps_step(tokens.contiguous(), group_t, int(max_t))

    def _steps_step(self, tokens, group_t, max_t) -> torch.Tensor:
        return self._step_call(tokens, group_t, max_t)

    def reorder(self, batch_idx: torch.Tensor, group_rows: torch.Tensor, max_rows: int):
        """beam search only: sequence j continues from the suffix rows of sequence batch_idx[j] (int64 [slots * fan], inside j's slot),
        of which slot g has written group_rows[g] (int32 [slots] on the device; 0: nothing of the slot moves), at most max_rows (host):
        ONE launch over all layers into the twin (ops.kv_suffix_reorder_steps), which the first call allocates -- a sampling call
        never does -- and which then becomes the suffix cache."""
        if group_rows.dtype != torch.int32 or group_rows.numel() != self.slots or not group_rows.is_contiguous():
            raise ValueError(f"InflightDecodeState.reorder: group_rows must be a contiguous int32 tensor of {self.slots} counts")
        if not 0 <= int(max_rows) <= self.S:
            raise ValueError(f"InflightDecodeState.reorder: {int(max_rows)} rows do not fit the suffix cache of {self.S} positions")
        if int(max_rows) == 0:
            return                                   # nothing generated yet: nothing to move
        if self.twin is None:
            self.twin = torch.zeros_like(self.suffix)
            self._twin_ptrs = self.prefix._ptrs(self.twin)
        ops.kv_suffix_reorder_steps(self.suffix, self.twin, batch_idx.contiguous(), group_rows, fan=self.fan, suffix_rows=self.S,
                                    max_rows=int(max_rows))
        self.suffix, self.twin = self.twin, self.suffix
        self._suffix_ptrs, self._twin_ptrs = self._twin_ptrs, self._suffix_ptrs


def make_inflight_state_fn(gpt, weights: str = "bf16"):
    """The make_state of sample_inflight_loop: (slots, fan, prefix_rows, suffix_rows) -> an InflightDecodeState on `weights`"""
    _check_weight_mode(weights)
    return lambda slots, fan, prefix_rows, suffix_rows: InflightDecodeState(gpt, slots, fan, prefix_rows, suffix_rows, weights)


KV_MODES = ("per_sequence", "shared_prefix")


def make_state_fn(gpt, kv: str = "per_sequence", weights: str = "bf16"):
    """The make_state of the loops for the keyword `kv`: "per_sequence" (DecodeState: every sequence owns a full cache) or
    "shared_prefix" (SharedPrefixDecodeState; the lockstep loops only), and for `weights`: "bf16", or "fp8" (the steps run on the
    decoder's DecodeWeightsQ8, which the first such state quantises)."""
    if kv not in KV_MODES:
        raise ValueError(f"kv must be one of {KV_MODES} (got {kv!r})")
    _check_weight_mode(weights)
    cls = DecodeState if kv == "per_sequence" else SharedPrefixDecodeState
    if weights == "bf16":
        return lambda batch, max_len: cls(gpt, batch, max_len)
    return lambda batch, max_len: cls(gpt, batch, max_len, weights)


# ---------------------------------------------------------------------------------------------- sampling helpers
def _filter_top_k(logits, top_k):                                                            # :1369-1373
    kth = torch.topk(logits, top_k)[0][..., -1, None]
    logits.masked_fill_(logits < kth, float("-inf"))


def _filter_top_p(logits, top_p):                                                            # :1376-1395
    sorted_logits, sorted_indices = torch.sort(logits, descending=True)
    cumulative = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
    filt = cumulative > top_p
    filt[:, 1:] = filt[:, :-1].clone()
    filt[..., 0] = 0
    logits.masked_fill_(filt.scatter(1, sorted_indices, filt), float("-inf"))


def sample_token(logits: torch.Tensor, top_k=0, top_p=0.0, temperature=1.0, vocab_size=None, generator=None) -> torch.Tensor:
    """models/modeling_distributed_gpt3.py:1398-1441.  Greedy (top_k == 1) runs on mpv_logprob_topk; the stochastic
    filters are a handful of torch calls on the [B, V] logits, as in the reference."""
    assert logits.ndim == 2
    if top_k == 1:
        assert top_p == 0.0, "cannot set both greedy and top-p samplings."
        samples = ops.logprob_topk(logits, 1)[1].view(-1)
    else:
        lg = logits.float().clone()
        if temperature != 1.0:
            lg.div_(temperature)
        if top_k > 1:
            assert top_p == 0.0, "cannot set both top-k and top-p samplings."
            _filter_top_k(lg, top_k)
        elif top_p > 0.0:
            assert top_p <= 1.0
            _filter_top_p(lg, top_p)
        samples = torch.multinomial(lg.softmax(dim=-1), num_samples=1, generator=generator).view(-1)
    if vocab_size:
        samples = torch.clamp(samples, min=0, max=vocab_size - 1)
    return samples


# ---------------------------------------------------------------------------------------------- search loops
def _gen_config(gpt):
    ex = gpt.config.extra
    return SimpleNamespace(tokens_to_generate=ex.get("tokens_to_generate", 100), eod_id=ex.get("eod_id", 7), top_k=ex.get("top_k", 0),
                           top_p=ex.get("top_p", 0.9), max_position_embeddings=gpt.config.max_position_embeddings,
                           vocab_size=gpt.config.vocab_size)


StepFn = Callable[[Optional[torch.Tensor], Optional[torch.Tensor]], torch.Tensor]


def _no_sample_scores(return_scores, who):
    if return_scores:
        raise ValueError(f"return_scores=True needs the lockstep sampling loop (sample_batched / generate(sampler=\"device\")): {who} "
                         "has no per-sample scores")


def _pad_for_generation(cfg, tokens, fill, prompt_length, query_embeds):
    """the prelude of every loop: the token table grows by tokens_to_generate columns of `fill` -> (tokens, final_len, Q), final_len
    clamped to max_position_embeddings and above prompt_length (the shortest prompt of the call), Q the number of query slots"""
    tokens = torch.cat((tokens, torch.full((tokens.size(0), cfg.tokens_to_generate), fill, dtype=torch.long, device=tokens.device)), dim=-1)
    final_len = min(tokens.size(1), cfg.max_position_embeddings)
    if prompt_length >= final_len:
        raise ValueError("context length + tokens_to_generate too large")
    return tokens, final_len, 0 if query_embeds is None else query_embeds.size(1)


def beam_search_loop(cfg, make_state: Callable[[int, int], object], tokens: torch.Tensor, query_embeds=None, beam_size=5,
                     num_return_gen=1, stop_token=None, prompt_length=None, topk_fn=None, return_scores=False):
    """models/modeling_distributed_gpt3.py:1737-1873.  `make_state(batch, max_len)` returns an object with
    .step(tokens, query_embeds) -> logits [beams, V] and .reorder(batch_idx, shared_prefix=n); `topk_fn(logits, k, add)` ->
    (values, indices) of log_softmax + add.  Both are injectable so the host logic can be driven from any logits source.
    return_scores=True is refused: the hypotheses carry their scores already (SampleScores belong to sample_batched_loop)."""
    _no_sample_scores(return_scores, "beam_search_loop")
    assert tokens.size(0) == 1
    dev = tokens.device
    prompt_length = int(prompt_length) if prompt_length is not None else tokens.size(1)
    stop_token = cfg.eod_id if stop_token is None else int(stop_token)
    tokens, final_len, Q = _pad_for_generation(cfg, tokens, stop_token, prompt_length, query_embeds)
    state = make_state(beam_size, final_len + Q)
    hyp = BeamHypotheses(beam_size)
    done = False
    # The search state lives on the host (round 4): the token table and the beam scores are python-side bookkeeping in the
    # reference too (:1799-1840 walks the candidates one .item() at a time); per step the device sees ONE [2, beams] int64
    # upload (source beam, new token), the scores it adds to the log-probabilities, and two small downloads of the candidates.
    scores_h = [0.0] * beam_size
    scores = torch.zeros(beam_size, dtype=torch.float32, device=dev)
    tokens_h = tokens.cpu().repeat(beam_size, 1)
    if query_embeds is not None:
        query_embeds = query_embeds.repeat(beam_size, 1, 1)
    prev, total_prompt, total_final = 0, prompt_length + Q, final_len + Q
    context_length = total_prompt
    t2u = tokens_h[:, :total_prompt - Q].to(dev)
    for context_length in range(total_prompt, total_final):
        logits = state.step(t2u, query_embeds if context_length == total_prompt else None)
        V = logits.size(-1)
        k2 = 2 * beam_size
        vals, idxs = topk_fn(logits, k2, scores)                                             # log_softmax + scores (:1790-1791)
        vals, idxs = vals.tolist(), idxs.tolist()
        if context_length == total_prompt:                                                   # all beams identical: row 0 only (:1793-1795)
            cand = [(vals[0][j], 0, idxs[0][j]) for j in range(k2)]
        else:
            cand = [(vals[b][j], b, idxs[b][j]) for b in range(beam_size) for j in range(k2)]
            cand.sort(key=lambda c: (-c[0], c[1] * V + c[2]))
            cand = cand[:k2]
        next_beams = []
        for rank, (beam_score, beam_id, token_id) in enumerate(cand):
            if token_id == stop_token:
                if rank >= beam_size:                                                        # :1809-1812
                    continue
                hyp.add(tokens_h[beam_id].clone(), beam_score, context_length + 1 - total_prompt)
            else:
                next_beams.append((token_id, beam_score, beam_id))
            if len(next_beams) == beam_size:
                break
        if hyp.is_done(max(c[0] for c in cand), context_length + 1 - total_prompt):
            done = True
            break
        best_h = [b[2] for b in next_beams]
        tokens_h = tokens_h[best_h, :]
        tokens_h[:, context_length - Q] = torch.tensor([b[0] for b in next_beams], dtype=torch.long)
        scores_h = [b[1] for b in next_beams]
        moved = torch.tensor([best_h, [b[0] for b in next_beams]], dtype=torch.long).to(dev)
        scores = torch.tensor(scores_h, dtype=torch.float32).to(dev)
        state.reorder(moved[0], shared_prefix=total_prompt)
        t2u = moved[1].view(-1, 1)
        prev = context_length
    if not done:
        for b in range(beam_size):
            hyp.add(tokens_h[b].clone(), scores_h[b], context_length + 1 - total_prompt)
    ranked = sorted(hyp.beams, key=lambda x: x[0], reverse=True)
    num_return_gen = min(num_return_gen, len(ranked))
    return SimpleNamespace(sequences=torch.stack([ranked[i][1] for i in range(num_return_gen)], dim=0).to(dev),
                           scores=torch.tensor([ranked[i][0] for i in range(num_return_gen)], dtype=torch.float32))


class BeamState:
    """The search state of beam_search_batched_loop for B clips x K beams, as device tensors (struct of arrays; the contract of
    include/mpv.h: mpv_beam_advance).  `tokens` is the current token table, `tokens_alt` the one the next advance writes;
    ops.beam_advance swaps them."""

    def __init__(self, tokens: torch.Tensor, beams: int):
        B, Lt = tokens.shape
        dev = tokens.device
        self.batch, self.beams, self.row_len = B, beams, Lt
        self.tokens = tokens.to(torch.int64)[:, None, :].repeat(1, beams, 1).contiguous()
        self.tokens_alt = torch.empty_like(self.tokens)
        self.scores = torch.zeros((B, beams), dtype=torch.float32, device=dev)
        self.hyp_score = torch.zeros((B, beams), dtype=torch.float64, device=dev)
        self.hyp_order = torch.zeros((B, beams), dtype=torch.int32, device=dev)
        self.hyp_tokens = torch.zeros((B, beams, Lt), dtype=torch.int64, device=dev)
        self.hyp_count = torch.zeros(B, dtype=torch.int32, device=dev)
        self.hyp_next = torch.zeros(B, dtype=torch.int32, device=dev)
        self.worst = torch.full((B,), 1e9, dtype=torch.float64, device=dev)
        self.done = torch.zeros(B, dtype=torch.int32, device=dev)
        self.src_row = torch.arange(B * beams, dtype=torch.int64, device=dev)
        self.next_tok = torch.zeros(B * beams, dtype=torch.int64, device=dev)

    ARRAYS = ("tokens", "scores", "hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "hyp_next", "worst", "done", "src_row", "next_tok")


def beam_search_batched_loop(cfg, make_state: Callable[[int, int], object], tokens: torch.Tensor, query_embeds=None, beam_size=5,
                             num_return_gen=1, stop_token=None, prompt_length: Optional[int] = None, topk_fn=None, advance_fn=None,
                             constraints: Optional["LogitsConstraints"] = None, constrain_fn=None, return_scores=False, beam_groups=1,
                             diversity_penalty=0.0, group_advance_fn=None, trie_fn=None):
    """Beam search for B clips in lockstep, the search state on the device: tokens [B, L], query_embeds [B, Q, H].  Every decode step
    advances all the clips' beams, so the decoder's weights are read once per generated position instead of once per clip and
    position, the prefill runs once per clip and the bookkeeping of a step is one kernel.  `make_state(batch, max_len)` -> an object
    with prefill_fan_out / step / reorder (DecodeState, SharedPrefixDecodeState); make_state and the *_fn are injectable as in
    beam_search_loop, and return_scores=True is refused as there.
    A step issues state.prefill_fan_out(prompts, query_embeds, fan) (the first) or state.step(bs.next_tok); constrain_fn; topk_fn(logits,
    m, bs.scores); the advance (per clip what one iteration of beam_search_loop does; it fills bs.src_row / bs.next_tok and swaps the
    token tables); the read that tells whether every clip is done -- nothing else goes to the host --; state.reorder(bs.src_row,
    shared_prefix=Q + prompt).  Finished clips are NOT compacted away: a clip that is done is frozen by the advance and keeps stepping
    as padding rows (stop token, identity re-order) until every clip is done or the length is exhausted.  After the loop the state is
    downloaded once; the final flush of the unfinished clips and the stable ranking run on the host (_ranked_hypotheses).
    `constraints` (a LogitsConstraints; None or inactive: no call and no launch is added): before topk_fn every step edits the raw
    logits of all rows -- the first step's and those of frozen clips too, which the advance ignores -- through constrain_fn
    (ops.logits_constrain) on the beams' token table, with the stop token as the termination id of min_new_tokens and the lowest
    finite bf16 as the ban value (include/mpv.h says why it is not -inf here).
    One prompt length, one group (prompt_length an int or None, beam_groups 1): fan = beam_size, m = 2 * beam_size, the advance is
    advance_fn (ops.beam_advance) with pos = prompt + n and cur_len = n + 1.  -> a list of B namespaces (sequences [n, Lt], scores
    [n]), clip by clip what beam_search_loop returns for it.
    beam_groups = G > 1: diverse (group) beam search.  beam_size is then K', the beams PER GROUP; the state holds B x G x K'
    sequences, a (clip, group) pair being a clip of the BeamState; fan = G * K'; m = 2K' + (G-1)K'; the advance is group_advance_fn
    with groups= and diversity_penalty= added (ops.beam_advance_groups: per clip, group after group, one iteration on the values
    lowered by diversity_penalty times the number of next beams that the groups before chose with the candidate's token at this
    step).  The re-order stays inside the (clip, group), so both KV states work as they are.  The host finish runs per (clip, group):
    -> per clip a namespace (sequences [n, Lt], scores [n], group [n] int64), group 0's best r = num_return_gen // G rows first, then
    group 1's, ...; a group with fewer hypotheses yields fewer rows.  From the second group on the scores are penalised search scores,
    not model likelihoods.  num_return_gen must be a multiple of G with r <= K'.
    prompt_length = a sequence of B lengths (either number of groups): ONE search over clips whose prompts differ in length; clip c's
    prompt is tokens[c, :prompt_length[c]].  The state gets the prompts right-padded and the lengths (prefill_fan_out(..., prompt_len=):
    SharedPrefixDecodeState; a DecodeState is refused); the beams' table is the left-padded one of _left_padded_table, which says why
    cur_len = 2 * (n + 1) then reproduces each clip's own search exactly; pos = P_max + n.  The loop runs until the shortest prompt's
    budget ends; where a longer prompt's budget ends the host sets the clip's bs.done on the device (the advance then freezes it:
    tokens and scores stay, include/mpv.h mpv_beam_advance) after saving which of these clips were not done -- no host read is added
    -- and _strip_left_padding flushes the beams of exactly those.  Raised before the first launch: include_prompt=True constraints
    (the pad columns would count as prompt), 2 * Lt > 2048 columns (the advance kernels' limit), what _mixed_prompt_state refuses.
    constraints.allowed_phrases (a PhraseTrie): after constrain_fn and before topk_fn every step keeps only the tokens that continue a
    row along the trie, through trie_fn (ops.logits_trie_mask) on the same table, column, termination id and ban value.  The scores are
    then renormalised over the allowed tokens.  With fewer allowed tokens than 2K the candidates include banned ones at BAN_BEAM-sized
    values; they rank behind every allowed one, die at the next step and may reach the hypothesis store, so the host finish drops every
    hypothesis whose generated part is not a phrase (trie.lookup: exact, no score threshold) and a clip may return fewer than
    num_return_gen rows; every result carries phrase_index [n] int64.  The columns behind every prompt are set to the stop token in the
    loop's table.  Raised before the first launch: what _active_trie refuses (min_new_tokens, a phrase with the stop token)."""
    _no_sample_scores(return_scores, "beam_search_batched_loop")
    B, dev, K = tokens.size(0), tokens.device, int(beam_size)
    G, lam, per_group = _beam_groups(beam_groups, diversity_penalty, num_return_gen, K)
    if G != 1:
        if group_advance_fn is None:
            raise ValueError("beam_groups > 1 needs a group_advance_fn (ops.beam_advance_groups)")
        advance, more = group_advance_fn, dict(groups=G, diversity_penalty=lam)
    else:
        advance, more = advance_fn, {}
    constraints_given, constraints = constraints, _active_constraints(constraints, constrain_fn)
    lens = _mixed_prompt_lengths(prompt_length, B, tokens.size(1))                         # None: one prompt length
    stop_token = cfg.eod_id if stop_token is None else int(stop_token)
    trie = _active_trie(constraints_given, trie_fn, [stop_token])
    if trie is not None:
        tokens = _stop_behind_prompts(tokens, lens if lens is not None else tokens.size(1) if prompt_length is None else int(prompt_length), stop_token)
    if lens is None:
        prompt_length = int(prompt_length) if prompt_length is not None else tokens.size(1)
        tokens, final_len, Q = _pad_for_generation(cfg, tokens, stop_token, prompt_length, query_embeds)
        state, total_final = make_state(B * G * K, final_len + Q), final_len + Q
        table, prompts, prefill_more, ends, len_scale = tokens, tokens[:, :prompt_length], {}, {}, 1
    else:
        if constraints is not None and constraints.include_prompt:
            raise ValueError("LogitsConstraints(include_prompt=True) does not combine with prompts of different lengths: the "
                             "left padding of the token table would count as prompt")
        prompt_length = max(lens)
        tokens, final_len, Q = _pad_for_generation(cfg, tokens, stop_token, prompt_length, query_embeds)
        if 2 * tokens.size(1) > 2048:
            raise ValueError(f"prompts of different lengths need a token table of {2 * tokens.size(1)} columns; the advance kernels take 2048")
        state, total_final = _mixed_prompt_state(cfg, make_state, B * G * K, Q, lens, final_len, "prompts of different lengths need")
        table, prompts, ends, flush, len_scale = _left_padded_table(tokens, lens, G, stop_token, final_len)
        prefill_more = dict(prompt_len=lens)
    bs = BeamState(table if G == 1 else table.repeat_interleave(G, 0), K)                  # pseudo-clip b * G + g: group g of clip b
    total_prompt, m = prompt_length + Q, 2 * K + (G - 1) * K
    for n, context_length in enumerate(range(total_prompt, total_final)):
        if n == 0:
            logits = state.prefill_fan_out(prompts.contiguous(), query_embeds, G * K, **prefill_more)
        else:
            logits = state.step(bs.next_tok.view(-1, 1))
        if constraints is not None:
            constrain_fn(logits, bs.tokens.view(B * G * K, -1), pos=context_length - Q, constraints=constraints, prompt_len_all=prompt_length,
                         eos_ids=[stop_token], ban_value=BAN_BEAM)
        if trie is not None:
            trie_fn(logits, bs.tokens.view(B * G * K, -1), pos=context_length - Q, trie=trie, prompt_len_all=prompt_length, eos_ids=[stop_token],
                    ban_value=BAN_BEAM)
        vals, idxs = topk_fn(logits, m, bs.scores.view(-1))                                  # log_softmax + scores (:1790-1791)
        advance(vals, idxs, bs, vocab=logits.size(-1), pos=context_length - Q, cur_len=len_scale * (n + 1), first=n == 0,
                stop_token=stop_token, **more)
        if n + 1 in ends:                                                                    # these clips' budgets end here: freeze them
            flush[ends[n + 1]] = 1 - bs.done[ends[n + 1]]
            bs.done[ends[n + 1]] = 1
        if bool(bs.done.all()):                                                              # the step's one host read
            break
        state.reorder(bs.src_row, shared_prefix=total_prompt)
    h = SimpleNamespace(**{k: getattr(bs, k).cpu() for k in BeamState.ARRAYS})              # one download
    if lens is not None:
        _strip_left_padding(h, lens, flush, len_scale)
    return _beam_results(h, B, G, K, per_group, dev, trie, lens if lens is not None else [prompt_length] * B, stop_token)


def _beam_groups(beam_groups, diversity_penalty, num_return_gen, K):
    """the checks of a beam loop's group arguments -> (G, lambda, rows returned per group); one group: (1, 0.0, num_return_gen)"""
    G = int(beam_groups)
    if G == 1:
        return 1, 0.0, num_return_gen
    if G < 1 or isinstance(beam_groups, bool):
        raise ValueError(f"beam_groups must be a positive integer (got {beam_groups!r})")
    lam = float(diversity_penalty)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"diversity_penalty must be finite and not negative (got {diversity_penalty!r})")
    if int(num_return_gen) % G or int(num_return_gen) // G > K or int(num_return_gen) < G:
        raise ValueError(f"num_return_gen ({num_return_gen}) must be a multiple of beam_groups ({G}) with at most beam_size ({K}) "
                         "rows per group")
    return G, lam, int(num_return_gen) // G


def _beam_results(h, B, G, K, per_group, dev, trie=None, prompt_lens=None, stop_token=None):
    """the downloaded BeamState arrays `h` of B clips x G groups -> the list of B result namespaces of the lockstep beam loops.
    trie (a PhraseTrie; prompt_lens: the clips' prompt lengths in the left-aligned rows of `h`): a hypothesis stays only if its
    generated part is a phrase, and the namespaces carry phrase_index [n] int64"""
    out = []
    for clip in range(B):
        ranked = [_ranked_hypotheses(h, clip * G + g, K) for g in range(G)]
        if trie is not None:                                                                 # best first, until per_group phrases are found
            kept = []
            for rg in ranked:
                kept.append([])
                for r in rg:
                    if len(kept[-1]) == per_group:
                        break
                    idx = trie.lookup(generated_part(r[1], prompt_lens[clip], stop_token))
                    if idx >= 0:
                        kept[-1].append(r + (idx,))
            ranked = kept
        ranked = [rg[:per_group] for rg in ranked]
        rows = [r[1] for rg in ranked for r in rg]
        res = SimpleNamespace(sequences=(torch.stack(rows, dim=0) if rows else h.tokens.new_zeros((0, h.tokens.size(-1)))).to(dev),
                              scores=torch.tensor([r[0] for rg in ranked for r in rg], dtype=torch.float32))
        if trie is not None:
            res.phrase_index = torch.tensor([r[-1] for rg in ranked for r in rg], dtype=torch.int64)
        if G > 1:
            res.group = torch.tensor([g for g, rg in enumerate(ranked) for _ in rg], dtype=torch.int64)
        out.append(res)
    return out


def _left_padded_table(tokens, lens, G, stop_token, final_len):
    """The token table of the lockstep beam search over prompts of `lens` tokens (tokens [B, Lt]: the padded input rows; G groups per
    clip) -> (table [B, 2 * Lt], prompts [B, P_max], ends, flush, len_scale = 2).
    The table is LEFT-padded with the stop token so that every prompt ends at column P_max = max(lens): topk_fn, the advance and
    constrain_fn then run as for one prompt length, with prompt_len_all = P_max and pos = P_max + n, and a generated token sits n
    columns behind every clip's prompt.  `prompts` are the prompts RIGHT-padded with the stop token, what the ragged prefill takes.
    Row length: the advance scores a hypothesis by value / row_len and tests worst >= best / cur_len, so the search depends on the
    table's width.  The padded table is 2 * Lt wide (Lt = L + tokens_to_generate, the width of the table of one prompt length;
    P_max - P_min + final_len <= 2 * Lt always) and the loop passes cur_len = len_scale * (n + 1): both sides of every comparison are
    then exactly half of what the Lt-wide table gives (a division by two is exact), so a clip's search is step for step the one of a
    loop over clips of its own length, and the stored scores are doubled -- exactly -- by _strip_left_padding.
    Budget: clip c generates at most final_len - lens[c] positions, as a search over clips of its length would: ends[step] holds the
    pseudo-clips (clip * G + group) to freeze after that step, and the loop notes in flush (int32 [B * G]) which were not done."""
    B, Lt, dev = tokens.size(0), tokens.size(1), tokens.device
    longest, shortest = max(lens), min(lens)
    lens_d = torch.as_tensor(lens, dtype=torch.long).to(dev)
    left = longest - lens_d                                                                # clip c's columns start at left[c]
    src = torch.arange(2 * Lt, device=dev)[None] - left[:, None]
    table = torch.where((src >= 0) & (src < Lt), tokens.gather(1, src.clamp(0, Lt - 1)), torch.full_like(src, stop_token))
    prompts = torch.where(torch.arange(longest, device=dev)[None] < lens_d[:, None], tokens[:, :longest],
                          torch.full_like(tokens[:, :longest], stop_token))
    ends = {}
    for c, pl in enumerate(lens):
        if pl != shortest:
            ends.setdefault(final_len - pl, []).extend(range(c * G, (c + 1) * G))
    ends = {k: torch.as_tensor(v, dtype=torch.long).to(dev) for k, v in ends.items()}
    return table, prompts, ends, torch.zeros(B * G, dtype=torch.int32, device=dev), 2


def _strip_left_padding(h, lens, flush, len_scale):
    """The finish of the search over _left_padded_table, on the downloaded BeamState arrays `h` (in place): every clip as a search over
    clips of its own length leaves it.  The rows lose their left padding and are Lt wide again (behind the generated tokens they hold
    the rest of the clip's input row, then the stop token); the hypothesis scores and the worst score, stored over the 2 * Lt wide
    table, are multiplied by len_scale (exact); and a pseudo-clip whose budget ended before it was done (flush) counts as not done, so
    that the host flushes its beams as it does for a clip the loop's end leaves unfinished."""
    K, Lt = h.tokens.size(1), h.tokens.size(2) // len_scale
    groups = h.tokens.size(0) // len(lens)
    cols = (torch.arange(Lt)[None] + (max(lens) - torch.as_tensor(lens))[:, None]).repeat_interleave(groups, 0)
    h.tokens = h.tokens.gather(2, cols[:, None, :].expand(-1, K, -1))
    h.hyp_tokens = h.hyp_tokens.gather(2, cols[:, None, :].expand(-1, K, -1))
    h.hyp_score, h.worst, h.done = h.hyp_score * len_scale, h.worst * len_scale, h.done * (1 - flush.cpu())


def _mixed_prompt_lengths(prompt_length, B, L, needed_by=None):
    """A loop's prompt_length: None or an int -> None (one prompt length; refused for the caller `needed_by`); a sequence or tensor of
    B lengths -> them as a list of ints in [1, L]"""
    lens = _int_list(prompt_length)
    if lens is None and needed_by:
        raise ValueError(f"{needed_by} needs prompt_length = {B} lengths, one per clip (got {prompt_length!r})")
    if lens is not None and (len(lens) != B or min(lens) < 1 or max(lens) > L):
        raise ValueError(f"prompt_length must be an int or {B} lengths in [1, {L}] (got {lens})")
    return lens


def _mixed_prompt_state(cfg, make_state, rows, Q, lens, final_len, who):
    """The decode state of a lockstep loop over clips whose prompts hold `lens` tokens -> (state, the positions it holds).  Every
    sequence steps until the shortest prompt's budget ends, the longer ones as padding rows by then, so Q + P_max + final_len - P_min -
    2 must be a row of the position table, and the state must take the prompt lengths: both are checked before the first launch."""
    longest, shortest = max(lens), min(lens)
    total_final = Q + longest + final_len - shortest
    if total_final - 2 >= cfg.max_position_embeddings:        # the last step's position of the longest prefix (frozen by then, but fed)
        raise ValueError(f"prompts of {shortest} .. {longest} tokens behind {Q} query slots step up to position {total_final - 2}; "
                         f"the position table has {cfg.max_position_embeddings} rows")
    state = make_state(rows, total_final)
    if not _takes_prompt_len(state):
        raise ValueError(f'{who} a state with prefill_fan_out(..., prompt_len=): kv="shared_prefix" (got a {type(state).__name__})')
    return state, total_final


def _takes_prompt_len(state) -> bool:
    import inspect
    fn = getattr(state, "prefill_fan_out", None)
    return fn is not None and "prompt_len" in inspect.signature(fn).parameters


def _ranked_hypotheses(h, b, K):
    """the host finish of the lockstep searches for pseudo-clip b of the downloaded BeamState arrays `h`: its stored hypotheses in
    insertion order, the final flush of its K beams unless it is done, and the stable ranking -- as beam_search_loop ends"""
    hyp = BeamHypotheses(K)
    for s in sorted(range(int(h.hyp_count[b])), key=lambda s: int(h.hyp_order[b, s])):      # insertion order
        hyp.beams.append((float(h.hyp_score[b, s]), h.hyp_tokens[b, s].clone(), None))
    hyp.worst_score = float(h.worst[b])
    if not bool(h.done[b]):
        for k in range(K):
            hyp.add(h.tokens[b, k].clone(), float(h.scores[b, k]))
    return sorted(hyp.beams, key=lambda x: x[0], reverse=True)


BAN_SAMPLING = float("-inf")                 # mpv_sample_advance: probability 0, never in the kept set
BAN_BEAM = -float.fromhex("0x1.fep127")      # the lowest finite bf16: mpv_logprob_topk would take exp(-inf + inf) on a slice of -inf only


class PhraseTrie:
    """A closed vocabulary of multi-token phrases as a trie, for LogitsConstraints(allowed_phrases=): the lockstep and in-flight loops
    then produce only members of the set, each followed by the termination id (include/mpv.h: mpv_logits_trie_mask; DESIGN.md section
    28).  phrases: non-empty sequences of token ids in [0, vocab) (lists or 1-D tensors), at most 255 tokens each.  Shared prefixes are
    merged; a phrase given twice is one terminal node that keeps the LOWEST phrase index.  The trie is flattened to four int32 arrays in
    CSR form, node 0 the root: child_begin [n_nodes + 1], child_tok [n_edges] (strictly ascending inside each node's run),
    child_node [n_edges], terminal [n_nodes] (the phrase index, or -1 where no phrase ends).
    .max_len: the longest phrase; .n_phrases: len(phrases), duplicates included; .lookup(seq) -> the phrase index of exactly `seq`, or
    -1 (on the host, exact); .arrays(device) -> the four arrays on `device`, built once per device.  Whether a phrase holds a
    termination id is checked by the loops, which know the ids (.contains(token))."""
    MAX_PHRASE_LEN, MAX_EDGES = 255, 2 ** 31 - 1

    def __init__(self, phrases, vocab: int):
        vocab = int(vocab)
        phrases = list(phrases)
        if not phrases:
            raise ValueError("PhraseTrie needs at least one phrase")
        children, terminal, n_edges, self.max_len = [{}], [-1], 0, 0
        for idx, ph in enumerate(phrases):
            seq = [int(t) for t in (ph.tolist() if torch.is_tensor(ph) else ph)]
            if not seq:
                raise ValueError(f"phrase {idx} is empty")
            if len(seq) > self.MAX_PHRASE_LEN:
                raise ValueError(f"phrase {idx} has {len(seq)} tokens; at most {self.MAX_PHRASE_LEN}")
            u = 0
            for t in seq:
                if not 0 <= t < vocab:
                    raise ValueError(f"phrase {idx}: token {t} is outside [0, {vocab})")
                v = children[u].get(t)
                if v is None:
                    n_edges += 1
                    if n_edges > self.MAX_EDGES:
                        raise ValueError(f"the trie has more than {self.MAX_EDGES} edges")
                    v = children[u][t] = len(children)
                    children.append({})
                    terminal.append(-1)
                u = v
            if terminal[u] < 0:
                terminal[u] = idx
            self.max_len = max(self.max_len, len(seq))
        self.vocab, self.n_phrases, self.n_nodes, self.n_edges = vocab, len(phrases), len(children), n_edges
        self.child_begin, self.child_tok, self.child_node, self.terminal = [0], [], [], terminal
        for kids in children:
            for t in sorted(kids):
                self.child_tok.append(t)
                self.child_node.append(kids[t])
            self.child_begin.append(len(self.child_tok))
        self._tokens = frozenset(self.child_tok)
        self._device = {}

    def contains(self, token: int) -> bool:
        """does any phrase hold `token`?"""
        return int(token) in self._tokens

    def lookup(self, seq) -> int:
        """-> the index of the phrase that is exactly `seq` (the lowest, if it was given more than once), or -1"""
        import bisect
        u = 0
        for t in (seq.tolist() if torch.is_tensor(seq) else seq):
            b, e = self.child_begin[u], self.child_begin[u + 1]
            j = bisect.bisect_left(self.child_tok, int(t), b, e)
            if j == e or self.child_tok[j] != int(t):
                return -1
            u = self.child_node[j]
        return self.terminal[u] if u else -1

    def arrays(self, device):
        """-> (child_begin, child_tok, child_node, terminal) as int32 tensors on `device`, made once per device"""
        key = str(torch.device(device))
        hit = self._device.get(key)
        if hit is None:
            hit = self._device[key] = tuple(torch.tensor(a, dtype=torch.int32).to(device)
                                            for a in (self.child_begin, self.child_tok, self.child_node, self.terminal))
        return hit


def as_phrase_trie(phrases, vocab: int, encode=None) -> "PhraseTrie":
    """a PhraseTrie as it is; a list of token lists (or tensors); or a list of strings, each tokenised by `encode` (str -> ids)"""
    if isinstance(phrases, PhraseTrie):
        return phrases
    phrases = list(phrases)
    if any(isinstance(p, str) for p in phrases):
        if encode is None:
            raise ValueError("allowed_phrases given as strings need a tokenizer")
        phrases = [list(encode(p)) if isinstance(p, str) else p for p in phrases]
    return PhraseTrie(phrases, vocab)


def generated_part(row, prompt_len: int, termination_id: int) -> list:
    """a result row (a list or 1-D tensor: prompt, generated tokens, padding) -> the tokens between the prompt and the first
    termination id behind it"""
    gen = (row.tolist() if torch.is_tensor(row) else list(row))[int(prompt_len):]
    return gen[:gen.index(int(termination_id))] if int(termination_id) in gen else gen


@dataclasses.dataclass
class LogitsConstraints:
    """What the lockstep loops may forbid or discourage (include/mpv.h: mpv_logits_constrain; ops.logits_constrain applies it to one
    step's logits on the device): the CTRL repetition penalty (1.0 = off), the no-repeat n-gram size (0 = off, at most 8),
    min_new_tokens (the termination tokens stay banned until that many tokens are generated), banned_token_ids (at most 1024 single
    tokens) and include_prompt (the penalty and the n-grams also see the prompt; default: the generated tokens only).
    The constraints act on the RAW logits -- before temperature, the top-k / top-p filter and log_softmax -- in sampling and in beam
    search alike.  (Hugging Face's beam search applies its processors to the log-probabilities instead, so a penalised beam score
    differs from theirs; for sampling the two orders agree with their processors run before their warpers.)
    allowed_phrases (a PhraseTrie; default None): what the loops REQUIRE -- every sequence is a phrase of the trie followed by the
    termination id.  After the edits above (a ban still wins) every step keeps only the tokens that continue the row's generated
    tokens along the trie (ops.logits_trie_mask*, include/mpv.h: mpv_logits_trie_mask).  The scores of such a call -- beam scores and
    sample log-probabilities alike -- are RENORMALISED ones: log_softmax runs over the allowed tokens only."""
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_new_tokens: int = 0
    banned_token_ids: tuple = ()
    include_prompt: bool = False
    allowed_phrases: Optional[PhraseTrie] = None

    def __post_init__(self):
        p = self.repetition_penalty
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not math.isfinite(p) or p <= 0:
            raise ValueError(f"repetition_penalty must be a finite number above 0 (got {p!r})")
        for name, hi in (("no_repeat_ngram_size", 8), ("min_new_tokens", None)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 0 or (hi is not None and v > hi):
                raise ValueError(f"{name} must be an integer in [0, {hi}] (got {v!r})" if hi else f"{name} must be a non-negative integer (got {v!r})")
        ids = tuple(self.banned_token_ids)
        for t in ids:
            if isinstance(t, bool) or not isinstance(t, int):
                raise ValueError(f"banned_token_ids must be integers (got {t!r})")
        if len(ids) > 1024:
            raise ValueError(f"at most 1024 banned_token_ids (got {len(ids)})")
        if self.allowed_phrases is not None and not isinstance(self.allowed_phrases, PhraseTrie):
            raise ValueError(f"allowed_phrases must be a PhraseTrie or None (got a {type(self.allowed_phrases).__name__})")
        self.repetition_penalty, self.banned_token_ids, self.include_prompt = float(p), ids, bool(self.include_prompt)
        self._device_ids = {}                    # ops.logits_constrain: the device copies of the id lists, made once

    @property
    def edits(self) -> bool:
        """is any of the edits of ops.logits_constrain on?"""
        return self.repetition_penalty != 1.0 or self.no_repeat_ngram_size > 0 or self.min_new_tokens > 0 or len(self.banned_token_ids) > 0

    @property
    def active(self) -> bool:
        return self.edits or self.allowed_phrases is not None


def _active_constraints(constraints, constrain_fn):
    """-> the constraints if constrain_fn has something to do (the edits; the trie is _active_trie's), else None"""
    if constraints is None or not constraints.edits:
        return None
    if constrain_fn is None:
        raise ValueError("active constraints need a constrain_fn (ops.logits_constrain)")
    return constraints


def _active_trie(constraints, trie_fn, eos_ids, eol_stop=False):
    """-> constraints.allowed_phrases, or None; with a trie, everything that cannot work is raised here, before the first launch"""
    trie = None if constraints is None else constraints.allowed_phrases
    if trie is None:
        return None
    if trie_fn is None:
        raise ValueError("allowed_phrases need a trie_fn (ops.logits_trie_mask)")
    if constraints.min_new_tokens > 0:
        raise ValueError(f"min_new_tokens ({constraints.min_new_tokens}) cannot be combined with allowed_phrases: a phrase ends with the "
                         "termination id that the minimum length bans")
    if eol_stop:
        raise ValueError("allowed_phrases cannot be combined with stop_on_eol / stop_on_double_eol: a phrase ends with one termination id")
    for t in eos_ids:
        if trie.contains(t):
            raise ValueError(f"an allowed phrase contains the termination id {int(t)}")
    return trie


# ---------------------------------------------------------------------------------------------- guided decoding
@dataclasses.dataclass
class Guidance:
    """Classifier-free guidance (contrastive decoding) for the lockstep loops (include/mpv.h: mpv_logits_guide):
    a second branch decodes the same prompts behind `query_embeds`, the query features of a "null" video, in lockstep, and every
    step continues from cond + (scale - 1) * (cond - uncond) on the max-centred logits of the two branches.  scale >= 0 (1: the
    conditional branch alone; above 1: away from what the language prior says without the clip); alpha in [0, 1): a token whose
    conditional probability is below alpha times the step's largest is banned (0: off) -- sampling only.  query_embeds: [Q, H] (one
    null clip for every clip of a call), [B * Q, H] or [B, Q, H].  scale == 1 with alpha == 0 is NO guidance: `active` is False, no
    second branch runs and no launch is added.
    The scores of a guided call -- SampleScores and beam scores alike -- are log-probabilities of the GUIDED distribution,
    renormalised over the vocabulary (over the tokens the plausibility ban left), not the model's likelihoods: as with
    LogitsConstraints(allowed_phrases=), log_softmax runs on the logits the step continued from."""
    scale: float = 1.0
    alpha: float = 0.0
    query_embeds: Optional[torch.Tensor] = None

    def __post_init__(self):
        for name, ok, rule in (("scale", lambda v: v >= 0.0, "a finite number that is not negative"), ("alpha", lambda v: 0.0 <= v < 1.0, "in [0, 1)")):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not ok(v):
                raise ValueError(f"guidance {name} must be {rule} (got {v!r})")
            setattr(self, name, float(v))
        if self.query_embeds is not None and not isinstance(self.query_embeds, torch.Tensor):
            raise ValueError(f"guidance query_embeds must be a tensor or None (got a {type(self.query_embeds).__name__})")

    @property
    def active(self) -> bool:
        return self.scale != 1.0 or self.alpha != 0.0

    def null_rows(self, query_embeds) -> torch.Tensor:
        """the null branch's query features for a call with query_embeds [B, Q, H] -> [B, Q, H] (a broadcast view), on its device and in
        its dtype; a missing tensor or a shape that is none of [Q, H], [B * Q, H], [B, Q, H] is refused"""
        if query_embeds is None or query_embeds.dim() != 3:
            raise ValueError("guidance needs the clips' query_embeds [B, Q, H]: the null branch replaces them")
        B, Q, H = query_embeds.shape
        n = self.query_embeds
        if n is None:
            raise ValueError(f"guidance needs query_embeds, the null video's query features [{Q}, {H}] or [{B * Q}, {H}]")
        if tuple(n.shape) not in ((Q, H), (B * Q, H), (B, Q, H), (1, Q, H)):
            raise ValueError(f"guidance query_embeds must be [{Q}, {H}], [{B * Q}, {H}] or [{B}, {Q}, {H}] (got {tuple(n.shape)})")
        return n.to(device=query_embeds.device, dtype=query_embeds.dtype).reshape(-1, Q, H).expand(B, Q, H)


class GuidedState:
    """A decode state of R sequences under guidance, for the loops as they are: `inner` is a state of 2R sequences -- rows [0, R) the
    clips, rows [R, 2R) the same prompts behind the null query features -- and every call is forwarded doubled: prefill_fan_out with
    both tensors (and a prompt_len list) doubled, step with the tokens doubled, reorder with cat([idx, idx + R]), so that the null
    branch follows the beams.  After each prefill or step guide_fn(logits[:R], logits[R:], scale=, alpha=, ban_value=) runs once
    (ops.logits_guide: one launch) and the view logits[:R] is returned: every editor, sampler, top-k and scorer works on guided logits
    unchanged.  Anything else (pos, kv_bytes, ...) is the inner state's."""

    def __init__(self, inner, rows: int, guidance: Guidance, guide_fn, ban_value: float):
        self.inner, self.rows, self.guidance, self.guide_fn, self.ban_value = inner, int(rows), guidance, guide_fn, float(ban_value)

    def __getattr__(self, name):                     # (only what the wrapper itself does not have)
        return getattr(self.__dict__["inner"], name)

    def _guided(self, logits):
        R = self.rows
        self.guide_fn(logits[:R], logits[R:], scale=self.guidance.scale, alpha=self.guidance.alpha, ban_value=self.ban_value)
        return logits[:R]

    def _prefill(self, tokens, query_embeds, fan, **kw):
        null = self.guidance.null_rows(query_embeds)
        if kw.get("prompt_len") is not None:
            kw["prompt_len"] = 2 * _int_list(kw["prompt_len"])
        return self._guided(self.inner.prefill_fan_out(torch.cat([tokens, tokens], 0), torch.cat([query_embeds, null], 0), fan, **kw))

    def prefill_fan_out(self, tokens, query_embeds, fan):
        return self._prefill(tokens, query_embeds, fan)

    def step(self, tokens):
        return self._guided(self.inner.step(torch.cat([tokens, tokens], 0)))

    def reorder(self, batch_idx, **kw):
        return self.inner.reorder(torch.cat([batch_idx, batch_idx + self.rows], 0), **kw)


class GuidedRaggedState(GuidedState):
    """GuidedState over an inner state whose prefill takes a prompt length per clip: prefill_fan_out has prompt_len= exactly when the
    inner state's has (_takes_prompt_len reads the signature)"""

    def prefill_fan_out(self, tokens, query_embeds, fan, prompt_len=None):
        return self._prefill(tokens, query_embeds, fan, **({} if prompt_len is None else dict(prompt_len=prompt_len)))


def guided_state_fn(make_state, guidance: Optional[Guidance], guide_fn, ban_value: float):
    """The make_state of a lockstep loop under `guidance`: (batch, max_len) -> a GuidedState around make_state(2 * batch, max_len).
    guide_fn is ops.logits_guide (injectable, as the loops' *_fn are); ban_value is BAN_SAMPLING in front of the sampler and BAN_BEAM
    in front of logprob_topk.  No guidance (None, or scale 1 with alpha 0): make_state itself is returned -- no second branch, no
    launch, the call sequence of the unguided loop."""
    if guidance is None or not guidance.active:
        return make_state
    if guide_fn is None:
        raise ValueError("guidance needs a guide_fn (ops.logits_guide)")

    def make(batch, max_len):
        inner = make_state(2 * int(batch), max_len)
        return (GuidedRaggedState if _takes_prompt_len(inner) else GuidedState)(inner, batch, guidance, guide_fn, ban_value)
    return make


def _guided_make_state(make_state, guidance, query_embeds, rows, weights, ban_value, who, beams=False):
    """what sample_batched / beam_search_batched make of guidance=: every refusal before the first launch, then guided_state_fn"""
    if guidance is None:
        return make_state
    if not isinstance(guidance, Guidance):
        raise ValueError(f"{who}: guidance must be a generation.Guidance or None (got a {type(guidance).__name__})")
    if not guidance.active:
        return make_state
    if beams and guidance.alpha > 0.0:
        raise ValueError(f"{who}: guidance alpha ({guidance.alpha}) needs a sampler: a banned token can enter the 2K candidates of a beam "
                         "step, and no exact host filter exists for it")
    guidance.null_rows(query_embeds)                                                       # the shape check
    if weights == "fp8" and 2 * int(rows) > _lib.W8_TILED_MAX_ROWS:
        raise ValueError(f'{who}: guidance doubles the {int(rows)} rows of the step, and decode_weights="fp8" takes at most '
                         f"{_lib.W8_TILED_MAX_ROWS}: the steps would run on the bf16 weights")
    return guided_state_fn(make_state, guidance, ops.logits_guide, ban_value)


def _no_inflight_guidance(guidance, who):
    if guidance is not None and (not isinstance(guidance, Guidance) or guidance.active):
        raise ValueError(f"{who} takes no guidance: the in-flight states hold one branch per slot (guided calls: sample_batched / "
                         "beam_search_batched)")


def _stop_behind_prompts(tokens, prompt_lens, stop_token):
    """tokens [B, L] -> a copy with the stop token in every column at and behind the clip's prompt length: a beam hypothesis is stored
    as its whole row, so with this its generated part is what generated_part() reads, whatever padding the caller's rows carried"""
    lens = torch.as_tensor(prompt_lens, dtype=torch.long).to(tokens.device).reshape(-1, 1)
    return torch.where(torch.arange(tokens.size(1), device=tokens.device)[None] < lens, tokens, torch.full_like(tokens, stop_token))


def sample_loop(cfg, make_state, tokens: torch.Tensor, query_embeds=None, temperature=1.0, use_eod_token_for_early_termination=True,
                stop_on_double_eol=False, stop_on_eol=False, termination_id=None, prompt_length=None, generator=None, return_scores=False):
    """models/modeling_distributed_gpt3.py:1620-1735.  return_scores=True is refused: the scores are sample_batched_loop's."""
    _no_sample_scores(return_scores, "sample_loop")
    B, dev = tokens.size(0), tokens.device
    lengths = prompt_length if prompt_length is not None else torch.tensor([tokens.size(1)], device=dev)
    lengths = torch.as_tensor(lengths, device=dev).view(-1)
    min_prompt = int(lengths.min().item())
    tokens, max_len, Q = _pad_for_generation(cfg, tokens, cfg.eod_id, min_prompt, query_embeds)
    state = make_state(B, max_len + Q)
    termination_id = cfg.eod_id if termination_id is None else int(termination_id)
    is_done = torch.zeros(B, dtype=torch.bool, device=dev)
    prev, total_min, total_max = 0, min_prompt + Q, max_len + Q
    context_length = total_min
    for context_length in range(total_min, total_max):
        t2u = tokens[:, max(prev - Q, 0):context_length - Q]
        logits = state.step(t2u, query_embeds if context_length == total_min else None)
        new = sample_token(logits, top_k=cfg.top_k, top_p=cfg.top_p, temperature=temperature, vocab_size=cfg.vocab_size,
                           generator=generator)
        started = lengths <= context_length - Q
        tokens[started, context_length - Q] = new[started]
        prev = context_length
        if stop_on_double_eol:
            done_token = ((new == 628) | ((new == 198) & (tokens[:, context_length - Q - 1] == 198))) & started
        elif stop_on_eol:
            done_token = ((new == 628) | (new == 198)) & started
        else:
            done_token = (new == termination_id) & started
        is_done |= done_token
        if use_eod_token_for_early_termination and bool(is_done.all()):
            break
    return tokens[:, :context_length + 1]      # (sic) the reference slices with the prefix-inclusive length (:1733)


class SampleState:
    """The state of sample_batched_loop for `rows` sequences, as device tensors (struct of arrays; the contract of include/mpv.h:
    mpv_sample_advance): the token table, the prompt lengths, the done flags, the tokens the next decode step consumes, the stream
    number that keys every row's uniforms, and the count of done rows (the loop's one host read per step)."""

    def __init__(self, tokens: torch.Tensor, prompt_len: torch.Tensor, streams: Optional[torch.Tensor] = None):
        R, Lt = tokens.shape
        dev = tokens.device
        self.rows, self.row_len = R, Lt
        self.tokens = tokens.to(torch.int64).contiguous().clone()
        self.prompt_len = prompt_len.to(device=dev, dtype=torch.int64).reshape(-1).expand(R).contiguous().clone()
        self.done = torch.zeros(R, dtype=torch.int32, device=dev)
        self.next_tok = torch.zeros(R, dtype=torch.int64, device=dev)
        self.stream = (torch.arange(R, dtype=torch.int64, device=dev) if streams is None
                       else torch.as_tensor(streams, device=dev).to(torch.int64).reshape(-1).contiguous().clone())
        assert self.stream.numel() == R, (self.stream.numel(), R)
        self.n_done = torch.zeros(1, dtype=torch.int32, device=dev)

    ARRAYS = ("tokens", "prompt_len", "done", "next_tok", "stream", "n_done")


class SampleScores:
    """The sequence scores of sample_batched_loop for `rows` sequences, as device tensors (struct of arrays; the contract of
    include/mpv.h: mpv_sample_score): live (1 until the row's terminating token has been scored), token_logprob (the model's
    log-probability of every generated token up to and including the terminating one; 0 at prompt positions and behind the
    termination), sum_logprob (their sum, added in position order) and count (their number)."""

    def __init__(self, rows: int, row_len: int, device):
        self.rows, self.row_len = int(rows), int(row_len)
        self.live = torch.ones(self.rows, dtype=torch.int32, device=device)
        self.token_logprob = torch.zeros((self.rows, self.row_len), dtype=torch.float32, device=device)
        self.sum_logprob = torch.zeros(self.rows, dtype=torch.float32, device=device)
        self.count = torch.zeros(self.rows, dtype=torch.int32, device=device)

    ARRAYS = ("live", "token_logprob", "sum_logprob", "count")


def sample_batched_loop(cfg, make_state, tokens: torch.Tensor, query_embeds=None, temperature=1.0, use_eod_token_for_early_termination=True,
                        stop_on_double_eol=False, stop_on_eol=False, termination_id=None, prompt_length=None, num_samples=1, seed=0,
                        streams=None, advance_fn=None, constraints: Optional["LogitsConstraints"] = None, constrain_fn=None,
                        return_scores=False, score_fn=None, mixed_prompts=False, trie_fn=None, tokens_to_generate=None):
    """Sampled generation for B clips x num_samples sequences in lockstep, the whole of a step's sampling and bookkeeping in one
    launch: tokens [B, L], query_embeds [B, Q, H]; sequence j belongs to clip j // num_samples.  The prefill runs once per clip
    (state.prefill_fan_out) and fans out to the clip's samples; afterwards a step is state.step(st.next_tok) and _Sampler.step:
    constrain_fn, advance_fn (filter, draw, write, termination; include/mpv.h states the semantics), score_fn.  Samples never swap KV
    caches, so nothing is re-ordered, and the host reads four bytes per step (the count of done rows).  Row j draws from the stream
    streams[j] (default j) of `seed`: its tokens do not depend on the other rows of the call.  cfg.top_k / cfg.top_p choose the
    filter as in sample_loop.  make_state and the *_fn are injectable as in beam_search_batched_loop.
    `constraints` (a LogitsConstraints; None or inactive: no call and no launch is added): between the step and advance_fn every
    step, the prefill's included, edits the raw logits through constrain_fn on st.tokens / st.prompt_len; rows still inside their
    prompt are left alone.  The termination ids of min_new_tokens are [termination_id], or [628, 198] under stop_on_eol; a banned
    logit is -inf, the sampler's "never drawn".  min_new_tokens with stop_on_double_eol is refused (a pair of tokens ends the row
    there, which a per-token ban cannot express).
    `return_scores` (default False: no call, no launch and no allocation is added, and the return value is the tensor alone): right
    after advance_fn every step, the prefill's included, score_fn records the model's log-probability of the token just written,
    from the logits advance_fn read (the constrained ones) -- rows still inside their prompt and rows that terminated in an earlier
    step are not scored; the terminating token is.  -> (tokens, scores): a SampleScores whose token_logprob is cut to the columns of
    `tokens`.
    mixed_prompts=False: prompt_length [B] (ragged lengths are allowed) or None.  The prefill covers the shortest prompt P_min, and
    the entries are the uniform ones (ops.sample_advance, ops.logits_constrain, ops.sample_score), called with pos = P_min + t: all
    rows work on one column, and advance_fn teacher-forces the rows whose prompt reaches further.  -> tokens [B * num_samples, n]
    with sample_loop's (prefix-inclusive, sic) slice n = Q + P_min + t + 1.
    mixed_prompts=True with prompt_length = B lengths: ONE loop over clips whose prompts differ in length WITHOUT teacher forcing.
    The table stays LEFT-aligned (clip c's prompt at columns [0, prompt_length[c]), final_len wide): a draw is a function of (seed,
    column, stream), so a clip's samples must not move with its neighbours' prompts.  The prefill is the ragged one
    (state.prefill_fan_out(..., prompt_len=): SharedPrefixDecodeState; any other state is refused), and the entries are the RAGGED
    ones (ops.sample_advance_ragged, ops.logits_constrain_ragged, ops.sample_score_ragged), called with step = t: row r works on
    column prompt_length[r] + t.  The loop ends when every row is done or after final_len - P_min steps; a clip with a longer prompt
    runs out of columns earlier and is frozen by the kernels (done, counted in n_done), with no host bookkeeping; it keeps stepping as
    padding rows, which _mixed_prompt_state checks against the position table before the first launch.  -> tokens [B * num_samples,
    n], n covering every written column; a row holds its prompt, its generated tokens and, behind them, the rest of its input row.
    constraints.allowed_phrases (a PhraseTrie): between constrain_fn and advance_fn every step keeps only the tokens that continue a row
    along the trie, through trie_fn (the ops.logits_trie_mask* of the mode) with the same table, lengths, column, termination id and
    -inf: a banned token is never drawn, so every row is a phrase followed by the termination id (and then draws that id until the
    loop ends).  score_fn then records log-probabilities RENORMALISED over the allowed tokens.  Raised before the first launch: what
    _active_trie refuses (min_new_tokens, stop_on_eol / stop_on_double_eol, a phrase with the termination id).
    tokens_to_generate (default None: cfg.tokens_to_generate): the columns this call appends to the table."""
    B, dev, N = tokens.size(0), tokens.device, int(num_samples)
    if tokens_to_generate is not None:
        cfg = SimpleNamespace(**dict(vars(cfg), tokens_to_generate=int(tokens_to_generate)))
    sampler = _Sampler(cfg, dict(num_samples=num_samples), temperature, seed, termination_id, stop_on_double_eol, stop_on_eol, advance_fn,
                       constraints, constrain_fn, return_scores, score_fn, "sample_score", trie_fn)
    R = B * N
    if mixed_prompts:
        lens = _mixed_prompt_lengths(prompt_length, B, tokens.size(1), "mixed_prompts=True")
        prompt = max(lens)                                        # the prefill's columns: the longest prompt, right-padded
        tokens, final_len, Q = _pad_for_generation(cfg, tokens, cfg.eod_id, prompt, query_embeds)
        state, _ = _mixed_prompt_state(cfg, make_state, R, Q, lens, final_len, "mixed_prompts=True needs")
        table, lengths = tokens[:, :final_len], torch.as_tensor(lens, dtype=torch.long).to(dev)
        prefill_more, steps, where, first = dict(prompt_len=lens), final_len - min(lens), "step", 0
    else:
        lengths = prompt_length if prompt_length is not None else torch.tensor([tokens.size(1)], device=dev)
        lengths = torch.as_tensor(lengths, device=dev).view(-1).expand(B)
        prompt = int(lengths.min().item())                        # the prefill's columns: the shortest prompt
        tokens, max_len, Q = _pad_for_generation(cfg, tokens, cfg.eod_id, prompt, query_embeds)
        state = make_state(R, max_len + Q)
        table = tokens
        prefill_more, steps, where, first = {}, max_len - prompt, "pos", prompt
    st = SampleState(table.repeat_interleave(N, dim=0), lengths.repeat_interleave(N), streams=streams)
    sc = SampleScores(R, st.row_len, dev) if return_scores else None
    t = 0
    for t in range(steps):
        if t == 0:
            logits = state.prefill_fan_out(tokens[:, :prompt].contiguous(), query_embeds, N, **prefill_more)
        else:
            logits = state.step(st.next_tok.view(-1, 1))
        sampler.step(logits, st, sc, **{where: first + t})
        if use_eod_token_for_early_termination and int(st.n_done.item()) == R:       # the step's one host read: 4 bytes
            break
    n = min(Q + prompt + t + 1, st.row_len)          # (sic) sample_loop slices with the prefix-inclusive length; the table may end before it
    if sc is not None:
        sc.token_logprob = sc.token_logprob[:, :n]
        return st.tokens[:, :n], sc
    return st.tokens[:, :n]


class _Sampler:
    """What sample_batched_loop and sample_inflight_loop do alike, built once per call: the checks of their common arguments, the
    termination triple (termination_id, termination_mode, the eos ids of min_new_tokens) and the three calls of a step."""

    def __init__(self, cfg, at_least_one: dict, temperature, seed, termination_id, stop_on_double_eol, stop_on_eol, advance_fn, constraints,
                 constrain_fn, return_scores, score_fn, score_name: str, trie_fn=None):
        if any(int(v) < 1 for v in at_least_one.values()):
            raise ValueError(f"{' and '.join(at_least_one)} must be at least 1 (got {', '.join(str(v) for v in at_least_one.values())})")
        if return_scores and score_fn is None:
            raise ValueError(f"return_scores=True needs a score_fn (ops.{score_name})")
        self.constraints = _active_constraints(constraints, constrain_fn)
        if self.constraints is not None and self.constraints.min_new_tokens > 0 and stop_on_double_eol:
            raise ValueError(f"min_new_tokens ({self.constraints.min_new_tokens}) cannot be combined with stop_on_double_eol")
        self.termination_id = cfg.eod_id if termination_id is None else int(termination_id)
        self.mode = 2 if stop_on_double_eol else 1 if stop_on_eol else 0
        self.eos_ids = [628, 198] if self.mode else [self.termination_id]
        self.trie = _active_trie(constraints, trie_fn, self.eos_ids, eol_stop=self.mode != 0)
        self.advance_fn, self.constrain_fn, self.score_fn, self.trie_fn = advance_fn, constrain_fn, score_fn, trie_fn
        self.draw = dict(temperature=temperature, top_k=cfg.top_k, top_p=cfg.top_p, seed=seed, vocab_size=cfg.vocab_size,
                         termination_mode=self.mode, termination_id=self.termination_id)

    def step(self, logits, st: "SampleState", sc: Optional["SampleScores"], **where):
        """constrain (active constraints only), the trie mask (allowed_phrases only), advance, score (sc given) on one step's logits; `where` is the entries' own keyword for
        the column a row works on: pos= (one for all), step= (the row's prompt length + step) or row_step= (a step per row)"""
        if self.constraints is not None:
            self.constrain_fn(logits, st.tokens, constraints=self.constraints, prompt_len=st.prompt_len, eos_ids=self.eos_ids,
                              ban_value=BAN_SAMPLING, **where)
        if self.trie is not None:
            self.trie_fn(logits, st.tokens, trie=self.trie, prompt_len=st.prompt_len, eos_ids=self.eos_ids, ban_value=BAN_SAMPLING, **where)
        self.advance_fn(logits, st, **where, **self.draw)
        if sc is not None:
            self.score_fn(logits, st, sc, **where)


def refill_min_default(slots: int) -> int:
    """sample_inflight_loop: the free slots a refill waits for, a quarter of the slots -- a staged prefill costs more than a decode step,
    and at 32 slots a wait for 8 was the fastest of 1 / 4 / 8 / 16 on both row counts measured"""
    return max(1, int(slots) // 4)


class _Slots:
    """The refill bookkeeping of the in-flight loops (sample_inflight_loop, beam_inflight_loop), the host's mirror as Python ints: per
    slot the clip it holds (-1: free) and the generation step its next advance works on; the n clips pass through in input order."""

    def __init__(self, n: int, slots: int, refill_min, budgets):
        self.n, self.slots, self.budgets = int(n), int(slots), budgets
        self.refill_min = min(self.slots, refill_min_default(self.slots) if refill_min is None else int(refill_min))
        if self.refill_min < 1:
            raise ValueError(f"refill_min must be at least 1 (got {self.refill_min})")
        self.clip_of, self.step_of, self.next_clip = [-1] * self.slots, [-1] * self.slots, 0

    def busy(self) -> bool:
        return self.next_clip < self.n or any(c >= 0 for c in self.clip_of)

    def refill(self):
        """-> (the slots that take a new clip now, their clips): all free slots (as far as clips are left) once refill_min are free, or
        when nothing runs; both empty otherwise"""
        free = [s for s in range(self.slots) if self.clip_of[s] < 0]
        if not (self.next_clip < self.n and free and (len(free) >= self.refill_min or len(free) == self.slots)):
            return [], []
        fresh = free[:self.n - self.next_clip]
        clips = list(range(self.next_clip, self.next_clip + len(fresh)))
        self.next_clip += len(fresh)
        for s, c in zip(fresh, clips):
            self.clip_of[s], self.step_of[s] = c, 0
        return fresh, clips

    def running(self):
        """the slots a decode step serves: those whose clip has advanced at least once"""
        return [s for s in range(self.slots) if self.clip_of[s] >= 0 and self.step_of[s] >= 1]

    def group_t(self):
        """per slot the suffix position of the decode step: step - 1, negative (idle) for a fresh and for a free slot"""
        return [self.step_of[s] - 1 if self.clip_of[s] >= 0 else -1 for s in range(self.slots)]

    def steps(self):
        """per slot the generation step of the advance; -1 for a free slot"""
        return [self.step_of[s] if self.clip_of[s] >= 0 else -1 for s in range(self.slots)]

    def advanced(self):
        """after the advance: every occupied slot is one step further -> the occupied slots"""
        active = [s for s in range(self.slots) if self.clip_of[s] >= 0]
        for s in active:
            self.step_of[s] += 1
        return active

    def spent(self, s) -> bool:
        return self.step_of[s] >= self.budgets[self.clip_of[s]]

    def release(self, s):
        self.clip_of[s], self.step_of[s] = -1, -1


def _inflight_budgets(cfg, max_new_tokens, default, lens, final_len, Q):
    """max_new_tokens (None: `default`, one budget per clip; an int; or one budget per clip) -> the clips' budgets, capped by the
    columns each prompt leaves in the table; the last position a clip feeds must be a row of the position table"""
    n = len(lens)
    budgets = _int_list(max_new_tokens)
    if budgets is None:
        budgets = list(default) if max_new_tokens is None else [int(max_new_tokens)] * n
    if len(budgets) != n or min(budgets) < 1:
        raise ValueError(f"max_new_tokens must be None, a positive int or {n} positive budgets (got {max_new_tokens!r})")
    budgets = [min(b, final_len - pl) for b, pl in zip(budgets, lens)]                      # the table's columns behind the prompt
    for c, (b, pl) in enumerate(zip(budgets, lens)):
        if Q + pl + b - 2 >= cfg.max_position_embeddings:
            raise ValueError(f"clip {c}: a prompt of {pl} tokens behind {Q} query slots with a budget of {b} feeds position {Q + pl + b - 2}; "
                             f"the position table has {cfg.max_position_embeddings} rows")
    return budgets


def sample_inflight_loop(cfg, make_state, tokens: torch.Tensor, query_embeds=None, temperature=1.0, use_eod_token_for_early_termination=True,
                         stop_on_double_eol=False, stop_on_eol=False, termination_id=None, prompt_length=None, num_samples=1, slots=32,
                         max_new_tokens=None, refill_min=None, seed=0, streams=None, advance_fn=None,
                         constraints: Optional["LogitsConstraints"] = None, constrain_fn=None, return_scores=False, score_fn=None, trie_fn=None):
    """sample_batched_loop's mixed mode with the finished clips' rows REFILLED in flight (continuous batching): tokens [n, L],
    query_embeds [n, Q, H], prompt_length n lengths; `slots` clips x num_samples sequences stay resident and the n clips of the
    call pass through them in input order.  A lockstep chunk is held until its slowest sequence ends while a decode step costs the
    same whatever the number of live rows; here a clip LEAVES when all its samples are done or its own budget is reached, and its
    slot goes to the next clip.  The table is the mixed mode's (left-aligned, final_len wide) and a draw is a function of (seed,
    column, stream), so a clip's rows do not depend on when, where or beside whom it runs: they are, on every column both wrote, those
    of sample_batched_loop(mixed_prompts=True) on that clip alone with the same streams.
    make_state(slots, fan, prefix_rows, suffix_rows) -> an InflightDecodeState (make_inflight_state_fn).  advance_fn / constrain_fn /
    score_fn are the _steps entries (ops.sample_advance_steps, ops.logits_constrain_steps, ops.sample_score_steps), called with
    row_step= (int32 [slots * num_samples] on the device: every row's own generation step, -1 for the rows of a free slot).
    The argument checks, the termination rule, constraints and return_scores are sample_batched_loop's (_Sampler).
    One iteration: (0) if at least refill_min slots are free (default refill_min_default(slots): a quarter of them; at most `slots`),
    or nothing runs, the next clips are installed (state.install: ONE staged ragged prefill for all of them); (1) ONE decode step
    (state.step(st.next_tok, group_t, max_t)) for the slots already running -- a slot just installed is idle in it --, none if
    nothing runs; (2) the prefill logits overwrite the rows of the slots just installed; (3) the sampler's step: one constrain
    launch, one advance launch and one score launch, every row on its own step; (4) the host, which mirrors every slot's
    step as Python ints, reads n_done (4 bytes) and -- only when that count is not the one it expects -- the done vector; clips that
    are done (unless use_eod_token_for_early_termination is False) or have used their budget leave: their token and score rows are
    gathered on the device into the result, in input order.
    max_new_tokens: None (cfg.tokens_to_generate for every clip), an int, or n budgets; a clip's budget is capped by the columns its
    prompt leaves in the table, and the last position it feeds, Q + prompt_length[c] + budget - 2, must be a row of the position
    table (a ValueError before the first launch otherwise).  When the input runs out, free slots idle until the last clip ends.
    -> SimpleNamespace(tokens [n * num_samples, final_len] (a row: its prompt, its generated tokens, behind them the rest of its
    input row), written [n] (list: the columns of clip c that hold prompt or generated tokens), scores (a SampleScores over all rows,
    or None), steps / prefills (decode steps and prefill passes issued)).
    constraints.allowed_phrases (a PhraseTrie) with trie_fn (ops.logits_trie_mask_steps): as in sample_batched_loop, every row on its
    own step; the default budget is then min(tokens_to_generate, trie.max_len + 1), the longest phrase and its termination id."""
    n, dev, N, slots = tokens.size(0), tokens.device, int(num_samples), int(slots)
    if advance_fn is None:
        raise ValueError("sample_inflight_loop needs an advance_fn (ops.sample_advance_steps)")
    sampler = _Sampler(cfg, dict(num_samples=num_samples, slots=slots), temperature, seed, termination_id, stop_on_double_eol, stop_on_eol,
                       advance_fn, constraints, constrain_fn, return_scores, score_fn, "sample_score_steps", trie_fn)
    lens = _mixed_prompt_lengths(prompt_length, n, tokens.size(1), "sample_inflight_loop")
    sl = _Slots(n, slots, refill_min, None)
    longest = max(lens)
    table, final_len, Q = _pad_for_generation(cfg, tokens, cfg.eod_id, longest, query_embeds)
    table = table[:, :final_len]
    default = int(cfg.tokens_to_generate) if sampler.trie is None else min(int(cfg.tokens_to_generate), sampler.trie.max_len + 1)
    budgets = sl.budgets = _inflight_budgets(cfg, max_new_tokens, [default] * n, lens, final_len, Q)
    R = slots * N
    state = make_state(slots, N, Q + longest, max(max(budgets) - 1, 1))
    streams = (torch.arange(n * N, dtype=torch.int64, device=dev) if streams is None
               else torch.as_tensor(streams, device=dev).to(torch.int64).reshape(-1))
    if streams.numel() != n * N:
        raise ValueError(f"streams must hold {n * N} numbers, one per sample (got {streams.numel()})")
    st = SampleState(table[:1].expand(R, -1), torch.zeros(1, dtype=torch.long, device=dev))
    sc = SampleScores(R, st.row_len, dev) if return_scores else None
    out_tokens = table.repeat_interleave(N, dim=0).contiguous()
    out_sc = SampleScores(n * N, st.row_len, dev) if return_scores else None
    written = list(lens)
    lens_d = torch.as_tensor(lens, dtype=torch.long).to(dev)
    within = torch.arange(N, device=dev)
    rows_of = lambda ids: (torch.as_tensor(ids, dtype=torch.long).to(dev)[:, None] * N + within[None]).reshape(-1)   # the N rows of each slot / clip
    logits = None
    clip_of, step_of, known_done = sl.clip_of, sl.step_of, [0] * slots                # the host's mirror (_Slots), and the done rows per slot
    while sl.busy():
        fresh, clips = sl.refill()
        if fresh:                                                                          # (0) the refill
            sel = torch.as_tensor(clips, dtype=torch.long).to(dev)
            first = state.install(fresh, table[sel, :longest].contiguous(), None if query_embeds is None else query_embeds[sel].contiguous(),
                                  [lens[c] for c in clips])
            fresh_rows = rows_of(fresh)
            src = rows_of(sel)
            st.tokens[fresh_rows] = out_tokens[src]                                        # the slot's rows, reset for their new clip
            st.prompt_len[fresh_rows] = lens_d[sel].repeat_interleave(N)
            st.stream[fresh_rows] = streams[src]
            st.done[fresh_rows] = 0
            if sc is not None:
                sc.live[fresh_rows], sc.sum_logprob[fresh_rows], sc.count[fresh_rows], sc.token_logprob[fresh_rows] = 1, 0.0, 0, 0.0
            for s in fresh:
                known_done[s] = 0
        running = sl.running()
        if running:                                                                        # (1) one decode step; fresh and free slots idle
            group_t = torch.tensor(sl.group_t(), dtype=torch.int32).to(dev)
            logits = state.step(st.next_tok.view(-1, 1), group_t, max(step_of[s] - 1 for s in running))
        elif logits is None:
            logits = torch.zeros((R, first.shape[1]), dtype=torch.bfloat16, device=dev)     # the first iteration; frozen rows read none of it
        if fresh:                                                                          # (2) the prefill logits of the fresh slots
            logits[fresh_rows] = first.repeat_interleave(N, dim=0)
        row_step = torch.tensor(sl.steps(), dtype=torch.int32).repeat_interleave(N).to(dev)
        sampler.step(logits, st, sc, row_step=row_step)                                    # (3) every row on its own step
        active = sl.advanced()                                                             # (4) the bookkeeping
        if use_eod_token_for_early_termination:
            expected = sum(known_done[s] for s in active) + N * (slots - len(active))      # frozen rows count as done
            if int(st.n_done.item()) != expected:                                          # the step's host read: 4 bytes; the vector on a change
                done_h = st.done.view(slots, N).ne(0).sum(dim=1).tolist()
                for s in active:
                    known_done[s] = done_h[s]
        leaving = [s for s in active if known_done[s] == N or sl.spent(s)]
        if leaving:
            rows = rows_of(leaving)
            dst = rows_of([clip_of[s] for s in leaving])
            out_tokens[dst] = st.tokens[rows]
            if sc is not None:
                out_sc.live[dst], out_sc.sum_logprob[dst], out_sc.count[dst] = sc.live[rows], sc.sum_logprob[rows], sc.count[rows]
                out_sc.token_logprob[dst] = sc.token_logprob[rows]
            for s in leaving:
                written[clip_of[s]] = lens[clip_of[s]] + step_of[s]
                sl.release(s)
                known_done[s] = 0
    return SimpleNamespace(tokens=out_tokens, written=written, scores=out_sc, steps=state.steps, prefills=state.prefills)


BEAM_RESULT_ARRAYS = ("tokens", "scores", "hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "hyp_next", "worst", "done")


def beam_inflight_loop(cfg, make_state, tokens: torch.Tensor, query_embeds=None, beam_size=5, num_return_gen=1, stop_token=None,
                       prompt_length=None, slots=32, max_new_tokens=None, refill_min=None, topk_fn=None, advance_fn=None,
                       constraints: Optional["LogitsConstraints"] = None, constrain_fn=None, return_scores=False, beam_groups=1,
                       diversity_penalty=0.0, trie_fn=None):
    """beam_search_batched_loop with the finished clips' slots REFILLED in flight, as sample_inflight_loop does for samples: tokens
    [n, L], query_embeds [n, Q, H], prompt_length n lengths; `slots` clips x G * K sequences stay resident (K = beam_size beams per
    group, G = beam_groups) and the n clips of the call pass through them in input order.  A clip LEAVES when all its groups are done
    or its budget is reached; its slot goes to the next clip (the refill rule, refill_min and their default are sample_inflight_loop's:
    _Slots).
    The token table is LEFT-aligned and Lt = L + tokens_to_generate wide, row_len = Lt for every clip: the table of the one-length
    lockstep search.  A hypothesis scores value / row_len, so clip c's search is the one beam_search_batched_loop(prompt_length=
    prompt_length[c]) runs on it -- no left padding, no len_scale -- and LogitsConstraints(include_prompt=True), which the mixed
    lockstep search has to refuse, is allowed here.
    make_state(slots, fan, prefix_rows, suffix_rows) -> an InflightDecodeState (make_inflight_state_fn), fan = G * K.  advance_fn is
    the _steps advance (ops.beam_advance_steps: one entry for one group and for several), constrain_fn the _steps constraint
    (ops.logits_constrain_steps), topk_fn as in beam_search_batched_loop; the group arguments are checked as there.  The search state
    is a BeamState of slots * G pseudo-clips; a free slot has done = 1 on the device and step -1.
    One iteration: (0) the refill (state.install); the fresh slots' rows of the CURRENT token table are reset to their clips' input
    rows and their search state is cleared (scores 0, hyp_count 0, hyp_next 0, worst 1e9, done 0); (1) ONE decode step
    (state.step(bs.next_tok, group_t, max_t)) for the slots already running, fresh and free slots idle in it; (2) the prefill logits
    overwrite the fresh slots' rows; (3) constrain_fn(..., row_step=, prompt_len=) with the stop token as termination id and BAN_BEAM
    (only with active constraints), topk_fn(logits, m, bs.scores), advance_fn(..., clip_prompt_len=, clip_step=), then the read of
    bs.done, int32 [slots * G]: the step's one host read; (4) the host mirrors every slot's step as Python ints: a clip whose G groups
    are all done, or whose budget is reached, leaves -- its BeamState rows are gathered ON THE DEVICE into the result arrays, in input
    order and with `done` as it stood, then the slot's done is set to 1; (5) state.reorder(bs.src_row, group_rows, max_rows) with
    group_rows[g] = group_t[g] + 1 for a slot that took part in this iteration's decode step and 0 otherwise.
    After the loop the result arrays are downloaded ONCE and every (clip, group) is finished by _ranked_hypotheses; a clip that left
    on its budget is not done, so its beams are flushed there as at the end of the lockstep loop.
    max_new_tokens: None, an int, or n budgets.  None gives final_len - prompt_length[c], the LOCKSTEP SEARCH's budget (NOT
    sample_inflight_loop's default of tokens_to_generate); budgets are capped by the table and the last position a clip feeds, Q +
    prompt_length[c] + budget - 2, must be a row of the position table (a ValueError before the first launch otherwise).
    -> a SimpleNamespace(results: the list of n namespaces beam_search_batched_loop returns (sequences, scores, group for G > 1),
    advances [n]: the positions every clip was advanced by before it left, steps / prefills: decode steps and prefill passes issued).
    constraints.allowed_phrases (a PhraseTrie) with trie_fn (ops.logits_trie_mask_steps): as in beam_search_batched_loop, between
    constrain_fn and topk_fn, every clip on its own step; the host finish drops the hypotheses that are no phrase and the results carry
    phrase_index.  The default budget is then min(final_len - prompt_length[c], trie.max_len + 1)."""
    _no_sample_scores(return_scores, "beam_inflight_loop")
    n, dev, K, slots = tokens.size(0), tokens.device, int(beam_size), int(slots)
    if advance_fn is None or topk_fn is None:
        raise ValueError("beam_inflight_loop needs a topk_fn (ops.logprob_topk) and an advance_fn (ops.beam_advance_steps)")
    if slots < 1 or K < 1:
        raise ValueError(f"slots and beam_size must be at least 1 (got {slots}, {K})")
    G, lam, per_group = _beam_groups(beam_groups, diversity_penalty, num_return_gen, K)
    constraints_given, constraints = constraints, _active_constraints(constraints, constrain_fn)
    lens = _mixed_prompt_lengths(prompt_length, n, tokens.size(1), "beam_inflight_loop")
    sl = _Slots(n, slots, refill_min, None)
    stop_token = cfg.eod_id if stop_token is None else int(stop_token)
    trie = _active_trie(constraints_given, trie_fn, [stop_token])
    if trie is not None:
        tokens = _stop_behind_prompts(tokens, lens, stop_token)
    longest = max(lens)
    table, final_len, Q = _pad_for_generation(cfg, tokens, stop_token, longest, query_embeds)
    sl.budgets = _inflight_budgets(cfg, max_new_tokens, [final_len - pl if trie is None else min(final_len - pl, trie.max_len + 1) for pl in lens],
                                   lens, final_len, Q)
    if table.size(1) > 2048:
        raise ValueError(f"a token table of {table.size(1)} columns; the advance kernels take 2048")
    fan, m = G * K, 2 * K + (G - 1) * K
    state = make_state(slots, fan, Q + longest, max(max(sl.budgets) - 1, 1))
    bs = BeamState(table[:1].expand(slots * G, -1), K)
    bs.done.fill_(1)                                                                       # free slots: frozen by the advance
    out = {k: torch.zeros((n * G,) + tuple(getattr(bs, k).shape[1:]), dtype=getattr(bs, k).dtype, device=dev) for k in BEAM_RESULT_ARRAYS}
    row_prompt_len = torch.zeros(slots * fan, dtype=torch.int64, device=dev)               # constrain_fn's, per sequence
    clip_prompt_len = torch.zeros(slots, dtype=torch.int32, device=dev)                    # advance_fn's, per slot
    lens_d = torch.as_tensor(lens, dtype=torch.long).to(dev)
    within = torch.arange(G, device=dev)
    pseudo = lambda ids: (torch.as_tensor(ids, dtype=torch.long).to(dev)[:, None] * G + within[None]).reshape(-1)   # the G pseudo-clips of each
    logits, advances = None, [0] * n
    while sl.busy():
        fresh, clips = sl.refill()
        if fresh:                                                                          # (0) the refill
            sel = torch.as_tensor(clips, dtype=torch.long).to(dev)
            first = state.install(fresh, table[sel, :longest].contiguous(), None if query_embeds is None else query_embeds[sel].contiguous(),
                                  [lens[c] for c in clips])
            rows, fresh_d = pseudo(fresh), torch.as_tensor(fresh, dtype=torch.long).to(dev)
            bs.tokens[rows] = table[sel].repeat_interleave(G, dim=0)[:, None, :]
            bs.scores[rows], bs.hyp_count[rows], bs.hyp_next[rows], bs.worst[rows], bs.done[rows] = 0.0, 0, 0, 1e9, 0
            clip_prompt_len[fresh_d] = lens_d[sel].to(torch.int32)
            row_prompt_len.view(slots, fan)[fresh_d] = lens_d[sel][:, None]
        running = sl.running()
        where = torch.tensor([sl.group_t(), sl.steps()], dtype=torch.int32).to(dev)        # one upload: suffix positions, generation steps
        group_t, clip_step = where[0], where[1]
        if running:                                                                        # (1) one decode step; fresh and free slots idle
            max_t = max(sl.step_of[s] - 1 for s in running)
            logits = state.step(bs.next_tok.view(-1, 1), group_t, max_t)
        elif logits is None:
            logits = torch.zeros((slots * fan, first.shape[1]), dtype=torch.bfloat16, device=dev)   # the first iteration; frozen rows read none of it
        if fresh:                                                                          # (2) the prefill logits of the fresh slots
            logits.view(slots, fan, -1)[fresh_d] = first[:, None, :]
        if constraints is not None or trie is not None:                                    # (3) every clip on its own step
            row_step = clip_step.repeat_interleave(fan)
        if constraints is not None:
            constrain_fn(logits, bs.tokens.view(slots * fan, -1), row_step=row_step, constraints=constraints,
                         prompt_len=row_prompt_len, eos_ids=[stop_token], ban_value=BAN_BEAM)
        if trie is not None:
            trie_fn(logits, bs.tokens.view(slots * fan, -1), row_step=row_step, trie=trie, prompt_len=row_prompt_len, eos_ids=[stop_token],
                    ban_value=BAN_BEAM)
        vals, idxs = topk_fn(logits, m, bs.scores.view(-1))
        advance_fn(vals, idxs, bs, groups=G, diversity_penalty=lam, vocab=logits.size(-1), clip_prompt_len=clip_prompt_len, clip_step=clip_step,
                   stop_token=stop_token)
        done_h = bs.done.view(slots, G).tolist()                                           # the step's one host read
        leaving = [s for s in sl.advanced() if all(done_h[s]) or sl.spent(s)]              # (4) the bookkeeping
        if leaving:
            rows, dst = pseudo(leaving), pseudo([sl.clip_of[s] for s in leaving])
            for k in BEAM_RESULT_ARRAYS:
                out[k][dst] = getattr(bs, k)[rows]
            bs.done[rows] = 1
            for s in leaving:
                advances[sl.clip_of[s]] = sl.step_of[s]
                sl.release(s)
        if running and sl.busy():                                                          # (5) the suffix rows follow their beams
            state.reorder(bs.src_row, (group_t + 1).clamp_(min=0), max_t + 1)
    h = SimpleNamespace(**{k: v.cpu() for k, v in out.items()})                            # one download
    return SimpleNamespace(results=_beam_results(h, n, G, K, per_group, dev, trie, lens, stop_token), advances=advances, steps=state.steps, prefills=state.prefills)


def pad_after_termination(tokens: torch.Tensor, prompt_len, termination_id: int, width: int, fill: int) -> torch.Tensor:
    """tokens [R, n] (what sample_batched_loop returns) -> [R, width]: every row keeps its columns up to and including the first
    `termination_id` at or behind column `prompt_len`; what follows (tokens drawn while other rows were still running, and the
    columns the loop never reached) is `fill`.  prompt_len: an int, or R lengths (a sequence or tensor: one per row, the mixed loop)."""
    R, n = tokens.shape
    out = torch.full((R, width), int(fill), dtype=tokens.dtype, device=tokens.device)
    out[:, :min(n, width)] = tokens[:, :width]
    col = torch.arange(width, device=tokens.device)[None]
    prompt_len = int(prompt_len) if _is_scalar(prompt_len) else torch.as_tensor(prompt_len, dtype=torch.long).to(tokens.device).view(R, 1)
    hit = (out == int(termination_id)) & (col >= prompt_len)
    first = torch.where(hit.any(dim=1), hit.int().argmax(dim=1), torch.full((R,), width, device=tokens.device))
    out[col > first[:, None]] = int(fill)
    return out


CONSENSUS_METRICS = ("rouge_l", "ngram_f")
ROUGE_BETA = 1.2                                   # the caption entry point's rouge_l (pycocoevalcap's Rouge)


def consensus_utility(counts, len_h, len_r, metric: str) -> torch.Tensor:
    """The utility u[h, r] in fp64 of candidate h judged against candidate r, from the integer overlap counts of ops.caption_overlap
    (include/mpv.h: mpv_caption_overlap) on the CPU: counts int [nA, nB, 5] or [nA * nB, 5] ([LCS, m1, m2, m3, m4] per pair, row-major),
    len_h [nA] and len_r [nB] the candidates' lengths.  The units are TOKEN IDS -- the caption entry point's corpus metrics are over
    CJK characters: the two agree in definition, not in unit.
    metric="rouge_l": P = lcs / len_h, R = lcs / len_r, u = (1 + b^2) P R / (R + b^2 P) with b = 1.2 and 0 when lcs = 0 -- rouge_l of
    the caption entry point for one reference; asymmetric, h is the candidate being judged.
    metric="ngram_f": the mean over the orders n = 1 .. 4 with g_h + g_r > 0 of 2 m_n / (g_h + g_r), g_x = max(len_x - n + 1, 0).
    Both: two empty candidates score 1, exactly one empty candidate scores 0."""
    if metric not in CONSENSUS_METRICS:
        raise ValueError(f"metric must be one of {CONSENSUS_METRICS} (got {metric!r})")
    F64 = torch.float64
    lh = torch.as_tensor(len_h).to("cpu", F64).reshape(-1, 1)
    lr = torch.as_tensor(len_r).to("cpu", F64).reshape(1, -1)
    nA, nB = lh.shape[0], lr.shape[1]
    c = torch.as_tensor(counts).to("cpu", F64).reshape(nA, nB, 5)
    both_empty = (lh == 0) & (lr == 0)
    one = torch.ones((), dtype=F64)
    if metric == "rouge_l":
        lcs = c[..., 0]
        p, r = lcs / torch.where(lh > 0, lh, one), lcs / torch.where(lr > 0, lr, one)
        b2 = ROUGE_BETA ** 2
        den = r + b2 * p
        u = torch.where(lcs > 0, (1 + b2) * p * r / torch.where(den > 0, den, one), torch.zeros((), dtype=F64))
    else:
        total, orders = torch.zeros((nA, nB), dtype=F64), torch.zeros((nA, nB), dtype=F64)
        for n in range(1, 5):
            g = (lh - n + 1).clamp(min=0) + (lr - n + 1).clamp(min=0)
            total = total + torch.where(g > 0, 2 * c[..., n] / torch.where(g > 0, g, one), torch.zeros((), dtype=F64))
            orders = orders + (g > 0).to(F64)
        u = total / torch.where(orders > 0, orders, one)
    return torch.where(both_empty, one, u)


def consensus_choice(u, weights=None):
    """u [nA, nB] (consensus_utility) -> (U [nA] fp64, index): U[h] = sum_r w_r u[h, r] / sum_r w_r over ALL the columns, h's own
    included -- every row is reduced in the same order (r ascending), so identical candidates get bit-identical U --, and index =
    argmax U, a tie going to the lowest index (None without rows; U within CONSENSUS_TIE of each other are tied: consensus_order).
    weights None: uniform, the Monte-Carlo estimate of the expected utility for samples."""
    u = torch.as_tensor(u).to("cpu", torch.float64)
    nA, nB = u.shape
    w = torch.ones(nB, dtype=torch.float64) if weights is None else torch.as_tensor(weights).to("cpu", torch.float64).reshape(-1)
    if w.numel() != nB:
        raise ValueError(f"{w.numel()} weights for {nB} references")
    acc, tot = torch.zeros(nA, dtype=torch.float64), 0.0
    for r in range(nB):                                      # a fixed order, the same for every row
        acc = acc + w[r] * u[:, r]
        tot = tot + float(w[r])
    U = acc / tot if nB and tot != 0.0 else acc
    order = consensus_order(U)
    return U, (order[0] if order else None)


CONSENSUS_TIE = 1e-12


def consensus_order(U) -> list:
    """the indices of U (fp64, in [0, 1]) by U descending, ties in index order.  Two U within CONSENSUS_TIE of each other count as
    TIED: the utilities are ratios of small integers, so different candidates often have exactly equal expected utilities (samples of
    one length whose LCS sums agree), and their fp64 sums may differ in the last bits -- rounding must not decide between them.  The
    order is built by selection: the lowest index among the remaining ones within the tie width of their maximum comes next."""
    vals = torch.as_tensor(U).to(torch.float64).tolist()
    left, order = list(range(len(vals))), []
    while left:
        top = max(vals[h] for h in left)
        pick = next(h for h in left if vals[h] >= top - CONSENSUS_TIE)
        order.append(pick)
        left.remove(pick)
    return order


class CiderStats:
    """The corpus statistics of CIDEr over TOKEN IDS, for ops.caption_cider (include/mpv.h: mpv_caption_cider).
    reference_sets: one list of reference token lists per clip; vocab: ids lie in [0, vocab), vocab <= 65535.  Built on the host, once.
    For every n-gram of the orders 1 .. n the document frequency df is the number of CLIPS with at least one reference that holds it
    (once per clip, however often and in however many of its references); log_ref_len = log(number of clips).
    An n-gram's key is exact: (id + 1) in 16 bits per token, the first token lowest, in one uint64 -- the order is implied and 0 is the
    empty slot.  The table is open addressing with linear probing over `capacity` slots, a power of two of at least twice the entry
    count (capacity= forces another power of two above the entry count): keys uint64 [capacity], idf float64 [capacity] =
    log_ref_len - log(max(1, df)) in fp64; the slot of a key is the library's splitmix64 finaliser of it masked by capacity - 1, the same
    function the kernel probes with.  A key that is not in the table weighs log_ref_len.
    .arrays(device) -> (keys, idf, log_ref_len), uploaded once per device; .lookup(ngram) -> the n-gram's idf by the host probe;
    .df(ngram) -> its document frequency; save(path) / CiderStats.load(path): plain tensors through torch.save;
    CiderStats.from_token_table(tokens, start, begin, term, vocab): from the padded layout the kernel reads."""
    MAX_VOCAB, ORDERS = 65535, 4

    def __init__(self, reference_sets, vocab: int, n: int = 4, capacity: Optional[int] = None):
        vocab, n = int(vocab), int(n)
        if not 1 <= vocab <= self.MAX_VOCAB:
            raise ValueError(f"CiderStats: vocab = {vocab} does not fit 16-bit key fields (ids + 1 <= {self.MAX_VOCAB})")
        if n != self.ORDERS:
            raise ValueError(f"CiderStats: the kernel counts the orders 1 .. {self.ORDERS} (got n = {n})")
        df = {}
        clips = 0
        for refs in reference_sets:
            clips += 1
            seen = set()
            for ref in refs:
                ref = [int(t) for t in (ref.tolist() if torch.is_tensor(ref) else ref)]
                if any(t < 0 or t >= vocab for t in ref):
                    raise ValueError(f"CiderStats: a reference holds an id outside [0, {vocab})")
                for k in range(1, n + 1):
                    for i in range(len(ref) - k + 1):
                        seen.add(self.key(ref[i:i + k]))
            for key in seen:                                     # once per clip
                df[key] = df.get(key, 0) + 1
        if clips < 1:
            raise ValueError("CiderStats: no clips")
        self.vocab, self.n, self.clips = vocab, n, clips
        self.log_ref_len = math.log(float(clips))
        keys = sorted(df)
        self._finish(keys, [df[k] for k in keys], capacity)

    @staticmethod
    def key(ngram) -> int:
        """the packed key of an n-gram of 1 .. 4 ids"""
        ngram = [int(t) for t in ngram]
        if not 1 <= len(ngram) <= CiderStats.ORDERS or any(t < 0 or t >= CiderStats.MAX_VOCAB for t in ngram):
            raise ValueError(f"CiderStats: an n-gram is 1 .. {CiderStats.ORDERS} ids in [0, {CiderStats.MAX_VOCAB}) (got {ngram})")
        return sum((t + 1) << (16 * i) for i, t in enumerate(ngram))

    def _finish(self, keys, dfs, capacity):
        import numpy as np
        entries = len(keys)
        cap = 2
        while cap < 2 * entries:
            cap *= 2
        if capacity is not None:
            cap = int(capacity)
            if cap < 2 or cap & (cap - 1) or cap <= entries:
                raise ValueError(f"CiderStats: capacity = {cap} must be a power of two above the {entries} entries")
        self.entries, self.capacity = entries, cap
        self.entry_keys = torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64))      # the bit patterns, ascending as unsigned
        self.entry_df = torch.tensor(dfs, dtype=torch.int64)
        idf = self.log_ref_len - torch.log(self.entry_df.clamp(min=1).to(torch.float64))
        tk, ti = torch.zeros(cap, dtype=torch.int64), torch.zeros(cap, dtype=torch.float64)
        _lib.check(_lib.lib().mpv_cider_table_fill(self.entry_keys.data_ptr(), idf.data_ptr(), entries, tk.data_ptr(), ti.data_ptr(), cap),
                   "mpv_cider_table_fill")
        self.keys, self.idf = tk.view(torch.uint64), ti
        self._device = {}

    def slot(self, ngram) -> int:
        """the table slot that holds the n-gram, -1 when the corpus does not"""
        return int(_lib.lib().mpv_cider_table_lookup(self.keys.data_ptr(), self.capacity, self.key(ngram)))

    def lookup(self, ngram) -> float:
        """idf of the n-gram by the host probe: log_ref_len for an n-gram the corpus does not hold"""
        s = self.slot(ngram)
        return self.log_ref_len if s < 0 else float(self.idf[s])

    def df(self, ngram) -> int:
        i = int(torch.searchsorted(self._unsigned_order(), self.key(ngram) - (1 << 63)))
        ok = i < self.entries and int(self._unsigned_order()[i]) == self.key(ngram) - (1 << 63)
        return int(self.entry_df[i]) if ok else 0

    def _unsigned_order(self):
        return self.entry_keys ^ torch.iinfo(torch.int64).min     # int64 that sorts as the uint64 keys do

    def arrays(self, device):
        """-> (keys uint64 [capacity], idf float64 [capacity], log_ref_len) with the tensors on `device`, uploaded once per device"""
        key = str(torch.device(device))
        hit = self._device.get(key)
        if hit is None:
            hit = self._device[key] = (self.keys.to(device), self.idf.to(device), self.log_ref_len)
        return hit

    def save(self, path):
        torch.save(dict(entry_keys=self.entry_keys, entry_df=self.entry_df, clips=torch.tensor(self.clips), vocab=torch.tensor(self.vocab),
                        n=torch.tensor(self.n), capacity=torch.tensor(self.capacity)), path)

    @classmethod
    def load(cls, path) -> "CiderStats":
        sd = torch.load(path, map_location="cpu")
        self = cls.__new__(cls)
        self.vocab, self.n, self.clips = int(sd["vocab"]), int(sd["n"]), int(sd["clips"])
        self.log_ref_len = math.log(float(self.clips))
        import numpy as np
        keys = sd["entry_keys"].numpy().view(np.uint64).tolist()
        self._finish(keys, sd["entry_df"].tolist(), int(sd["capacity"]))
        return self

    @classmethod
    def from_token_table(cls, tokens, start, begin, term: int, vocab: int, n: int = 4, capacity: Optional[int] = None) -> "CiderStats":
        """tokens int64 [rows, width] (any device), start: the rows' first columns, begin: the clips' CSR offsets over the rows, term:
        the id that ends a row -- the references' table as ops.caption_cider reads it"""
        rows = tokens.cpu().tolist()
        start = [int(s) for s in (start.tolist() if torch.is_tensor(start) else start)]
        begin = [int(b) for b in (begin.tolist() if torch.is_tensor(begin) else begin)]
        refs = [generated_part(row, s, int(term)) for row, s in zip(rows, start)]
        return cls([refs[a:b] for a, b in zip(begin, begin[1:])], vocab, n, capacity)


def _sampler_config(gpt, top_k=None, top_p=None):
    """_gen_config with the filter overridden: giving either of top_k / top_p replaces both (the other one is then off)"""
    cfg = _gen_config(gpt)
    if top_k is not None or top_p is not None:
        cfg.top_k, cfg.top_p = int(top_k or 0), float(top_p or 0.0)
    return cfg


# sampler mode -> the names in `ops` of its (advance, constrain, score) functions; they say where a row works by pos=, step=, row_step=
SAMPLER_OPS = {"uniform": ("sample_advance", "logits_constrain", "sample_score"),
               "ragged": ("sample_advance_ragged", "logits_constrain_ragged", "sample_score_ragged"),
               "steps": ("sample_advance_steps", "logits_constrain_steps", "sample_score_steps")}


TRIE_OPS = {"uniform": "logits_trie_mask", "ragged": "logits_trie_mask_ragged", "steps": "logits_trie_mask_steps"}


def _trie_fn(mode: str, constraints) -> dict:
    """the trie_fn keyword of a loop for constraints with allowed_phrases, looked up in `ops` at the call; nothing without them"""
    if constraints is None or constraints.allowed_phrases is None:
        return {}
    return dict(trie_fn=getattr(ops, TRIE_OPS[mode]))


def _sampler_fns(mode: str, return_scores) -> dict:
    """a sampler mode's advance_fn / constrain_fn keywords (with return_scores also the score keywords), looked up in `ops` at the call"""
    advance, constrain, score = (getattr(ops, name) for name in SAMPLER_OPS[mode])
    return dict(advance_fn=advance, constrain_fn=constrain, **(dict(return_scores=True, score_fn=score) if return_scores else {}))


def install(gpt_cls):
    """Adds sample / beam_search / generate to DistributedGPT3 (same signatures as the reference methods), and beam_search_batched /
    sample_batched."""

    def sample(self, tokens, query_embeds=None, temperature=1.0, decode_weights="bf16", **kw):
        _no_sample_scores(kw.pop("return_scores", False), "sample")
        return sample_loop(_gen_config(self), make_state_fn(self, weights=decode_weights), tokens, query_embeds=query_embeds, temperature=temperature, **kw)

    def beam_search(self, tokens, query_embeds=None, beam_size=5, num_return_gen=1, stop_token=None, decode_weights="bf16", **kw):
        _no_sample_scores(kw.pop("return_scores", False), "beam_search")
        return beam_search_loop(_gen_config(self), make_state_fn(self, weights=decode_weights), tokens, query_embeds=query_embeds, beam_size=beam_size,
                                num_return_gen=num_return_gen, stop_token=stop_token, prompt_length=kw.pop("prompt_length", None),
                                topk_fn=lambda lg, k, add: ops.logprob_topk(lg, k, add=add))

    def beam_search_batched(self, tokens, query_embeds=None, beam_size=5, num_return_gen=1, stop_token=None, kv="per_sequence",
                            constraints=None, beam_groups=1, diversity_penalty=0.0, decode_weights="bf16", guidance=None, **kw):
        """beam_search for tokens [B, L] / query_embeds [B, Q, H] with one prompt length (prompt_length an int) or one per clip
        (a sequence of B lengths: beam_search_batched_loop's mixed mode, kv="shared_prefix" only), B clips in lockstep -> a list of B results;
        kv="shared_prefix" keeps the visual prefix and the prompt once per clip (SharedPrefixDecodeState); constraints: a
        LogitsConstraints, applied on the device every step (with allowed_phrases: a closed set of phrases, the results carry
        phrase_index and renormalised scores); beam_groups = G > 1: diverse beam search, G groups of beam_size beams
        each with diversity_penalty between them (beam_search_batched_loop; ops.beam_advance_groups); decode_weights="fp8": the steps
        run on the decoder's e4m3 codes (DecodeWeightsQ8); guidance: a Guidance with alpha 0 -- the state holds 2 * B * G * beam_size
        sequences, the second half behind the null query features, and every step's logits are guided by one launch
        (guided_state_fn, ops.logits_guide); the scores are then those of the guided distribution"""
        _no_sample_scores(kw.pop("return_scores", False), "beam_search_batched")
        make_state = _guided_make_state(make_state_fn(self, kv, decode_weights), guidance, query_embeds,
                                        tokens.size(0) * int(beam_groups) * int(beam_size), decode_weights, BAN_BEAM, "beam_search_batched", beams=True)
        groups = {} if int(beam_groups) == 1 else dict(beam_groups=beam_groups, diversity_penalty=diversity_penalty,
                                                       group_advance_fn=ops.beam_advance_groups)      # one group: none of the three keywords
        return beam_search_batched_loop(_gen_config(self), make_state, tokens, query_embeds=query_embeds, beam_size=beam_size,
                                        num_return_gen=num_return_gen, stop_token=stop_token, prompt_length=kw.pop("prompt_length", None),
                                        topk_fn=lambda lg, k, add: ops.logprob_topk(lg, k, add=add), advance_fn=ops.beam_advance,
                                        constraints=constraints, constrain_fn=ops.logits_constrain, **groups, **_trie_fn("uniform", constraints))

    def sample_batched(self, tokens, query_embeds=None, temperature=1.0, num_samples=1, seed=0, streams=None, top_k=None, top_p=None,
                       kv="per_sequence", constraints=None, return_scores=False, decode_weights="bf16", mixed_prompts=False, guidance=None,
                       **kw):
        """sample with the sampler on the device (sample_batched_loop): tokens [B, L] -> [B * num_samples, n]; top_k / top_p override
        the configuration's values; the draws are those of (seed, position, streams[row]) -- not torch's generator;
        kv="shared_prefix" keeps the visual prefix and the shortest prompt once per clip (SharedPrefixDecodeState); constraints: a
        LogitsConstraints, applied on the device every step (with allowed_phrases: every row is a phrase of the trie and the scores
        are renormalised over the allowed tokens); return_scores=True: -> (tokens, SampleScores), the model's
        log-probability of every generated token, recorded on the device every step (ops.sample_score); decode_weights="fp8": the
        steps run on the decoder's e4m3 codes (DecodeWeightsQ8); mixed_prompts=True with prompt_length = B lengths and
        kv="shared_prefix": ONE loop over clips whose prompts differ in length, the table left-aligned and every row on its own
        column (sample_batched_loop's mixed mode: ops.sample_advance_ragged / logits_constrain_ragged / sample_score_ragged);
        guidance: a Guidance -- the state holds 2 * B * num_samples sequences, the second half behind the null query features, and
        every step's logits are guided by one launch before anything else reads them (guided_state_fn, ops.logits_guide); the
        scores are then log-probabilities of the guided, renormalised distribution"""
        make_state = make_state_fn(self, kv, decode_weights)
        if mixed_prompts and kv != "shared_prefix":
            raise ValueError(f'mixed_prompts=True needs kv="shared_prefix" (got {kv!r}): only the shared-prefix decode step takes a '
                             "prefix length per clip")
        make_state = _guided_make_state(make_state, guidance, query_embeds, tokens.size(0) * int(num_samples), decode_weights, BAN_SAMPLING,
                                        "sample_batched")
        return sample_batched_loop(_sampler_config(self, top_k, top_p), make_state, tokens, query_embeds=query_embeds, temperature=temperature,
                                   num_samples=num_samples, seed=seed, streams=streams, constraints=constraints,
                                   mixed_prompts=bool(mixed_prompts), **_sampler_fns("ragged" if mixed_prompts else "uniform", return_scores),
                                   **_trie_fn("ragged" if mixed_prompts else "uniform", constraints), **kw)

    def sample_inflight(self, tokens, query_embeds=None, temperature=1.0, num_samples=1, slots=32, seed=0, streams=None, top_k=None, top_p=None,
                        constraints=None, return_scores=False, decode_weights="bf16", max_new_tokens=None, refill_min=None, guidance=None,
                        **kw):
        """sample_batched(mixed_prompts=True, kv="shared_prefix") over a whole data set with the finished clips' slots refilled in
        flight (sample_inflight_loop: continuous batching): tokens [n, L], prompt_length n lengths; `slots` clips x num_samples
        sequences stay resident; max_new_tokens: a budget per clip (None: tokens_to_generate); top_k=1 is a greedy captioner.
        -> a namespace: tokens [n * num_samples, final_len], written [n], scores (SampleScores or None), steps, prefills"""
        _no_inflight_guidance(guidance, "sample_inflight")
        return sample_inflight_loop(_sampler_config(self, top_k, top_p), make_inflight_state_fn(self, decode_weights), tokens,
                                    query_embeds=query_embeds, temperature=temperature, num_samples=num_samples, slots=slots, seed=seed,
                                    streams=streams, max_new_tokens=max_new_tokens, refill_min=refill_min, constraints=constraints,
                                    **_sampler_fns("steps", return_scores), **_trie_fn("steps", constraints), **kw)

    def beam_search_inflight(self, tokens, query_embeds=None, beam_size=5, num_return_gen=1, stop_token=None, prompt_length=None, slots=32,
                             max_new_tokens=None, refill_min=None, beam_groups=1, diversity_penalty=0.0, constraints=None,
                             decode_weights="bf16", guidance=None, **kw):
        """beam_search_batched(kv="shared_prefix") over a whole data set with the finished clips' slots refilled in flight
        (beam_inflight_loop): tokens [n, L], prompt_length n lengths; `slots` clips x beam_groups * beam_size sequences stay resident;
        max_new_tokens: a budget per clip (None: the lockstep search's, up to the end of the table).  -> a namespace: results (the
        list of n results of beam_search_batched), steps, prefills"""
        _no_inflight_guidance(guidance, "beam_search_inflight")
        return beam_inflight_loop(_gen_config(self), make_inflight_state_fn(self, decode_weights), tokens, query_embeds=query_embeds,
                                  beam_size=beam_size, num_return_gen=num_return_gen, stop_token=stop_token, prompt_length=prompt_length,
                                  slots=slots, max_new_tokens=max_new_tokens, refill_min=refill_min, beam_groups=beam_groups,
                                  diversity_penalty=diversity_penalty, constraints=constraints,
                                  topk_fn=lambda lg, k, add: ops.logprob_topk(lg, k, add=add), advance_fn=ops.beam_advance_steps,
                                  constrain_fn=ops.logits_constrain_steps, **_trie_fn("steps", constraints), **kw)

    @torch.no_grad()
    def generate(self, tokens, do_sample=True, termination_id=None, *args, **kw):                # :1875-1880
        """sampler="device" (keyword; not in the reference, default "torch"): do_sample=True runs sample_batched, which takes
        kv="per_sequence" | "shared_prefix" (the per-clip loops keep a cache per sequence) and constraints= (a LogitsConstraints; the
        per-clip loops have none) and return_scores=True (-> (tokens, SampleScores); refused everywhere else).
        decode_weights="fp8" (every loop; default "bf16"): the decode steps run on e4m3 codes of the weights (DecodeWeightsQ8)"""
        sampler = kw.pop("sampler", "torch")
        _check_weight_mode(kw.get("decode_weights", "bf16"))
        if sampler not in ("torch", "device"):
            raise ValueError(f"sampler must be 'torch' or 'device' (got {sampler!r})")
        if kw.get("kv", "per_sequence") not in KV_MODES:
            raise ValueError(f"kv must be one of {KV_MODES} (got {kw['kv']!r})")
        lockstep = do_sample and sampler == "device"
        if not lockstep:                                       # the per-clip loops: what only the lockstep loops take is refused
            if kw.pop("kv", "per_sequence") != "per_sequence":
                raise ValueError('kv="shared_prefix" needs a lockstep loop: do_sample=True with sampler="device", or beam_search_batched')
            if kw.pop("constraints", None) is not None:
                raise ValueError('constraints need a lockstep loop: do_sample=True with sampler="device", or beam_search_batched')
            _no_sample_scores(kw.pop("return_scores", False), "generate without do_sample=True and sampler=\"device\"")
            if kw.pop("guidance", None) is not None:
                raise ValueError('guidance needs a lockstep loop: do_sample=True with sampler="device", or beam_search_batched')
        was = self.training
        self.eval()
        try:
            if lockstep:
                return self.sample_batched(tokens, termination_id=termination_id, *args, **kw)
            if do_sample:
                return self.sample(tokens, termination_id=termination_id, *args, **kw)
            return self.beam_search(tokens, stop_token=termination_id, *args, **kw)
        finally:
            self.train(was)

    gpt_cls.sample, gpt_cls.beam_search, gpt_cls.generate = sample, beam_search, generate
    gpt_cls.beam_search_batched, gpt_cls.sample_batched = beam_search_batched, sample_batched
    gpt_cls.sample_inflight = torch.no_grad()(sample_inflight)
    gpt_cls.beam_search_inflight = torch.no_grad()(beam_search_inflight)
