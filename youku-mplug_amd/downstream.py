"""Generation + classification heads on the gfx950 kernels -- drop-ins for
models/distributed_gpt3.py:431-657 (DistributedGPT3_Cls) and :988-1218 (DistributedGPT3_Retrieval_Cls, the ITM
re-ranker of downstream/run_retrieval_distributed_gpt3_itm.py).

Both run the frozen decoder twice per step on the same visual prefix:
  * generation pass: caption cross-entropy with a per-sample prompt-length loss mask (:1097-1102, 1121-1127);
  * prompt pass (use_cls): the last valid hidden state goes through cls_head = Linear-ReLU-Linear and a
    cross-entropy against `labels` (:1129-1153).
The ITM model first appends query_features[negative_indices] (:1105-1108), so text/prompt/labels carry
B + len(negative_indices) rows.  forward(..., train=False) returns the scores the eval loops rank by
(:1156-1212 / :596-651).  Same constructor contract and parameter names as the reference; forward returns
(loss_caption, loss_cls) attached to autograd through one Function (as pretrain.py does).
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
from types import SimpleNamespace
from typing import Optional, Sequence

import torch
from torch import nn

from . import generation, ops
from .ops import ACT_RELU
from .pretrain import DistributedGPT3_Pretrain
from .gpt3 import GPT3Config
from .vision import Linear, grad_of

_PAD = 8   # GEMM / cross-entropy column granule: the class dimension is padded to it


def shared_prefix_split(ids: torch.Tensor, first_out: torch.Tensor, last_out: torch.Tensor, group_size: int, Q: int):
    """The split rule of shared-prefix scoring.  ids [n, L] (n = groups * group_size; the rows of one group share a video);
    first_out / last_out [n]: token position j of the first / last output of each row (the hidden row at Q + j is read: a scored
    position or a pooled row), first_out = L and last_out = -1 for a row without outputs.  -> (P, Lc):
      P = Q + t with t the longest common token prefix of every group's rows, capped so that no output lies inside the prefix
      (t <= first_out of every row) and at least one token is left to the continuations (t <= L - 1); one P for the call, the
      minimum over groups;
      Lc = rows from P to the last output of the chunk (trailing rows only ever follow every output of a causal decoder), >= 1."""
    n, L = ids.shape
    assert n % group_size == 0 and L >= 1
    g = ids.view(n // group_size, group_size, L)
    same = (g == g[:, :1]).all(dim=1).to(torch.int32)                        # [groups, L]: column shared by every row of the group
    common = same.cumprod(dim=1).sum(dim=1)                                  # longest common prefix per group
    cap = first_out.view(n // group_size, group_size).min(dim=1).values
    t, last = torch.stack([torch.minimum(common, cap).min().clamp(max=L - 1), last_out.max().to(common.dtype)]).tolist()   # one host sync
    P = Q + t
    Lc = max(last + Q + 1 - P, 1)
    return P, Lc


class _GenClsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, model, args, pipeline=None):
        """pipeline (default: model._forward_pipeline): what runs the forward -> ((loss_caption, loss_cls), the tape _backward_pipeline reads)"""
        (lc, lk), tape = (model._forward_pipeline if pipeline is None else pipeline)(*args)
        ctx.model, ctx.tape = model, tape
        return lc, lk

    @staticmethod
    def backward(ctx, g_caption, g_cls):
        ctx.model._backward_pipeline(ctx.tape, g_caption.contiguous().float(), g_cls.contiguous().float())
        ctx.tape = None
        return torch.zeros(1, device=g_caption.device), None, None, None


class _GenCls(DistributedGPT3_Pretrain):
    ITM = False
    CONTRASTIVE = "ignore"          # the reference's Cls / Retrieval_Cls never read use_contrastive: no head is built

    def __init__(self, config: Optional[dict] = None, tokenizer=None, *, visual_cfg: Optional[dict] = None,
                 text_cfg: Optional[GPT3Config] = None, device="cuda"):
        config = dict(config or {})
        if visual_cfg is not None and "num_frames" in config:          # TimeSformer(num_frames=config['num_frames']) (:441, :998)
            visual_cfg = dict(visual_cfg, num_frames=config["num_frames"])
        # The pre-train class implements both options below; the generation / classification pipelines of this file do not
        # (their hidden-only prompt pass records no decoder weight-gradient inputs, and _query_features has no visual_norm
        # stage), and no shipped recipe sets either: refuse loudly instead of training silently wrong.
        if not config.get("freeze_text_decoder", True):
            raise NotImplementedError("freeze_text_decoder: false (models/distributed_gpt3.py:492, 722, 1049) is implemented for "
                                      "DistributedGPT3_Pretrain only; the ITM / classification / caption models refuse it")
        super().__init__(config, tokenizer, visual_cfg=visual_cfg, text_cfg=text_cfg, device=device)
        if not isinstance(self.visual_norm, nn.Identity):
            raise NotImplementedError("connect_ln (models/distributed_gpt3.py:513-516, 1070-1073) is implemented for "
                                      "DistributedGPT3_Pretrain only; the ITM / classification / caption models refuse it")
        self.use_cls = config.get("use_cls", False)                                         # :523 / :1079
        if self.use_cls:
            H = self.text_width
            self.num_classes = config["num_classes"]
            self.cls_head = nn.Sequential(Linear(H, H, device=device), nn.ReLU(), Linear(H, self.num_classes, device=device))

    # ------------------------------------------------------------------ pieces
    def _query_features(self, video, tape):
        B = video.shape[0]
        Q, Hh = self.num_learnable_token, self.text_width
        emb = self.visual_encoder.forward_features(video.to(torch.bfloat16), tape["vit"])
        image_query = self.attn_pool.forward_pool(self.learnable_queries, emb, B, emb.shape[0] // B, tape["pool"])
        tape["image_query"] = image_query
        return ops.gemm(image_query, self.visual_fc.weight, B * Q, Hh, self.vision_width, bias=self.visual_fc.bias)

    def _expand(self, qf, src: Sequence[int]):
        """rows of sample src[j] for every output sample j (negatives / per-text repeats)."""
        Q, Hh = self.num_learnable_token, self.text_width
        s = torch.as_tensor(list(src), dtype=torch.long, device=qf.device)
        idx = (s[:, None] * Q + torch.arange(Q, device=qf.device)[None]).reshape(-1).contiguous()
        return ops.gather_rows(qf, idx, idx.numel(), Hh)

    @staticmethod
    def _gen_targets(ids, mask, prompt_lengths, Q):
        n = ids.shape[0]
        targets = torch.cat([ids[:, 1:], ids[:, 1:2]], dim=1)                                 # :1097-1098 (last column unused)
        tla = mask[:, 1:].clone()
        pl = torch.as_tensor(prompt_lengths, device=ids.device).view(-1, 1)
        tla[torch.arange(tla.shape[1], device=ids.device)[None] < pl] = 0                     # :1100-1102
        targets = torch.cat([torch.full((n, Q), 100, dtype=torch.long, device=ids.device), targets], dim=1)
        loss_mask = torch.cat([torch.zeros((n, Q), dtype=torch.long, device=ids.device), tla], dim=1)
        return targets, loss_mask

    def _cls_logits(self, qf_rows, p_ids, p_mask, tape):
        """prompt pass -> pooled last valid hidden state -> cls_head logits (class dim padded to 8 with -1e30 bias)."""
        n, Lp = p_ids.shape
        Q, H = self.num_learnable_token, self.text_width
        S = Q + Lp
        out = self.text_decoder.forward_lm(qf_rows, p_ids, None, None, tape["gpt2"], hidden_only=True, pass_index=1)
        rows = (torch.arange(n, device=p_ids.device) * S + Q + p_mask.sum(dim=-1) - 1).contiguous()      # :1149-1150
        pooled = ops.gather_rows(out["last_hidden_state"].reshape(n * S, H), rows, n, H)
        logits, (z, a, w2, Cp) = self._cls_head_logits(pooled)
        tape.update(rows=rows, pooled=pooled, z=z, a=a, w2=w2, Cp=Cp, n2=n, S2=S)
        return logits

    def _cls_head_logits(self, pooled):
        """cls_head = Linear-ReLU-Linear on pooled [n, H] -> (logits [n, Cp], (z, a, w2, Cp) for the backward)."""
        n, H, C = pooled.shape[0], self.text_width, self.num_classes
        l0, l2 = self.cls_head[0], self.cls_head[2]
        z = torch.empty((n, H), dtype=torch.bfloat16, device=pooled.device)
        a = ops.gemm(pooled, l0.weight, n, H, H, bias=l0.bias, act=ACT_RELU, preact_out=z)
        Cp = (C + _PAD - 1) // _PAD * _PAD
        w2 = torch.zeros((Cp, H), dtype=torch.bfloat16, device=a.device)
        b2 = torch.full((Cp,), -1e30, dtype=torch.bfloat16, device=a.device)
        w2[:C].copy_(l2.weight.detach())
        b2[:C].copy_(l2.bias.detach())
        logits = ops.gemm(a, w2, n, Cp, H, bias=b2)
        return logits, (z, a, w2, Cp)

    # ------------------------------------------------------------------ pipelines
    def _forward_pipeline(self, video, ids, mask, prompt_lengths, p_ids, p_mask, negative_indices, labels):
        Bv = video.shape[0]
        Q = self.num_learnable_token
        tape = {"vit": {}, "pool": {}, "gpt": {}, "gpt2": {}}
        qf = self._query_features(video, tape)
        src = list(range(Bv)) + ([int(i) for i in negative_indices] if self.ITM else [])
        qf_rows = self._expand(qf, src) if self.ITM else qf                                   # :1105-1108
        targets, loss_mask = self._gen_targets(ids, mask, prompt_lengths, Q)
        out = self.text_decoder.forward_lm(qf_rows, ids, targets, loss_mask, tape["gpt"])
        loss_caption = out["loss"]
        tape.update(src=src, Bv=Bv)
        if self.use_cls:
            logits = self._cls_logits(qf_rows, p_ids, p_mask, tape)
            n = len(src)
            w = torch.full((n,), 1.0 / n, dtype=torch.float32, device=logits.device)         # F.cross_entropy mean (:1153)
            dlog = torch.empty_like(logits)
            _, loss_cls = ops.cross_entropy(logits, labels.contiguous().view(-1), w, n, tape["Cp"], dlogits=dlog)
            tape["dlog"] = dlog
        else:
            loss_cls = torch.zeros((), dtype=torch.float32, device=loss_caption.device)      # :1155
        return (loss_caption, loss_cls), tape

    def _backward_pipeline(self, tape, g_caption, g_cls):
        Bv, src = tape["Bv"], tape["src"]
        Q, Hh, D = self.num_learnable_token, self.text_width, self.vision_width
        if tape.get("shared_prefix"):      # forward_scst(training_pass="shared_prefix"): one prefix per clip, nothing to fold
            dq_rows = self.text_decoder.backward_shared_prefix_lm(tape["gpt"], g_caption)
        else:
            dq_rows = self.text_decoder.backward_lm(tape["gpt"], g_caption)
        if self.use_cls:
            n, S, Cp, C = tape["n2"], tape["S2"], tape["Cp"], self.num_classes
            l0, l2 = self.cls_head[0], self.cls_head[2]
            dlog, a, z, pooled = tape["dlog"], tape["a"], tape["z"], tape["pooled"]
            gscale = g_cls.reshape(1)
            gw2 = ops.gemm(dlog, a, Cp, Hh, n, trans_a=True, trans_b=True, alpha_dev=gscale)
            gb2 = ops.colsum(dlog, n, Cp)
            grad_of(l2.weight).copy_(gw2[:C])
            grad_of(l2.bias).copy_((gb2[:C].float() * g_cls).to(torch.bfloat16))
            dz = ops.gemm(dlog, tape["w2"], n, Hh, Cp, trans_b=True, alpha_dev=gscale, act_bwd_z=z, act_bwd=ACT_RELU)
            ops.gemm(dz, pooled, Hh, Hh, n, trans_a=True, trans_b=True, out=grad_of(l0.weight))
            ops.colsum(dz, n, Hh, out=grad_of(l0.bias))
            dpooled = ops.gemm(dz, l0.weight, n, Hh, Hh, trans_b=True)
            dlh = torch.zeros((n * S, Hh), dtype=torch.bfloat16, device=dz.device)
            ops.scatter_rows(dpooled, tape["rows"], dlh, n, Hh)
            dq2 = self.text_decoder.backward_lm(tape["gpt2"], None, d_last_hidden=dlh, accumulate_lora=True)   # second pass of the step
            dq_rows = ops.add(dq_rows, dq2)
        # fold the expanded rows back onto the videos they came from, in row order (reproducible)
        per = Q * Hh
        dqf = dq_rows[:Bv * Q]
        if len(src) > Bv:
            dqf = dqf.clone()
            flat_all, flat = dq_rows.view(-1), dqf.view(-1)
            for j in range(Bv, len(src)):
                b = src[j]
                ops.add(flat[b * per:(b + 1) * per], flat_all[j * per:(j + 1) * per], out=flat[b * per:(b + 1) * per])
        iq = tape["image_query"]
        ops.colsum(dqf, Bv * Q, Hh, out=grad_of(self.visual_fc.bias))
        ops.gemm(dqf, iq, Hh, D, Bv * Q, trans_a=True, trans_b=True, out=grad_of(self.visual_fc.weight))
        diq = ops.gemm(dqf, self.visual_fc.weight, Bv * Q, D, Hh, trans_b=True)
        demb = self.attn_pool.backward_pool(diq, self.learnable_queries, tape["pool"])
        if self.on_stage_grads_ready is not None:
            self.on_stage_grads_ready("head")
        self.visual_encoder.backward_features(demb, tape["vit"])

    @torch.no_grad()
    def _scores(self, video, text, prompt_text):
        """train=False: generation score -sum(losses * loss_mask) per (video, text) and the cls_head score."""
        Bv = video.shape[0]
        Q = self.num_learnable_token
        ids, mask = text.input_ids, text.attention_mask
        t = ids.shape[0] // Bv
        tape = {"vit": {}, "pool": {}, "gpt": {}, "gpt2": {}}
        qf = self._query_features(video, tape)
        rep = [b for b in range(Bv) for _ in range(t)]                                        # '(v t)' / '(b c)' ordering
        qf_rep = self._expand(qf, rep)
        targets, loss_mask = self._gen_targets(ids, mask, text.prompt_lengths, Q)
        out = self.text_decoder.forward_lm(qf_rep, ids, targets, loss_mask, tape["gpt"])
        gen = (-(out["losses"] * loss_mask).sum(dim=-1)).view(Bv, t)                           # :1180-1181 / :618-619
        cls = None
        if self.use_cls:
            per_video = not self.ITM                                                           # :622-647 vs :1183-1208
            logits = self._cls_logits(qf if per_video else qf_rep, prompt_text.input_ids, prompt_text.attention_mask, tape)
            logits = logits[:, :self.num_classes].float()
            cls = torch.softmax(logits, dim=-1)[:, 1].view(Bv, t) if self.ITM else logits
        return (gen if self.ITM else torch.softmax(gen, dim=-1)), cls

    # ------------------------------------------------------------------ shared-prefix scoring (evaluation)
    @torch.no_grad()
    def encode_video(self, video):
        """query features [B * Q, H] of a video batch: run once, then score any number of text chunks against them
        (score_shared_prefix(..., query_features=...))."""
        return self._query_features(video, {"vit": {}, "pool": {}})

    def _shared_prefix_pass(self, qf, ids, group_size, first_out, last_out, out_rows, loss_mask=None, targets=None):
        """Prefix pass over the groups' shared rows + continuation pass over each row's own rows.  out_rows [n]: hidden row
        (absolute position) to pool, or None; loss_mask / targets [n, S-1] / [n, S]: the scored positions.  -> (losses per row
        [n] summed over its scored positions, pooled hidden [n, H])."""
        Q = self.num_learnable_token
        n, L = ids.shape
        dec = self.text_decoder
        P, Lc = shared_prefix_split(ids, first_out, last_out, group_size, Q)
        t = P - Q
        assert n % group_size == 0 and qf.shape[0] == (n // group_size) * Q, \
            f"{n} rows in groups of {group_size} need the query features of {n // group_size} videos, got {qf.shape[0] // Q}"
        prefix = dec.forward_prefix(qf, ids[::group_size, :t].contiguous())
        assert prefix["P"] == P and prefix["B"] == n // group_size
        cont = ids[:, t:t + Lc].contiguous()
        kw, sel = {}, None
        if loss_mask is not None:
            lm = torch.zeros((n, P + Lc), dtype=loss_mask.dtype, device=ids.device)
            w = min(loss_mask.shape[1], P + Lc)
            lm[:, :w] = loss_mask[:, :w]
            sel = lm[:, P:].nonzero()                                                       # (row, i) of every scored position
            kw.update(loss_rows=(sel[:, 0] * Lc + sel[:, 1]).contiguous(), labels=targets[sel[:, 0], P + sel[:, 1]].contiguous())
        if out_rows is not None:
            kw.update(hidden_rows=(torch.arange(n, device=ids.device) * Lc + out_rows - P).contiguous())
        out = dec.forward_continuation(prefix, cont, group_size, **kw)
        losses = None
        if sel is not None:
            losses = torch.zeros(n, dtype=torch.float32, device=ids.device).index_add_(0, sel[:, 0], out["losses"])
        return losses, out.get("hidden")

    @torch.no_grad()
    def score_shared_prefix(self, text, prompt_text, *, video=None, query_features=None):
        """What forward(..., train=False) returns (the same shapes and post-processing), computed with every video's shared rows
        -- its query features and the tokens all its candidates share -- run once (gpt3.DistributedGPT3.forward_prefix) and
        each candidate's own rows against them (forward_continuation, ops.attn_prefix_fwd).  Exact up to bf16 summation order."""
        assert (video is None) != (query_features is None), "pass exactly one of video / query_features"
        qf = self.encode_video(video) if query_features is None else query_features
        Q = self.num_learnable_token
        Bv = qf.shape[0] // Q
        ids, mask = text.input_ids, text.attention_mask
        n, L = ids.shape
        if qf.shape[0] != Bv * Q or Bv == 0 or n % Bv != 0:
            raise ValueError(f"query features of {qf.shape[0] / Q:g} videos ({qf.shape[0]} rows of Q = {Q}) do not divide the {n} "
                             f"text rows into equal groups: pass the features of the video batch the texts were built for")
        t = n // Bv
        targets, loss_mask = self._gen_targets(ids, mask, text.prompt_lengths, Q)
        scored = loss_mask[:, Q:] != 0                                                       # [n, L-1]: hidden row Q + j scored
        j = torch.arange(scored.shape[1], device=ids.device)
        first = torch.where(scored, j, L).min(dim=1).values if scored.shape[1] else torch.full((n,), L, device=ids.device)
        last = torch.where(scored, j, -1).max(dim=1).values if scored.shape[1] else torch.full((n,), -1, device=ids.device)
        losses, _ = self._shared_prefix_pass(qf, ids, t, first, last, None, loss_mask=loss_mask, targets=targets)
        gen = (-losses).view(Bv, t)
        cls = None
        if self.use_cls:
            if self.ITM:
                p_ids, p_mask = prompt_text.input_ids, prompt_text.attention_mask
                pj = p_mask.sum(dim=-1) - 1                                                  # pooled token (:1149-1150)
                _, pooled = self._shared_prefix_pass(qf, p_ids, t, pj, pj, Q + pj)
                logits, _ = self._cls_head_logits(pooled)
                cls = torch.softmax(logits[:, :self.num_classes].float(), dim=-1)[:, 1].view(Bv, t)
            else:                                                                            # one prompt per video (:622-647)
                tape = {"gpt2": {}}
                cls = self._cls_logits(qf, prompt_text.input_ids, prompt_text.attention_mask, tape)[:, :self.num_classes].float()
        return (gen if self.ITM else torch.softmax(gen, dim=-1)), cls

    def _run(self, image, text, prompt_text, negative_indices, labels, train):
        if not train:
            return self._scores(image, text, prompt_text)
        args = (image, text.input_ids, text.attention_mask, text.prompt_lengths,
                None if prompt_text is None else prompt_text.input_ids, None if prompt_text is None else prompt_text.attention_mask,
                negative_indices, labels)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _GenClsFn.apply(self._anchor, self, args)
        return self._forward_pipeline(*args)[0]


class DistributedGPT3_Cls(_GenCls):
    """models/distributed_gpt3.py:431-657."""
    ITM = False

    def forward(self, image, text=None, prompt_text=None, labels=None, train=True):
        return self._run(image, text, prompt_text, None, labels, train)


class DistributedGPT3_Retrieval_Cls(_GenCls):
    """models/distributed_gpt3.py:988-1218."""
    ITM = True

    def forward(self, image, text=None, prompt_text=None, negative_indices=None, labels=None, train=True):
        return self._run(image, text, prompt_text, negative_indices, labels, train)


class DistributedGPT3_Caption(_GenCls):
    """models/distributed_gpt3.py:661-814: caption fine-tuning loss (prompt tokens masked out) and beam-search
    captioning on the KV-cache decode path (generation.py)."""
    ITM = False

    def forward(self, image, text=None):
        return self._run(image, text, None, None, None, True)[0]                              # :768-789 returns loss_caption only

    SCST_BASELINES = ("mean_others", "greedy")
    SCST_TRAINING_PASSES = ("per_sequence", "shared_prefix")
    SCST_MAX_OPERAND_BYTES = 0x7FFFFFF0          # mpv_gemm_bf16 refuses an operand of this many bytes or more

    def forward_scst(self, image, text, references, *, cider, num_samples=5, baseline="mean_others", temperature=1.0, top_k=None, top_p=None,
                     seed=None, max_new_tokens=None, termination_id=None, rollouts=None, training_pass="per_sequence"):
        """Self-critical sequence training (not in the reference): one step's loss from the model's OWN sampled
        captions, each weighted by its CIDEr against the clip's references minus a baseline.  text: the prompts as in generate, ONE prompt
        length per call; references[b]: clip b's reference captions, a non-empty list of token lists; cider: the corpus statistics, a
        generation.CiderStats.  In order:
          1. the query features, once per clip, in the model's mode, on the tape;
          2. under no_grad and with the decoder in eval mode (the decode path must see no dropout), num_samples = N captions per clip from
             those features through the device sampler (text_decoder.sample_batched, kv="shared_prefix"; temperature / top_k / top_p as in
             generate; seed None: derived from text_decoder.step_seed, so a resumed run repeats its rollouts; max_new_tokens None: the
             decoder's tokens_to_generate); baseline="greedy" adds one top_k=1 caption per clip.  rollouts: an int64 table
             [B * N, <= prompt + max_new_tokens] in the sampler's output layout (row b * N + s) that REPLACES the sampling;
          3. the rewards r [B, N]: ONE ops.caption_cider call on the sampler's padded table against the references' table (one upload);
          4. the advantages, fp32 on the device: "mean_others" A[b, n] = mean_{m != n}(r[b, n] - r[b, m]) (N >= 2), "greedy"
             A[b, n] = r[b, n] - r_greedy[b];
          5. ONE training pass of the frozen decoder over the B * N sequences [query slots | prompt | sample], the query rows repeated
             (_expand; sequence s * B + b: the fold of _backward_pipeline then adds a clip's rows in sample order), the loss window from the
             prompt's last position on, the weight of a generated position up to and including the terminating token A[b, n] / T with T
             the number of such positions in the call, 0 elsewhere: loss = sum_t w_t CE_t, the weights handed to the CE kernel as they
             are (signed: no normalisation by their sum, which is near zero);
             training_pass="shared_prefix" (default "per_sequence": the pass above) runs step 5 on a shared prefix instead, as the
             rollout does: every clip's P = Q + prompt - 1 prefix rows ONCE and its N samples as packed, ragged
             continuations [last prompt token, s_0 .. s_{T-2}] with targets [s_0 .. s_{T-1}] of its T live positions
             (text_decoder.forward_shared_prefix_lm; one read of the B * N live counts builds the layout) -- the same targets and the
             same weights A[b, n] / T on B P + sum T rows instead of B N (Q + width), no _expand and no fold.  That pass applies NO
             decoder dropout (hidden or attention), whatever the model's mode; the visual tower and the abstractor stay in the model's mode;
          6. backward through _GenClsFn / _backward_pipeline.
        -> (loss, stats): stats = dict(reward, baseline, length, terminated), the means over the B * N samples, read from the device once."""
        o = self._scst_options(SimpleNamespace(text=text, references=references, cider=cider, num_samples=num_samples, baseline=baseline,
                                               temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, max_new_tokens=max_new_tokens,
                                               termination_id=termination_id, rollouts=rollouts,
                                               training_pass=training_pass))                           # every refusal comes first
        holder = {}
        args = (image, o, holder)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            loss = _GenClsFn.apply(self._anchor, self, args, self._scst_pipeline)[0]
        else:
            loss = self._scst_pipeline(*args)[0][0]
        reward, base, length, terminated = holder["stats"].tolist()                          # stats: one read, at the end
        return loss, dict(reward=reward, baseline=base, length=length, terminated=terminated)

    def _scst_options(self, o):
        """forward_scst's arguments as a namespace -> the same namespace, checked and completed before anything is launched: B, N, pl (the
        one prompt length), width (the token table's columns), term, seed, the references as host lists"""
        if o.baseline not in self.SCST_BASELINES:
            raise ValueError(f"baseline must be one of {self.SCST_BASELINES} (got {o.baseline!r})")
        if o.training_pass not in self.SCST_TRAINING_PASSES:
            raise ValueError(f"training_pass must be one of {self.SCST_TRAINING_PASSES} (got {o.training_pass!r})")
        o.N = int(o.num_samples)
        if o.N < 1:
            raise ValueError(f"num_samples must be at least 1 (got {o.N})")
        if o.baseline == "mean_others" and o.N < 2:
            raise ValueError('baseline="mean_others" compares a sample with the clip\'s other samples: num_samples must be at least 2 (got 1)')
        if not isinstance(o.cider, generation.CiderStats):
            raise ValueError(f"cider must be a generation.CiderStats (got {type(o.cider).__name__})")
        gc = generation._gen_config(self.text_decoder)
        if gc.vocab_size > o.cider.vocab:                # the kernel packs id + 1 into 16 bits: a sampled id beyond the table's would alias
            raise ValueError(f"cider was built for a vocabulary of {o.cider.vocab} ids, the decoder draws from {gc.vocab_size}: its keys "
                             "would alias (CiderStats holds at most 65535 ids)")
        ids, mask = o.text.input_ids, o.text.attention_mask
        o.B = ids.shape[0]
        if len(o.references) != o.B:
            raise ValueError(f"{len(o.references)} reference lists for {o.B} clips")
        o.refs = [[[int(t) for t in (r.tolist() if torch.is_tensor(r) else r)] for r in refs] for refs in o.references]
        for b, refs in enumerate(o.refs):
            if not refs:
                raise ValueError(f"clip {b} has no references: a self-critical reward needs at least one per clip")
        lengths = (mask.sum(-1) - 1).tolist()
        if len(set(lengths)) != 1:
            raise ValueError(f"forward_scst takes one prompt length per call (got {sorted(set(lengths))}): group the clips by prompt length")
        o.pl = int(lengths[0])
        if o.pl < 1:
            raise ValueError("every clip needs a prompt of at least one token")
        o.budget = gc.tokens_to_generate if o.max_new_tokens is None else int(o.max_new_tokens)
        o.width = min(o.pl + o.budget, gc.max_position_embeddings)
        if o.budget < 1 or o.width <= o.pl:
            raise ValueError(f"no room to generate: prompt of {o.pl} tokens, max_new_tokens {o.budget}, {gc.max_position_embeddings} positions")
        if o.width - o.pl > ops._lib.CAPTION_OVERLAP_MAX_LEN:
            raise ValueError(f"a row of {o.width} columns behind a prompt of {o.pl} tokens can hold a caption of more than "
                             f"{ops._lib.CAPTION_OVERLAP_MAX_LEN} tokens: lower max_new_tokens")
        if max(len(r) for refs in o.refs for r in refs) > ops._lib.CAPTION_OVERLAP_MAX_LEN:
            raise ValueError(f"a reference holds more than {ops._lib.CAPTION_OVERLAP_MAX_LEN} tokens")
        # the training pass is ONE decoder pass over B * N sequences: its largest GEMM operands -- the MLP's [rows, ffn] activation and
        # the loss window's [rows, vocab] logits, bf16 -- must stay under the GEMM entry's 2 GiB operand limit (include/mpv.h)
        cfg = self.text_decoder.config
        rows, wrows = o.B * o.N * (self.num_learnable_token + o.width), o.B * o.N * (o.width - o.pl)
        if o.training_pass == "shared_prefix":      # this mode's rows: every prefix once, at most the budget per sample
            P = self.num_learnable_token + o.pl - 1
            self.text_decoder._shared_prefix_lm_check(P, o.width - o.pl)
            rows = o.B * P + wrows
        worst = max(rows * cfg.ffn_hidden_size, wrows * cfg.vocab_size, rows * 3 * cfg.hidden_size) * 2
        if worst >= self.SCST_MAX_OPERAND_BYTES:
            raise ValueError(f"one training pass over {o.B} clips x {o.N} samples of {self.num_learnable_token + o.width} positions needs a "
                             f"GEMM operand of {worst} bytes, larger than 2 GiB: pass fewer clips per forward_scst call")
        o.termination_id, o.term = self._termination(o.termination_id)
        if not 0 <= o.term < gc.vocab_size:                      # it pads the rollouts, which the training pass embeds
            raise ValueError(f"termination_id = {o.term} is no token of the vocabulary [0, {gc.vocab_size})")
        if o.rollouts is not None:
            r = o.rollouts
            if r.dtype != torch.int64 or r.ndim != 2 or r.shape[0] != o.B * o.N or not o.pl < r.shape[1] <= o.width:
                raise ValueError(f"rollouts must be int64 [{o.B * o.N}, {o.pl + 1} .. {o.width}] (got {r.dtype} {tuple(r.shape)})")
            if int(r.min()) < 0 or int(r.max()) >= gc.vocab_size:
                raise ValueError(f"rollouts hold ids outside the vocabulary [0, {gc.vocab_size})")
        if o.seed is None:
            o.seed = (int(self.text_decoder.step_seed) ^ 0x5C57C1DE) & 0x3FFFFFFFFFFFFFFF
        return o

    def _scst_rollout(self, o, qf, N, **filt):
        """N sampled captions per clip on the query features qf [B, Q, H] -> the padded device table [B * N, width], row b * N + s"""
        toks = self.text_decoder.sample_batched(o.text.input_ids[:, :o.pl].contiguous(), query_embeds=qf, temperature=o.temperature,
                                                num_samples=N, seed=o.seed, termination_id=o.termination_id, kv="shared_prefix",
                                                prompt_length=torch.full((o.B,), o.pl, device=qf.device), tokens_to_generate=o.budget, **filt)
        return generation.pad_after_termination(toks, o.pl, o.term, o.width, o.term)

    def _scst_pipeline(self, video, o, holder):
        """forward_scst's steps 1 - 5 -> ((loss, 0), the tape of _backward_pipeline); holder["stats"]: the four means, on the device"""
        B, N, pl, W, term = o.B, o.N, o.pl, o.width, o.term
        Q, Hh = self.num_learnable_token, self.text_width
        tape = {"vit": {}, "pool": {}, "gpt": {}, "gpt2": {}}
        qf = self._query_features(video, tape)                                               # 1. in the model's mode, on the tape
        dev = qf.device
        # 2. the decode path sees no dropout -- and no live adapters: the C decode drivers sample from the MERGED weights (a no-op without adapters)
        with torch.no_grad(), _eval_mode(self), self.text_decoder.lora_merged():
            q3 = qf.view(B, Q, Hh)
            if o.rollouts is None:
                table = self._scst_rollout(o, q3, N, top_k=o.top_k, top_p=o.top_p)
            else:
                table = generation.pad_after_termination(o.rollouts.to(dev), pl, term, W, term)
            rows = table.view(B, N, W)
            if o.baseline == "greedy":
                rows = torch.cat([rows, self._scst_rollout(o, q3, 1, top_k=1).view(B, 1, W)], dim=1)
        K = rows.shape[1]
        flat = [r for refs in o.refs for r in refs]                                          # 3. the references: one table, one upload
        Wr = max(max(len(r) for r in flat), 1)
        ref_table = torch.tensor([r + [term] * (Wr - len(r)) for r in flat], dtype=torch.int64).to(dev)
        ref_begin = [0]
        for refs in o.refs:
            ref_begin.append(ref_begin[-1] + len(refs))
        _, score = ops.caption_cider(rows.reshape(B * K, W).contiguous(), [pl] * (B * K), list(range(0, B * K + 1, K)), ref_table,
                                     [0] * len(flat), ref_begin, term=term, stats=o.cider)
        r_all = score.view(B, K).to(torch.float32)
        r = r_all[:, :N]
        if o.baseline == "greedy":                                                           # 4. fp32, on the device
            adv = r - r_all[:, N:]
        else:                  # mean_{m != n}(r_n - r_m): the differences of equal rewards are exactly 0, whatever N
            adv = (r[:, :, None] - r[:, None, :]).sum(dim=2) / (N - 1)
        gen = table[:, pl:]                                                                  # [B * N, W - pl], row b * N + s
        is_term = gen == term
        live = (is_term.cumsum(dim=1) - is_term.to(torch.int64)) == 0                        # up to and including the terminating token
        T = live.sum().to(torch.float32)
        weights = adv.reshape(B * N, 1) * live.to(torch.float32) / T
        ended = is_term.any(dim=1)
        holder["stats"] = torch.stack([r.mean(), (r - adv).mean(), (live.sum(dim=1) - ended.to(torch.int64)).to(torch.float32).mean(),
                                       ended.to(torch.float32).mean()])
        if o.training_pass == "shared_prefix":
            # 5. on a shared prefix: ONE read of the live counts; sample (b, n) is the packed continuation b * N + n of group b
            counts = live.sum(dim=1).tolist()
            layout = ops.PackedLayout(counts, [N] * B, device=dev)
            at = torch.tensor([i * (W - pl) + t for i, T_i in enumerate(counts) for t in range(T_i)], dtype=torch.long).to(dev)
            pick = lambda t: t.reshape(-1)[at].contiguous()
            out = self.text_decoder.forward_shared_prefix_lm(qf, table.view(B, N, W)[:, 0, :pl - 1].contiguous(), pick(table[:, pl - 1:W - 1]),
                                                             layout, (pick(gen), pick(weights)), tape["gpt"])
            tape.update(src=list(range(B)), Bv=B, shared_prefix=True)
            return (out["loss"], torch.zeros((), dtype=torch.float32, device=dev)), tape
        # 5. sequence s * B + b: the first B rows are the clips' own, what _backward_pipeline's fold expects
        order = lambda t: t.view(B, N, -1).transpose(0, 1).reshape(N * B, -1).contiguous()
        src = list(range(B)) * N
        wl = W - pl
        out = self.text_decoder.forward_lm(self._expand(qf, src), order(table), None, None, tape["gpt"], loss_window=(Q + pl - 1, wl),
                                           window_targets=(order(gen).view(-1), order(weights).view(-1)))
        tape.update(src=src, Bv=B)
        return (out["loss"], torch.zeros((), dtype=torch.float32, device=dev)), tape

    @torch.no_grad()
    def generate(self, image, text, termination_id=None, batched=False, clips_per_search=32, do_sample=False, num_samples=1, temperature=1.0,
                 top_k=None, top_p=None, seed=0, kv_cache="per_sequence", repetition_penalty=None, no_repeat_ngram_size=0, min_new_tokens=0,
                 banned_token_ids=None, constrain_prompt=False, return_scores=False, best_of=False, length_penalty=1.0, query_features=None,
                 beam_groups=1, diversity_penalty=0.0, rerank_by_logprob=False, decode_weights="bf16", mixed_prompts=False, sample_mixed_prompts=False,
                 inflight=False, max_new_tokens=None, refill_min=None, beam_inflight=False, allowed_phrases=None, consensus=None,
                 rerank_by_consensus=None, guidance_scale=1.0, guidance_alpha=0.0, guidance_query_features=None, **kw):
        """One beam search per sample (:790-809): prompt = text.input_ids[i, :mask.sum()-1], prefix = its query features.
        batched=True (not in the reference, default off): the clips are grouped by prompt length and every group is searched in
        lockstep, `clips_per_search` clips at a time (generation.beam_search_batched_loop: the decoder's weights are read once per
        generated position of a chunk, not once per clip; the prefill runs once per clip).  Same return value: one [n, Lt] tensor
        per clip, in input order.  KV memory is what bounds clips_per_search: a chunk holds clips_per_search x beam_size sequences
        in both copies of the cache -- at 1.3B dims 88 MB per sequence of 300 positions, so 32 clips x 5 beams x 2 copies is about
        28 GB; halve clips_per_search to halve it.
        kv_cache="shared_prefix" (default "per_sequence"; batched=True and do_sample=True only): the query slots and the prompt, the
        same in every beam or sample of a clip, are cached once per clip and only the generated positions per sequence
        (generation.SharedPrefixDecodeState): nl * (clips * P + (1 or 2) * clips * K * S) * 3H * 2 bytes for P shared and S generated
        positions -- 264 + 36 positions at 1.3B dims: 32 clips x 5 beams take about 5.9 GB instead of 28 GB, 32 clips x 16 samples
        (no second copy) about 7.9 GB instead of 45 GB per copy of the cache.
        do_sample=True (not in the reference, default off): `num_samples` SAMPLED captions per clip instead of the beam search, with
        the sampler on the device (generation.sample_batched_loop; temperature, top_k / top_p -- None: the decoder's configuration --
        and seed as there).  The clips are grouped and chunked as with batched=True; sample s of clip i (its index in this call) draws
        from stream i * num_samples + s, so a clip's samples depend neither on clips_per_search nor on the other clips of the call.
        A chunk stops when all of its sequences have terminated, and a terminated sequence goes on drawing until then (as in the
        reference's sample): every row is therefore cut behind its first termination token and padded with that token to the full
        width Lt = prompt columns + tokens_to_generate, which is what makes the result independent of the chunking.
        -> per clip one [num_samples, Lt] tensor, in input order.
        repetition_penalty / no_repeat_ngram_size / min_new_tokens / banned_token_ids / constrain_prompt (batched=True and do_sample=True
        only; defaults off): a generation.LogitsConstraints applied to every step's raw logits on the device (one launch,
        ops.logits_constrain) -- the CTRL penalty on tokens already generated, no n-gram of that size twice, no termination token
        before min_new_tokens tokens, ids that are never produced; constrain_prompt=True lets the penalty and the n-grams see the
        prompt too.  They combine with kv_cache="shared_prefix".
        return_scores=True (do_sample=True only; default off): -> (res, scores); scores[i] is a dict of CPU tensors for clip i, in input
        order: sum_logprob [N] fp32 (the model's log-probability of sample s: the sum over its generated tokens up to and including the
        terminating one), count [N] int32 (how many tokens that is) and token_logprob [N, Lt] fp32 (0 at prompt positions, behind the
        termination and in the columns the chunk never reached: the table is padded like the tokens).  The scores are recorded on the
        device, one launch per step (ops.sample_score), from the RAW logits under the constraints: temperature, top_k and top_p shape
        the proposal, not the score.
        best_of=True (do_sample=True only; default off): one [1, Lt] tensor per clip, sample argmax_s sum_logprob[s] / count[s] **
        length_penalty of the clip's num_samples samples (fp64 on the host, once per chunk, from the chunk's one download; a tie goes to
        the lowest sample index; a sample with count 0 scores -inf); with return_scores the dict holds the chosen sample's entries
        ([1], [1], [1, Lt]) and `index`, its number.
        A clip's TOKENS stay independent of clips_per_search and of its neighbours.  Its SCORES are bit-identical only at an equal row
        count: the decode step's GEMM dispatch depends on the number of rows (DESIGN.md sections 13, 17, 18), which moves the logits in
        their last bf16 digit.  A near-tie in best_of may therefore resolve differently under another chunking.
        query_features (default None: computed from `image` here): the clips' encode_video() output, for a caller that also needs it
        elsewhere (score_captions); `image` is then not consulted.
        beam_groups = G > 1 (batched=True only; default 1): diverse (group) beam search -- `beam_size` beams PER GROUP, G * beam_size at
        most 16, a later group penalised by diversity_penalty for every beam of an earlier group that chose the same token at the same
        step (generation.beam_search_batched_loop, ops.beam_advance_groups).  -> per clip one [n, Lt] tensor, n <= num_return_gen (a
        multiple of G): group 0's best num_return_gen // G rows first, then group 1's, ...  It combines with kv_cache and the constraints.
        rerank_by_logprob=True (batched=True only; default off): -> (res, scores).  Each clip's n candidates -- the tokens between the
        prompt and the first termination token, possibly none -- are scored by score_captions on this call's query features (no second
        ViT pass; a beam's search score is length-normalised over the whole row and, in a later group, penalised: it is no likelihood),
        and the clip's rows are reordered by sum_logprob / count ** length_penalty descending, ties in search order: row 0 is
        best_sample's choice.  A hypothesis that fills its row without a termination token is scored whole, terminator included: one
        position more than the search fed, at most the LAST row of the position table (the search generates up to column final_len - 1
        and never feeds it; the scoring does) -- never outside it.  scores[i] is score_captions' dict in the new order (best = 0) plus group [n] int64, the group every row
        came from (zeros without groups).
        decode_weights="fp8" (every path; default "bf16"): the decode steps run on e4m3 codes of the decoder's weights, quantised on the
        device on first use (generation.DecodeWeightsQ8; the scoring of rerank_by_logprob stays on the bf16 weights).  It combines with
        kv_cache, the constraints, the scores and the groups.
        mixed_prompts=True (batched=True with kv_cache="shared_prefix" only; default off): the clips are NOT grouped by prompt length.
        They are chunked by clips_per_search in input order and every chunk is ONE lockstep search over its prompts, whatever their
        lengths (generation.beam_search_batched_loop's mixed mode: a per-clip prefix length in the decode steps, the beams' token
        table left-padded, every clip with the budget of positions its own length leaves).  Prompts that carry per-video text (a
        title, a question) then cost one search per chunk instead of one per distinct length.  Same return value; a clip's rows are
        those of the grouped call.  It combines with beam_groups, the constraints, rerank_by_logprob and decode_weights; do_sample,
        kv_cache="per_sequence" and constrain_prompt=True are refused (DESIGN.md section 23 says why).
        sample_mixed_prompts=True (do_sample=True with kv_cache="shared_prefix" only; default off): the same for the SAMPLED captions.
        The clips are chunked by clips_per_search in input order and every chunk is ONE lockstep loop over its prompts, whatever their
        lengths (generation.sample_batched_loop's mixed mode: the token table stays left-aligned and every row draws, is constrained and
        is scored at its own column, so a clip's samples still depend neither on clips_per_search nor on its neighbours; a clip whose
        columns run out before the chunk ends is frozen on the device).  Streams, return value, scores and best_of are those of the
        grouped call.  It combines with num_samples, temperature, top_k / top_p, seed, return_scores, best_of, decode_weights and the
        constraints, constrain_prompt=True included (this table has no padding); use without do_sample=True and
        kv_cache="per_sequence" are refused.
        inflight=True (do_sample=True with kv_cache="shared_prefix" only; default off): the sampled captions of ALL the clips in one
        loop that keeps clips_per_search clips (slots) x num_samples sequences resident and gives a finished clip's slot to the next
        clip while the others go on (generation.sample_inflight_loop: continuous batching; a suffix position per clip in the decode
        step, a generation step per row in the sampler-side kernels).  A lockstep chunk is held until its slowest caption ends; here a
        clip leaves when all its samples have terminated or after max_new_tokens tokens (None: tokens_to_generate; an int or one budget
        per clip, capped by the table's columns), and refills wait for refill_min free slots.  Prompts may differ in length as with
        sample_mixed_prompts, and streams, return value, return_scores and best_of are that call's: a clip's tokens depend neither on
        its slot nor on when it entered.  top_k=1 makes it a greedy captioner.  Use without do_sample=True or with
        kv_cache="per_sequence" is refused.
        beam_inflight=True (batched=True with kv_cache="shared_prefix" only; default off): the same for the BEAM search -- ONE loop over
        all the clips, prompt lengths from the attention mask, that keeps clips_per_search clips (slots) x beam_groups * beam_size
        sequences resident; a clip leaves when all its groups are done or after max_new_tokens positions (None: up to the end of the
        table, the lockstep search's budget; an int or one budget per clip), and refills wait for refill_min free slots
        (generation.beam_inflight_loop: a generation step per clip in the advance kernel, a row count per clip in the suffix
        re-order).  The return value is the batched call's.  It combines with beam_groups, diversity_penalty, rerank_by_logprob,
        decode_weights and the constraints, constrain_prompt=True included (this table has no padding).  Refused with do_sample, without
        batched=True, with kv_cache="per_sequence" and together with mixed_prompts=True.
        allowed_phrases (batched=True and do_sample=True only; default None: no call and no launch is added): a closed vocabulary --
        a generation.PhraseTrie, a list of token lists, or a list of strings tokenised with the model's tokenizer.  Every caption is
        then one of the phrases followed by the termination id: each step keeps only the tokens that continue a sequence along the
        trie (generation.LogitsConstraints(allowed_phrases=), ops.logits_trie_mask*; one launch per step, a cost independent of the
        number of phrases -- DESIGN.md section 28).  The tensors keep their shapes.  batched=True: -> (res, info); info[i] is a dict of
        CPU tensors for clip i: phrase_index [n] int64 (the index of row r's phrase in the list) and scores [n] fp32, the search's
        scores; a clip returns the best min(num_return_gen, phrases the search reached) rows.  do_sample=True: with return_scores the
        clip's dict also holds phrase_index [N].  All these scores are RENORMALISED over the allowed tokens, not the model's
        likelihoods over the vocabulary.  It combines with kv_cache, decode_weights, beam_groups, the mixed and in-flight modes and the
        other constraints except min_new_tokens; rerank_by_logprob is refused (score the phrases with score_captions instead).
        consensus="rouge_l" | "ngram_f" (do_sample=True only; default None: no call and no launch is added): one [1, Lt] tensor per
        clip, the CONSENSUS (minimum-Bayes-risk) choice among its num_samples samples: the sample h with the largest mean utility
        U[h] = mean_r u(h, r) over all the clip's samples r, itself included (generation.consensus_utility / consensus_choice: ROUGE-L
        with beta 1.2, or the mean F of the clipped 1..4-gram matches; a tie goes to the lowest sample index).  Likelihood prefers
        short, generic captions; this prefers the caption the other samples agree with.  The pairwise overlap counts are taken on the
        device from the padded token table the call has built anyway (ops.caption_overlap: one launch set per chunk) and come down in
        the chunk's one download beside the tokens and scores; the utilities are fp64 on the host.  The utilities are over TOKEN IDS,
        the entry point's corpus metrics over CJK characters.  A candidate holds at most 255 tokens: a table with more generated
        columns than that is refused before anything runs.  With return_scores the clip's dict holds the chosen sample's entries and
        `index` as with best_of, plus consensus [N] fp64, U of every sample.  It works in the grouped, sample_mixed_prompts and
        inflight modes; together with best_of it is refused.
        rerank_by_consensus="rouge_l" | "ngram_f" (batched=True only; default None): -> (res, info).  Each clip's returned hypotheses
        are reordered by U descending, ties in search order (one ops.caption_overlap call over all the clips' rows: the clips may
        return different numbers of rows); info[i] holds consensus [n] fp64 and group [n] int64 in the new order.  Refused together
        with rerank_by_logprob and with allowed_phrases.
        guidance_scale / guidance_alpha / guidance_query_features (batched=True and do_sample=True only; defaults 1.0 / 0.0 / None: no
        second branch, no launch, the call made before the feature existed): classifier-free guidance, also known as contrastive
        decoding (generation.Guidance).  Every chunk decodes a second, "null-video" branch of the same prompts in
        lockstep and each step continues from cond + (guidance_scale - 1) * (cond - uncond) on the max-centred logits (one launch,
        ops.logits_guide, before the constraints, the trie, the sampler, the scores and the top-k): a scale above 1 pushes a frozen
        decoder away from its language prior towards what the clip says.  guidance_alpha in (0, 1) (do_sample=True only) also bans
        every token whose conditional probability is below alpha times the step's largest.  guidance_query_features: None -- the
        query features of an all-zero normalised clip of this call's frame count and resolution, one batch-1 encode_video() per
        call, broadcast to all clips and not cached across calls (the weights may have changed) -- or a tensor [Q, H] (broadcast) or
        [B * Q, H] (one null clip per clip).  clips_per_search still counts CLIPS: a chunk's state holds 2 * clips * fan sequences,
        so its KV memory doubles.  Scores under guidance (return_scores, best_of, the search's own) are log-probabilities of the
        guided, renormalised distribution, not the model's likelihoods; rerank_by_logprob scores the unguided model.  It combines with
        kv_cache, the constraints, allowed_phrases, beam_groups, the mixed-prompt modes and decode_weights="fp8" (refused when 2 * clips
        * fan exceeds the 512 rows the FP8 step takes).  Refused: use with the per-clip search, with inflight / beam_inflight, alpha > 0
        with the beam search, a negative or non-finite scale, alpha outside [0, 1), features of another shape."""
        o = self._generate_options(SimpleNamespace(**locals()))       # every refusal comes first: a refused call runs no ViT pass
        Q, Hh = self.num_learnable_token, self.text_width
        Bv = image.shape[0] if query_features is None else query_features.shape[0] // Q
        with _eval_mode(self):
            qf = (self._query_features(image, {"vit": {}, "pool": {}}) if query_features is None else query_features).view(Bv, Q, Hh)
            if o.guided:
                null = o.guidance_query_features                              # None: the zero clip's, one batch-1 pass per call
                null = self.encode_video(torch.zeros((1,) + tuple(image.shape[1:]), dtype=image.dtype, device=image.device)) if null is None else null
                o.null = null.view(-1, Q, Hh)                                 # [1, Q, H]: every clip's; [n, Q, H]: one per clip
            if do_sample:
                return self._generate_samples(o, qf)
            if batched:
                return self._generate_beams(o, qf)
            res = []
            for i in range(o.n):
                out = self.text_decoder.generate(text.input_ids[i:i + 1], query_embeds=qf[i:i + 1], termination_id=o.termination_id,
                                                 do_sample=False, prompt_length=o.lengths[i], **o.kw)
                res.append(out.sequences.cpu())
            return res

    def _termination(self, termination_id):
        """the termination_id of generate / score_captions -> (the id forwarded to the decoder: the caller's, else the tokenizer's eos,
        else None; term: that id as an int, the decoder's eod_id where it is None -- what the decoder's loops make of it)"""
        if termination_id is None:
            tok = getattr(self, "tokenizer", None)
            termination_id = tok.tokenizer.eos if tok is not None else None
        return termination_id, generation._gen_config(self.text_decoder).eod_id if termination_id is None else int(termination_id)

    def _generate_options(self, o):
        """generate's arguments as a namespace -> the same namespace, checked and completed, before anything runs.  The refusals keep
        one order: the keyword combinations (_refuse_keyword_combinations), then what the per-clip search cannot do, then the sizes of
        the mode.  kw becomes what is forwarded to the decoder: a keyword is there only when its feature is on (absent keyword: the
        call is the one made before the feature existed), and the in-flight calls take no kv.  Added for the routines below:
        termination_id / term (_termination), trie, n, lengths (the prompts' token counts) and, for the samplers, N, scored and width"""
        _refuse_keyword_combinations(o)
        kw = dict(o.kw)
        if o.decode_weights != "bf16":
            kw["decode_weights"] = o.decode_weights
        if int(o.beam_groups) != 1:
            kw.update(beam_groups=int(o.beam_groups), diversity_penalty=o.diversity_penalty)
        lockstep = o.do_sample or o.batched
        if (o.return_scores or o.best_of) and not o.do_sample:
            raise ValueError(f"return_scores / best_of need do_sample=True (got return_scores={o.return_scores!r}, best_of={o.best_of!r}): "
                             "beam hypotheses carry their own scores")
        if o.kv_cache not in generation.KV_MODES:
            raise ValueError(f"kv_cache must be one of {generation.KV_MODES} (got {o.kv_cache!r})")
        if o.kv_cache != "per_sequence":
            if not lockstep:
                raise ValueError('kv_cache="shared_prefix" needs batched=True or do_sample=True (the per-clip search keeps a cache per beam)')
            kw["kv"] = o.kv_cache
        if o.repetition_penalty is not None or o.no_repeat_ngram_size or o.min_new_tokens or o.banned_token_ids or o.constrain_prompt:
            if not lockstep:
                raise ValueError("repetition_penalty / no_repeat_ngram_size / min_new_tokens / banned_token_ids / constrain_prompt need "
                                 f"batched=True or do_sample=True (got repetition_penalty={o.repetition_penalty!r}, no_repeat_ngram_size="
                                 f"{o.no_repeat_ngram_size!r}, min_new_tokens={o.min_new_tokens!r}, banned_token_ids={o.banned_token_ids!r}, "
                                 f"constrain_prompt={o.constrain_prompt!r}): the per-clip search has no constraints")
            kw["constraints"] = generation.LogitsConstraints(
                repetition_penalty=1.0 if o.repetition_penalty is None else o.repetition_penalty, no_repeat_ngram_size=o.no_repeat_ngram_size,
                min_new_tokens=o.min_new_tokens, banned_token_ids=tuple(o.banned_token_ids or ()), include_prompt=o.constrain_prompt)
        o.trie = None
        if o.allowed_phrases is not None:
            if not lockstep:
                raise ValueError("allowed_phrases need batched=True or do_sample=True: the per-clip search has no constraints")
            if o.rerank_by_logprob:
                raise ValueError("allowed_phrases do not combine with rerank_by_logprob: score the phrases with score_captions")
            tok = getattr(self, "tokenizer", None)
            o.trie = generation.as_phrase_trie(o.allowed_phrases, generation._gen_config(self.text_decoder).vocab_size,
                                               None if tok is None else (lambda s: _encode_phrase(tok, s)))
            kw["constraints"] = dataclasses.replace(kw.get("constraints") or generation.LogitsConstraints(), allowed_phrases=o.trie)
        o.termination_id, o.term = self._termination(o.termination_id)
        o.n = o.text.input_ids.shape[0]
        o.lengths = (o.text.attention_mask.sum(-1) - 1).tolist()
        if o.do_sample:
            o.N = int(o.num_samples)
            if int(o.clips_per_search) < 1 or o.N < 1:
                raise ValueError(f"clips_per_search and num_samples must be at least 1 (got {o.clips_per_search}, {o.num_samples})")
            gc = generation._gen_config(self.text_decoder)
            o.width = min(o.text.input_ids.shape[1] + gc.tokens_to_generate, gc.max_position_embeddings)
            o.scored = bool(o.return_scores or o.best_of)
            if o.scored:
                kw["return_scores"] = True
            if o.consensus is not None and o.lengths and o.width - int(min(o.lengths)) > ops._lib.CAPTION_OVERLAP_MAX_LEN:
                raise ValueError(f"consensus: a row of {o.width} columns behind a prompt of {int(min(o.lengths))} tokens can hold a candidate "
                                 f"of more than {ops._lib.CAPTION_OVERLAP_MAX_LEN} tokens")
            if o.sample_mixed_prompts and not o.inflight:
                kw["mixed_prompts"] = True
        elif o.batched and int(o.clips_per_search) < 1:
            raise ValueError(f"clips_per_search must be at least 1 (got {o.clips_per_search})")
        if o.inflight or o.beam_inflight:
            kw.pop("kv", None)
        o.guided = self._guidance_options(o, lockstep)
        o.kw = kw
        return o

    @staticmethod
    def _chunk_kw(o, sel):
        """the keywords a lockstep chunk of the clips `sel` forwards to the decoder: o.kw, under guidance with the chunk's Guidance"""
        if not o.guided:
            return o.kw
        null = o.null[0] if o.null.shape[0] == 1 else o.null[sel]
        return dict(o.kw, guidance=generation.Guidance(o.guidance_scale, o.guidance_alpha, null))

    def _guidance_options(self, o, lockstep) -> bool:
        """the refusals of guidance_scale / guidance_alpha / guidance_query_features -> is the call guided?  (the Guidance itself is
        built in generate, once the null features exist)"""
        g = generation.Guidance(o.guidance_scale, o.guidance_alpha)           # scale and alpha: its own checks
        if not g.active:
            return False
        if not lockstep:
            raise ValueError("guidance_scale / guidance_alpha need batched=True or do_sample=True: the per-clip search has one branch")
        if o.inflight or o.beam_inflight:
            raise ValueError("guidance does not combine with inflight=True / beam_inflight=True: the in-flight states hold one branch per slot")
        if g.alpha > 0.0 and not o.do_sample:
            raise ValueError(f"guidance_alpha ({g.alpha}) needs do_sample=True: a banned token can enter the 2K candidates of a beam step")
        Q, Hh = self.num_learnable_token, self.text_width
        fan = o.N if o.do_sample else int(o.beam_groups) * int(o.kw.get("beam_size", 5))
        rows = 2 * min(int(o.clips_per_search), o.n) * fan
        if o.decode_weights == "fp8" and rows > ops._lib.W8_TILED_MAX_ROWS:
            raise ValueError(f'guidance doubles a chunk to {rows} rows (2 x clips x fan); decode_weights="fp8" takes at most '
                             f"{ops._lib.W8_TILED_MAX_ROWS}: lower clips_per_search")
        nf = o.guidance_query_features
        if nf is None:
            if o.image is None:
                raise ValueError("guidance needs `image` (the null clip takes its frame count and resolution) or guidance_query_features")
        elif not torch.is_tensor(nf) or tuple(nf.shape) not in ((Q, Hh), (o.n * Q, Hh)):
            raise ValueError(f"guidance_query_features must be [{Q}, {Hh}] or [{o.n * Q}, {Hh}] "
                             f"(got {tuple(nf.shape) if torch.is_tensor(nf) else type(nf).__name__})")
        return True

    # ------------------------------------------------------------------ the sampled family: three modes, one finish
    def _generate_samples(self, o, qf):
        """do_sample=True.  Each mode hands over (the padded device table [rows, width] with N rows per clip, its SampleScores or None,
        the column at which every row's generated part starts, the clips it covers): the in-flight loop once for the whole call, the
        lockstep loops once per chunk."""
        res, scores = [None] * o.n, [None] * o.n
        for toks, sc, starts, clips in (self._sampled_inflight(o, qf) if o.inflight else self._sampled_chunks(o, qf)):
            self._finish_samples(o, toks, sc, starts, clips, res, scores)
        return (res, scores) if o.return_scores else res

    def _sampled_inflight(self, o, qf):
        """inflight=True: ONE loop over all clips, clips_per_search slots resident"""
        out = self.text_decoder.sample_inflight(o.text.input_ids, query_embeds=qf.contiguous(), temperature=o.temperature, num_samples=o.N,
                                                slots=int(o.clips_per_search), seed=o.seed, top_k=o.top_k, top_p=o.top_p,
                                                termination_id=o.termination_id, prompt_length=[int(x) for x in o.lengths],
                                                max_new_tokens=o.max_new_tokens, refill_min=o.refill_min, **o.kw)
        starts = [int(x) for x in o.lengths for _ in range(o.N)]
        col = torch.arange(out.tokens.shape[1], device=out.tokens.device)[None]
        end = torch.as_tensor([w for w in out.written for _ in range(o.N)], dtype=torch.long).to(out.tokens.device)[:, None]
        toks = torch.where(col < end, out.tokens, torch.full_like(out.tokens, o.term))              # behind a clip's budget: padding
        yield generation.pad_after_termination(toks, starts, o.term, o.width, o.term), out.scores if o.scored else None, starts, range(o.n)

    def _sampled_chunks(self, o, qf):
        """the lockstep loops: one per chunk of clips with one prompt length, or (sample_mixed_prompts) per chunk in input order with
        its clips' lengths; sample s of clip i draws from stream i * N + s whatever the chunk"""
        mixed, N = o.sample_mixed_prompts, o.N
        for pl, chunk in _clip_chunks(o.lengths, o.clips_per_search, by_length=not mixed):
            sel = torch.as_tensor(chunk, dtype=torch.long, device=qf.device)
            streams = (sel[:, None] * N + torch.arange(N, device=qf.device)[None]).reshape(-1)
            out = self.text_decoder.sample_batched(o.text.input_ids[sel], query_embeds=qf[sel].contiguous(), temperature=o.temperature,
                                                   num_samples=N, seed=o.seed, streams=streams, top_k=o.top_k, top_p=o.top_p,
                                                   termination_id=o.termination_id,
                                                   prompt_length=pl if mixed else torch.full((len(sel),), pl, device=qf.device),
                                                   **self._chunk_kw(o, sel))
            toks, sc = out if o.scored else (out, None)
            starts = [x for x in pl for _ in range(N)] if mixed else [pl] * (len(chunk) * N)
            yield generation.pad_after_termination(toks, starts if mixed else pl, o.term, o.width, o.term), sc, starts, chunk

    def _finish_samples(self, o, toks, sc, starts, clips, res, scores):
        """a mode's padded device table -> res / scores of its clips, from ONE download (_download_rows) that carries the scores and,
        with consensus, the overlap counts beside the tokens; then the clip's one caption (consensus, best_of) and phrase_index"""
        N, picks = o.N, None
        if o.consensus is not None:
            toks, tlp, slp, cnt, picks = _consensus_samples(toks, sc, starts, N, o.term, o.width, o.consensus)
        elif sc is not None:
            toks, tlp, slp, cnt = _download_scored(toks, sc, o.width)
        else:
            toks = toks.cpu()
        for j, i in enumerate(clips):
            rows = slice(j * N, (j + 1) * N)
            res[i] = toks[rows]
            entry = None if sc is None else dict(sum_logprob=slp[rows], count=cnt[rows], token_logprob=tlp[rows])
            chosen = None
            if picks is not None:
                chosen = dict(index=picks[j][1], consensus=picks[j][0])
            elif o.best_of:
                chosen = dict(index=best_sample(entry["sum_logprob"], entry["count"], o.length_penalty))
            if chosen is not None:
                b = chosen["index"]
                res[i] = res[i][b:b + 1]
                if entry is not None:
                    entry = dict({k: v[b:b + 1] for k, v in entry.items()}, **chosen)
            if entry is not None:
                scores[i] = _with_phrase_index(entry, o.trie, res[i], o.lengths[i], o.term)

    # ------------------------------------------------------------------ the beam family: one collect, one reorder
    def _generate_beams(self, o, qf):
        """batched=True: the in-flight search over all clips or one lockstep search per chunk, then at most one re-rank"""
        n, dec = o.n, self.text_decoder
        res, groups_of, info = [None] * n, [None] * n, [None] * n

        def collect(clips, outs):
            for i, out in zip(clips, outs):
                res[i] = out.sequences.cpu()
                groups_of[i] = getattr(out, "group", None)
                info[i] = dict(phrase_index=getattr(out, "phrase_index", None), scores=out.scores)
        if o.beam_inflight:                                                  # ONE loop over all clips, clips_per_search slots resident
            collect(range(n), dec.beam_search_inflight(o.text.input_ids, query_embeds=qf.contiguous(), stop_token=o.termination_id,
                                                       prompt_length=[int(x) for x in o.lengths], slots=int(o.clips_per_search),
                                                       max_new_tokens=o.max_new_tokens, refill_min=o.refill_min, **o.kw).results)
        else:                               # grouped by prompt length, or (mixed_prompts) in input order with the chunk's lengths
            for pl, chunk in _clip_chunks(o.lengths, o.clips_per_search, by_length=not o.mixed_prompts):
                sel = torch.as_tensor(chunk, dtype=torch.long, device=qf.device)
                collect(chunk, dec.beam_search_batched(o.text.input_ids[sel], query_embeds=qf[sel].contiguous(), stop_token=o.termination_id,
                                                       prompt_length=pl, **self._chunk_kw(o, sel)))
        if o.trie is not None:
            return res, info
        if o.rerank_by_consensus is not None:
            picks = _consensus_rows(res, o.lengths, o.term, o.rerank_by_consensus, qf.device)
            ranked, tail = [(generation.consensus_order(U), dict(consensus=U)) for U, _ in picks], {}   # ties keep the search order
        elif o.rerank_by_logprob:
            ranked, tail = self._rank_by_logprob(o, qf, res), dict(best=0)
        else:
            return res
        for i, (order, columns) in enumerate(ranked):
            grp = groups_of[i] if groups_of[i] is not None else torch.zeros(len(order), dtype=torch.int64)
            res[i] = res[i][order]
            info[i] = dict({k: v[order] for k, v in columns.items()}, group=grp[order], **tail)
        return res, info

    def _rank_by_logprob(self, o, qf, res):
        """rerank_by_logprob: score every clip's hypotheses (the tokens between the prompt and the first termination token) with
        score_captions on this call's query features -> (order, score columns) per clip, best first as best_sample ranks"""
        cands = [[generation.generated_part(row, o.lengths[i], o.term) for row in res[i].tolist()] for i in range(o.n)]
        scores = self.score_captions(None, o.text, cands, query_features=qf.reshape(-1, self.text_width), termination_id=o.term,
                                     clips_per_pass=o.clips_per_search, length_penalty=o.length_penalty)
        for sc in scores:
            norm = [_normalised(lp, c, o.length_penalty) for lp, c in zip(sc["sum_logprob"].tolist(), sc["count"].tolist())]
            order = sorted(range(len(norm)), key=lambda s: -norm[s])                         # stable: ties keep the search order
            yield order, {k: sc[k] for k in ("sum_logprob", "count", "token_logprob")}


    @torch.no_grad()
    def score_captions(self, image, text, candidates, *, query_features=None, termination_id=None, score_termination=True,
                       clips_per_pass=32, length_penalty=1.0):
        """The model's log-likelihood of GIVEN captions (not in the reference): per-token NLL / perplexity of reference captions,
        ranking of candidate answers, re-scoring of captions from elsewhere.  text: the prompts as in generate (the prompt of clip i is
        text.input_ids[i, :mask.sum()-1]; at least one token); candidates[i]: a list, possibly empty, of caption token sequences for
        clip i (1-D int64 tensors or lists; caption tokens only: no prompt, no terminator, no padding).  Pass exactly one of image and
        query_features (encode_video's output: many candidate sets can be scored against one ViT pass).
        The clips are grouped by prompt length and chunked by clips_per_pass as generate does.  Per chunk: one prefix pass over the
        query slots and prompt[:-1] (text_decoder.forward_prefix), then ONE packed continuation pass (forward_continuation_packed,
        ops.attn_prefix_packed_fwd) in which candidate c is the rows [last prompt token, c_0 .. c_{n-1}] with the targets [c_0 ..
        c_{n-1}, termination]: the candidates lie end to end at their own lengths, so no padding row goes through the decoder or the
        LM head.  score_termination=False drops the last row (the terminator is not scored; an empty candidate is then an error).  One
        download per chunk; a candidate's sum is taken on the host in fp64, in position order, and stored as fp32.
        -> one dict per clip, in input order, of CPU tensors shaped like generate(..., return_scores=True)'s entries: sum_logprob [C_i]
        fp32, count [C_i] int32, token_logprob [C_i, Lmax_i] fp32 (zero-padded behind each candidate's count), and best =
        best_sample(sum_logprob, count, length_penalty), None for a clip without candidates.  The quantity is the one SampleScores
        records: the log-probability of every token up to and including the terminating one, from the raw logits, without constraints.
        A candidate's scores are bit-identical only at an equal row count of the pass: the GEMM dispatch depends on the number of rows
        (DESIGN.md sections 13, 17, 18, 20), which moves the logits in their last bf16 digit -- as for generate's scores."""
        if (image is None) == (query_features is None):
            raise ValueError("pass exactly one of image / query_features")
        if int(clips_per_pass) < 1:
            raise ValueError(f"clips_per_pass must be at least 1 (got {clips_per_pass})")
        Q, Hh = self.num_learnable_token, self.text_width
        ids_all, mask = text.input_ids, text.attention_mask
        n = ids_all.shape[0]
        if len(candidates) != n:
            raise ValueError(f"{len(candidates)} candidate lists for {n} clips")
        lengths = (mask.sum(-1) - 1).tolist()
        if any(pl < 1 for pl in lengths):
            raise ValueError(f"every clip needs a prompt of at least one token (prompt lengths {lengths})")
        cands = [[[int(t) for t in (c.tolist() if torch.is_tensor(c) else c)] for c in cl] for cl in candidates]
        if not score_termination and any(len(c) == 0 for cl in cands for c in cl):
            raise ValueError("an empty candidate has nothing to score with score_termination=False")
        with _eval_mode(self):
            qf = self._query_features(image, {"vit": {}, "pool": {}}) if query_features is None else query_features
            if qf.shape[0] != n * Q:
                raise ValueError(f"query features of {qf.shape[0] / Q:g} clips ({qf.shape[0]} rows of Q = {Q}) for {n} prompts")
            qf = qf.view(n, Q, Hh)
            _, term = self._termination(termination_id)
            host_ids = ids_all.tolist()                                          # the prompts' last tokens, on the host
            res = [None] * n
            for i in range(n):
                if not cands[i]:
                    res[i] = dict(sum_logprob=torch.zeros(0, dtype=torch.float32), count=torch.zeros(0, dtype=torch.int32),
                                  token_logprob=torch.zeros((0, 0), dtype=torch.float32), best=None)
            for pl, chunk in _prompt_length_chunks(lengths, clips_per_pass):
                clips = [i for i in chunk if cands[i]]
                if not clips:
                    continue
                rows_in, rows_tgt, cont_len = [], [], []
                for i in clips:
                    for c in cands[i]:
                        seq_in, seq_tgt = [host_ids[i][pl - 1]] + c, c + [term]
                        if not score_termination:
                            seq_in, seq_tgt = seq_in[:-1], seq_tgt[:-1]
                        rows_in += seq_in
                        rows_tgt += seq_tgt
                        cont_len.append(len(seq_in))
                dev = qf.device
                layout = ops.PackedLayout(cont_len, [len(cands[i]) for i in clips], device=dev)
                sel = torch.as_tensor(clips, dtype=torch.long, device=dev)
                prefix = self.text_decoder.forward_prefix(qf[sel].reshape(-1, Hh).contiguous(), ids_all[sel, :pl - 1].contiguous())
                both = torch.tensor([rows_in, rows_tgt], dtype=torch.long).to(dev)                       # one upload
                out = self.text_decoder.forward_continuation_packed(prefix, both[0], layout, labels=both[1])
                tlp = out["token_logprob"].cpu()                                                          # the chunk's one download
                at, k = 0, 0
                for i in clips:
                    C_i = len(cands[i])
                    lens = cont_len[k:k + C_i]
                    table = torch.zeros((C_i, max(lens)), dtype=torch.float32)
                    sums = []
                    for j, ln in enumerate(lens):
                        row = tlp[at:at + ln]
                        table[j, :ln] = row
                        acc = 0.0
                        for x in row.tolist():                               # fp64, in position order
                            acc += x
                        sums.append(acc)
                        at += ln
                    k += C_i
                    entry = dict(sum_logprob=torch.tensor(sums, dtype=torch.float64).to(torch.float32),
                                 count=torch.tensor(lens, dtype=torch.int32), token_logprob=table)
                    entry["best"] = best_sample(entry["sum_logprob"], entry["count"], length_penalty)
                    res[i] = entry
            return res


@contextlib.contextmanager
def _eval_mode(model):
    """the model in eval mode inside the block, back in the mode it was in behind it"""
    was = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was)


def _refuse_keyword_combinations(o):
    """generate's rules on which keywords go together, as functions of the keywords alone (o: a namespace of them), in one order: a
    call that breaks several gets the first one's message"""
    generation._check_weight_mode(o.decode_weights)
    for name, metric in (("consensus", o.consensus), ("rerank_by_consensus", o.rerank_by_consensus)):
        if metric is not None and metric not in generation.CONSENSUS_METRICS:
            raise ValueError(f"{name} must be one of {generation.CONSENSUS_METRICS} or None (got {metric!r})")
    beams = o.batched and not o.do_sample
    if o.consensus is not None:
        if not o.do_sample:
            raise ValueError("consensus needs do_sample=True (beam hypotheses: batched=True with rerank_by_consensus=)")
        if o.best_of:
            raise ValueError(f"consensus={o.consensus!r} does not combine with best_of=True: both choose the clip's one caption")
    if o.rerank_by_consensus is not None:
        if not beams:
            raise ValueError("rerank_by_consensus needs batched=True without do_sample (sampled captions: consensus=)")
        if o.rerank_by_logprob:
            raise ValueError(f"rerank_by_consensus={o.rerank_by_consensus!r} does not combine with rerank_by_logprob=True: both order the "
                             "clip's hypotheses")
        if o.allowed_phrases is not None:
            raise ValueError("rerank_by_consensus does not combine with allowed_phrases: the phrases of a closed vocabulary are "
                             "alternatives, not paraphrases")
    if int(o.beam_groups) != 1 and not beams:
        raise ValueError(f"beam_groups={o.beam_groups!r} needs batched=True without do_sample: the per-clip search and the samplers have no groups")
    if o.rerank_by_logprob and not beams:
        raise ValueError("rerank_by_logprob needs batched=True without do_sample (sampled captions: best_of=True)")
    if o.mixed_prompts:
        if o.do_sample:
            raise ValueError("mixed_prompts does not combine with do_sample: a sampled token is a function of its table column, "
                             "which the left padding would make depend on the longest prompt of the chunk (sampled captions over "
                             "prompts of different lengths: sample_mixed_prompts=True)")
        if not o.batched:
            raise ValueError("mixed_prompts needs batched=True: the per-clip search has one prompt per call")
        if o.kv_cache != "shared_prefix":
            raise ValueError(f'mixed_prompts needs kv_cache="shared_prefix" (got {o.kv_cache!r}): only the shared-prefix decode step '
                             "takes a prefix length per clip")
        if o.constrain_prompt:
            raise ValueError("mixed_prompts does not combine with constrain_prompt=True: the left padding of the token table would "
                             "count as prompt")
    if o.sample_mixed_prompts:
        if not o.do_sample:
            raise ValueError("sample_mixed_prompts needs do_sample=True (the beam search over prompts of different lengths: "
                             "mixed_prompts=True)")
        if o.kv_cache != "shared_prefix":
            raise ValueError(f'sample_mixed_prompts needs kv_cache="shared_prefix" (got {o.kv_cache!r}): only the shared-prefix decode '
                             "step takes a prefix length per clip")
    if o.inflight:
        if not o.do_sample:
            raise ValueError("inflight needs do_sample=True (beam search in flight: batched=True with beam_inflight=True; greedy "
                             "captions: do_sample=True with top_k=1)")
        if o.kv_cache != "shared_prefix":
            raise ValueError(f'inflight needs kv_cache="shared_prefix" (got {o.kv_cache!r}): only the shared-prefix decode step takes a '
                             "suffix position per clip")
    if o.beam_inflight:
        if o.do_sample:
            raise ValueError("beam_inflight does not combine with do_sample (sampled captions in flight: inflight=True)")
        if not o.batched:
            raise ValueError("beam_inflight needs batched=True: the per-clip search has one clip per call")
        if o.kv_cache != "shared_prefix":
            raise ValueError(f'beam_inflight needs kv_cache="shared_prefix" (got {o.kv_cache!r}): only the shared-prefix decode step takes '
                             "a suffix position per clip")
        if o.mixed_prompts:
            raise ValueError("beam_inflight does not combine with mixed_prompts=True: the in-flight search takes prompts of different "
                             "lengths as it is")
    if not (o.inflight or o.beam_inflight) and (o.max_new_tokens is not None or o.refill_min is not None):
        raise ValueError("max_new_tokens / refill_min belong to inflight=True (sampled captions) or beam_inflight=True (beam search)")


def _encode_phrase(tok, s):
    """the tokens of the string `s` alone: what the tokenizer makes of it without the opening and the closing token"""
    enc = tok([s], padding="longest", truncation=False, return_tensors="pt")
    ids = enc["input_ids"][0, :int(enc["attention_mask"][0].sum())].tolist()
    if ids and ids[0] == tok.tokenizer.bos:
        ids = ids[1:]
    if ids and ids[-1] == tok.tokenizer.eos:
        ids = ids[:-1]
    return ids


def _with_phrase_index(entry, trie, rows, prompt_len, term):
    """generate(allowed_phrases=, return_scores=True): the clip's score dict with phrase_index [rows] int64 (-1: no phrase)"""
    if trie is None:
        return entry
    return dict(entry, phrase_index=torch.tensor([trie.lookup(generation.generated_part(r, prompt_len, term)) for r in rows.tolist()],
                                                 dtype=torch.int64))


def _prompt_length_chunks(lengths, per_chunk):
    """the clips grouped by prompt length (ascending), each group cut into chunks of at most per_chunk clips in input order
    -> (prompt length, clip indices) per chunk: one lockstep search, or one scoring pass"""
    for pl in sorted(set(lengths)):
        group = [i for i, x in enumerate(lengths) if x == pl]
        for c in range(0, len(group), int(per_chunk)):
            yield pl, group[c:c + int(per_chunk)]


def _clip_chunks(lengths, per_chunk, by_length: bool):
    """generate's lockstep chunks of at most per_chunk clips -> (prompt length, clip indices) per chunk, the clips grouped by prompt
    length (_prompt_length_chunks); or, by_length=False, (the clips' prompt lengths, clip indices) in input order: the mixed modes"""
    if by_length:
        for pl, chunk in _prompt_length_chunks(lengths, per_chunk):
            yield int(pl), chunk
    else:
        for c in range(0, len(lengths), int(per_chunk)):
            chunk = list(range(c, min(c + int(per_chunk), len(lengths))))
            yield [int(lengths[i]) for i in chunk], chunk


def _normalised(sum_logprob, count, length_penalty) -> float:
    """sum_logprob / count ** length_penalty in fp64; -inf for a sequence of no tokens"""
    return float(sum_logprob) / float(count) ** float(length_penalty) if count > 0 else -math.inf


def best_sample(sum_logprob, count, length_penalty: float = 1.0) -> int:
    """argmax_s sum_logprob[s] / count[s] ** length_penalty in fp64; a tie goes to the lowest index, a sample with count 0 scores -inf"""
    best, best_score = 0, -math.inf
    for s, (lp, c) in enumerate(zip(sum_logprob.tolist(), count.tolist())):
        score = _normalised(lp, c, length_penalty)
        if score > best_score:
            best, best_score = s, score
    return best


def _download_rows(parts):
    """device tensors [R, c_k] of any dtypes -> their CPU copies in ONE device-to-host copy: the rows are packed byte-wise side by side"""
    R = parts[0].shape[0]
    packed = torch.cat([p.contiguous().view(torch.uint8).view(R, -1) for p in parts], dim=1).cpu()
    out, at = [], 0
    for p in parts:
        nb = p.shape[1] * p.element_size()
        out.append(packed[:, at:at + nb].contiguous().view(p.dtype).view(R, p.shape[1]))
        at += nb
    return out


def _download_scored(tokens, sc, width: int, extra=()):
    """tokens int64 [R, width] (padded) and a generation.SampleScores -> CPU (tokens, token_logprob [R, width] padded with 0,
    sum_logprob [R], count [R]) in ONE device-to-host copy (_download_rows); extra: further [R, c] device tensors that ride along and
    follow the four in the result"""
    R = tokens.shape[0]
    tlp = torch.zeros((R, width), dtype=torch.float32, device=tokens.device)
    w = min(width, sc.token_logprob.shape[1])
    tlp[:, :w] = sc.token_logprob[:, :w]
    out = _download_rows((tokens.contiguous(), tlp, sc.sum_logprob.view(R, 1), sc.count.view(R, 1)) + tuple(extra))
    return (out[0], out[1], out[2].view(R), out[3].view(R)) + tuple(out[4:])


def _consensus_samples(toks, sc, starts, N: int, term: int, width: int, metric: str):
    """generate(consensus=): toks int64 [R, width] on the device (padded; N rows per clip, the generated part of row r from column
    starts[r] on), sc the chunk's generation.SampleScores or None -> CPU (tokens, token_logprob, sum_logprob, count -- None without
    sc --, [(U [N] fp64, index) per clip]).  The overlap counts of every clip's N x N pairs are taken on the device
    (ops.caption_overlap) and come down in the chunk's ONE download, N * 5 integers beside every row; the utilities and the choice are
    fp64 on the host (generation.consensus_utility / consensus_choice)."""
    R = toks.shape[0]
    toks = toks.contiguous()
    ln, _, counts = ops.caption_overlap(toks, [int(s) for s in starts], list(range(0, R + 1, N)), term=term)
    extra = (ln.view(R, 1), counts.view(R, N * 5))         # clip j's pairs (a, b) row-major: row j * N + a holds its N pairs
    if sc is None:
        toks, ln, counts = _download_rows((toks,) + extra)
        tlp = slp = cnt = None
    else:
        toks, tlp, slp, cnt, ln, counts = _download_scored(toks, sc, width, extra)
    picks = []
    for j in range(R // N):
        rows = slice(j * N, (j + 1) * N)
        u = generation.consensus_utility(counts[rows].reshape(N, N, 5), ln[rows].view(N), ln[rows].view(N), metric)
        picks.append(generation.consensus_choice(u))
    return toks, tlp, slp, cnt, picks


def _consensus_rows(res, starts, term: int, metric: str, device):
    """generate(rerank_by_consensus=): res[i] int64 [n_i, L_i] on the CPU (clip i's hypotheses, the generated part from column
    starts[i] on) -> [(U [n_i] fp64, index) per clip].  ONE table of all the clips' rows (padded with `term` to the widest), one
    upload, one ops.caption_overlap call over ragged groups with a start per row, one download."""
    counts_of = [int(r.shape[0]) for r in res]
    W = max([int(r.shape[1]) for r in res] + [1])
    table = torch.full((sum(counts_of), W), int(term), dtype=torch.int64)
    begin, row_start = [0], []
    for r, s in zip(res, starts):
        table[begin[-1]:begin[-1] + r.shape[0], :r.shape[1]] = r
        begin.append(begin[-1] + int(r.shape[0]))
        row_start += [int(s)] * int(r.shape[0])
    if not table.shape[0]:
        return [generation.consensus_choice(torch.zeros((0, 0), dtype=torch.float64)) for _ in res]
    ln, _, counts = ops.caption_overlap(table.to(device), row_start, begin, term=term)
    pair_begin = [0]
    for c in counts_of:
        pair_begin.append(pair_begin[-1] + c * c)
    flat = torch.cat([ln.view(-1), counts.view(-1)]).cpu()            # one download
    ln, counts = flat[:table.shape[0]], flat[table.shape[0]:].view(-1, 5)
    picks = []
    for i, c in enumerate(counts_of):
        u = generation.consensus_utility(counts[pair_begin[i]:pair_begin[i + 1]].reshape(c, c, 5), ln[begin[i]:begin[i + 1]],
                                         ln[begin[i]:begin[i + 1]], metric)
        picks.append(generation.consensus_choice(u))
    return picks


def synthetic_gencls_model(shapes, kind: str, num_classes: int = 2, device="cuda", num_frames=None):
    """Random-init ITM ("itm") or classification ("cls") model from a PathConfig-like shapes object."""
    vis = dict(img_size=shapes.img_size, patch_size=shapes.patch_size, depth=shapes.vit_depth,
               num_frames=num_frames or shapes.num_frames, embed_dim=shapes.vit_dim, num_heads=shapes.vit_heads,
               mlp_ratio=shapes.vit_mlp_ratio, clip_model=True)
    txt = GPT3Config(vocab_size=shapes.vocab, hidden_size=shapes.hidden, ffn_hidden_size=shapes.ffn,
                     num_hidden_layers=shapes.layers, num_attention_heads=shapes.heads, max_position_embeddings=shapes.max_pos,
                     layernorm_epsilon=shapes.gpt_ln_eps)
    klass = {"itm": DistributedGPT3_Retrieval_Cls, "cls": DistributedGPT3_Cls, "caption": DistributedGPT3_Caption}[kind]
    return klass({"num_learnable_token": shapes.num_queries, "_synthetic": True, "use_cls": kind != "caption", "num_classes": num_classes},
                 visual_cfg=vis, text_cfg=txt, device=device)
