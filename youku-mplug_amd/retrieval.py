"""DistributedGPT3_Retrieval (ITC) on the gfx950 kernels -- drop-in for models/distributed_gpt3.py:817-985
(BASELINE.json configs[4]).

video feature = L2-normalised vision_proj(ViT cls);  text feature = L2-normalised text_proj(hidden state at the last
valid token of a text-only GPT forward);  features (+ sample ids) are all-gathered over the data-parallel group
(models/distributed_utils.py:285-311: all-gather forward, reduce-scatter backward -- here one RCCL
all_gather_into_tensor / reduce_scatter_tensor each way);  sim/temp;  soft-target cross-entropy in both directions.
The decoder is frozen and nothing trainable sits below the text hidden state, so the text tower has NO backward.
"""
from __future__ import annotations

import json
from typing import Optional

import torch
import torch.distributed as dist
from torch import nn

from . import ops
from .gpt3 import DistributedGPT3, GPT3Config
from .vision import AttentionPool, Linear, TimeSformer, _param, grad_of


def gather_cat(x: torch.Tensor, group=None) -> torch.Tensor:
    """cat(all_gather(x)) along dim 0 (identity at world size 1)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return x
    out = torch.empty((dist.get_world_size(group) * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    dist.all_gather_into_tensor(out, x.contiguous(), group=group)
    return out


def reduce_scatter_sum(g_all: torch.Tensor, group=None) -> torch.Tensor:
    """Backward of gather_cat: this rank's slice of the sum over ranks (models/distributed_utils.py:299-311)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return g_all
    w, r = dist.get_world_size(group), dist.get_rank(group)
    n = g_all.shape[0] // w
    if dist.get_backend(group) == "nccl":
        out = torch.empty((n,) + tuple(g_all.shape[1:]), dtype=g_all.dtype, device=g_all.device)
        dist.reduce_scatter_tensor(out, g_all.contiguous(), op=dist.ReduceOp.SUM, group=group)
        return out
    g = g_all.clone()            # gloo has no reduce_scatter: all-reduce and slice (the reference falls back similarly)
    dist.all_reduce(g, op=dist.ReduceOp.SUM, group=group)
    return g[r * n:(r + 1) * n].contiguous()


class _RetrievalStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, model, video, ids, mask, idx):
        loss, tape = model._forward_pipeline(video, ids, mask, idx)
        ctx.model, ctx.tape = model, tape
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        ctx.model._backward_pipeline(ctx.tape, grad_loss.contiguous().float())
        ctx.tape = None
        return torch.zeros(1, device=grad_loss.device), None, None, None, None, None


class DistributedGPT3_Retrieval(nn.Module):
    def __init__(self, config: Optional[dict] = None, tokenizer=None, *, visual_cfg: Optional[dict] = None,
                 text_cfg: Optional[GPT3Config] = None, device="cuda"):
        super().__init__()
        config = dict(config or {})
        self.tokenizer = tokenizer
        if visual_cfg is None:
            visual_cfg = json.load(open(config["visual_cfg"], "r"))
        if text_cfg is None:
            text_cfg = GPT3Config.from_json_file(config["text_cfg"])
        self.visual_encoder = TimeSformer(
            img_size=visual_cfg["img_size"], num_frames=config.get("num_frames", visual_cfg.get("num_frames", 4)),
            patch_size=visual_cfg["patch_size"], embed_dim=visual_cfg["embed_dim"], depth=visual_cfg["depth"],
            num_heads=visual_cfg["num_heads"], mlp_ratio=visual_cfg["mlp_ratio"], eps=1e-6, init_std=0.015,
            clip_model=visual_cfg.get("clip_model", False), device=device)                                   # :825-841
        if config.get("text_decoder") and not config.get("_synthetic", False):
            self.text_decoder = DistributedGPT3(model_dir=config["text_decoder"], device=device)            # :864-870
        else:
            self.text_decoder = DistributedGPT3(config=text_cfg, device=device)
        if config.get("freeze_vit", False):
            for name, p in self.visual_encoder.named_parameters():
                if not any(x in name for x in ("time", "temporal")):
                    p.requires_grad = False
        if not config.get("freeze_text_decoder", True):
            raise NotImplementedError("the gfx950 path implements the frozen-decoder recipe "
                                      "(configs/retrieval/retrieval_gpt3_1.3B_youku_v0.yaml: freeze_text_decoder: true)")
        for p in self.text_decoder.parameters():
            p.requires_grad = False
        lora_rank = int(config.get("lora_rank", 0) or 0)       # LoRA adapters on the frozen decoder: 0 = off
        if lora_rank:
            self.text_decoder.add_lora(lora_rank, config.get("lora_alpha", None))
        self.vision_width, self.text_width = visual_cfg["embed_dim"], self.text_decoder.config.hidden_size
        self.num_learnable_token = config.get("num_learnable_token", 256)
        # parameters that exist in the reference state-dict but are unused by the ITC forward (:942-945 commented out)
        self.learnable_queries = _param(1, self.num_learnable_token, self.vision_width, std=0.015, device=device)
        self.attn_pool = AttentionPool(self.vision_width, num_heads=visual_cfg["num_heads"], mlp_ratio=visual_cfg["mlp_ratio"],
                                       eps=1e-6, std=0.02, device=device)
        self.visual_fc = Linear(self.vision_width, self.text_width, std=0.015, device=device)
        self.visual_norm = nn.Identity()
        embed_dim = config.get("contrastive_embed_dim", 256)                                                # :904-907
        assert embed_dim % 8 == 0
        self.vision_proj = Linear(self.vision_width, embed_dim, device=device)
        self.text_proj = Linear(self.text_width, embed_dim, device=device)
        self.temp = nn.Parameter(torch.ones([], dtype=torch.bfloat16, device=device) * config.get("temp", 0.07))
        self._anchor = torch.zeros(1, device=device, requires_grad=True)
        self.on_stage_grads_ready = None
        self.process_group = None

    def no_weight_decay(self):
        return {"visual_encoder.pos_embed", "visual_encoder.cls_token", "visual_encoder.temporal_embed"}

    def unused_parameters(self):
        """No gradient ever reaches these in the ITC forward: the engine must not update (weight-decay) them."""
        return [self.learnable_queries, *self.attn_pool.parameters(), *self.visual_fc.parameters()]

    # ------------------------------------------------------------------ towers
    def _vision_tower(self, video, tape):
        B = video.shape[0]
        D, E = self.vision_width, self.vision_proj.out_features
        emb = self.visual_encoder.forward_features(video.to(torch.bfloat16), tape["vit"])
        S = emb.shape[0] // B
        cls = torch.empty((B, D), dtype=torch.bfloat16, device=emb.device)
        ops.copy_rows(emb, cls, B, D, smap=(1, S, 0))                                                       # image_embeds[:, 0]
        vp = ops.gemm(cls, self.vision_proj.weight, B, E, D, bias=self.vision_proj.bias)
        vf, vn = ops.l2norm_fwd(vp, B, E)
        tape.update(B=B, S=S, cls=cls, vp=vp, vn=vn, vf=vf)
        return vf

    def _text_tower(self, ids, mask, tape):
        B, L = ids.shape
        H, E = self.text_width, self.text_proj.out_features
        gpt_tape = {}
        out = self.text_decoder.forward_lm(None, ids, None, None, gpt_tape, hidden_only=True)
        last = mask.sum(dim=-1) - 1                                                                         # :958-959
        rows = torch.arange(B, device=ids.device) * L + last
        if self.text_decoder.lora_live():       # the text tower is no longer frozen below `pooled`: keep the pass for _backward_pipeline
            tape.update(gpt_text=gpt_tape, text_rows=rows.contiguous(), text_L=L)
        pooled = ops.gather_rows(out["last_hidden_state"].reshape(B * L, H), rows.contiguous(), B, H)
        tp = ops.gemm(pooled, self.text_proj.weight, B, E, H, bias=self.text_proj.bias)
        tf, tn = ops.l2norm_fwd(tp, B, E)
        tape.update(pooled=pooled, tp=tp, tn=tn, tf=tf)
        return tf

    @torch.no_grad()
    def extract_vision_feature(self, image):
        return self._vision_tower(image, {"vit": {}})

    @torch.no_grad()
    def extract_text_feature(self, text):
        return self._text_tower(text.input_ids, text.attention_mask, {})

    # ------------------------------------------------------------------ search
    @torch.no_grad()
    def search_videos(self, text, index: "RetrievalIndex", k: int, **how):
        """-> (scores fp32 [B, k], indices int64 [B, k]): the k best rows of a video-feature index for each tokenised title; `how`:
        the keywords of RetrievalIndex.search (scale, use_prior, normalised)"""
        return index.search(self.extract_text_feature(text), k, **how)

    @torch.no_grad()
    def search_texts(self, video, index: "RetrievalIndex", k: int, **how):
        """-> (scores, indices): the k best rows of a text-feature index for each clip; `how` as in search_videos"""
        return index.search(self.extract_vision_feature(video), k, **how)

    # ------------------------------------------------------------------ pipelines
    def _forward_pipeline(self, video, ids, mask, idx):
        tape = {"vit": {}}
        vf = self._vision_tower(video, tape)
        tf = self._text_tower(ids, mask, tape)
        B, E = vf.shape
        g = self.process_group
        v_all, t_all = gather_cat(vf, g), gather_cat(tf, g)                                                 # :962-963
        ids_loc = idx.reshape(-1).contiguous()
        ids_all = gather_cat(ids_loc, g)                                                                    # :964
        WB = v_all.shape[0]
        assert WB % 8 == 0, "global batch must be a multiple of 8 for the similarity GEMMs"
        inv_temp = (1.0 / self.temp.detach().float()).reshape(1)
        sim_i2t = ops.gemm(vf, t_all, B, WB, E, out_f32=True, alpha_dev=inv_temp)                           # :966
        sim_t2i = ops.gemm(tf, v_all, B, WB, E, out_f32=True, alpha_dev=inv_temp)                           # :967
        scale = 0.5 / B                                                                                     # mean over rows, /2 (:976-978)
        l1, ds1, dt1 = ops.soft_target_ce(sim_i2t, ids_loc, ids_all, scale, B, WB)
        l2, ds2, dt2 = ops.soft_target_ce(sim_t2i, ids_loc, ids_all, scale, B, WB)
        loss = (l1.sum() + l2.sum()) * scale
        tape.update(v_all=v_all, t_all=t_all, ds1=ds1, ds2=ds2, dts=dt1.sum() + dt2.sum(), inv_temp=inv_temp, WB=WB, E=E)
        return loss, tape

    def _backward_pipeline(self, tape, grad_loss):
        B, S, E, WB = tape["B"], tape["S"], tape["E"], tape["WB"]
        D, H = self.vision_width, self.text_width
        g = self.process_group
        coef = (tape["inv_temp"] * grad_loss.reshape(1)).contiguous()
        vf, tf, v_all, t_all, ds1, ds2 = tape["vf"], tape["tf"], tape["v_all"], tape["t_all"], tape["ds1"], tape["ds2"]
        dv = ops.gemm(ds1, t_all, B, E, WB, trans_b=True, alpha_dev=coef)                                   # d sim_i2t / d v
        dt_all = ops.gemm(ds1, vf, WB, E, B, trans_a=True, trans_b=True, alpha_dev=coef)                    # d sim_i2t / d t_all
        dt = ops.gemm(ds2, v_all, B, E, WB, trans_b=True, alpha_dev=coef)
        dv_all = ops.gemm(ds2, tf, WB, E, B, trans_a=True, trans_b=True, alpha_dev=coef)
        dv = ops.add(dv, reduce_scatter_sum(dv_all, g))                                                     # all_gather backward
        dt = ops.add(dt, reduce_scatter_sum(dt_all, g))
        # d temp: sim = raw / temp  ->  dL/dtemp = -(1/temp) * sum(dsim * sim)
        grad_of(self.temp).copy_((-(tape["dts"]) * tape["inv_temp"][0] * grad_loss.reshape(())).to(torch.bfloat16))
        # text head (no backward below `pooled`: frozen decoder)
        dtp = ops.l2norm_bwd(dt, tape["tp"], tape["tn"], B, E)
        ops.colsum(dtp, B, E, out=grad_of(self.text_proj.bias))
        ops.gemm(dtp, tape["pooled"], E, H, B, trans_a=True, trans_b=True, out=grad_of(self.text_proj.weight))
        if "gpt_text" in tape:                  # live LoRA adapters: the text tower's backward, seeded at the pooled rows
            dpooled = ops.gemm(dtp, self.text_proj.weight, B, H, E, trans_b=True)
            dlh = torch.zeros((B * tape["text_L"], H), dtype=torch.bfloat16, device=dtp.device)
            ops.scatter_rows(dpooled, tape["text_rows"], dlh, B, H)
            self.text_decoder.backward_lm(tape["gpt_text"], None, d_last_hidden=dlh)
        # vision head
        dvp = ops.l2norm_bwd(dv, tape["vp"], tape["vn"], B, E)
        ops.colsum(dvp, B, E, out=grad_of(self.vision_proj.bias))
        ops.gemm(dvp, tape["cls"], E, D, B, trans_a=True, trans_b=True, out=grad_of(self.vision_proj.weight))
        dcls = ops.gemm(dvp, self.vision_proj.weight, B, D, E, trans_b=True)
        if self.on_stage_grads_ready is not None:
            self.on_stage_grads_ready("head")
        demb = torch.zeros((B * S, D), dtype=torch.bfloat16, device=dcls.device)
        ops.copy_rows(dcls, demb, B, D, dmap=(1, S, 0))
        self.visual_encoder.backward_features(demb, tape["vit"])

    @torch.no_grad()
    def forward_backward(self, image, text, idx):
        """forward + backward without autograd (see DistributedGPT3_Pretrain.forward_backward): the capturable form of the step"""
        loss, tape = self._forward_pipeline(image, text.input_ids, text.attention_mask, idx)
        self._backward_pipeline(tape, torch.ones((), dtype=torch.float32, device=loss.device))
        return loss

    def forward(self, image, text, idx):
        ids, mask = text.input_ids, text.attention_mask
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _RetrievalStep.apply(self._anchor, self, image, ids, mask, idx)
        return self._forward_pipeline(image, ids, mask, idx)[0]


def synthetic_retrieval_model(shapes, device="cuda", num_frames=None, embed_dim=256) -> DistributedGPT3_Retrieval:
    vis = dict(img_size=shapes.img_size, patch_size=shapes.patch_size, depth=shapes.vit_depth,
               num_frames=num_frames or shapes.num_frames, embed_dim=shapes.vit_dim, num_heads=shapes.vit_heads,
               mlp_ratio=shapes.vit_mlp_ratio, clip_model=True)
    txt = GPT3Config(vocab_size=shapes.vocab, hidden_size=shapes.hidden, ffn_hidden_size=shapes.ffn,
                     num_hidden_layers=shapes.layers, num_attention_heads=shapes.heads, max_position_embeddings=shapes.max_pos,
                     layernorm_epsilon=shapes.gpt_ln_eps)
    return DistributedGPT3_Retrieval({"num_learnable_token": shapes.num_queries, "_synthetic": True, "contrastive_embed_dim": embed_dim,
                                      "num_frames": num_frames or shapes.num_frames}, visual_cfg=vis, text_cfg=txt, device=device)


class _FeatureIndex:
    """Storage shared by the two indexes: items of shape `_item` appended in order into a buffer that grows geometrically.
    storage="bf16" keeps the rows as they come.  storage="fp8" keeps e4m3 codes (one byte per element) and one power-of-two fp32
    scale per row, quantised on the device by ops.quantize_rows_e4m3 as the rows are added: half the bytes, searched by the *_q8
    ops, whose results are bit for bit those of the bf16 ops on dequantized() (include/mpv.h, "Searches over an FP8 gallery")."""

    def _init_storage(self, item, device, capacity, storage="bf16"):
        if storage not in ("bf16", "fp8"):
            raise ops._lib.MpvError(f"{type(self).__name__}: storage must be 'bf16' or 'fp8' (got {storage!r})")
        self._item, self.device, self.size, self.storage = tuple(item), torch.device(device), 0, storage
        self._rows = self._scales = None
        self._allocate(max(int(capacity), 1))

    def _allocate(self, capacity):
        """storage for `capacity` items, the first `size` of them copied over"""
        dtype = torch.bfloat16 if self.storage == "bf16" else torch.uint8
        rows = torch.empty((capacity,) + self._item, dtype=dtype, device=self.device)
        scales = torch.empty((capacity,) + self._item[:-1], dtype=torch.float32, device=self.device) if self.storage == "fp8" else None
        if self.size:
            rows[:self.size].copy_(self._rows[:self.size])
            if scales is not None:
                scales[:self.size].copy_(self._scales[:self.size])
        self._rows, self._scales = rows, scales

    def __len__(self):
        return self.size

    @property
    def capacity(self):
        return self._rows.shape[0]

    @property
    def features(self):
        """the items added so far: a view of the storage, bf16 [size, *item shape]"""
        if self.storage != "bf16":
            raise ops._lib.MpvError(f"{type(self).__name__}.features: an fp8 index keeps codes and scales (.codes, .scales); "
                                    "dequantized() builds the bf16 rows, at twice the index's bytes")
        return self._rows[:self.size]

    def _fp8(self, what):
        if self.storage != "fp8":
            raise ops._lib.MpvError(f"{type(self).__name__}.{what}: only an index with storage='fp8' has it")

    @property
    def codes(self):
        """fp8 storage: the e4m3 codes added so far, a view of the storage, uint8 [size, *item shape]"""
        self._fp8("codes")
        return self._rows[:self.size]

    @property
    def scales(self):
        """fp8 storage: the row scales added so far, a view of the storage, fp32 [size] ([size, group] for grouped items)"""
        self._fp8("scales")
        return self._scales[:self.size]

    def dequantized(self):
        """fp8 storage: the bf16 rows the index stands for, deq(code) * scale (exact: the scales are powers of two) -- a new tensor of
        twice the index's bytes, for checks and re-scoring, not for searching"""
        self._fp8("dequantized()")
        return (self.codes.view(torch.float8_e4m3fn).float() * self.scales[..., None]).to(torch.bfloat16)

    @property
    def nbytes(self):
        """bytes of the items added so far (rows, and scales when there are any)"""
        n = self._rows[:self.size].numel() * self._rows.element_size()
        return n + (self._scales[:self.size].numel() * 4 if self._scales is not None else 0)

    def _append(self, features):
        n, first = features.shape[0], self.size
        if first + n > self.capacity:
            self._allocate(max(2 * self.capacity, first + n))
        if self.storage == "bf16":
            self._rows[first:first + n].copy_(features)
        elif n:
            codes, scale = ops.quantize_rows_e4m3(features.contiguous().reshape(-1, self._item[-1]))
            self._rows[first:first + n].copy_(codes.view((n,) + self._item))
            self._scales[first:first + n].copy_(scale.view((n,) + self._item[:-1]))
        self.size = first + n
        return first

    def _targets(self, target, q, noun):
        """target -> int64 [Nq, n_t] on the queries' device, every entry in [-1, size)"""
        target = torch.as_tensor(target, dtype=torch.int64, device=q.device).reshape(q.shape[0], -1)
        if target.numel() and (int(target.max()) >= self.size or int(target.min()) < -1):
            raise ops._lib.MpvError(f"{type(self).__name__}.rank: target {noun} must be in [-1, {self.size}) "
                                    f"(got {int(target.min())} .. {int(target.max())})")
        return target


class _RowTerms:
    """What a RetrievalIndex keeps per row once priors, exclusions or a normaliser are used (never before): each of `prior` (fp32),
    `excluded` (bool) and `lse` (fp32, with the `bank` and `beta` it was fitted on) is storage of the index's capacity or None;
    `cache` holds the effective terms built from them, per (use_prior, normalised), until one of the three changes."""

    def __init__(self):
        self.prior = self.excluded = self.lse = self.bank = self.beta = None
        self.cache = {}


class RetrievalIndex(_FeatureIndex):
    """Gallery of L2-normalised bf16 feature rows (what extract_vision_feature / extract_text_feature return) searched on the
    device by ops.sim_topk / ops.sim_rank: the [queries, gallery] score matrix is never built.  Rows keep the order they were
    added in; row i of the index is the i-th feature ever added.  Storage grows geometrically, so `add` does not re-allocate
    per call.  Order rule of both searches: higher score first, equal scores by the lower row index (include/mpv.h).

    Per-row terms (include/mpv.h, "Searches with per-row priors"): a prior added to a row's score (set_prior), rows left out
    (exclude / include) and the inverted-softmax normaliser lse[g] = log sum_b exp(beta * <b, g>) over a bank of queries
    (fit_normaliser; QB-Norm, or dual softmax when the bank is the test queries themselves).  A search then scores row g as
    scale * <q, g> + prior[g] - lse[g], or not at all when it is excluded, through ops.sim_topk_prior / ops.sim_rank_prior.  An
    index on which none of the three was ever used runs the plain ops and keeps nothing per row."""

    def __init__(self, dim: int, device="cuda", capacity: int = 1024, storage: str = "bf16"):
        if dim % 32 != 0 or not 32 <= dim <= 1024:
            raise ops._lib.MpvError(f"RetrievalIndex: dim ({dim}) must be a multiple of 32 in [32, 1024]")
        self.dim = dim
        self._init_storage((dim,), device, capacity, storage)

    def _check(self, feats, what):
        if not torch.is_tensor(feats) or feats.dtype != torch.bfloat16:
            raise ops._lib.MpvError(f"RetrievalIndex.{what}: features must be a bfloat16 tensor (the towers emit bf16; got "
                                    f"{getattr(feats, 'dtype', type(feats))})")
        if feats.dim() != 2 or feats.shape[1] != self.dim:
            raise ops._lib.MpvError(f"RetrievalIndex.{what}: features must be [rows, {self.dim}] (got {tuple(feats.shape)})")

    def add(self, features):
        """append rows; -> the index of the first one.  With per-row terms in use the new rows get prior 0, are not excluded, and
        get their normaliser from the bank that was fitted -- for the new rows only: lse[g] depends on row g alone, bit for bit."""
        self._check(features, "add")
        first = self._append(features)
        terms = getattr(self, "_terms", None)
        if terms is not None and self.size > first:
            new = slice(first, self.size)
            if terms.prior is not None:
                terms.prior[new] = 0
            if terms.excluded is not None:
                terms.excluded[new] = False
            if terms.lse is not None:
                terms.lse[new] = self._bank_lse(terms.bank, terms.beta, new)
            terms.cache.clear()
        return first

    # ------------------------------------------------------------------ per-row terms
    def _allocate(self, capacity):
        super()._allocate(capacity)
        terms = getattr(self, "_terms", None)
        if terms is not None:
            for name in ("prior", "excluded", "lse"):
                old = getattr(terms, name)
                if old is not None:
                    grown = torch.zeros(capacity, dtype=old.dtype, device=self.device)
                    grown[:self.size].copy_(old[:self.size])
                    setattr(terms, name, grown)

    def _row_terms(self, name=None, dtype=torch.float32):
        """the per-row state, created on first use; `name`: that array too, zeros of the index's capacity"""
        terms = getattr(self, "_terms", None)
        if terms is None:
            terms = self._terms = _RowTerms()
        if name is not None and getattr(terms, name) is None:
            setattr(terms, name, torch.zeros(self.capacity, dtype=dtype, device=self.device))
        terms.cache.clear()
        return terms

    def _rows_arg(self, rows, what):
        rows = torch.as_tensor(rows, dtype=torch.int64, device=self.device).reshape(-1)
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= self.size):
            raise ops._lib.MpvError(f"RetrievalIndex.{what}: rows must be in [0, {self.size}) (got {int(rows.min())} .. {int(rows.max())})")
        return rows

    def set_prior(self, values, rows=None):
        """prior[rows] = values (fp32; rows None: all rows, values a scalar or one per row).  -inf leaves a row out, as exclude does.
        Rows added later get 0."""
        values = torch.as_tensor(values, dtype=torch.float32, device=self.device)
        if torch.isnan(values).any():
            raise ops._lib.MpvError("RetrievalIndex.set_prior: a prior must not be NaN")
        if rows is None:
            if values.dim() > 0 and tuple(values.shape) != (self.size,):
                raise ops._lib.MpvError(f"RetrievalIndex.set_prior: values must be a scalar or of shape ({self.size},) "
                                        f"(got {tuple(values.shape)})")
            self._row_terms("prior").prior[:self.size] = values
        else:
            rows = self._rows_arg(rows, "set_prior")
            if values.dim() > 0 and values.numel() != rows.numel():
                raise ops._lib.MpvError(f"RetrievalIndex.set_prior: {values.numel()} values for {rows.numel()} rows")
            self._row_terms("prior").prior[rows] = values.reshape(-1) if values.dim() > 0 else values

    @property
    def prior(self):
        """the priors of the rows added so far (a view, fp32 [size]), or None when none was ever set"""
        terms = getattr(self, "_terms", None)
        return None if terms is None or terms.prior is None else terms.prior[:self.size]

    def clear_prior(self):
        if self.prior is not None:
            self._row_terms().prior = None

    def exclude(self, rows):
        """leave these rows out of every search and rank from now on (as results, as competitors and as targets)"""
        rows = self._rows_arg(rows, "exclude")
        self._row_terms("excluded", torch.bool).excluded[rows] = True

    def include(self, rows):
        """take rows back in that exclude() left out"""
        rows = self._rows_arg(rows, "include")
        if getattr(self, "_terms", None) is not None and self._terms.excluded is not None:
            self._row_terms().excluded[rows] = False

    @property
    def excluded(self):
        """bool [size]: the rows that are left out"""
        terms = getattr(self, "_terms", None)
        if terms is None or terms.excluded is None:
            return torch.zeros(self.size, dtype=torch.bool, device=self.device)
        return terms.excluded[:self.size]

    def _bank_lse(self, bank, beta, rows):
        if self.storage == "fp8":
            return ops.sim_bank_lse_q8(bank, self._rows[rows], self._scales[rows].contiguous(), beta)
        return ops.sim_bank_lse(bank, self._rows[rows], beta)

    def fit_normaliser(self, bank_features, beta):
        """inverted softmax over a bank of queries, bf16 [n, dim]: keeps the bank and beta, computes lse[g] = log sum_b
        exp(beta * <b, g>) for the rows present (ops.sim_bank_lse); `add` computes it for new rows.  Searches are then normalised by
        default: scores beta * <q, g> - lse[g]."""
        self._check(bank_features, "fit_normaliser")
        beta = float(beta)
        if bank_features.shape[0] == 0 or beta != beta or beta in (float("inf"), float("-inf")):
            raise ops._lib.MpvError(f"RetrievalIndex.fit_normaliser: a non-empty bank and a finite beta are needed (got "
                                    f"{bank_features.shape[0]} rows, beta {beta})")
        bank = bank_features.detach().to(self.device).contiguous().clone()
        lse = self._bank_lse(bank, beta, slice(0, self.size)) if self.size else None
        terms = self._row_terms("lse")
        terms.bank, terms.beta = bank, beta
        if lse is not None:
            terms.lse[:self.size] = lse

    @property
    def normaliser(self):
        """(bank bf16 [n, dim], beta, lse fp32 [size]) of fit_normaliser, or None"""
        terms = getattr(self, "_terms", None)
        return None if terms is None or terms.lse is None else (terms.bank, terms.beta, terms.lse[:self.size])

    def clear_normaliser(self):
        if self.normaliser is not None:
            terms = self._row_terms()
            terms.lse = terms.bank = terms.beta = None

    def _effective(self, what, scale, use_prior, normalised, always=False):
        """-> (term fp32 [size] or None, scale): the per-row term of this call, (prior) + (-lse) + (-inf where excluded), and the
        scale that goes with it (beta when normalised).  None: nothing applies and the plain op serves (`always`: a term of zeros
        instead, for a rank with a scale, which only the prior entry applies)."""
        terms = getattr(self, "_terms", None)
        has_prior = terms is not None and terms.prior is not None
        has_norm = terms is not None and terms.lse is not None
        for name, asked, has, how in (("use_prior", use_prior, has_prior, "set_prior"), ("normalised", normalised, has_norm, "fit_normaliser")):
            if asked and not has:
                raise ops._lib.MpvError(f"RetrievalIndex.{what}: {name}=True, but {how}() was never called on this index")
        use_prior = has_prior if use_prior is None else bool(use_prior)
        normalised = has_norm if normalised is None else bool(normalised)
        if normalised:
            if scale is not None:
                raise ops._lib.MpvError(f"RetrievalIndex.{what}: a normalised search scores beta * <q, g> - lse[g] with the beta of "
                                        f"fit_normaliser ({terms.beta}); pass no scale, or normalised=False")
            scale = terms.beta
        if not (use_prior or normalised or always or (terms is not None and terms.excluded is not None)):
            return None, scale
        if terms is None:
            terms = self._row_terms()
        key = (use_prior, normalised)
        if key not in terms.cache:
            term = torch.zeros(self.size, dtype=torch.float32, device=self.device)
            if use_prior:
                term += terms.prior[:self.size]
            if normalised:
                term -= terms.lse[:self.size]
            if terms.excluded is not None:
                term.masked_fill_(terms.excluded[:self.size], float("-inf"))
            terms.cache[key] = term
        return terms.cache[key], scale

    def search(self, query_features, k: int, scale=None, use_prior=None, normalised=None):
        """-> (scores fp32 [Nq, k], indices int64 [Nq, k]), best first; (-inf, -1) beyond the rows that can be returned.
        use_prior / normalised: None = yes if a prior is set / a normaliser is fitted; True where there is none is refused.
        normalised uses scale = beta (a scale passed as well is refused); the scores are then beta * s - lse[g] (+ prior[g]).
        Excluded rows are never returned."""
        self._check(query_features, "search")
        if not 1 <= int(k) <= 32:
            raise ops._lib.MpvError(f"RetrievalIndex.search: k ({k}) must be in [1, 32]")
        if self.size == 0:
            raise ops._lib.MpvError("RetrievalIndex.search: the index is empty")
        term, scale = self._effective("search", scale, use_prior, normalised)
        q = query_features.contiguous()
        if term is not None:
            if self.storage == "fp8":
                return ops.sim_topk_prior_q8(q, self.codes, self.scales, term, int(k), scale=scale)
            return ops.sim_topk_prior(q, self.features, term, int(k), scale=scale)
        if self.storage == "fp8":
            return ops.sim_topk_q8(q, self.codes, self.scales, int(k), scale=scale)
        return ops.sim_topk(q, self.features, int(k), scale=scale)

    def rank(self, query_features, target, scale=None, use_prior=None, normalised=None):
        """-> int32 [Nq]: the best rank (0 = first) among each query's target rows; target int64 [Nq] or [Nq, n_t], -1 = unused.
        scale, use_prior, normalised as in search: the ranks are those under the scores search returns.  An excluded target is no
        target (the index size when a query has no other)."""
        self._check(query_features, "rank")
        if self.size == 0:
            raise ops._lib.MpvError("RetrievalIndex.rank: the index is empty")
        target = self._targets(target, query_features, "rows")
        term, scale = self._effective("rank", scale, use_prior, normalised, always=scale is not None)
        q = query_features.contiguous()
        if term is not None:
            if self.storage == "fp8":
                return ops.sim_rank_prior_q8(q, self.codes, self.scales, term, target, scale=scale)
            return ops.sim_rank_prior(q, self.features, term, target, scale=scale)
        if self.storage == "fp8":
            return ops.sim_rank_q8(q, self.codes, self.scales, target)
        return ops.sim_rank(q, self.features, target)


class MaxSimIndex(_FeatureIndex):
    """Gallery of ITEMS that are groups of `group` L2-normalised bf16 rows (the pre-train model's extract_vision_feature returns
    [B, Q, E]: group = Q; its extract_text_feature returns [B, E]: group = 1), searched on the device by ops.maxsim_topk /
    ops.maxsim_rank under the query-max score: s(query, item) = max over the rows of both of <a, b>.  A grouped index takes
    single-row queries [nq, dim]; a group == 1 index takes single-row queries or grouped ones [nq, Q, dim].  Neither the row
    products nor a [queries, items] matrix are built.  Surface, growth and order rule of RetrievalIndex."""

    def __init__(self, dim: int, group: int = 1, device="cuda", capacity: int = 1024, storage: str = "bf16"):
        if dim % 32 != 0 or not 32 <= dim <= 1024:
            raise ops._lib.MpvError(f"MaxSimIndex: dim ({dim}) must be a multiple of 32 in [32, 1024]")
        if not 1 <= int(group) <= 1024:
            raise ops._lib.MpvError(f"MaxSimIndex: group ({group}) must be in [1, 1024]")
        self.dim, self.group = dim, int(group)
        self._init_storage((self.group, dim), device, capacity, storage)

    def _check(self, feats, what, groups):
        if not torch.is_tensor(feats) or feats.dtype != torch.bfloat16:
            raise ops._lib.MpvError(f"MaxSimIndex.{what}: features must be a bfloat16 tensor (the towers emit bf16; got "
                                    f"{getattr(feats, 'dtype', type(feats))})")
        if feats.dim() == 2 and 1 in groups and feats.shape[1] == self.dim:
            return feats[:, None, :]
        if feats.dim() == 3 and feats.shape[2] == self.dim and (groups is any or feats.shape[1] in groups) and feats.shape[1] >= 1:
            return feats
        raise ops._lib.MpvError(f"MaxSimIndex.{what}: features of shape {tuple(feats.shape)} do not fit an index of group {self.group}, "
                                f"dim {self.dim}")

    def add(self, features):
        """append items [n, group, dim] ([n, dim] when group == 1); -> the index of the first one"""
        return self._append(self._check(features, "add", (self.group,)))

    def _query(self, query_features, what):
        # a grouped index is searched with one row per query; an index of single rows with single rows or with groups of any size
        q = self._check(query_features, what, (1,) if self.group > 1 else any)
        if self.storage == "fp8" and q.shape[1] > 1:
            raise ops._lib.MpvError(f"MaxSimIndex.{what}: grouped queries {tuple(q.shape)} against an fp8 index: in that direction the "
                                    "index is the resident side of the search, which is bf16 only -- keep such (title) indexes in bf16")
        if self.size == 0:
            raise ops._lib.MpvError(f"MaxSimIndex.{what}: the index is empty")
        return q.contiguous()

    def search(self, query_features, k: int, scale=None):
        """-> (scores fp32 [Nq, k], indices int64 [Nq, k]), best first; (-inf, -1) beyond the index size"""
        q = self._query(query_features, "search")
        if not 1 <= int(k) <= 32:
            raise ops._lib.MpvError(f"MaxSimIndex.search: k ({k}) must be in [1, 32]")
        if self.storage == "fp8":
            return ops.maxsim_topk_q8(q, self.codes, self.scales, int(k), scale=scale)
        return ops.maxsim_topk(q, self.features, int(k), scale=scale)

    def rank(self, query_features, target):
        """-> int32 [Nq]: the best rank (0 = first) among each query's target items; target int64 [Nq] or [Nq, n_t], -1 = unused"""
        q = self._query(query_features, "rank")
        target = self._targets(target, q, "items")
        if self.storage == "fp8":
            return ops.maxsim_rank_q8(q, self.codes, self.scales, target)
        return ops.maxsim_rank(q, self.features, target)
