"""DistributedGPT3_Pretrain on the gfx950 kernels -- drop-in for models/distributed_gpt3.py:31-226.

Same constructor contract (config dict with visual_cfg / text_cfg / text_decoder / megatron_cfg /
freeze_* / num_learnable_token keys, or an explicit PathShapes for synthetic runs), same
forward(video, text) -> (loss_caption, loss_contrastive), same parameter names/shapes.
forward() returns a loss tensor that is attached to autograd through ONE Function whose
backward replays the hand-written backward pipeline (vision.py / gpt3.py) and writes the
parameter gradients in place, so `loss.backward()` / `engine.backward(loss)` work unchanged.
"""
from __future__ import annotations

import json
from types import SimpleNamespace
from typing import Optional

import torch
from torch import nn

from . import ops
from .gpt3 import DistributedGPT3, GPT3Config
from .vision import AttentionPool, Linear, TimeSformer, _param, convert_pretrained_vit, grad_of


class _StepFn(torch.autograd.Function):
    """Bridges the explicit forward/backward pipeline into autograd (one node per step).  Outputs: loss_caption, and with the
    contrastive head on a second one, loss_contrastive."""

    @staticmethod
    def forward(ctx, anchor, model, video, ids, mask, prompt_lengths=None):
        loss, tape = model._forward_pipeline(video, ids, mask, prompt_lengths=prompt_lengths)
        ctx.model, ctx.tape = model, tape
        return (loss, tape["loss_ita"]) if "loss_ita" in tape else loss

    @staticmethod
    def backward(ctx, grad_loss, grad_ita=None):
        # (an output that took no part in the loss arrives as a zero tensor: autograd materialises missing gradients)
        g_ita = None if grad_ita is None else grad_ita.contiguous().float()
        ctx.model._backward_pipeline(ctx.tape, grad_loss.contiguous().float(), g_ita)
        ctx.tape = None
        return torch.zeros(1, device=grad_loss.device), None, None, None, None, None


class DistributedGPT3_Pretrain(nn.Module):
    # what a subclass does with config['use_contrastive']: "build" the ITC head, "refuse" it, or "ignore" the key as the
    # reference's generation / classification models do (they never read it)
    CONTRASTIVE = "build"

    def __init__(self, config: Optional[dict] = None, tokenizer=None, *, visual_cfg: Optional[dict] = None,
                 text_cfg: Optional[GPT3Config] = None, device="cuda"):
        super().__init__()
        config = dict(config or {})
        self.tokenizer = tokenizer
        if visual_cfg is None:
            visual_cfg = json.load(open(config["visual_cfg"], "r"))                       # :36
        if text_cfg is None:
            text_cfg = GPT3Config.from_json_file(config["text_cfg"])                      # :37
        self.visual_encoder = self._build_visual_encoder(config, visual_cfg, device)
        self._init_visual_encoder_from_ckpt(visual_cfg)                                   # :56-72
        if config.get("text_decoder") and not config.get("_synthetic", False):
            self.text_decoder = DistributedGPT3(model_dir=config["text_decoder"], device=device)          # :78-84
        else:
            self.text_decoder = DistributedGPT3(config=text_cfg, device=device)
        if config.get("freeze_vit", False):                                               # :86-89
            for name, p in self.visual_encoder.named_parameters():
                if not any(x in name for x in ("time", "temporal")):
                    p.requires_grad = False
        if config.get("freeze_text_decoder", True):                                       # :91-93 (every shipped recipe freezes it)
            for p in self.text_decoder.parameters():
                p.requires_grad = False
        # LoRA adapters on the frozen decoder's q/k/v projections (no reference counterpart): lora_rank 0 = off
        lora_rank = int(config.get("lora_rank", 0) or 0)
        if lora_rank:
            if not config.get("freeze_text_decoder", True):
                raise ValueError("lora_rank > 0 needs freeze_text_decoder: true: adapters go on a frozen decoder")
            self.text_decoder.add_lora(lora_rank, config.get("lora_alpha", None))
        self.vision_width = visual_cfg["embed_dim"]
        self.text_width = self.text_decoder.config.hidden_size
        self.num_learnable_token = config.get("num_learnable_token", 256)                 # :102
        self.learnable_queries = _param(1, self.num_learnable_token, self.vision_width, std=0.015, device=device)
        self.attn_pool = AttentionPool(self.vision_width, num_heads=visual_cfg["num_heads"], mlp_ratio=visual_cfg["mlp_ratio"],
                                       eps=1e-6, std=0.02, device=device)                 # :106-109
        self.visual_fc = Linear(self.vision_width, self.text_width, std=0.015, device=device)   # :111,116
        self.visual_norm = nn.Identity()
        if visual_cfg.get("connect_ln", False):                                           # :112-115
            from .vision import LayerNormWithForceFP32
            self.visual_norm = LayerNormWithForceFP32(self.text_width, eps=1e-6, device=device)
        self.use_contrastive = bool(config.get("use_contrastive", False)) and self.CONTRASTIVE != "ignore"
        if self.use_contrastive:                                                          # :122-127
            self._check_contrastive_supported(config)
            E = config.get("contrastive_embed_dim", 256)      # the reference reads this key; the YAML's `embed_dim` is not used
            if E % 8:
                raise ValueError(f"contrastive_embed_dim ({E}) must be a multiple of 8")
            self.vision_proj = Linear(self.vision_width, E, device=device)
            self.text_proj = Linear(self.text_width, E, device=device)
            self.temp = nn.Parameter(torch.ones([], dtype=torch.bfloat16, device=device) * config.get("temp", 0.07))
        self.prompt = config.get("prompt", "")
        self._anchor = torch.zeros(1, device=device, requires_grad=True)
        self.on_stage_grads_ready = None      # engine hook(stage_name)

    def _build_visual_encoder(self, config, visual_cfg, device):
        return TimeSformer(
            img_size=visual_cfg["img_size"], num_frames=visual_cfg["num_frames"], patch_size=visual_cfg["patch_size"],
            embed_dim=visual_cfg["embed_dim"], depth=visual_cfg["depth"], num_heads=visual_cfg["num_heads"],
            mlp_ratio=visual_cfg["mlp_ratio"], eps=1e-6, init_std=0.015, clip_model=visual_cfg.get("clip_model", False),
            device=device)                                                                # :39-54

    def _init_visual_encoder_from_ckpt(self, visual_cfg):
        """models/distributed_gpt3.py:56-72: `pretrained_ckpt` of the visual config ("clip/<path>.pth" in every shipped
        config, configs/models/clip-b16.json:2) initialises the vision tower, strict=False; a missing file raises as
        torch.load does in the reference.  `timm/<name>` needs the timm package and network access: refused loudly."""
        pretrained = visual_cfg.get("pretrained_ckpt", None)
        if pretrained is None:
            return None
        if pretrained.startswith("timm"):
            raise NotImplementedError("pretrained_ckpt 'timm/...' needs the timm model zoo (not available here); "
                                      "the shipped configs use 'clip/<file>.pth'")
        if not pretrained.startswith("clip"):
            return None
        path = "/".join(pretrained.split("/")[1:])
        weights = convert_pretrained_vit(torch.load(path, map_location="cpu"))
        own = self.visual_encoder.state_dict()
        weights = {k: (v.to(own[k].dtype) if k in own else v) for k, v in weights.items()}
        msg = self.visual_encoder.load_state_dict(weights, strict=False)
        print("Initialize Vision Encoder from CKPT {}".format(path))
        print(msg)
        return msg

    def no_weight_decay(self):
        return {"visual_encoder.pos_embed", "visual_encoder.cls_token", "visual_encoder.temporal_embed"}       # :224-226

    def _check_contrastive_supported(self, config):
        """use_contrastive is built for this class with the frozen decoder (every shipped recipe); refuse the rest loudly."""
        if self.CONTRASTIVE != "build":
            raise NotImplementedError(f"use_contrastive is implemented for DistributedGPT3_Pretrain only, not {type(self).__name__} "
                                      "(the image model pools the caption pass's hidden states instead, models/distributed_gpt3.py:378-382)")
        if not config.get("freeze_text_decoder", True):
            raise NotImplementedError("use_contrastive with freeze_text_decoder: false would need a backward through the text-only "
                                      "decoder pass; the gfx950 path implements the frozen-decoder recipe")

    # ---------------------------------------------------------------- contrastive head (models/distributed_gpt3.py:168-212)
    def _contrastive_forward(self, tape, ids, mask):
        """query-max ITC: loss_ita (fp32 scalar, device) into the tape; no host synchronisation anywhere."""
        from .retrieval import gather_cat
        B, L = ids.shape
        Q, D, Hh, E = self.num_learnable_token, self.vision_width, self.text_width, self.vision_proj.out_features
        if B % 8:
            raise ValueError(f"use_contrastive: the per-rank batch ({B}) must be a multiple of 8 (operand rule of the head's GEMMs)")
        # live LoRA adapters: the text-only pass is no longer frozen below `pooled` -- keep its tape for _contrastive_backward
        text_tape = {} if self.text_decoder.lora_live() else None
        pooled, tp, tf, tn = self._itc_text_features(ids, mask, text_tape)
        iq = tape["image_query"]
        vp, vf, vn = self._itc_vision_features(iq, B)
        g = getattr(self, "process_group", None)
        v_all, t_all = gather_cat(vf, g), gather_cat(tf, g)                                                    # :184-185
        WB = t_all.shape[0]
        rank = torch.distributed.get_rank(g) if WB > B else 0
        inv_temp = (1.0 / self.temp.detach().float()).reshape(1)
        sim_i2t, arg1 = ops.maxsim_fwd(vf, t_all, B, Q, WB, E, alpha_dev=inv_temp)                             # :187-195
        sim_t2i, arg2 = ops.maxsim_fwd(v_all, tf, WB, Q, B, E, alpha_dev=inv_temp, trans=True)                 # :197-204
        target = torch.arange(rank * B, rank * B + B, device=ids.device)                                       # :206-208
        scale = 0.5 / B                                                                                        # (mean + mean) / 2
        l1, ds1, dt1 = ops.smoothed_ce(sim_i2t, target, 0.1, scale, B, WB)                                     # :211-212
        l2, ds2, dt2 = ops.smoothed_ce(sim_t2i, target, 0.1, scale, B, WB)
        tape["loss_ita"] = (l1.sum() + l2.sum()) * scale
        tape["itc"] = dict(B=B, WB=WB, E=E, pooled=pooled, vp=vp, vn=vn, vf=vf, tp=tp, tn=tn, tf=tf, v_all=v_all, t_all=t_all,
                           arg1=arg1, arg2=arg2, ds1=ds1, ds2=ds2, dts=dt1.sum() + dt2.sum(), inv_temp=inv_temp)
        if text_tape is not None:
            tape["itc"].update(gpt_text=text_tape, L=L)

    def _itc_text_features(self, ids, mask, gpt_tape=None):
        """-> (pooled [B, Hh], tp [B, E], tf = tp / |tp| bf16, tn): the title side of the head, shared by the loss and extract_text_feature"""
        B, L = ids.shape
        Hh, E = self.text_width, self.vision_proj.out_features
        # text-only pass of the frozen decoder (:169-176): hidden states after the final LayerNorm; its LM head / CE are unused in
        # the reference and skipped here.  pass_index 1: its dropout masks are not the caption pass's.
        out = self.text_decoder.forward_lm(None, ids, None, None, {} if gpt_tape is None else gpt_tape, hidden_only=True, pass_index=1)
        rows = torch.arange(B, device=ids.device) * L + (mask.sum(dim=-1) - 1)                                  # :181
        if gpt_tape is not None:
            gpt_tape["pooled_rows"] = rows.contiguous()
        pooled = ops.gather_rows(out["last_hidden_state"].reshape(B * L, Hh), rows.contiguous(), B, Hh)
        tp = ops.gemm(pooled, self.text_proj.weight, B, E, Hh, bias=self.text_proj.bias)                       # :182
        tf, tn = ops.l2norm_fwd(tp, B, E)
        return pooled, tp, tf, tn

    def _itc_vision_features(self, image_query, B):
        """-> (vp [B*Q, E], vf = vp / |vp| bf16, vn): the clip side of the head, shared by the loss and extract_vision_feature"""
        Q, D, E = self.num_learnable_token, self.vision_width, self.vision_proj.out_features
        vp = ops.gemm(image_query, self.vision_proj.weight, B * Q, E, D, bias=self.vision_proj.bias)           # :178
        vf, vn = ops.l2norm_fwd(vp, B * Q, E)
        return vp, vf, vn

    # ---------------------------------------------------------------- zero-shot retrieval with the contrastive head
    def _need_contrastive(self, what):
        if not self.use_contrastive:
            raise RuntimeError(f"{type(self).__name__}.{what} needs the contrastive head: build the model with use_contrastive: true "
                               "(vision_proj / text_proj / temp do not exist otherwise)")

    @torch.no_grad()
    def extract_vision_feature(self, video):
        """video [B, 3, T, H, W] -> bf16 [B, Q, E], unit rows: the `vf` operand of the query-max loss for this batch, bit for bit"""
        self._need_contrastive("extract_vision_feature")
        B = video.shape[0]
        emb = self.visual_encoder.forward_features(video.to(torch.bfloat16), {})
        image_query = self.attn_pool.forward_pool(self.learnable_queries, emb, B, emb.shape[0] // B, {})
        return self._itc_vision_features(image_query, B)[1].view(B, self.num_learnable_token, -1)

    @torch.no_grad()
    def extract_text_feature(self, text):
        """text (input_ids, attention_mask [B, L]) -> bf16 [B, E], unit rows: the `tf` operand of the loss for this batch, bit for bit"""
        self._need_contrastive("extract_text_feature")
        return self._itc_text_features(text.input_ids, text.attention_mask)[2]

    @torch.no_grad()
    def search_videos(self, text, index, k):
        """the k best clips of a retrieval.MaxSimIndex of clip features ([n, Q, E]) per title: (scores / temp, indices), best first"""
        return index.search(self.extract_text_feature(text), k, scale=1.0 / float(self.temp))

    @torch.no_grad()
    def search_texts(self, video, index, k):
        """the k best titles of a retrieval.MaxSimIndex of title features ([n, E]) per clip: (scores / temp, indices), best first"""
        return index.search(self.extract_vision_feature(video), k, scale=1.0 / float(self.temp))

    def _contrastive_backward(self, tape, grad_ita):
        """gradients of the head (projections, temp) and d image_query [B*Q, D]; the text tower below `pooled` is frozen."""
        from .retrieval import reduce_scatter_sum
        c = tape["itc"]
        B, WB, E = c["B"], c["WB"], c["E"]
        Q, D, Hh = self.num_learnable_token, self.vision_width, self.text_width
        g = getattr(self, "process_group", None)
        coef = (c["inv_temp"] * grad_ita.reshape(1)).contiguous()
        G1 = ops.maxsim_route(c["ds1"], c["arg1"], B, Q, WB)                       # d sim_i2t / d <v[i,q], t_all[j]>   [B*Q, WB]
        G2 = ops.maxsim_route(c["ds2"], c["arg2"], WB, Q, B, trans=True)           # d sim_t2i / d <t[i], v_all[j,q]>   [WB*Q, B]
        dv = ops.gemm(G1, c["t_all"], B * Q, E, WB, trans_b=True, alpha_dev=coef)
        dt_all = ops.gemm(G1, c["vf"], WB, E, B * Q, trans_a=True, trans_b=True, alpha_dev=coef)
        dt = ops.gemm(G2, c["v_all"], B, E, WB * Q, trans_a=True, trans_b=True, alpha_dev=coef)
        dv_all = ops.gemm(G2, c["tf"], WB * Q, E, B, trans_b=True, alpha_dev=coef)
        dv = ops.add(dv, reduce_scatter_sum(dv_all, g))                            # all_gather backward
        dt = ops.add(dt, reduce_scatter_sum(dt_all, g))
        # d temp: sim = raw / temp  ->  dL/dtemp = -(1/temp) * sum(dsim * sim)
        grad_of(self.temp).copy_((-(c["dts"]) * c["inv_temp"][0] * grad_ita.reshape(())).to(torch.bfloat16))
        dtp = ops.l2norm_bwd(dt, c["tp"], c["tn"], B, E)
        ops.colsum(dtp, B, E, out=grad_of(self.text_proj.bias))
        ops.gemm(dtp, c["pooled"], E, Hh, B, trans_a=True, trans_b=True, out=grad_of(self.text_proj.weight))
        if "gpt_text" in c:             # live LoRA adapters: the text-only pass's backward, seeded at the pooled rows (first pass of the step)
            dpooled = ops.gemm(dtp, self.text_proj.weight, B, Hh, E, trans_b=True)
            dlh = torch.zeros((B * c["L"], Hh), dtype=torch.bfloat16, device=dtp.device)
            ops.scatter_rows(dpooled, c["gpt_text"]["pooled_rows"], dlh, B, Hh)
            self.text_decoder.backward_lm(c["gpt_text"], None, d_last_hidden=dlh)
        dvp = ops.l2norm_bwd(dv, c["vp"], c["vn"], B * Q, E)
        ops.colsum(dvp, B * Q, E, out=grad_of(self.vision_proj.bias))
        ops.gemm(dvp, tape["image_query"], E, D, B * Q, trans_a=True, trans_b=True, out=grad_of(self.vision_proj.weight))
        return ops.gemm(dvp, self.vision_proj.weight, B * Q, D, E, trans_b=True)

    # ---------------------------------------------------------------- pipeline
    def _forward_pipeline(self, video, ids, mask, want_logits=False, prompt_lengths=None):
        B = video.shape[0]
        Q, Hh = self.num_learnable_token, self.text_width
        tape = {"vit": {}, "pool": {}, "gpt": {}}
        emb = self.visual_encoder.forward_features(video.to(torch.bfloat16), tape["vit"])
        S_img = emb.shape[0] // B
        image_query = self.attn_pool.forward_pool(self.learnable_queries, emb, B, S_img, tape["pool"])      # :134
        qf = ops.gemm(image_query, self.visual_fc.weight, B * Q, Hh, self.vision_width, bias=self.visual_fc.bias)   # :136
        tape["image_query"] = image_query
        if not isinstance(self.visual_norm, nn.Identity):                                 # connect_ln: visual_norm(visual_fc(.))
            vn = self.visual_norm
            tape["qf_raw"] = qf
            qf, tape["vn_mean"], tape["vn_rstd"] = ops.layernorm_fwd(qf, vn.weight, vn.bias, vn.eps, B * Q, Hh)
        if not want_logits and Q > 0 and ids.shape[1] > 0:
            # training / loss-only evaluation: labels and loss weights of the L text positions from one kernel (the Q query slots
            # in front never carry loss, :142-159): LM head + CE run on that window and no [B, S] target tensors are built
            pl = None if prompt_lengths is None else torch.as_tensor(prompt_lengths, device=ids.device, dtype=torch.long).contiguous()
            out = self.text_decoder.forward_lm(qf, ids, None, None, tape["gpt"], loss_window=(Q, ids.shape[1]),
                                               window_targets=ops.caption_targets(ids, mask, pl))
            tape["out"] = out
            if self.use_contrastive:
                self._contrastive_forward(tape, ids, mask)
            return out["loss"], tape
        # targets / loss mask exactly as :142-159 (filler id 100 is always masked)
        targets = torch.cat([ids[:, 1:], ids[:, 1:2]], dim=1)
        targets = torch.cat([torch.full((B, Q), 100, dtype=torch.long, device=ids.device), targets], dim=1)
        tla = mask[:, 1:]
        if prompt_lengths is not None:                                                    # models/distributed_gpt3.py:348-351
            pl = torch.as_tensor(prompt_lengths, device=ids.device).view(-1, 1)
            tla = tla.clone()
            tla[torch.arange(tla.shape[1], device=ids.device)[None] < pl] = 0
        loss_mask = torch.cat([torch.zeros((B, Q), dtype=torch.long, device=ids.device), tla], dim=1)
        # the Q query slots in front never carry loss (zeros above): LM head + CE on the L text positions only
        out = self.text_decoder.forward_lm(qf, ids, targets, loss_mask, tape["gpt"], want_logits=want_logits,
                                           loss_window=(Q, ids.shape[1]))
        tape["out"] = out
        return out["loss"], tape

    def _backward_pipeline(self, tape, grad_loss, grad_ita=None):
        B = tape["vit"]["B"]
        Q, Hh, D = self.num_learnable_token, self.text_width, self.vision_width
        diq_itc = None
        if "itc" in tape:               # every head gradient is complete before the "head" bucket is reported below
            diq_itc = self._contrastive_backward(tape, grad_ita if grad_ita is not None else torch.zeros((), device=grad_loss.device))
        if "itc" in tape and "gpt_text" in tape["itc"]:      # the adapters' gradients of the text-only pass are already in place
            dqf = self.text_decoder.backward_lm(tape["gpt"], grad_loss, accumulate_lora=True)
        else:
            dqf = self.text_decoder.backward_lm(tape["gpt"], grad_loss)
        iq = tape["image_query"]
        if "qf_raw" in tape:
            vn = self.visual_norm
            dqf = ops.layernorm_bwd(dqf, tape["qf_raw"], vn.weight, tape["vn_mean"], tape["vn_rstd"], B * Q, Hh,
                                    dgamma=grad_of(vn.weight), dbeta=grad_of(vn.bias))
        ops.colsum(dqf, B * Q, Hh, out=grad_of(self.visual_fc.bias))
        ops.gemm(dqf, iq, Hh, D, B * Q, trans_a=True, trans_b=True, out=grad_of(self.visual_fc.weight))
        diq = ops.gemm(dqf, self.visual_fc.weight, B * Q, D, Hh, trans_b=True)
        if diq_itc is not None:
            diq = ops.add(diq, diq_itc)
        demb = self.attn_pool.backward_pool(diq, self.learnable_queries, tape["pool"])
        if self.on_stage_grads_ready is not None:
            self.on_stage_grads_ready("head")
        self.visual_encoder.backward_features(demb, tape["vit"])

    # ---------------------------------------------------------------- reference-shaped API
    def forward(self, image, text):
        ids, mask = text.input_ids, text.attention_mask
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            out = _StepFn.apply(self._anchor, self, image, ids, mask)
            loss, lita = out if isinstance(out, tuple) else (out, None)
        else:
            loss, tape = self._forward_pipeline(image, ids, mask)
            lita = tape.get("loss_ita")
        if not self.use_contrastive:
            return loss, torch.zeros((), device=loss.device)                               # :218-219
        return loss, lita                                                                  # :221

    @torch.no_grad()
    def forward_backward(self, image, text):
        """forward + backward of one micro-batch WITHOUT autograd: what `loss, _ = model(image, text); loss.backward()` does, as two
        direct calls of the explicit pipeline.  Gradients land in the same .grad views.  This is the form a HIP graph can capture
        (engine.graph_step): under autograd the anchor's AccumulateGrad node runs on the stream the anchor was created on, not
        on the capturing stream.
        With use_contrastive the step's loss is loss_caption + loss_contrastive; both parts stay readable afterwards (also after a
        graph replay, which rewrites the same buffers) as `self.loss_caption` / `self.loss_contrastive`."""
        loss, tape = self._forward_pipeline(image, text.input_ids, text.attention_mask, prompt_lengths=getattr(text, "prompt_lengths", None))
        one = torch.ones((), dtype=torch.float32, device=loss.device)
        if "itc" not in tape:
            self._backward_pipeline(tape, one)
            return loss
        self._backward_pipeline(tape, one, one)
        self.loss_caption, self.loss_contrastive = loss, tape["loss_ita"]
        return loss + tape["loss_ita"]

    @torch.no_grad()
    def forward_outputs(self, image, text):
        """Evaluation helper: full decoder outputs (logits, losses, last_hidden_state, loss)."""
        _, tape = self._forward_pipeline(image, text.input_ids, text.attention_mask, want_logits=True)
        return SimpleNamespace(**tape["out"])


class DistributedGPT3_Pretrain_Image(DistributedGPT3_Pretrain):
    """models/distributed_gpt3.py:229-427 with use_eva_g: the EVA-ViT-g image encoder in front of the same abstractor and
    frozen decoder; forward(image [B,3,H,W], text) -> (loss_caption, loss_contrastive); `text.prompt_lengths`, when
    present, is masked out of the caption loss (:348-351).  use_contrastive is refused (its head differs, :378-382)."""
    CONTRASTIVE = "refuse"

    def _build_visual_encoder(self, config, visual_cfg, device):
        from .eva_vit import create_eva_vit_g
        if not config.get("use_eva_g", False):
            raise NotImplementedError("the image path is built for use_eva_g: true (models/distributed_gpt3.py:256-261)")
        over = {k: visual_cfg[k] for k in ("embed_dim", "depth", "num_heads", "mlp_ratio", "patch_size") if k in visual_cfg
                and config.get("_synthetic", False)}
        return create_eva_vit_g(img_size=visual_cfg["img_size"], drop_path_rate=visual_cfg.get("drop_path", False) or 0.0,
                                device=device, **over)

    def no_weight_decay(self):
        return {"visual_encoder.pos_embed", "visual_encoder.cls_token"}                      # :425-427

    def forward(self, image, text):
        ids, mask = text.input_ids, text.attention_mask
        pl = getattr(text, "prompt_lengths", None)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            loss = _StepFn.apply(self._anchor, self, image, ids, mask, pl)
        else:
            loss, _ = self._forward_pipeline(image, ids, mask, prompt_lengths=pl)
        return loss, torch.zeros((), device=loss.device)


def synthetic_image_model(shapes, device="cuda", **eva) -> "DistributedGPT3_Pretrain_Image":
    """Random-init image model; `eva` overrides (embed_dim, depth, num_heads, mlp_ratio, patch_size) for reduced shapes."""
    vis = dict(img_size=shapes.img_size, num_frames=1, embed_dim=eva.get("embed_dim", 1408), num_heads=eva.get("num_heads", 16),
               mlp_ratio=eva.get("mlp_ratio", 4.3637), depth=eva.get("depth", 40), patch_size=eva.get("patch_size", 14))
    txt = GPT3Config(vocab_size=shapes.vocab, hidden_size=shapes.hidden, ffn_hidden_size=shapes.ffn,
                     num_hidden_layers=shapes.layers, num_attention_heads=shapes.heads, max_position_embeddings=shapes.max_pos,
                     layernorm_epsilon=shapes.gpt_ln_eps)
    return DistributedGPT3_Pretrain_Image({"num_learnable_token": shapes.num_queries, "_synthetic": True, "use_eva_g": True},
                                          visual_cfg=vis, text_cfg=txt, device=device)


def synthetic_model(shapes, device="cuda", num_frames=None, use_contrastive=False, temp=0.07) -> DistributedGPT3_Pretrain:
    """Random-init model from a shapes object with the fields of oracle.weights.PathConfig (the
    product never imports oracle/: tests pass the dataclass in).  use_contrastive / temp: the ITC head of the recipe keys."""
    vis = dict(img_size=shapes.img_size, patch_size=shapes.patch_size, depth=shapes.vit_depth,
               num_frames=num_frames or shapes.num_frames, embed_dim=shapes.vit_dim, num_heads=shapes.vit_heads,
               mlp_ratio=shapes.vit_mlp_ratio, clip_model=True, connect_ln=bool(getattr(shapes, "connect_ln", False)))
    txt = GPT3Config(vocab_size=shapes.vocab, hidden_size=shapes.hidden, ffn_hidden_size=shapes.ffn,
                     num_hidden_layers=shapes.layers, num_attention_heads=shapes.heads, max_position_embeddings=shapes.max_pos,
                     layernorm_epsilon=shapes.gpt_ln_eps)
    config = {"num_learnable_token": shapes.num_queries, "_synthetic": True}
    if use_contrastive:
        config.update(use_contrastive=True, temp=temp)
    return DistributedGPT3_Pretrain(config, visual_cfg=vis, text_cfg=txt, device=device)
