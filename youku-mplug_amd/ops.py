"""Tensor-level wrappers over the C ABI (include/mpv.h).  PyTorch is used only for device
memory and streams; every function here launches hand-written gfx950 kernels on the current
stream.  No CPU / eager fallback exists: non-CUDA tensors raise.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import os

import torch

from . import _lib
from ._lib import AttnDesc, GemmEpilogue, check

ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_RELU, ACT_DERIV = (_lib.CONSTANTS["MPV_ACT_" + n] for n in ("NONE", "GELU_ERF", "GELU_TANH", "RELU", "DERIV"))
# MPV_GELU_DERIV=0 (measurement knob): the MLPs park the pre-activation z and the dgrad epilogue evaluates GELU'(z), as until round 3.
# Default: the forward epilogue parks GELU'(z) itself and the dgrad epilogue is one multiply (include/mpv.h: preact_deriv, MPV_ACT_DERIV).
GELU_DERIV_FWD = os.environ.get("MPV_GELU_DERIV", "1") != "0"
RowMap = Tuple[int, int, int]
IDENT: RowMap = (0, 0, 0)

_ws = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.MpvError("mpv ops run on the GPU only (no CPU fallback): got a CPU tensor")


def workspace(nbytes: int, device) -> torch.Tensor:
    """Stream-ordered scratch shared by all ops launched on one (device, stream) pair, grown on demand: launches on
    different streams may run concurrently and must not share split-K partials or arrival counters."""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream)
    w = _ws.get(key)
    if w is None or w.numel() < nbytes:
        w = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = w
    return w


gemm_calls = 0      # mpv_gemm_bf16 calls of this process (profiles: per-call traffic = counter totals / calls; a call may be several row-band launches)


def gemm(a: torch.Tensor, b: torch.Tensor, M: int, N: int, K: int, *, out: Optional[torch.Tensor] = None,
         trans_a: bool = False, trans_b: bool = False, lda: Optional[int] = None, ldb: Optional[int] = None,
         ldc: Optional[int] = None, bias=None, act: int = 0, preact_out=None, residual=None, ldr: int = 0,
         act_bwd_z=None, act_bwd: int = 0, ldz: int = 0, dropout_p: float = 0.0, seed: int = 0, offset: int = 0,
         alpha_dev=None, alpha: float = 0.0, amap: RowMap = IDENT, cmap: RowMap = IDENT, kmap: RowMap = IDENT,
         out_rows: Optional[int] = None, accumulate: bool = False, out_f32: bool = False, colsum_out=None,
         tile_hint: int = 0, row_tap_out=None, row_tap_group: int = 0, split_hint: int = 0, gm_hint: int = 0,
         preact_deriv: bool = False, z_is_deriv: bool = False, keep_output: bool = False, colscale=None) -> torch.Tensor:
    """C[M,N] = epilogue(sum_k A(m,k) B(n,k)).  See include/mpv.h:mpv_gemm_bf16.
    colscale = (ncols, s): output columns below ncols leave as bf16(bf16(acc + bias) * s) (the q third of a packed qkv product).
    preact_deriv (forward of an MLP's first product): preact_out receives act'(z) instead of z; z_is_deriv (the matching dgrad):
    act_bwd_z is that tensor, multiply by it.  A call-site PAIR: both follow the one knob GELU_DERIV_FWD.
    keep_output: the output is small and read right behind this launch by a latency-bound kernel: plain instead of non-temporal stores."""
    global gemm_calls
    gemm_calls += 1
    _need_cuda(a, b)
    lda = lda if lda is not None else (M if trans_a else K)
    ldb = ldb if ldb is not None else (N if trans_b else K)
    ldc = ldc if ldc is not None else N
    if out is None:
        rows = out_rows if out_rows is not None else M
        out = torch.empty((rows, ldc), dtype=torch.float32 if out_f32 else torch.bfloat16, device=a.device)
    ep = GemmEpilogue()
    ep.a_group, ep.a_stride, ep.a_offset = amap
    ep.c_group, ep.c_stride, ep.c_offset = cmap
    ep.k_group, ep.k_stride, ep.k_offset = kmap
    ep.bias = _p(bias)
    ep.act = act
    ep.preact_out = _p(preact_out)
    ep.residual = _p(residual)
    ep.ldr = ldr
    ep.act_bwd_z = _p(act_bwd_z)
    ep.ldz = ldz
    ep.act_bwd = act_bwd
    ep.dropout_p = dropout_p
    ep.seed = seed
    ep.offset = offset
    ep.alpha_dev = _p(alpha_dev)
    ep.alpha = alpha
    ep.out_f32 = int(out_f32)
    ep.accumulate = int(accumulate)
    ep.colsum_out = _p(colsum_out)
    ep.tile_hint = tile_hint
    ep.row_tap_out = _p(row_tap_out)
    ep.row_tap_group = row_tap_group
    ep.split_hint = split_hint
    ep.gm_hint = gm_hint
    ep.preact_deriv = int(bool(preact_deriv and GELU_DERIV_FWD and preact_out is not None))
    ep.keep_output = int(bool(keep_output))
    if colscale is not None:
        ep.colscale_cols, ep.colscale = int(colscale[0]), float(colscale[1])
    if z_is_deriv and GELU_DERIV_FWD and act_bwd_z is not None:
        ep.act_bwd = ACT_DERIV
    ws, wsn = None, 0
    if not out_f32:
        wsn = _lib.lib().mpv_gemm_workspace_size(M, N, K, int(trans_a), int(trans_b))
        ws = workspace(wsn, a.device)
        wsn = ws.numel()
    check(_lib.lib().mpv_gemm_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, lda, ldb, ldc, int(trans_a),
                                   int(trans_b), C.byref(ep), _p(ws), wsn, _stream()), "mpv_gemm_bf16")
    return out


def layernorm_fwd(x, gamma, beta, eps: float, rows: int, cols: int, *, out=None, xmap: RowMap = IDENT,
                  ymap: RowMap = IDENT, out_rows: Optional[int] = None, ldx: Optional[int] = None,
                  ldy: Optional[int] = None, want_stats: bool = True):
    _need_cuda(x, gamma, beta)
    ldx = ldx or cols
    ldy = ldy or cols
    if out is None:
        out = torch.empty((out_rows if out_rows is not None else rows, ldy), dtype=torch.bfloat16, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if want_stats else None
    check(_lib.lib().mpv_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), _p(mean), _p(rstd),
                                       rows, cols, ldx, ldy, eps, *xmap, *ymap, _stream()), "mpv_layernorm_fwd")
    return out, mean, rstd


LN_DPARAM_DEFER = _lib.CONSTANTS["MPV_LN_DPARAM_DEFER"]


class LnDparamBatch:
    """dgamma / dbeta reductions of several LayerNorm backward calls batched into one two-launch finish (mpv_layernorm_dparam_finish).
    Pass it as `defer=` to layernorm_bwd: the call then leaves its per-workgroup partials in a buffer of this batch (kept
    and reused across steps) instead of launching its own two reduce kernels; finish() folds every pending entry on the
    current stream.  Entries of one batch must target distinct parameters."""

    def __init__(self):
        self._bufs = []
        self._pending = []
        self.cols = None

    def slot(self, nbytes: int, device) -> torch.Tensor:
        i = len(self._pending)
        while len(self._bufs) <= i:
            self._bufs.append(None)
        b = self._bufs[i]
        if b is None or b.numel() < nbytes or b.device != torch.device(device):
            b = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self._bufs[i] = b
        return b

    def add(self, buf, nrows, dgamma, dbeta, accumulate, cols):
        assert self.cols in (None, cols), "one LnDparamBatch serves LayerNorms of one width"
        self.cols = cols
        self._pending.append((buf, nrows, dgamma, dbeta, int(accumulate)))

    def finish(self):
        n = len(self._pending)
        if n == 0:
            return
        vp, ip = C.c_void_p * n, C.c_int * n
        check(_lib.lib().mpv_layernorm_dparam_finish(vp(*[e[0].data_ptr() for e in self._pending]), ip(*[e[1] for e in self._pending]),
                                                     vp(*[e[2].data_ptr() for e in self._pending]), vp(*[e[3].data_ptr() for e in self._pending]),
                                                     ip(*[e[4] for e in self._pending]), n, self.cols, _stream()),
              "mpv_layernorm_dparam_finish")
        self._pending = []


def layernorm_bwd(dy, x, gamma, mean, rstd, rows: int, cols: int, *, dres=None, dx=None, dx_drop=None,
                  dropout_p: float = 0.0, seed: int = 0, offset: int = 0, dgamma=None, dbeta=None,
                  accumulate_dparams: bool = False, xmap: RowMap = IDENT, ymap: RowMap = IDENT,
                  ldx: Optional[int] = None, ldy: Optional[int] = None, dx_rows: Optional[int] = None,
                  defer: Optional[LnDparamBatch] = None):
    _need_cuda(dy, x, gamma)
    ldx = ldx or cols
    ldy = ldy or cols
    if dx is None:
        dx = torch.empty((dx_rows if dx_rows is not None else rows, ldx), dtype=torch.bfloat16, device=x.device)
    ws, wsn = None, 0
    mode = int(accumulate_dparams)
    if dgamma is not None:
        wsn = _lib.lib().mpv_layernorm_bwd_workspace_size(cols)
        if defer is not None:
            ws = defer.slot(wsn, x.device)
            defer.add(ws, _lib.lib().mpv_layernorm_bwd_partial_rows(rows), dgamma, dbeta, accumulate_dparams, cols)
            mode = LN_DPARAM_DEFER
        else:
            ws = workspace(wsn, x.device)
        wsn = ws.numel()
    check(_lib.lib().mpv_layernorm_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                       _p(dres), dx.data_ptr(), _p(dx_drop), dropout_p, seed, offset, _p(dgamma), _p(dbeta),
                                       mode, rows, cols, ldx, ldy, *xmap, *ymap, _p(ws), wsn, _stream()),
          "mpv_layernorm_bwd")
    return dx


def ln_stream_fwd(h_in, add, gamma, beta, eps: float, rows: int, cols: int, *, h_out=None, out=None, hmap: RowMap = IDENT,
                  amap: RowMap = IDENT, ymap: RowMap = IDENT, out_rows: Optional[int] = None, h_rows: Optional[int] = None,
                  add_dropout_p: float = 0.0, seed: int = 0, offset: int = 0):
    """The decoder's residual stream in fp32 (include/mpv.h: mpv_ln_stream_fwd): h' = h_in + add in fp32, y = LN(h') in bf16.
    h_in is the fp32 stream, or the bf16 embedding output for the first LayerNorm; add None: plain LN of h_in.
    add_dropout_p > 0: `add` is dropped here (mpv_ln_stream_fwd_drop: the index / threshold / rounding of the GEMM's dropout epilogue).
    -> (y, h' (fp32, None without add), mean, rstd)."""
    _need_cuda(h_in, gamma, beta)
    if out is None:
        out = torch.empty((out_rows if out_rows is not None else rows, cols), dtype=torch.bfloat16, device=h_in.device)
    if add is not None and h_out is None:
        h_out = torch.empty((h_rows if h_rows is not None else h_in.shape[0], cols), dtype=torch.float32, device=h_in.device)
    mean = torch.empty(rows, dtype=torch.float32, device=h_in.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=h_in.device)
    check(_lib.lib().mpv_ln_stream_fwd_drop(h_in.data_ptr(), int(h_in.dtype == torch.bfloat16), _p(add), _p(h_out) if add is not None else None,
                                       gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, cols,
                                       cols, cols, cols, eps, *hmap, *amap, *ymap, float(add_dropout_p) if add is not None else 0.0, seed, offset, _stream()), "mpv_ln_stream_fwd_drop")
    return out, (h_out if add is not None else None), mean, rstd


def ln_stream_bwd(dy, x, gamma, mean, rstd, rows: int, cols: int, *, dres=None, dx=None, dx_drop=None, dropout_p: float = 0.0,
                  seed: int = 0, offset: int = 0, xmap: RowMap = IDENT, ymap: RowMap = IDENT, dx_rows: Optional[int] = None):
    """LayerNorm backward of the frozen decoder with x read from the fp32 stream (no parameter gradients)."""
    _need_cuda(dy, x, gamma)
    assert x.dtype == torch.float32
    if dx is None:
        dx = torch.empty((dx_rows if dx_rows is not None else rows, cols), dtype=torch.bfloat16, device=x.device)
    check(_lib.lib().mpv_ln_stream_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(dres), dx.data_ptr(),
                                       _p(dx_drop), dropout_p, seed, offset, rows, cols, cols, cols, *xmap, *ymap, _stream()),
          "mpv_ln_stream_bwd")
    return dx


class AttnLayout:
    """Strides (in elements) of q/k/v/o for mpv_attn_*: (batch, head, row)."""

    def __init__(self, q, k, v, o):
        self.q, self.k, self.v, self.o = q, k, v, o


def _attn_desc(q, k, v, o, lse, lay: AttnLayout, batch, heads, sq, sk, hd, causal, scale, scale_q_bf16, dropout_p, seed,
               offset):
    d = AttnDesc()
    d.q, d.k, d.v, d.o, d.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), _p(lse)
    d.q_bs, d.q_hs, d.q_rs = lay.q
    d.k_bs, d.k_hs, d.k_rs = lay.k
    d.v_bs, d.v_hs, d.v_rs = lay.v
    d.o_bs, d.o_hs, d.o_rs = lay.o
    d.batch, d.heads, d.sq, d.sk, d.head_dim = batch, heads, sq, sk, hd
    d.causal, d.scale, d.scale_q_bf16 = int(causal), scale, int(scale_q_bf16)
    d.dropout_p, d.seed, d.offset = dropout_p, seed, offset
    return d


def attn_fwd(q, k, v, o, lay: AttnLayout, batch, heads, sq, sk, hd, *, causal=False, scale=1.0, scale_q_bf16=False,
             dropout_p=0.0, seed=0, offset=0):
    """q/k/v/o are tensors whose data_ptr() is element (0,0,0,0) under `lay`; returns lse [batch, heads, sq]."""
    _need_cuda(q, k, v, o)
    lse = torch.empty((batch, heads, sq), dtype=torch.float32, device=q.device)
    d = _attn_desc(q, k, v, o, lse, lay, batch, heads, sq, sk, hd, causal, scale, scale_q_bf16, dropout_p, seed, offset)
    check(_lib.lib().mpv_attn_fwd(C.byref(d), _stream()), "mpv_attn_fwd")
    return lse


def attn_bwd(q, k, v, o, lse, do, dq, dk, dv, lay: AttnLayout, batch, heads, sq, sk, hd, *, causal=False, scale=1.0,
             scale_q_bf16=False, dropout_p=0.0, seed=0, offset=0):
    _need_cuda(q, k, v, o, do, dq, dk, dv)
    delta = torch.empty((batch, heads, sq), dtype=torch.float32, device=q.device)
    d = _attn_desc(q, k, v, o, lse, lay, batch, heads, sq, sk, hd, causal, scale, scale_q_bf16, dropout_p, seed, offset)
    check(_lib.lib().mpv_attn_bwd(C.byref(d), do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(),
                                  _stream()), "mpv_attn_bwd")


def attn_plan(role, q, k, v, o, lay: AttnLayout, batch, heads, sq, sk, hd, *, causal=False, scale=1.0, scale_q_bf16=False, dropout_p=0.0):
    """What attn_fwd (role 0) / attn_bwd (role 1: dQ, 2: dK/dV) would launch for these arguments (include/mpv.h:
    mpv_attn_plan_describe): dict(variant, grid, block, lds_bytes, lds_limit).  Launches nothing; for tests and tools."""
    d = _attn_desc(q, k, v, o, o, lay, batch, heads, sq, sk, hd, causal, scale, scale_q_bf16, dropout_p, 0, 0)
    info = _lib.AttnPlanInfo()
    check(_lib.lib().mpv_attn_plan_describe(C.byref(d), role, C.byref(info)), "mpv_attn_plan_describe")
    return dict(variant=info.variant.decode(), grid=(info.grid_x, info.grid_y), block=info.block, lds_bytes=info.lds_bytes,
                lds_limit=info.lds_limit)


def attn_prefix_fwd(q, k, v, pk, pv, o, lay: AttnLayout, prefix_lay: Tuple[Tuple[int, int, int], Tuple[int, int, int]], n_cont,
                    group_size, heads, cont_len, prefix_len, hd, *, scale=1.0):
    """Causal attention of n_cont continuations (cont_len rows each; q/k/v/o strided (continuation, head, row) by `lay`) against
    the prefix_len-row prefix of their group c // group_size (pk/pv strided (group, head, row) by prefix_lay = (k strides,
    v strides)): query row i sees every prefix key and its own keys j <= i.  include/mpv.h: mpv_attn_prefix_fwd."""
    _need_cuda(q, k, v, o, pk, pv)
    d = _lib.AttnPrefixDesc()
    d.q, d.k, d.v, d.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    d.pk, d.pv = (_p(pk), _p(pv)) if prefix_len > 0 else (None, None)      # no prefix: nothing of pk / pv is read
    d.q_cs, d.q_hs, d.q_rs = lay.q
    d.k_cs, d.k_hs, d.k_rs = lay.k
    d.v_cs, d.v_hs, d.v_rs = lay.v
    d.o_cs, d.o_hs, d.o_rs = lay.o
    (d.pk_gs, d.pk_hs, d.pk_rs), (d.pv_gs, d.pv_hs, d.pv_rs) = prefix_lay
    d.n_cont, d.group_size, d.n_groups = n_cont, group_size, (n_cont + group_size - 1) // group_size
    d.heads, d.cont_len, d.prefix_len, d.head_dim, d.scale = heads, cont_len, prefix_len, hd, scale
    check(_lib.lib().mpv_attn_prefix_fwd(C.byref(d), _stream()), "mpv_attn_prefix_fwd")
    return o


class PackedLayout:
    """The packed layout of ragged continuations (include/mpv.h: mpv_attn_prefix_packed_layout), built once per pass: cont_len[c] rows
    for continuation c, conts_per_group[g] consecutive continuations for group g.  Host side: cont_len, conts_per_group, seg_start_host,
    group_row_host, rows, max_group_rows and pos_in_cont[r] = r - seg_start[r]; with a device, the two index arrays as int32 device
    tensors seg_start and group_row (two views of one upload; None without a device)."""

    def __init__(self, cont_len, conts_per_group, device=None):
        self.cont_len = [int(x) for x in cont_len]
        self.conts_per_group = [int(x) for x in conts_per_group]
        nc, ng = len(self.cont_len), len(self.conts_per_group)
        cl = (C.c_int32 * max(nc, 1))(*self.cont_len)
        cg = (C.c_int32 * max(ng, 1))(*self.conts_per_group)
        total = sum(self.cont_len)
        # the function validates before it writes: what it will refuse (a length < 1, 2^30 rows or more) gets no buffer to speak of
        seg = (C.c_int32 * (total if nc and min(self.cont_len) >= 1 and total < (1 << 30) else 1))()
        grp = (C.c_int32 * (ng + 1))()
        rows, mgr = C.c_int(0), C.c_int(0)
        check(_lib.lib().mpv_attn_prefix_packed_layout(cl, nc, cg, ng, seg, grp, C.byref(rows), C.byref(mgr)),
              "mpv_attn_prefix_packed_layout")
        self.rows, self.max_group_rows, self.n_groups, self.n_cont = rows.value, mgr.value, ng, nc
        self.seg_start_host = list(seg[:self.rows])
        self.group_row_host = list(grp)
        self.pos_in_cont = [r - s for r, s in enumerate(self.seg_start_host)]
        self.seg_start = self.group_row = None
        if device is not None:
            both = torch.tensor(self.seg_start_host + self.group_row_host, dtype=torch.int32).to(device)      # one copy
            self.seg_start, self.group_row = both[:self.rows], both[self.rows:]


def _prefix_packed_desc(d, q, k, v, pk, pv, row_strides, prefix_lay, layout: PackedLayout, heads, prefix_len, hd, scale, *more):
    """what the packed entries share: the GPU-only check of every tensor and the operand, stride and shape fields of `d`"""
    _need_cuda(q, k, v, pk, pv, layout.seg_start, layout.group_row, *more)
    d.q, d.k, d.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    d.pk, d.pv = (_p(pk), _p(pv)) if prefix_len > 0 else (None, None)      # no prefix: nothing of pk / pv is read
    d.seg_start, d.group_row = _p(layout.seg_start), _p(layout.group_row)
    (d.q_rs, d.q_hs), (d.k_rs, d.k_hs), (d.v_rs, d.v_hs), (d.o_rs, d.o_hs) = row_strides
    (d.pk_gs, d.pk_hs, d.pk_rs), (d.pv_gs, d.pv_hs, d.pv_rs) = prefix_lay
    d.rows, d.n_groups, d.max_group_rows = layout.rows, layout.n_groups, layout.max_group_rows
    d.heads, d.prefix_len, d.head_dim, d.scale = heads, prefix_len, hd, scale
    return d


def attn_prefix_packed_fwd(q, k, v, pk, pv, o, row_strides, prefix_lay: Tuple[Tuple[int, int, int], Tuple[int, int, int]],
                           layout: PackedLayout, heads, prefix_len, hd, *, scale=1.0):
    """Causal attention of the packed, ragged continuations of `layout` (packed row r of q/k/v/o strided (row, head) by row_strides
    = (q, k, v, o) pairs) against the prefix_len-row prefix of their group (pk/pv strided (group, head, row) by prefix_lay = (k
    strides, v strides)): query row r sees every prefix key of its group and its own keys seg_start[r] <= kr <= r.
    include/mpv.h: mpv_attn_prefix_packed_fwd."""
    d = _prefix_packed_desc(_lib.AttnPrefixPackedDesc(), q, k, v, pk, pv, row_strides, prefix_lay, layout, heads, prefix_len, hd, scale, o)
    d.o = o.data_ptr()
    check(_lib.lib().mpv_attn_prefix_packed_fwd(C.byref(d), _stream()), "mpv_attn_prefix_packed_fwd")
    return o


def attn_prefix_packed_fwd_lse(q, k, v, pk, pv, o, row_strides, prefix_lay, layout: PackedLayout, heads, prefix_len, hd, *, scale=1.0,
                               lse=None):
    """attn_prefix_packed_fwd for training: the same o bit for bit, and -> lse, fp32 [heads, rows] (contiguous; a new tensor unless
    given), the statistic of every row's one softmax that attn_prefix_packed_bwd needs.  include/mpv.h: mpv_attn_prefix_packed_fwd_lse."""
    d = _prefix_packed_desc(_lib.AttnPrefixPackedDesc(), q, k, v, pk, pv, row_strides, prefix_lay, layout, heads, prefix_len, hd, scale, o,
                            lse)
    d.o = o.data_ptr()
    if lse is None:
        lse = torch.empty((heads, layout.rows), dtype=torch.float32, device=q.device)
    check(_lib.lib().mpv_attn_prefix_packed_fwd_lse(C.byref(d), lse.data_ptr(), _stream()), "mpv_attn_prefix_packed_fwd_lse")
    return lse


def attn_prefix_packed_bwd(q, k, v, pk, pv, o, lse, do, dq, dk, dv, dpk, dpv, row_strides, prefix_lay, layout: PackedLayout, heads,
                           prefix_len, hd, *, scale=1.0, accumulate_prefix=False):
    """The backward of attn_prefix_packed_fwd_lse: dq / dk / dv of the packed rows (strided as q / k / v; do as o) and the groups' dpk /
    dpv (strided as pk / pv), the sums over all rows of a group; accumulate_prefix adds them to what dpk / dpv hold (fp32 sum, one
    rounding) instead of overwriting.  No atomics, deterministic.  include/mpv.h: mpv_attn_prefix_packed_bwd."""
    d = _prefix_packed_desc(_lib.AttnPrefixPackedBwdDesc(), q, k, v, pk, pv, row_strides, prefix_lay, layout, heads, prefix_len, hd, scale,
                            o, lse, do, dq, dk, dv, dpk, dpv)
    d.o, d.dO, d.lse = o.data_ptr(), do.data_ptr(), lse.data_ptr()
    d.dq, d.dk, d.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    d.dpk, d.dpv = (_p(dpk), _p(dpv)) if prefix_len > 0 else (None, None)
    delta = torch.empty((heads, layout.rows), dtype=torch.float32, device=q.device)
    d.delta = delta.data_ptr()
    d.accumulate_prefix = int(bool(accumulate_prefix))
    check(_lib.lib().mpv_attn_prefix_packed_bwd(C.byref(d), _stream()), "mpv_attn_prefix_packed_bwd")


def attn_decode_shared_fwd(q, k, v, pk, pv, o, lay: AttnLayout, prefix_lay: Tuple[Tuple[int, int, int], Tuple[int, int, int]], n_seq,
                           group_size, heads, prefix_len, own_len, hd, *, scale=1.0):
    """One decode step's attention of n_seq sequences (ONE query row each; q/k/v/o strided (sequence, head, row) by `lay`, the row
    stride of q and o is not used) against the prefix_len-row prefix of their group s // group_size (pk/pv strided (group, head,
    row) by prefix_lay = (k strides, v strides)) and their own own_len rows of k/v: one softmax over both key sets.
    include/mpv.h: mpv_attn_decode_shared_fwd."""
    return _attn_decode_shared(q, k, v, pk, pv, o, lay, prefix_lay, n_seq, group_size, heads, prefix_len, own_len, hd, scale, None, False)


def attn_decode_shared_ragged_fwd(q, k, v, pk, pv, o, lay: AttnLayout, prefix_lay, n_seq, group_size, heads, prefix_len, group_prefix_len,
                                  own_len, hd, *, scale=1.0):
    """attn_decode_shared_fwd with a prefix length per group: group_prefix_len int32 [n_groups] on the device, every entry in
    [1, prefix_len] (the caller's promise; prefix_len is the upper bound).  include/mpv.h: mpv_attn_decode_shared_ragged_fwd."""
    if group_prefix_len is not None:
        _need_cuda(group_prefix_len)
        n_groups = (n_seq + group_size - 1) // max(group_size, 1)
        if group_prefix_len.dtype != torch.int32 or not group_prefix_len.is_contiguous() or group_prefix_len.numel() < n_groups:
            raise ValueError(f"group_prefix_len must be a contiguous int32 tensor of {n_groups} lengths")
    return _attn_decode_shared(q, k, v, pk, pv, o, lay, prefix_lay, n_seq, group_size, heads, prefix_len, own_len, hd, scale,
                               group_prefix_len, True)


def attn_decode_shared_steps_fwd(q, k, v, pk, pv, o, lay: AttnLayout, prefix_lay, n_seq, group_size, heads, prefix_len, group_prefix_len,
                                 own_len, group_own_len, hd, *, scale=1.0):
    """attn_decode_shared_ragged_fwd with an own length per group as well: group_own_len int32 [n_groups] on the device, every entry in
    [0, own_len] (own_len is the upper bound; 0: the group is idle and its o rows become zeros).
    include/mpv.h: mpv_attn_decode_shared_steps_fwd."""
    n_groups = (n_seq + group_size - 1) // max(group_size, 1)
    for name, t in (("group_prefix_len", group_prefix_len), ("group_own_len", group_own_len)):
        if t is not None:
            _need_cuda(t)
            if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < n_groups:
                raise ValueError(f"{name} must be a contiguous int32 tensor of {n_groups} lengths")
    return _attn_decode_shared(q, k, v, pk, pv, o, lay, prefix_lay, n_seq, group_size, heads, prefix_len, own_len, hd, scale,
                               group_prefix_len, True, group_own_len, True)


def _attn_decode_shared(q, k, v, pk, pv, o, lay, prefix_lay, n_seq, group_size, heads, prefix_len, own_len, hd, scale, glen, ragged,
                        gown=None, steps=False):
    _need_cuda(q, k, v, o, pk, pv)
    d = _lib.AttnDecodeSharedDesc()
    d.q, d.k, d.v, d.o, d.pk, d.pv = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), pk.data_ptr(), pv.data_ptr()
    d.q_ss, d.q_hs = lay.q[:2]
    d.k_ss, d.k_hs, d.k_rs = lay.k
    d.v_ss, d.v_hs, d.v_rs = lay.v
    d.o_ss, d.o_hs = lay.o[:2]
    (d.pk_gs, d.pk_hs, d.pk_rs), (d.pv_gs, d.pv_hs, d.pv_rs) = prefix_lay
    d.n_seq, d.group_size, d.n_groups = n_seq, group_size, (n_seq + group_size - 1) // max(group_size, 1)
    d.heads, d.prefix_len, d.own_len, d.head_dim, d.scale = heads, prefix_len, own_len, hd, scale
    if steps:
        check(_lib.lib().mpv_attn_decode_shared_steps_fwd(C.byref(d), _p(glen), _p(gown), _stream()), "mpv_attn_decode_shared_steps_fwd")
    elif ragged:
        check(_lib.lib().mpv_attn_decode_shared_ragged_fwd(C.byref(d), _p(glen), _stream()), "mpv_attn_decode_shared_ragged_fwd")
    else:
        check(_lib.lib().mpv_attn_decode_shared_fwd(C.byref(d), _stream()), "mpv_attn_decode_shared_fwd")
    return o


TEMPORAL_SHORT_MAX_T = 16     # mpv_temporal_attn_fwd / _bwd: the VALU kernels
TEMPORAL_MAX_T = 64            # mpv_temporal_attn_long_fwd / _bwd: the matrix-core kernels (one or four 32 x 32 score tiles)


def _temporal_entry(T, short, long):
    """The entry point for a clip of T frames: the short family up to 16 frames (unchanged), the long one for 17..64."""
    if T > TEMPORAL_MAX_T:
        raise ValueError(f"temporal attention supports at most {TEMPORAL_MAX_T} frames per clip, got T={T}")
    return short if T <= TEMPORAL_SHORT_MAX_T else long


def temporal_attn_fwd(qkv, out, n_outer, outer_stride, n_inner, inner_offset, t_stride, T, heads, hd, scale):
    name = _temporal_entry(T, "mpv_temporal_attn_fwd", "mpv_temporal_attn_long_fwd")
    _need_cuda(qkv, out)
    check(getattr(_lib.lib(), name)(qkv.data_ptr(), out.data_ptr(), n_outer, outer_stride, n_inner, inner_offset,
                                    t_stride, T, heads, hd, scale, _stream()), name)


def temporal_attn_bwd(qkv, dout, dqkv, n_outer, outer_stride, n_inner, inner_offset, t_stride, T, heads, hd, scale):
    name = _temporal_entry(T, "mpv_temporal_attn_bwd", "mpv_temporal_attn_long_bwd")
    _need_cuda(qkv, dout, dqkv)
    check(getattr(_lib.lib(), name)(qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), n_outer, outer_stride, n_inner,
                                    inner_offset, t_stride, T, heads, hd, scale, _stream()), name)


def temporal_attn_long_plan(n_outer, n_inner, T, heads, hd, bwd=False):
    """What mpv_temporal_attn_long_fwd (bwd=False) / _bwd would launch (include/mpv.h: mpv_temporal_attn_long_plan_describe):
    dict(variant, grid, block, lds_bytes, lds_limit).  Launches nothing; for tests and tools."""
    info = _lib.AttnPlanInfo()
    check(_lib.lib().mpv_temporal_attn_long_plan_describe(n_outer, n_inner, T, heads, hd, int(bool(bwd)), C.byref(info)),
          "mpv_temporal_attn_long_plan_describe")
    return dict(variant=info.variant.decode(), grid=(info.grid_x, info.grid_y), block=info.block, lds_bytes=info.lds_bytes,
                lds_limit=info.lds_limit)


def im2col_patches(video, B, Cc, T, H, W, P, kpad):
    _need_cuda(video)
    rows = B * T * (H // P) * (W // P)
    cols = torch.empty((rows, kpad), dtype=torch.bfloat16, device=video.device)
    check(_lib.lib().mpv_im2col_patches(video.data_ptr(), cols.data_ptr(), B, Cc, T, H, W, P, kpad, _stream()),
          "mpv_im2col_patches")
    return cols


def vit_embed_assemble_fwd(patch, cls_token, pos_embed, temporal_embed, B, T, N, D):
    x = torch.empty((B * T * (N + 1), D), dtype=torch.bfloat16, device=patch.device)
    check(_lib.lib().mpv_vit_embed_assemble_fwd(patch.data_ptr(), cls_token.data_ptr(), pos_embed.data_ptr(),
                                                temporal_embed.data_ptr(), x.data_ptr(), B, T, N, D, _stream()),
          "mpv_vit_embed_assemble_fwd")
    return x


def vit_embed_assemble_bwd(dx, dpatch, dcls, dpos, dtemporal, B, T, N, D):
    check(_lib.lib().mpv_vit_embed_assemble_bwd(dx.data_ptr(), dpatch.data_ptr(), dcls.data_ptr(), dpos.data_ptr(),
                                                dtemporal.data_ptr(), B, T, N, D, _stream()), "mpv_vit_embed_assemble_bwd")


def vit_cls_merge_fwd(xt, a, B, T, N1, D, out=None):
    y = out if out is not None else torch.empty_like(xt)
    check(_lib.lib().mpv_vit_cls_merge_fwd(xt.data_ptr(), a.data_ptr(), y.data_ptr(), B, T, N1, D, _stream()),
          "mpv_vit_cls_merge_fwd")
    return y


def vit_cls_fix_fwd(xt, tap, y, B, T, N1, D):
    """y (= xt + a on all rows) gets its cls slots rewritten: xt_cls + bf16(mean_t tap)."""
    check(_lib.lib().mpv_vit_cls_fix_fwd(xt.data_ptr(), tap.data_ptr(), y.data_ptr(), B, T, N1, D, _stream()), "mpv_vit_cls_fix_fwd")
    return y


def vit_cls_merge_bwd_inplace(dy, B, T, N1, D):
    """dy's cls rows <- their mean over t, in place; returns the saved originals [B*T, D] (restore with copy_rows)."""
    saved = torch.empty((B * T, D), dtype=torch.bfloat16, device=dy.device)
    check(_lib.lib().mpv_vit_cls_merge_bwd_inplace(dy.data_ptr(), saved.data_ptr(), B, T, N1, D, _stream()),
          "mpv_vit_cls_merge_bwd_inplace")
    return saved


def vit_cls_merge_bwd(dy, B, T, N1, D, out=None):
    da = out if out is not None else torch.empty_like(dy)
    check(_lib.lib().mpv_vit_cls_merge_bwd(dy.data_ptr(), da.data_ptr(), B, T, N1, D, _stream()), "mpv_vit_cls_merge_bwd")
    return da


def copy_rows(src, dst, rows, cols, smap: RowMap = IDENT, dmap: RowMap = IDENT, lds=None, ldd=None):
    check(_lib.lib().mpv_copy_rows(src.data_ptr(), dst.data_ptr(), rows, cols, lds or cols, ldd or cols, *smap, *dmap,
                                   _stream()), "mpv_copy_rows")
    return dst


def colsum(x, rows, cols, *, out=None, ld=None, rmap: RowMap = IDENT, accumulate=False):
    if out is None:
        out = torch.empty(cols, dtype=torch.bfloat16, device=x.device)
    wsn = _lib.lib().mpv_colsum_workspace_size(cols)
    ws = workspace(wsn, x.device)
    check(_lib.lib().mpv_colsum(x.data_ptr(), out.data_ptr(), rows, cols, ld or cols, *rmap, int(accumulate), ws.data_ptr(),
                                ws.numel(), _stream()), "mpv_colsum")
    return out


def add(a, b, out=None):
    out = out if out is not None else torch.empty_like(a)
    check(_lib.lib().mpv_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "mpv_add")
    return out


def accum_f32(acc, g, first: bool):
    """acc (fp32) = g if first else acc + g, g bf16: the gradient-accumulation window sum."""
    check(_lib.lib().mpv_accum_f32(acc.data_ptr(), g.data_ptr(), g.numel(), int(first), _stream()), "mpv_accum_f32")
    return acc


def f32_to_bf16(src, dst):
    check(_lib.lib().mpv_f32_to_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), _stream()), "mpv_f32_to_bf16")
    return dst


def copy_segments(pairs):
    """[(src, dst), ...] of equally sized contiguous bf16 tensors: dst[i] <- src[i], one launch."""
    n = len(pairs)
    if n == 0:
        return
    vp, lp = C.c_void_p * n, C.c_int64 * n
    check(_lib.lib().mpv_copy_segments(vp(*[s.data_ptr() for s, _ in pairs]), vp(*[d.data_ptr() for _, d in pairs]),
                                       lp(*[d.numel() for _, d in pairs]), n, _stream()), "mpv_copy_segments")


def vit_compose_bwd_finish(dwc_wpT, dbc, bp, wf, dwf, dbp, D):
    """dwf <- bf16(float(dwc_wpT) + dbc (x) bp);  dbp <- Wf^T dbc  (include/mpv.h: mpv_vit_compose_bwd_finish)."""
    check(_lib.lib().mpv_vit_compose_bwd_finish(dwc_wpT.data_ptr(), dbc.data_ptr(), bp.data_ptr(), wf.data_ptr(), dwf.data_ptr(),
                                                dbp.data_ptr(), D, _stream()), "mpv_vit_compose_bwd_finish")


def _ptr_table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def gemm_batched(a_list, b_list, c_list, M, N, K, trans_a=False, trans_b=False):
    """c_list[i] <- a_list[i] op b_list[i] for every i in ONE launch (include/mpv.h: mpv_gemm_bf16_batched): mpv_gemm_bf16's operand
    forms, one shape, contiguous bf16 operands, plain epilogue."""
    global gemm_calls
    n = len(a_list)
    assert n == len(b_list) == len(c_list) and n > 0
    _need_cuda(*a_list, *b_list, *c_list)
    lda = M if trans_a else K
    ldb = N if trans_b else K
    gemm_calls += 1
    check(_lib.lib().mpv_gemm_bf16_batched(_ptr_table(a_list), _ptr_table(b_list), _ptr_table(c_list), n, M, N, K, lda, ldb, N,
                                           int(trans_a), int(trans_b), _stream()), "mpv_gemm_bf16_batched")
    return c_list


def vit_compose_bias_batched(wf_list, bp_list, bf_list, bc_list, D):
    """bc[i] <- bf16(Wf[i] bp[i] + bf[i]) for every block in one launch (include/mpv.h: mpv_vit_compose_bias_batched)."""
    _need_cuda(*wf_list, *bp_list, *bf_list, *bc_list)
    check(_lib.lib().mpv_vit_compose_bias_batched(_ptr_table(wf_list), _ptr_table(bp_list), _ptr_table(bf_list), _ptr_table(bc_list),
                                                  len(wf_list), D, _stream()), "mpv_vit_compose_bias_batched")


def vit_compose_bwd_finish_batched(dwc_wpT, dbc, bp, wf, dwf, dbp, D):
    """mpv_vit_compose_bwd_finish for every block in one launch (lists of tensors)."""
    _need_cuda(*dwc_wpT, *dbc, *bp, *wf, *dwf, *dbp)
    check(_lib.lib().mpv_vit_compose_bwd_finish_batched(_ptr_table(dwc_wpT), _ptr_table(dbc), _ptr_table(bp), _ptr_table(wf), _ptr_table(dwf),
                                                        _ptr_table(dbp), len(wf), D, _stream()), "mpv_vit_compose_bwd_finish_batched")


def caption_targets(ids, attention_mask, prompt_len=None):
    """-> (labels int64 [B*L], weights fp32 [B*L]) of the L text positions (include/mpv.h: mpv_caption_targets)."""
    _need_cuda(ids, attention_mask)
    B, L = ids.shape
    labels = torch.empty(B * L, dtype=torch.long, device=ids.device)
    weights = torch.empty(B * L, dtype=torch.float32, device=ids.device)
    check(_lib.lib().mpv_caption_targets(ids.contiguous().data_ptr(), attention_mask.contiguous().data_ptr(), _p(prompt_len), B, L,
                                         labels.data_ptr(), weights.data_ptr(), _stream()), "mpv_caption_targets")
    return labels, weights


def gpt_embed_fwd(query, ids, wte, wpe, B, Q, L, H, dropout_p=0.0, seed=0, offset=0):
    if Q + L > wpe.shape[0]:      # nn.Embedding would raise on the position ids (models/modeling_distributed_gpt3.py:640-666)
        raise _lib.MpvError(f"sequence of {Q + L} positions exceeds max_position_embeddings = {wpe.shape[0]}")
    h = torch.empty((B * (Q + L), H), dtype=torch.bfloat16, device=wte.device)
    check(_lib.lib().mpv_gpt_embed_fwd(_p(query), ids.data_ptr(), wte.data_ptr(), wpe.data_ptr(), h.data_ptr(), B, Q, L, H,
                                       dropout_p, seed, offset, _stream()), "mpv_gpt_embed_fwd")
    return h


def gpt_embed_rows_fwd(ids, pos, pos_host, wte, wpe, rows, H):
    """out[r] = wte[ids[r]] + wpe[pos[r]] for packed rows (ids int64 [rows], pos int32 [rows] on the device; include/mpv.h:
    mpv_gpt_embed_rows_fwd).  pos_host: the same positions as a host list -- they are checked against wpe here, without a sync."""
    if len(pos_host) != rows or min(pos_host) < 0:
        raise _lib.MpvError(f"{len(pos_host)} host positions (smallest {min(pos_host, default=0)}) for {rows} rows")
    if max(pos_host) >= wpe.shape[0]:      # nn.Embedding would raise on the position ids
        raise _lib.MpvError(f"sequence of {max(pos_host) + 1} positions exceeds max_position_embeddings = {wpe.shape[0]}")
    _need_cuda(ids, pos, wte, wpe)
    out = torch.empty((rows, H), dtype=torch.bfloat16, device=wte.device)
    check(_lib.lib().mpv_gpt_embed_rows_fwd(ids.data_ptr(), pos.data_ptr(), wte.data_ptr(), wpe.data_ptr(), out.data_ptr(), rows, H,
                                            wpe.shape[0], _stream()), "mpv_gpt_embed_rows_fwd")
    return out


def gpt_embed_bwd_full(dh, rows, H, dropout_p=0.0, seed=0, offset=0):
    """dropout-masked gradient of every row of the embedding output (trainable decoder): include/mpv.h"""
    out = torch.empty((rows, H), dtype=torch.bfloat16, device=dh.device)
    check(_lib.lib().mpv_gpt_embed_bwd_full(dh.data_ptr(), out.data_ptr(), rows, H, dropout_p, seed, offset, _stream()), "mpv_gpt_embed_bwd_full")
    return out


def gpt_embed_bwd(dh, B, Q, L, H, dropout_p=0.0, seed=0, offset=0):
    dq = torch.empty((B * Q, H), dtype=torch.bfloat16, device=dh.device)
    check(_lib.lib().mpv_gpt_embed_bwd(dh.data_ptr(), dq.data_ptr(), B, Q, L, H, dropout_p, seed, offset, _stream()),
          "mpv_gpt_embed_bwd")
    return dq


def cross_entropy(logits, labels, weight, rows, vocab, *, ld=None, dlogits=None, want_losses=True):
    """Returns (losses[rows] fp32, loss_sum fp32 scalar tensor)."""
    losses = torch.empty(rows, dtype=torch.float32, device=logits.device) if want_losses else None
    loss_sum = torch.zeros((), dtype=torch.float32, device=logits.device)
    check(_lib.lib().mpv_cross_entropy(logits.data_ptr(), labels.data_ptr(), _p(weight), _p(losses), loss_sum.data_ptr(),
                                       _p(dlogits), rows, vocab, ld or vocab, _stream()), "mpv_cross_entropy")
    return losses, loss_sum


def grad_sumsq(grad_flat, sumsq):
    """sumsq += sum g^2, bit-reproducible (include/mpv.h: per-workgroup partials in the workspace, added in a fixed order)"""
    ws = workspace(_lib.lib().mpv_grad_sumsq_workspace_size(), grad_flat.device)
    check(_lib.lib().mpv_grad_sumsq(grad_flat.data_ptr(), grad_flat.numel(), sumsq.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "mpv_grad_sumsq")


def adamw_step(p16, master, m, v, g16, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, sumsq=None, max_norm=0.0):
    check(_lib.lib().mpv_adamw_step(p16.data_ptr(), master.data_ptr(), m.data_ptr(), v.data_ptr(), g16.data_ptr(), p16.numel(),
                                    lr, beta1, beta2, eps, wd, step, grad_scale, _p(sumsq), max_norm, _stream()),
          "mpv_adamw_step")


def adamw_step_grouped(p16, master, m, v, g16, tile_group, lrs, wds, beta1, beta2, eps, step, grad_scale=1.0, sumsq=None,
                       max_norm=0.0):
    n = len(lrs)
    arr = (C.c_float * n)
    check(_lib.lib().mpv_adamw_step_grouped(p16.data_ptr(), master.data_ptr(), m.data_ptr(), v.data_ptr(), g16.data_ptr(),
                                            p16.numel(), tile_group.data_ptr(), arr(*lrs), arr(*wds), n, beta1, beta2, eps, step,
                                            grad_scale, _p(sumsq), max_norm, _stream()), "mpv_adamw_step_grouped")


def store_words(dst: torch.Tensor, words):
    """dst (device, 4-byte aligned) <- up to 32 32-bit words, by value in the launch (include/mpv.h: mpv_store_words)"""
    n = len(words)
    check(_lib.lib().mpv_store_words(dst.data_ptr(), (C.c_uint32 * n)(*words), n, _stream()), "mpv_store_words")


def store_u64(dst: torch.Tensor, values):
    words = []
    for v in values:
        v &= 0xFFFFFFFFFFFFFFFF
        words += [v & 0xFFFFFFFF, v >> 32]
    store_words(dst, words)


def adamw_hyper_upload(lrs, wds, beta1, beta2, step, hyper_dev: torch.Tensor):
    """hyper_dev (device float32[18]) <- lr[8], wd[8], 1/(1-beta1^step), 1/sqrt(1-beta2^step), exactly as the by-value entry computes them"""
    n = len(lrs)
    arr = (C.c_float * n)
    out = (C.c_float * 18)()
    check(_lib.lib().mpv_adamw_hyper_pack(arr(*lrs), arr(*wds), n, beta1, beta2, step, out), "mpv_adamw_hyper_pack")
    store_words(hyper_dev, list((C.c_uint32 * 18).from_buffer(out)))


def adamw_step_grouped_dev(p16, master, m, v, g16, tile_group, hyper_dev, beta1, beta2, eps, grad_scale=1.0, sumsq=None, max_norm=0.0):
    """adamw_step_grouped with lr / weight decay / bias corrections read from device memory (hyper_dev float32[18]): include/mpv.h"""
    check(_lib.lib().mpv_adamw_step_grouped_dev(p16.data_ptr(), master.data_ptr(), m.data_ptr(), v.data_ptr(), g16.data_ptr(),
                                                p16.numel(), tile_group.data_ptr(), hyper_dev.data_ptr(), beta1, beta2, eps, grad_scale,
                                                _p(sumsq), max_norm, _stream()), "mpv_adamw_step_grouped_dev")


def l2norm_fwd(x, rows, cols, eps=1e-12):
    y = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    nrm = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(_lib.lib().mpv_l2norm_fwd(x.data_ptr(), y.data_ptr(), nrm.data_ptr(), rows, cols, eps, _stream()), "mpv_l2norm_fwd")
    return y, nrm


def l2norm_bwd(dy, x, nrm, rows, cols):
    dx = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    check(_lib.lib().mpv_l2norm_bwd(dy.data_ptr(), x.data_ptr(), nrm.data_ptr(), dx.data_ptr(), rows, cols, _stream()), "mpv_l2norm_bwd")
    return dx


def gather_rows(src, idx, rows, cols, ld=None):
    dst = torch.empty((rows, cols), dtype=torch.bfloat16, device=src.device)
    check(_lib.lib().mpv_gather_rows(src.data_ptr(), idx.data_ptr(), dst.data_ptr(), rows, cols, ld or cols, _stream()), "mpv_gather_rows")
    return dst


def scatter_rows(src, idx, dst, rows, cols, ld=None):
    check(_lib.lib().mpv_scatter_rows(src.data_ptr(), idx.data_ptr(), dst.data_ptr(), rows, cols, ld or cols, _stream()), "mpv_scatter_rows")
    return dst


def quantize_rows_e4m3(w: torch.Tensor, N: Optional[int] = None, K: Optional[int] = None, ldw: Optional[int] = None):
    """include/mpv.h mpv_quantize_rows_e4m3: w [N, K] bf16 (row pitch ldw) -> (codes uint8 [N, K], scale fp32 [N]); e4m3fn codes of
    w / scale with scale the power of two of the contract ("FP8 decoder weights")."""
    _need_cuda(w)
    N = w.shape[0] if N is None else N
    K = w.shape[1] if K is None else K
    ldw = (w.stride(0) if w.dim() == 2 else K) if ldw is None else ldw
    codes = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    scale = torch.empty((N,), dtype=torch.float32, device=w.device)
    check(_lib.lib().mpv_quantize_rows_e4m3(w.data_ptr(), N, K, ldw, codes.data_ptr(), scale.data_ptr(), _stream()), "mpv_quantize_rows_e4m3")
    return codes, scale


def gpt_embed_rows_w8_fwd(ids, pos, pos_host, codes, scale, wpe, rows, H):
    """gpt_embed_rows_fwd with the token rows read as deq(code) * scale from the tied embedding's codes (uint8 [vocab, H]) and scales
    (fp32 [vocab]); include/mpv.h: mpv_gpt_embed_rows_w8_fwd.  pos_host is checked against wpe as there."""
    if len(pos_host) != rows or min(pos_host) < 0:
        raise _lib.MpvError(f"{len(pos_host)} host positions (smallest {min(pos_host, default=0)}) for {rows} rows")
    if max(pos_host) >= wpe.shape[0]:
        raise _lib.MpvError(f"sequence of {max(pos_host) + 1} positions exceeds max_position_embeddings = {wpe.shape[0]}")
    _need_cuda(ids, pos, codes, scale, wpe)
    out = torch.empty((rows, H), dtype=torch.bfloat16, device=wpe.device)
    check(_lib.lib().mpv_gpt_embed_rows_w8_fwd(ids.data_ptr(), pos.data_ptr(), codes.data_ptr(), scale.data_ptr(), wpe.data_ptr(),
                                               out.data_ptr(), rows, H, wpe.shape[0], _stream()), "mpv_gpt_embed_rows_w8_fwd")
    return out


def _gemm_w8(entry, a, codes, scale, M, N, K, out, lda, ldw, ldc, bias, act, residual, ldr, cmap, out_rows, other, tail=()):
    _need_cuda(a, codes, scale)
    ldc = ldc if ldc is not None else N
    if out is None:
        out = torch.empty((out_rows if out_rows is not None else M, ldc), dtype=torch.bfloat16, device=a.device)
    ep = GemmEpilogue()
    ep.c_group, ep.c_stride, ep.c_offset = cmap
    ep.bias, ep.act, ep.residual, ep.ldr = _p(bias), act, _p(residual), ldr
    for k, v in other.items():
        setattr(ep, k, v)
    check(getattr(_lib.lib(), entry)(a.data_ptr(), codes.data_ptr(), scale.data_ptr(), out.data_ptr(), M, N, K, lda if lda is not None else K,
                                     ldw if ldw is not None else K, ldc, C.byref(ep), *tail, _stream()), entry)
    return out


def gemm_w8(a: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor, M: int, N: int, K: int, *, out: Optional[torch.Tensor] = None,
            lda: Optional[int] = None, ldw: Optional[int] = None, ldc: Optional[int] = None, bias=None, act: int = 0, residual=None,
            ldr: int = 0, cmap: RowMap = IDENT, out_rows: Optional[int] = None, **other) -> torch.Tensor:
    """include/mpv.h mpv_gemm_w8: C[M, N] = epi(scale[n] * sum_k A[m, k] deq(codes[n, k])), 1 <= M <= 512, the decode step's
    epilogues only (bias, act = ACT_GELU_TANH, residual / ldr, cmap).  `other`: further GemmEpilogue fields by name -- the library
    refuses every one of them."""
    return _gemm_w8("mpv_gemm_w8", a, codes, scale, M, N, K, out, lda, ldw, ldc, bias, act, residual, ldr, cmap, out_rows, other)


def gemm_w8_tiled(a: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor, M: int, N: int, K: int, *, out: Optional[torch.Tensor] = None,
                  lda: Optional[int] = None, ldw: Optional[int] = None, ldc: Optional[int] = None, bias=None, act: int = 0, residual=None,
                  ldr: int = 0, cmap: RowMap = IDENT, out_rows: Optional[int] = None, use_workspace: bool = True, **other) -> torch.Tensor:
    """include/mpv.h mpv_gemm_w8_tiled: gemm_w8's product, keywords and refusals on the kernel built for 97-512 rows.
    use_workspace=False passes a null workspace (the result is the same bits)."""
    ws = workspace(1, a.device) if use_workspace and a.is_cuda else None
    return _gemm_w8("mpv_gemm_w8_tiled", a, codes, scale, M, N, K, out, lda, ldw, ldc, bias, act, residual, ldr, cmap, out_rows, other,
                    (_p(ws), ws.numel() if ws is not None else 0))


def gather_rows_ld(src, idx, dst, rows, cols, lds, ldd):
    check(_lib.lib().mpv_gather_rows_ld(src.data_ptr(), idx.data_ptr(), dst.data_ptr(), rows, cols, lds, ldd, _stream()), "mpv_gather_rows_ld")
    return dst


def logprob_topk(logits, k, add=None, rows=None, vocab=None, ld=None):
    """-> (values fp32 [rows,k], indices int64 [rows,k]) of log_softmax(logits) + add[:,None], descending."""
    rows = rows if rows is not None else logits.shape[0]
    vocab = vocab if vocab is not None else logits.shape[-1]
    val = torch.empty((rows, k), dtype=torch.float32, device=logits.device)
    idx = torch.empty((rows, k), dtype=torch.int64, device=logits.device)
    ws = workspace(_lib.lib().mpv_logprob_topk_workspace_size(rows, k), logits.device)
    check(_lib.lib().mpv_logprob_topk(logits.data_ptr(), _p(add), rows, vocab, ld or vocab, k, val.data_ptr(), idx.data_ptr(),
                                      ws.data_ptr(), ws.numel(), _stream()), "mpv_logprob_topk")
    return val, idx


def _beam_advance(who, d, m, cand_val, cand_idx, st, vocab, pos, cur_len, first, stop_token, more=()):
    """beam_advance / beam_advance_groups / beam_advance_steps on the descriptor d (batch, and what the entry adds, are set): checks the
    candidates against [rows, m], fills d from the state and the step, calls mpv_<who> (`more`: the arguments behind the descriptor)
    and swaps the token tables"""
    rows = st.batch * st.beams
    if (cand_val.dtype, cand_idx.dtype) != (torch.float32, torch.int64) or tuple(cand_val.shape) != (rows, m) or \
            tuple(cand_idx.shape) != (rows, m) or not (cand_val.is_contiguous() and cand_idx.is_contiguous()):
        raise _lib.MpvError(f"{who}: candidates must be contiguous fp32 / int64 [{rows}, {m}] "
                            f"(got {cand_val.dtype} {tuple(cand_val.shape)}, {cand_idx.dtype} {tuple(cand_idx.shape)})")
    d.cand_val, d.cand_idx, d.tokens_in, d.tokens_out = cand_val.data_ptr(), cand_idx.data_ptr(), st.tokens.data_ptr(), st.tokens_alt.data_ptr()
    for n in ("scores", "hyp_score", "hyp_order", "hyp_tokens", "hyp_count", "hyp_next", "worst", "done", "src_row", "next_tok"):
        setattr(d, n, getattr(st, n).data_ptr())
    d.beams, d.row_len, d.vocab, d.pos, d.cur_len, d.first, d.stop_token = st.beams, st.row_len, int(vocab), int(pos), int(cur_len), int(bool(first)), int(stop_token)
    check(getattr(_lib.lib(), "mpv_" + who)(C.byref(d), *more, _stream()), "mpv_" + who)
    st.tokens, st.tokens_alt = st.tokens_alt, st.tokens
    return st.src_row, st.next_tok


def beam_advance(cand_val, cand_idx, st, *, vocab, pos, cur_len, first, stop_token):
    """One position of the lockstep beam search over st.batch clips x st.beams beams (include/mpv.h: mpv_beam_advance; st is a
    generation.BeamState).  cand_val fp32 / cand_idx int64 [batch * beams, 2 * beams]: logprob_topk(logits, 2 * beams, add=st.scores).
    Updates the state in place, fills st.src_row / st.next_tok and swaps st.tokens with st.tokens_alt."""
    _need_cuda(cand_val, cand_idx, st.tokens)
    return _beam_advance("beam_advance", _lib.BeamAdvanceDesc(batch=st.batch), 2 * st.beams, cand_val, cand_idx, st, vocab, pos, cur_len, first,
                         stop_token)


def beam_advance_groups(cand_val, cand_idx, st, *, groups, diversity_penalty, vocab, pos, cur_len, first, stop_token):
    """One position of the lockstep GROUP beam search (include/mpv.h: mpv_beam_advance_groups): st is a generation.BeamState whose
    st.batch pseudo-clips are (clip, group) pairs, `groups` consecutive ones per clip, of st.beams beams each.  cand_val fp32 /
    cand_idx int64 [st.batch * st.beams, m], m = (groups + 1) * st.beams: logprob_topk(logits, m, add=st.scores).  Updates the state
    in place, fills st.src_row / st.next_tok and swaps st.tokens with st.tokens_alt, as beam_advance does."""
    _need_cuda(cand_val, cand_idx, st.tokens)
    groups = int(groups)
    if groups < 1 or st.batch % groups:
        raise _lib.MpvError(f"beam_advance_groups: the state's {st.batch} (clip, group) pairs are no multiple of groups = {groups}")
    d = _lib.BeamAdvanceGroupsDesc(batch=st.batch // groups, groups=groups, diversity_penalty=float(diversity_penalty))
    return _beam_advance("beam_advance_groups", d, (groups + 1) * st.beams, cand_val, cand_idx, st, vocab, pos, cur_len, first, stop_token)


def beam_advance_steps(cand_val, cand_idx, st, *, groups=1, diversity_penalty=0.0, vocab, clip_prompt_len, clip_step, stop_token):
    """beam_advance (groups = 1) / beam_advance_groups with a generation step per clip (include/mpv.h: mpv_beam_advance_steps; clips
    that entered a running search at different times): clip_prompt_len / clip_step int32 [st.batch // groups] on the device, one value
    per real clip; the table is left-aligned and clip c works on column clip_prompt_len[c] + clip_step[c] with cur_len =
    clip_step[c] + 1.  A clip with a negative step, or whose column lies behind the table, is frozen with all its groups."""
    _need_cuda(cand_val, cand_idx, st.tokens, clip_prompt_len, clip_step)
    groups = int(groups)
    if groups < 1 or st.batch % groups:
        raise _lib.MpvError(f"beam_advance_steps: the state's {st.batch} (clip, group) pairs are no multiple of groups = {groups}")
    clips = st.batch // groups
    for name, t in (("clip_prompt_len", clip_prompt_len), ("clip_step", clip_step)):
        if t is not None and (t.dtype != torch.int32 or t.numel() != clips or not t.is_contiguous()):
            raise _lib.MpvError(f"beam_advance_steps: {name} must be a contiguous int32 tensor of {clips} values")
    d = _lib.BeamAdvanceGroupsDesc(batch=clips, groups=groups, diversity_penalty=float(diversity_penalty))
    return _beam_advance("beam_advance_steps", d, (groups + 1) * st.beams, cand_val, cand_idx, st, vocab, 0, 0, False, stop_token,
                         (_p(clip_prompt_len), _p(clip_step)))


def kv_suffix_reorder_steps(src, dst, idx, group_rows, *, fan, suffix_rows, max_rows):
    """The beam re-order of the in-flight suffix cache in one launch over all layers (include/mpv.h: mpv_kv_suffix_reorder_steps): src /
    dst bf16 [nl, n_groups * fan * suffix_rows, 3H]; sequence j of clip g = j // fan gets the first clamp(group_rows[g], 0, max_rows)
    suffix rows of sequence idx[j] (int64 [n_groups * fan], inside the clip); group_rows int32 [n_groups].  -> dst"""
    _need_cuda(src, dst, idx, group_rows)
    ok = src is not None and dst is not None and src.dtype == dst.dtype == torch.bfloat16 and src.dim() == 3 and src.shape == dst.shape and \
        src.is_contiguous() and dst.is_contiguous() and src.shape[2] % 3 == 0 and src.shape[1] % (int(fan) * int(suffix_rows)) == 0
    if not ok:
        raise _lib.MpvError(f"kv_suffix_reorder_steps: src and dst must be contiguous bf16 [nl, n_groups * {fan} * {suffix_rows}, 3H] of one shape")
    nl, n_groups, hidden = src.shape[0], src.shape[1] // (int(fan) * int(suffix_rows)), src.shape[2] // 3
    if idx is not None and (idx.dtype != torch.int64 or idx.numel() != n_groups * int(fan) or not idx.is_contiguous()):
        raise _lib.MpvError(f"kv_suffix_reorder_steps: idx must be a contiguous int64 tensor of {n_groups * int(fan)} rows")
    if group_rows is not None and (group_rows.dtype != torch.int32 or group_rows.numel() != n_groups or not group_rows.is_contiguous()):
        raise _lib.MpvError(f"kv_suffix_reorder_steps: group_rows must be a contiguous int32 tensor of {n_groups} counts")
    check(_lib.lib().mpv_kv_suffix_reorder_steps(src.data_ptr(), dst.data_ptr(), nl, n_groups, int(fan), int(suffix_rows), _p(idx), _p(group_rows),
                                                 int(max_rows), hidden, _stream()), "mpv_kv_suffix_reorder_steps")
    return dst


TERMINATION_ID, TERMINATION_EOL, TERMINATION_DOUBLE_EOL = 0, 1, 2     # mpv_sample_advance_desc.termination_mode


def sample_advance_desc(logits, st, *, pos, temperature=1.0, top_k=0, top_p=0.0, seed=0, vocab_size=None, termination_mode=TERMINATION_ID,
                        termination_id=0, u_override=None, out_kept=None, out_mass=None, out_token=None, vocab=None, ld=None):
    """The descriptor of one mpv_sample_advance call (include/mpv.h) for logits bf16 [rows, ld] and a generation.SampleState."""
    d = _lib.SampleAdvanceDesc()
    d.logits, d.stream_id, d.u_override, d.prompt_len = _p(logits), _p(st.stream), _p(u_override), _p(st.prompt_len)
    d.tokens, d.done, d.next_tok, d.n_done = _p(st.tokens), _p(st.done), _p(st.next_tok), _p(st.n_done)
    d.out_kept, d.out_mass, d.out_token = _p(out_kept), _p(out_mass), _p(out_token)
    d.ld = int(ld) if ld is not None else (logits.stride(0) if logits is not None else 0)
    d.seed, d.termination_id = int(seed) & 0xFFFFFFFFFFFFFFFF, int(termination_id)
    d.rows, d.row_len, d.pos = st.rows, st.row_len, int(pos)
    d.vocab = int(vocab) if vocab is not None else (logits.shape[-1] if logits is not None else 0)
    d.top_k, d.vocab_size, d.termination_mode = int(top_k), int(vocab_size or 0), int(termination_mode)
    d.temperature, d.top_p = float(temperature), float(top_p)
    return d


def _where(entry, rows, pos, step, row_step):
    """How the three forms of a sampler entry say on which column a row works -> (the descriptor's pos, the arguments behind the
    descriptor): the uniform form a column `pos` for all rows; the ragged form a generation `step` in the descriptor's pos (row r:
    column prompt_len[r] + step); the steps form, neither given, row_step int32 [rows] on the device behind the descriptor"""
    if pos is not None or step is not None:
        return int(step if pos is None else pos), ()
    if row_step is None or row_step.dtype != torch.int32 or row_step.numel() != rows or not row_step.is_contiguous():
        raise _lib.MpvError(f"{entry}: row_step must be a contiguous int32 tensor of {rows} steps")
    _need_cuda(row_step)
    return 0, (_p(row_step),)


def _sample_advance(entry, logits, st, *, pos=None, step=None, row_step=None, u_override=None, out_kept=None, out_mass=None, out_token=None,
                    **desc):
    """the body of sample_advance, sample_advance_ragged and sample_advance_steps, which pass all their arguments on: `entry` is the C
    entry's name without the mpv_ prefix, `desc` what sample_advance_desc takes besides"""
    _need_cuda(logits, st.tokens, u_override, out_kept, out_mass, out_token)
    pos, more = _where(entry, st.rows, pos, step, row_step)
    if logits.dtype != torch.bfloat16 or logits.ndim != 2 or logits.shape[0] < st.rows or logits.stride(1) != 1:
        raise _lib.MpvError(f"{entry}: logits must be bf16 [{st.rows}, ld] with unit column stride (got {logits.dtype} {tuple(logits.shape)})")
    for name, t, dt in (("u_override", u_override, torch.float32), ("out_kept", out_kept, torch.int32), ("out_mass", out_mass, torch.float32),
                        ("out_token", out_token, torch.int64)):
        if t is not None and (t.dtype != dt or t.numel() < st.rows or not t.is_contiguous()):
            raise _lib.MpvError(f"{entry}: {name} must be contiguous {dt} [{st.rows}]")
    d = sample_advance_desc(logits, st, pos=pos, u_override=u_override, out_kept=out_kept, out_mass=out_mass, out_token=out_token, **desc)
    check(getattr(_lib.lib(), "mpv_" + entry)(C.byref(d), *more, _stream()), "mpv_" + entry)
    return st.next_tok


def sample_advance(logits, st, *, pos, temperature=1.0, top_k=0, top_p=0.0, seed=0, vocab_size=None, termination_mode=TERMINATION_ID,
                   termination_id=0, u_override=None, out_kept=None, out_mass=None, out_token=None, vocab=None, ld=None):
    """One position of sampled generation for st.rows sequences in one launch (include/mpv.h: mpv_sample_advance; st is a
    generation.SampleState): temperature, the top-k / top-p filter, the draw with the counter-based uniform of (seed, pos, st.stream),
    the write into st.tokens[:, pos] behind the prompt, st.next_tok, st.done and st.n_done.  logits bf16 [rows, ld], the first `vocab`
    columns are read.  u_override fp32 [rows] replaces the uniform; out_kept int32 / out_mass fp32 / out_token int64 [rows] are optional
    diagnostics.  -> st.next_tok"""
    return _sample_advance("sample_advance", **locals())


def sample_advance_ragged(logits, st, *, step, temperature=1.0, top_k=0, top_p=0.0, seed=0, vocab_size=None, termination_mode=TERMINATION_ID,
                          termination_id=0, u_override=None, out_kept=None, out_mass=None, out_token=None, vocab=None, ld=None):
    """sample_advance for a LEFT-ALIGNED table of prompts of different lengths (include/mpv.h: mpv_sample_advance_ragged): generation
    step `step` >= 0; row r draws, with the counter of its own column st.prompt_len[r] + step, into st.tokens[r, that column].  A row
    whose column lies behind the table is frozen: nothing read or written but st.done[r] = 1 and st.next_tok[r] = its last token.
    -> st.next_tok"""
    return _sample_advance("sample_advance_ragged", **locals())


def sample_advance_steps(logits, st, *, row_step, temperature=1.0, top_k=0, top_p=0.0, seed=0, vocab_size=None, termination_mode=TERMINATION_ID,
                         termination_id=0, u_override=None, out_kept=None, out_mass=None, out_token=None, vocab=None, ld=None):
    """sample_advance_ragged with a generation step per row (include/mpv.h: mpv_sample_advance_steps; rows of clips that entered a
    running loop at different times): row_step int32 [rows] on the device; row r draws at column st.prompt_len[r] + row_step[r].  A
    row with a negative step, or whose column lies behind the table, is frozen.  -> st.next_tok"""
    return _sample_advance("sample_advance_steps", **locals())


def _constraint_ids(constraints, device, eos_ids):
    """(eos, banned) int64 device arrays of a generation.LogitsConstraints, made once per (device, eos_ids) and kept on the object"""
    key = (str(device), tuple(int(t) for t in eos_ids))
    hit = constraints._device_ids.get(key)
    if hit is None:
        hit = (torch.tensor(key[1], dtype=torch.int64, device=device), torch.tensor(constraints.banned_token_ids, dtype=torch.int64, device=device))
        constraints._device_ids[key] = hit
    return hit


def _logits_constrain(entry, logits, tokens, *, pos=None, step=None, row_step=None, constraints, prompt_len, prompt_len_all=0, eos_ids, ban_value,
                      vocab, ld):
    """the body of logits_constrain, logits_constrain_ragged and logits_constrain_steps, which pass all their arguments on: `entry` is
    the C entry's name without the mpv_ prefix"""
    if pos is None and prompt_len is None:                # a column per row is counted from the row's prompt length
        raise _lib.MpvError(f"{entry}: prompt_len int64 [rows] is required")
    _need_cuda(logits, tokens, prompt_len)
    if logits.dtype != torch.bfloat16 or logits.ndim != 2 or logits.stride(1) != 1:
        raise _lib.MpvError(f"{entry}: logits must be bf16 [rows, ld] with unit column stride (got {logits.dtype} {tuple(logits.shape)})")
    rows = logits.shape[0]
    if tokens.dtype != torch.int64 or tokens.ndim != 2 or tokens.shape[0] != rows or not tokens.is_contiguous():
        raise _lib.MpvError(f"{entry}: tokens must be contiguous int64 [{rows}, row_len] (got {tokens.dtype} {tuple(tokens.shape)})")
    if prompt_len is not None and (prompt_len.dtype != torch.int64 or prompt_len.numel() != rows or not prompt_len.is_contiguous()):
        raise _lib.MpvError(f"{entry}: prompt_len must be contiguous int64 [{rows}]")
    eos, banned = _constraint_ids(constraints, logits.device, eos_ids)
    pos, more = _where(entry, rows, pos, step, row_step)
    d = _lib.LogitsConstrainDesc()
    d.logits, d.tokens, d.prompt_len = _p(logits), _p(tokens), _p(prompt_len)
    d.eos_ids, d.banned_ids = (_p(eos) if eos.numel() else None), (_p(banned) if banned.numel() else None)
    d.ld, d.prompt_len_all = int(ld) if ld is not None else logits.stride(0), int(prompt_len_all)
    d.rows, d.vocab, d.row_len, d.pos = rows, int(vocab) if vocab is not None else logits.shape[-1], tokens.shape[1], int(pos)
    d.n_eos, d.n_banned, d.ngram, d.min_new_tokens = eos.numel(), banned.numel(), constraints.no_repeat_ngram_size, constraints.min_new_tokens
    d.include_prompt, d.penalty, d.ban_value = int(constraints.include_prompt), constraints.repetition_penalty, float(ban_value)
    check(getattr(_lib.lib(), "mpv_" + entry)(C.byref(d), *more, _stream()), "mpv_" + entry)
    return logits


def logits_constrain(logits, tokens, *, pos, constraints, prompt_len=None, prompt_len_all=0, eos_ids=(), ban_value=float("-inf"), vocab=None,
                     ld=None):
    """One step's generation constraints, in place and in one launch (include/mpv.h: mpv_logits_constrain; constraints is a
    generation.LogitsConstraints): repetition penalty, no-repeat n-gram, min_new_tokens (bans eos_ids while fewer tokens are generated)
    and the banned ids, on logits bf16 [rows, ld] (the first `vocab` columns) from the histories in tokens int64 [rows, row_len] below
    column `pos`.  prompt_len int64 [rows] (rows with prompt_len > pos are left alone), or None: prompt_len_all for every row.  A
    banned logit becomes ban_value (-inf for the sampler, the lowest finite bf16 in front of logprob_topk).  -> logits"""
    return _logits_constrain("logits_constrain", **locals())


def logits_constrain_ragged(logits, tokens, *, step, constraints, prompt_len, eos_ids=(), ban_value=float("-inf"), vocab=None, ld=None):
    """logits_constrain for a LEFT-ALIGNED table of prompts of different lengths (include/mpv.h: mpv_logits_constrain_ragged):
    generation step `step` >= 0; row r's history is tokens[r, start : prompt_len[r] + step] with start = 0 under include_prompt and
    prompt_len[r] otherwise, and `step` tokens count as generated.  prompt_len int64 [rows] is required.  A row whose column lies behind
    the table is left alone.  -> logits"""
    return _logits_constrain("logits_constrain_ragged", **locals())


def logits_constrain_steps(logits, tokens, *, row_step, constraints, prompt_len, eos_ids=(), ban_value=float("-inf"), vocab=None, ld=None):
    """logits_constrain_ragged with a generation step per row (include/mpv.h: mpv_logits_constrain_steps): row_step int32 [rows] on the
    device; row r's history ends in front of column prompt_len[r] + row_step[r] and row_step[r] tokens count as generated.  A row with
    a negative step, or whose column lies behind the table, is left alone.  -> logits"""
    return _logits_constrain("logits_constrain_steps", **locals())


def logits_guide(cond, uncond, *, scale, alpha=0.0, ban_value=float("-inf"), vocab=None):
    """One step's guidance, in place and in one launch (include/mpv.h: mpv_logits_guide): cond bf16 [rows, ld_c] becomes
    bf16(c + (scale - 1) * (c - u)) on the max-centred rows c, u of cond and uncond bf16 [rows, ld_u] (read only; it may be other rows
    of cond's allocation), over the first `vocab` columns.  alpha in (0, 1): a token whose conditional probability is below alpha times
    the row's largest becomes ban_value (-inf for the sampler, the lowest finite bf16 in front of logprob_topk); 0: off.  scale - 1 and
    log(alpha) are computed here, on the host, and passed as fp32.  -> cond"""
    _need_cuda(cond, uncond)
    for name, t in (("cond", cond), ("uncond", uncond)):
        if t.dtype != torch.bfloat16 or t.ndim != 2 or t.stride(1) != 1:
            raise _lib.MpvError(f"logits_guide: {name} must be bf16 [rows, ld] with unit column stride (got {t.dtype} {tuple(t.shape)})")
    if uncond.shape[0] != cond.shape[0]:
        raise _lib.MpvError(f"logits_guide: cond has {cond.shape[0]} rows, uncond {uncond.shape[0]}")
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:                           # (NaN fails both comparisons)
        raise _lib.MpvError(f"logits_guide: alpha ({alpha}) must be in [0, 1]")
    d = _lib.LogitsGuideDesc()
    d.cond, d.uncond, d.ld_c, d.ld_u = _p(cond), _p(uncond), cond.stride(0), uncond.stride(0)
    d.rows, d.vocab = cond.shape[0], int(vocab) if vocab is not None else min(cond.shape[-1], uncond.shape[-1])
    d.scale_m1, d.plaus_log, d.ban_value = float(scale) - 1.0, math.log(alpha) if alpha > 0.0 else float("-inf"), float(ban_value)
    check(_lib.lib().mpv_logits_guide(C.byref(d), _stream()), "mpv_logits_guide")
    return cond


def _logits_trie_mask(entry, logits, tokens, *, pos=None, step=None, row_step=None, trie, prompt_len, prompt_len_all=0, eos_ids, ban_value,
                      node_out, vocab, ld):
    """the body of logits_trie_mask, logits_trie_mask_ragged and logits_trie_mask_steps, which pass all their arguments on: `entry` is
    the C entry's name without the mpv_ prefix"""
    if pos is None and prompt_len is None:                # a column per row is counted from the row's prompt length
        raise _lib.MpvError(f"{entry}: prompt_len int64 [rows] is required")
    _need_cuda(logits, tokens, prompt_len, node_out)
    if logits.dtype != torch.bfloat16 or logits.ndim != 2 or logits.stride(1) != 1:
        raise _lib.MpvError(f"{entry}: logits must be bf16 [rows, ld] with unit column stride (got {logits.dtype} {tuple(logits.shape)})")
    rows = logits.shape[0]
    if tokens.dtype != torch.int64 or tokens.ndim != 2 or tokens.shape[0] != rows or not tokens.is_contiguous():
        raise _lib.MpvError(f"{entry}: tokens must be contiguous int64 [{rows}, row_len] (got {tokens.dtype} {tuple(tokens.shape)})")
    if prompt_len is not None and (prompt_len.dtype != torch.int64 or prompt_len.numel() != rows or not prompt_len.is_contiguous()):
        raise _lib.MpvError(f"{entry}: prompt_len must be contiguous int64 [{rows}]")
    if node_out is not None and (node_out.dtype != torch.int32 or node_out.numel() != rows or not node_out.is_contiguous()):
        raise _lib.MpvError(f"{entry}: node_out must be contiguous int32 [{rows}]")
    key = (str(logits.device), tuple(int(t) for t in eos_ids))
    eos = trie._device.get(key)                           # the termination ids on the device, made once per (device, ids) and kept on the trie
    if eos is None:
        eos = trie._device[key] = torch.tensor(key[1], dtype=torch.int64, device=logits.device)
    arrays = trie.arrays(logits.device)
    pos, more = _where(entry, rows, pos, step, row_step)
    d = _lib.LogitsTrieDesc()
    d.logits, d.tokens, d.prompt_len, d.eos_ids, d.node_out = _p(logits), _p(tokens), _p(prompt_len), (_p(eos) if eos.numel() else None), _p(node_out)
    d.child_begin, d.child_tok, d.child_node, d.terminal = (_p(a) for a in arrays)
    d.ld, d.prompt_len_all = int(ld) if ld is not None else logits.stride(0), int(prompt_len_all)
    d.rows, d.vocab, d.row_len, d.pos = rows, int(vocab) if vocab is not None else logits.shape[-1], tokens.shape[1], int(pos)
    d.n_eos, d.n_nodes, d.n_edges, d.ban_value = eos.numel(), trie.n_nodes, trie.n_edges, float(ban_value)
    check(getattr(_lib.lib(), "mpv_" + entry)(C.byref(d), *more, _stream()), "mpv_" + entry)
    return logits


def logits_trie_mask(logits, tokens, *, pos, trie, prompt_len=None, prompt_len_all=0, eos_ids, ban_value=float("-inf"), node_out=None, vocab=None,
                     ld=None):
    """One step's closed-vocabulary mask, in place and in one launch (include/mpv.h: mpv_logits_trie_mask; trie is a
    generation.PhraseTrie): in logits bf16 [rows, ld] (the first `vocab` columns) only the tokens that continue tokens[r, prompt_len[r] :
    pos] along the trie keep their bits -- and eos_ids where a phrase ends, or alone once the row has left the trie -- every other column
    becomes ban_value.  prompt_len int64 [rows] (rows with prompt_len > pos are left alone), or None: prompt_len_all for every row.
    node_out int32 [rows] (optional): the node every row stands on, -1 dead, -2 untouched.  -> logits"""
    return _logits_trie_mask("logits_trie_mask", **locals())


def logits_trie_mask_ragged(logits, tokens, *, step, trie, prompt_len, eos_ids, ban_value=float("-inf"), node_out=None, vocab=None, ld=None):
    """logits_trie_mask for a LEFT-ALIGNED table of prompts of different lengths (include/mpv.h: mpv_logits_trie_mask_ragged): row r
    works on column prompt_len[r] + step; a row whose column lies behind the table is left alone.  -> logits"""
    return _logits_trie_mask("logits_trie_mask_ragged", **locals())


def logits_trie_mask_steps(logits, tokens, *, row_step, trie, prompt_len, eos_ids, ban_value=float("-inf"), node_out=None, vocab=None, ld=None):
    """logits_trie_mask_ragged with a generation step per row (include/mpv.h: mpv_logits_trie_mask_steps): row_step int32 [rows] on the
    device; a row with a negative step, or whose column lies behind the table, is left alone.  -> logits"""
    return _logits_trie_mask("logits_trie_mask_steps", **locals())


def _sample_score(entry, logits, st, sc, *, pos=None, step=None, row_step=None, vocab, ld):
    """the body of sample_score, sample_score_ragged and sample_score_steps, which pass all their arguments on: `entry` is the C
    entry's name without the mpv_ prefix"""
    _need_cuda(logits, st.tokens, sc.token_logprob)
    if logits.dtype != torch.bfloat16 or logits.ndim != 2 or logits.shape[0] < st.rows or logits.stride(1) != 1:
        raise _lib.MpvError(f"{entry}: logits must be bf16 [{st.rows}, ld] with unit column stride (got {logits.dtype} {tuple(logits.shape)})")
    if sc.rows != st.rows or sc.row_len != st.row_len:
        raise _lib.MpvError(f"{entry}: scores of [{sc.rows}, {sc.row_len}] for a state of [{st.rows}, {st.row_len}]")
    for name, t, dt, shape in (("live", sc.live, torch.int32, (st.rows,)), ("token_logprob", sc.token_logprob, torch.float32, (st.rows, st.row_len)),
                               ("sum_logprob", sc.sum_logprob, torch.float32, (st.rows,)), ("count", sc.count, torch.int32, (st.rows,))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != logits.device:
            raise _lib.MpvError(f"{entry}: {name} must be contiguous {dt} {list(shape)} on {logits.device}")
    pos, more = _where(entry, st.rows, pos, step, row_step)
    d = _lib.SampleScoreDesc()
    d.logits, d.tokens, d.prompt_len, d.done = _p(logits), _p(st.tokens), _p(st.prompt_len), _p(st.done)
    d.live, d.token_logprob, d.sum_logprob, d.count = _p(sc.live), _p(sc.token_logprob), _p(sc.sum_logprob), _p(sc.count)
    d.ld = int(ld) if ld is not None else logits.stride(0)
    d.rows, d.vocab, d.row_len, d.pos = st.rows, int(vocab) if vocab is not None else logits.shape[-1], st.row_len, int(pos)
    check(getattr(_lib.lib(), "mpv_" + entry)(C.byref(d), *more, _stream()), "mpv_" + entry)
    return sc


def sample_score(logits, st, sc, *, pos, vocab=None, ld=None):
    """The model's log-probability of the token sample_advance has just written into st.tokens[:, pos], for st.rows sequences in one
    launch on the current stream (include/mpv.h: mpv_sample_score; st is the loop's generation.SampleState, sc a
    generation.SampleScores): log_softmax of logits bf16 [rows, ld] (the first `vocab` columns, what sample_advance read), into
    sc.token_logprob[:, pos], sc.sum_logprob and sc.count.  Rows with st.prompt_len > pos and rows whose sc.live is 0 are skipped;
    sc.live follows st.done.  -> sc"""
    return _sample_score("sample_score", **locals())


def sample_score_ragged(logits, st, sc, *, step, vocab=None, ld=None):
    """sample_score right after sample_advance_ragged (include/mpv.h: mpv_sample_score_ragged): generation step `step` >= 0; row r's
    token at its own column st.prompt_len[r] + step is scored into sc.token_logprob[r, that column].  Frozen rows (the column lies
    behind the table) and rows whose sc.live is 0 are skipped.  -> sc"""
    return _sample_score("sample_score_ragged", **locals())


def sample_score_steps(logits, st, sc, *, row_step, vocab=None, ld=None):
    """sample_score right after sample_advance_steps (include/mpv.h: mpv_sample_score_steps): row r's token at its own column
    st.prompt_len[r] + row_step[r] is scored.  Frozen rows and rows whose sc.live is 0 are skipped.  -> sc"""
    return _sample_score("sample_score_steps", **locals())


def _caption_sides(who, tok_a, start_a, begin_a, tok_b, start_b, begin_b, width_a, width_b):
    """what caption_overlap and caption_cider check and lay out on the host before any launch (`who` names the caller in the
    messages) -> (host: [start_a, begin_a, start_b, begin_b] as CPU int32 tensors, shape: (rows, width, row stride) per side, groups,
    pair_begin int64 [groups + 1]: the running sums of nA_g * nB_g)"""
    _need_cuda(tok_a, tok_b)
    host, shape = [], []
    for name, tok, start, begin, width in (("a", tok_a, start_a, begin_a, width_a), ("b", tok_b, start_b, begin_b, width_b)):
        if tok.dtype != torch.int64 or tok.ndim != 2 or (tok.shape[0] > 1 and tok.shape[1] > 1 and tok.stride(1) != 1):
            raise _lib.MpvError(f"{who}: tok_{name} must be int64 [rows, width] with unit column stride (got {tok.dtype} {tuple(tok.shape)})")
        width = tok.shape[1] if width is None else int(width)
        if width > tok.shape[1]:
            raise ValueError(f"{who}: width_{name} = {width} for a table of {tok.shape[1]} columns")
        start = torch.as_tensor(start, dtype=torch.int32, device="cpu").reshape(-1)
        begin = torch.as_tensor(begin, dtype=torch.int32, device="cpu").reshape(-1)
        if start.numel() != tok.shape[0]:
            raise ValueError(f"{who}: {start.numel()} start_{name} for {tok.shape[0]} rows")
        if start.numel() and width - int(start.min()) > _lib.CAPTION_OVERLAP_MAX_LEN:
            raise ValueError(f"{who}: a row of table {name} can hold a candidate of {width - int(start.min())} tokens "
                             f"(width {width}, start {int(start.min())}); at most {_lib.CAPTION_OVERLAP_MAX_LEN}")
        host += [start, begin]
        shape.append((tok.shape[0], width, tok.stride(0) if tok.shape[0] > 1 else max(width, 1)))
    groups = host[1].numel() - 1
    if groups != host[3].numel() - 1 or groups < 0:
        raise ValueError(f"{who}: begin_a / begin_b describe {groups} and {host[3].numel() - 1} groups")
    na, nb = host[1].to(torch.int64).diff(), host[3].to(torch.int64).diff()
    pair_begin = torch.cat([torch.zeros(1, dtype=torch.int64), (na * nb).cumsum(0)])
    return host, shape, groups, pair_begin


def _caption_upload(d, host, pair_begin, dev):
    """ONE upload of the pair offsets (int64) and the four int32 arrays; the descriptor's device and host pointers to them.  -> what
    must stay alive until the call has been made"""
    packed = torch.cat([pair_begin.view(torch.uint8)] + [h.contiguous().view(torch.uint8) for h in host])
    up = packed.to(dev)
    at, dptr, hptr = 0, [], []
    for h in [pair_begin] + host:
        dptr.append(up.data_ptr() + at)
        hptr.append(packed.data_ptr() + at)
        at += h.numel() * h.element_size()
    d.pair_begin, d.start_a, d.begin_a, d.start_b, d.begin_b = dptr
    d.host_pair_begin, d.host_start_a, d.host_begin_a, d.host_start_b, d.host_begin_b = hptr
    return packed, up


def caption_overlap(tok_a, start_a, begin_a, tok_b=None, start_b=None, begin_b=None, *, term, width_a=None, width_b=None):
    """Pairwise overlap counts between caption candidates on the current stream (include/mpv.h: mpv_caption_overlap).  tok_x: int64
    [rows_x, >= width_x] on the device with unit column stride (the row stride may exceed the width; width_x defaults to the column
    count); start_x: rows_x first generated columns and begin_x: the groups' CSR offsets [groups + 1], both HOST sequences or CPU
    tensors.  Side b defaults to side a (a clip's candidates against each other).  -> (len_a [rows_a], len_b [rows_b], counts
    [pairs, 5]) int32 on the device: the candidates' lengths and, group after group, its nA x nB pairs row-major with [LCS, m1, m2,
    m3, m4] each.  Raises ValueError before any launch when a row could hold a candidate of more than 255 tokens."""
    same = tok_b is None
    if same:
        if start_b is not None or begin_b is not None or width_b is not None:
            raise ValueError("caption_overlap: start_b / begin_b / width_b without tok_b")
        tok_b, start_b, begin_b, width_b = tok_a, start_a, begin_a, width_a
    host, shape, groups, pair_begin = _caption_sides("caption_overlap", tok_a, start_a, begin_a, tok_b, start_b, begin_b, width_a, width_b)
    dev = tok_a.device
    pairs = max(int(pair_begin[-1]), 0)
    len_a = torch.empty(shape[0][0], dtype=torch.int32, device=dev)
    len_b = len_a if same else torch.empty(shape[1][0], dtype=torch.int32, device=dev)
    counts = torch.empty((pairs, 5), dtype=torch.int32, device=dev)
    if groups == 0:
        return len_a, len_b, counts
    d = _lib.CaptionOverlapDesc()
    keep = _caption_upload(d, host, pair_begin, dev)
    some = torch.zeros(2, dtype=torch.int64, device=dev)               # what a side without rows, or a call without pairs, points at
    ptr = lambda t: t.data_ptr() if t.numel() else some.data_ptr()
    d.tok_a, d.tok_b, d.len_a, d.len_b, d.counts = ptr(tok_a), ptr(tok_b), ptr(len_a), ptr(len_b), ptr(counts)
    (d.rows_a, d.width_a, d.ld_a), (d.rows_b, d.width_b, d.ld_b) = shape
    d.term, d.groups = int(term), groups
    if same:                                                            # one table: the library computes its lengths once
        d.start_b, d.begin_b = d.start_a, d.begin_a
    check(_lib.lib().mpv_caption_overlap(C.byref(d), _stream()), "mpv_caption_overlap")
    return len_a, len_b, counts


def caption_cider(tok_a, start_a, begin_a, tok_b, start_b, begin_b, *, term, stats, sigma=6.0, width_a=None, width_b=None):
    """CIDEr of caption candidates (side a) against references (side b) on the current stream (include/mpv.h: mpv_caption_cider).  The
    tables, starts and CSR offsets are caption_overlap's; stats: the corpus statistics, a generation.CiderStats (or the tuple its
    arrays(device) returns: (keys uint64 [cap], idf fp64 [cap], log_ref_len)).  -> (pair [pairs, 4], score [rows_a]) fp64 on the
    device: per (candidate, reference) pair of a group, row-major, the similarity of the orders 1 .. 4 after the length penalty, and
    per candidate 10 * mean_n(sum_r pair / R) (0.0 in a group without references).  Raises ValueError before any launch when a row
    could hold a candidate of more than 255 tokens."""
    host, shape, groups, pair_begin = _caption_sides("caption_cider", tok_a, start_a, begin_a, tok_b, start_b, begin_b, width_a, width_b)
    dev = tok_a.device
    keys, idf, log_ref_len = stats.arrays(dev) if hasattr(stats, "arrays") else stats
    _need_cuda(keys, idf)
    if keys.dtype != torch.uint64 or idf.dtype != torch.float64 or keys.ndim != 1 or keys.shape != idf.shape or not keys.is_contiguous() \
            or not idf.is_contiguous() or keys.device != dev or idf.device != dev:
        raise _lib.MpvError(f"caption_cider: the corpus table must be contiguous uint64 / float64 [capacity] on {dev} "
                            f"(got {keys.dtype} {tuple(keys.shape)}, {idf.dtype} {tuple(idf.shape)})")
    pairs = max(int(pair_begin[-1]), 0)
    pair = torch.empty((pairs, _lib.CAPTION_CIDER_ORDERS), dtype=torch.float64, device=dev)
    score = torch.empty(shape[0][0], dtype=torch.float64, device=dev)
    if groups == 0:
        return pair, score
    d = _lib.CaptionCiderDesc()
    keep = _caption_upload(d, host, pair_begin, dev)
    some = torch.zeros(4, dtype=torch.float64, device=dev)             # what a side without rows, or a call without pairs, points at
    ptr = lambda t: t.data_ptr() if t.numel() else some.data_ptr()
    d.tok_a, d.tok_b, d.pair, d.score = ptr(tok_a), ptr(tok_b), ptr(pair), ptr(score)
    d.table_keys, d.table_idf, d.table_capacity = keys.data_ptr(), idf.data_ptr(), keys.numel()
    d.log_ref_len, d.sigma = float(log_ref_len), float(sigma)
    (d.rows_a, d.width_a, d.ld_a), (d.rows_b, d.width_b, d.ld_b) = shape
    d.term, d.groups = int(term), groups
    ws = workspace(_lib.lib().mpv_caption_cider_workspace_size(C.byref(d)), dev)
    check(_lib.lib().mpv_caption_cider(C.byref(d), ws.data_ptr(), ws.numel(), _stream()), "mpv_caption_cider")
    return pair, score


def sample_tokens(logits, *, temperature=1.0, top_k=0, top_p=0.0, seed=0, streams=None, vocab_size=None, vocab=None):
    """One-off draw: -> int64 [rows], the token sample_advance draws at pos 0 for every row of logits bf16 [rows, ld] (no prompt, no
    termination; vary `seed` or `streams` for another draw)."""
    from .generation import SampleState
    rows = logits.shape[0]
    st = SampleState(torch.zeros((rows, 1), dtype=torch.int64, device=logits.device), torch.zeros(rows, dtype=torch.int64, device=logits.device),
                     streams=streams)
    sample_advance(logits, st, pos=0, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, vocab_size=vocab_size, termination_id=-1,
                   vocab=vocab)
    return st.tokens.view(-1)


def soft_target_ce(sim, row_ids, col_ids, scale, rows, cols, want_grad=True):
    losses = torch.empty(rows, dtype=torch.float32, device=sim.device)
    dsim = torch.empty((rows, cols), dtype=torch.bfloat16, device=sim.device) if want_grad else None
    dts = torch.empty(rows, dtype=torch.float32, device=sim.device) if want_grad else None
    check(_lib.lib().mpv_soft_target_ce(sim.data_ptr(), row_ids.data_ptr(), col_ids.data_ptr(), scale, losses.data_ptr(), _p(dsim),
                                        _p(dts), rows, cols, _stream()), "mpv_soft_target_ce")
    return losses, dsim, dts


def maxsim_fwd(a, t, R, Q, C, E, *, alpha_dev=None, trans=False):
    """-> (sim fp32, arg int32): alpha * max_q <a[r,q], t[c]> and its argmax (ties to the lowest q), [R,C] or [C,R] with trans.
    a bf16 [R*Q, E], t bf16 [C, E]; alpha_dev fp32 device scalar (include/mpv.h: mpv_maxsim_fwd)."""
    _need_cuda(a, t)
    shape = (C, R) if trans else (R, C)
    sim = torch.empty(shape, dtype=torch.float32, device=a.device)
    arg = torch.empty(shape, dtype=torch.int32, device=a.device)
    check(_lib.lib().mpv_maxsim_fwd(a.data_ptr(), t.data_ptr(), _p(alpha_dev), sim.data_ptr(), arg.data_ptr(), R, Q, C, E,
                                    int(trans), _stream()), "mpv_maxsim_fwd")
    return sim, arg


def maxsim_route(dsim, arg, R, Q, C, *, trans=False):
    """-> G bf16 [R*Q, C] = dsim(r, c) where arg(r, c) == q, else 0 (include/mpv.h: mpv_maxsim_route)"""
    _need_cuda(dsim, arg)
    g = torch.empty((R * Q, C), dtype=torch.bfloat16, device=dsim.device)
    check(_lib.lib().mpv_maxsim_route(dsim.data_ptr(), arg.data_ptr(), g.data_ptr(), R, Q, C, int(trans), _stream()), "mpv_maxsim_route")
    return g


def smoothed_ce(sim, target, eps, scale, rows, cols, want_grad=True):
    """-> (losses fp32 [rows], dsim bf16 [rows, cols], dts fp32 [rows]): cross-entropy with label smoothing eps (include/mpv.h)"""
    _need_cuda(sim, target)
    losses = torch.empty(rows, dtype=torch.float32, device=sim.device)
    dsim = torch.empty((rows, cols), dtype=torch.bfloat16, device=sim.device) if want_grad else None
    dts = torch.empty(rows, dtype=torch.float32, device=sim.device) if want_grad else None
    check(_lib.lib().mpv_smoothed_ce(sim.data_ptr(), target.data_ptr(), eps, scale, losses.data_ptr(), _p(dsim), _p(dts), rows, cols,
                                     _stream()), "mpv_smoothed_ce")
    return losses, dsim, dts


def _sim_desc(q, g, k, scale, slices, g_dtype=torch.bfloat16):
    """mpv_sim_search_desc over bf16 feature rows q [Nq, D], g [Ng, D] (rows contiguous; a row stride is allowed); the *_q8 ops
    pass g_dtype=torch.uint8: the gallery is e4m3 codes and its row stride counts codes"""
    _need_cuda(q, g)
    for name, t, want in (("queries", q, torch.bfloat16), ("gallery", g, g_dtype)):
        if t.dtype != want:
            raise _lib.MpvError(f"sim search: {name} must be {want} (got {t.dtype})")
        if t.dim() != 2 or t.shape[0] == 0:
            raise _lib.MpvError(f"sim search: {name} must be a non-empty [rows, dim] matrix (got {tuple(t.shape)})")
        if t.stride(1) != 1:
            raise _lib.MpvError(f"sim search: {name} rows must be contiguous (strides {t.stride()})")
    if q.shape[1] != g.shape[1]:
        raise _lib.MpvError(f"sim search: feature widths differ ({q.shape[1]} vs {g.shape[1]})")
    d = _lib.SimSearchDesc()
    d.queries, d.gallery = q.data_ptr(), g.data_ptr()
    d.q_rs, d.g_rs = q.stride(0) if q.shape[0] > 1 else q.shape[1], g.stride(0) if g.shape[0] > 1 else g.shape[1]
    d.nq, d.ng, d.dim, d.k, d.slices = q.shape[0], g.shape[0], q.shape[1], k, slices
    d.scale = 1.0 if scale is None else float(scale)
    return d


def _row_pointers(g_scale):
    """the per-row arguments between the descriptor and the outputs: none, the row scales, or a tuple of tensors in order"""
    if g_scale is None:
        return ()
    return tuple(t.data_ptr() for t in (g_scale if isinstance(g_scale, tuple) else (g_scale,)))


def _search_topk(name, d, q, k, g_scale=None):
    """vals / idx [Nq, k] filled by mpv_<name> on descriptor d, with the workspace mpv_<name>_workspace_size asks for; g_scale: the
    row scales that the *_q8 entries take after the descriptor, or a tuple of per-row tensors in the entry's order (the *_prior entries)"""
    vals = torch.empty((q.shape[0], k), dtype=torch.float32, device=q.device)
    idx = torch.empty((q.shape[0], k), dtype=torch.int64, device=q.device)
    lib = _lib.lib()
    extra = _row_pointers(g_scale)
    ws = workspace(max(getattr(lib, f"mpv_{name}_workspace_size")(C.byref(d), *extra), 1), q.device)
    check(getattr(lib, f"mpv_{name}")(C.byref(d), *extra, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          f"mpv_{name}")
    return vals, idx


def _search_rank(name, d, q, target, queries="queries", g_scale=None):
    """rank [Nq] filled by mpv_<name> on descriptor d for target int64 [Nq] or [Nq, n_t]; g_scale as in _search_topk"""
    _need_cuda(target)
    if target.dtype != torch.int64:
        raise _lib.MpvError(f"{name}: target must be int64 (got {target.dtype})")
    target = target.reshape(target.shape[0], -1).contiguous()
    if target.shape[0] != q.shape[0]:
        raise _lib.MpvError(f"{name}: {target.shape[0]} target rows for {q.shape[0]} {queries}")
    n_t = target.shape[1]
    rank = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
    lib = _lib.lib()
    extra = _row_pointers(g_scale)
    ws = workspace(max(getattr(lib, f"mpv_{name}_workspace_size")(C.byref(d), *extra, n_t), 1), q.device)
    check(getattr(lib, f"mpv_{name}")(C.byref(d), *extra, target.data_ptr(), n_t, rank.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          f"mpv_{name}")
    return rank


def sim_topk(q, g, k, scale=None, slices=0):
    """-> (vals fp32 [Nq, k], idx int64 [Nq, k]): the k largest scale * <q_i, g_j> per query, descending, ties to the lower j,
    (-inf, -1) beyond Ng; `slices` gallery slices per query tile (0 = choose), the result does not depend on it
    (include/mpv.h: mpv_sim_topk)."""
    return _search_topk("sim_topk", _sim_desc(q, g, k, scale, slices), q, k)


def sim_rank(q, g, target, slices=0):
    """-> rank int32 [Nq]: the best rank among the query's target rows (target int64 [Nq] or [Nq, n_t], -1 = unused slot); the rank of
    row t is the number of rows j with <q, g_j> > <q, g_t>, or equal and j < t (include/mpv.h: mpv_sim_rank)."""
    return _search_rank("sim_rank", _sim_desc(q, g, 0, None, slices), q, target)


def _code_scales(what, codes, g_scale):
    """the row scales of a gallery of codes: fp32, contiguous, one per row (codes [.., dim] -> g_scale [..])"""
    _need_cuda(g_scale)
    if g_scale.dtype != torch.float32 or tuple(g_scale.shape) != tuple(codes.shape[:-1]) or not g_scale.is_contiguous():
        raise _lib.MpvError(f"{what}: g_scale must be a contiguous float32 tensor of shape {tuple(codes.shape[:-1])}, one scale per row of "
                            f"codes (got {g_scale.dtype} {tuple(g_scale.shape)})")
    return g_scale


def sim_topk_q8(q, codes, g_scale, k, scale=None, slices=0):
    """sim_topk over a gallery of e4m3 codes uint8 [Ng, D] (row pitch a multiple of 16) with g_scale fp32 [Ng], as
    quantize_rows_e4m3 returns them: the score of row j is g_scale[j] * <q_i, deq(codes_j)>.  For power-of-two scales the result is
    bit for bit sim_topk on the bf16 gallery deq(codes) * g_scale (include/mpv.h: mpv_sim_topk_q8)."""
    d = _sim_desc(q, codes, k, scale, slices, g_dtype=torch.uint8)
    return _search_topk("sim_topk_q8", d, q, k, g_scale=_code_scales("sim_topk_q8", codes, g_scale))


def sim_rank_q8(q, codes, g_scale, target, slices=0):
    """sim_rank over a gallery of e4m3 codes (sim_topk_q8; include/mpv.h: mpv_sim_rank_q8)"""
    d = _sim_desc(q, codes, 0, None, slices, g_dtype=torch.uint8)
    return _search_rank("sim_rank_q8", d, q, target, g_scale=_code_scales("sim_rank_q8", codes, g_scale))


def _row_terms(what, g, prior):
    """the per-row terms of a search with priors: fp32, contiguous, one per gallery row"""
    _need_cuda(prior)
    if prior.dtype != torch.float32 or tuple(prior.shape) != (g.shape[0],) or not prior.is_contiguous():
        raise _lib.MpvError(f"{what}: prior must be a contiguous float32 tensor of shape ({g.shape[0]},), one term per gallery row "
                            f"(got {prior.dtype} {tuple(prior.shape)})")
    return prior


def sim_topk_prior(q, g, prior, k, scale=None, slices=0):
    """sim_topk with one fp32 additive term per gallery row: the score of row j is fl(fl(scale * <q_i, g_j>) + prior[j]) (two
    roundings, no fused multiply-add).  A row whose score is -inf or NaN is left out altogether (prior[j] = -inf is a filter); a
    query with fewer than k eligible rows gets the (-inf, -1) tail (include/mpv.h: mpv_sim_topk_prior)."""
    d = _sim_desc(q, g, k, scale, slices)
    return _search_topk("sim_topk_prior", d, q, k, g_scale=(_row_terms("sim_topk_prior", g, prior),))


def sim_rank_prior(q, g, prior, target, scale=None, slices=0):
    """sim_rank under the scores of sim_topk_prior -- `scale` IS applied here, the order depends on it.  A target that is not
    eligible is no target; rows that are not eligible are never counted (include/mpv.h: mpv_sim_rank_prior)."""
    d = _sim_desc(q, g, 0, scale, slices)
    return _search_rank("sim_rank_prior", d, q, target, g_scale=(_row_terms("sim_rank_prior", g, prior),))


def sim_topk_prior_q8(q, codes, g_scale, prior, k, scale=None, slices=0):
    """sim_topk_prior over a gallery of e4m3 codes with row scales (sim_topk_q8; include/mpv.h: mpv_sim_topk_prior_q8)"""
    d = _sim_desc(q, codes, k, scale, slices, g_dtype=torch.uint8)
    extra = (_code_scales("sim_topk_prior_q8", codes, g_scale), _row_terms("sim_topk_prior_q8", codes, prior))
    return _search_topk("sim_topk_prior_q8", d, q, k, g_scale=extra)


def sim_rank_prior_q8(q, codes, g_scale, prior, target, scale=None, slices=0):
    """sim_rank_prior over a gallery of e4m3 codes with row scales (include/mpv.h: mpv_sim_rank_prior_q8)"""
    d = _sim_desc(q, codes, 0, scale, slices, g_dtype=torch.uint8)
    extra = (_code_scales("sim_rank_prior_q8", codes, g_scale), _row_terms("sim_rank_prior_q8", codes, prior))
    return _search_rank("sim_rank_prior_q8", d, q, target, g_scale=extra)


def _bank_lse(name, bank, g, beta, g_dtype, g_scale=None):
    _need_cuda(bank, g)
    for what, t, want in (("bank", bank, torch.bfloat16), ("gallery", g, g_dtype)):
        if t.dtype != want or t.dim() != 2 or t.shape[0] == 0 or t.stride(1) != 1:
            raise _lib.MpvError(f"{name}: {what} must be a non-empty {want} [rows, dim] matrix with contiguous rows "
                                f"(got {t.dtype} {tuple(t.shape)}, strides {t.stride()})")
    if bank.shape[1] != g.shape[1]:
        raise _lib.MpvError(f"{name}: feature widths differ ({bank.shape[1]} vs {g.shape[1]})")
    d = _lib.SimBankDesc()
    d.bank, d.gallery = bank.data_ptr(), g.data_ptr()
    d.b_rs, d.g_rs = bank.stride(0) if bank.shape[0] > 1 else bank.shape[1], g.stride(0) if g.shape[0] > 1 else g.shape[1]
    d.nb, d.ng, d.dim, d.beta = bank.shape[0], g.shape[0], g.shape[1], float(beta)
    lse = torch.empty(g.shape[0], dtype=torch.float32, device=g.device)
    extra = () if g_scale is None else (g_scale.data_ptr(),)
    check(getattr(_lib.lib(), f"mpv_{name}")(C.byref(d), *extra, lse.data_ptr(), None, 0, _stream()), f"mpv_{name}")
    return lse


def sim_bank_lse(bank, g, beta):
    """-> lse fp32 [Ng]: lse[j] = log sum_b exp(beta * <bank_b, g_j>) over the bank bf16 [Nb, D], kept against a running max (any
    finite beta).  lse[j] depends on (bank, beta, row j) alone, bit for bit.  sim_topk_prior(q, g, -lse, k, scale=beta) is the
    inverted-softmax (QB-Norm) search (include/mpv.h: mpv_sim_bank_lse)."""
    return _bank_lse("sim_bank_lse", bank, g, beta, torch.bfloat16)


def sim_bank_lse_q8(bank, codes, g_scale, beta):
    """sim_bank_lse over a gallery of e4m3 codes with row scales: bit for bit sim_bank_lse on bf16(deq(codes) * g_scale)
    (include/mpv.h: mpv_sim_bank_lse_q8)"""
    return _bank_lse("sim_bank_lse_q8", bank, codes, beta, torch.uint8, g_scale=_code_scales("sim_bank_lse_q8", codes, g_scale))


def _maxsim_side(name, t, dtype=torch.bfloat16):
    """-> (rows per item, row stride in elements) of bf16 features [n, dim] (one row per item) or [n, group, dim]; dtype uint8: e4m3
    codes, the stride counts codes"""
    if t.dtype != dtype:
        raise _lib.MpvError(f"maxsim search: {name} must be {dtype} (got {t.dtype})")
    if t.dim() not in (2, 3) or t.shape[0] == 0 or t.shape[-2] == 0:
        raise _lib.MpvError(f"maxsim search: {name} must be a non-empty [items, dim] or [items, group, dim] tensor (got {tuple(t.shape)})")
    if t.stride(-1) != 1:
        raise _lib.MpvError(f"maxsim search: {name} rows must be contiguous (strides {t.stride()})")
    if t.dim() == 2:
        return 1, (t.stride(0) if t.shape[0] > 1 else t.shape[1])
    rs = t.stride(1) if t.shape[1] > 1 else (t.stride(0) if t.shape[0] > 1 else t.shape[2])
    if t.shape[0] > 1 and t.stride(0) != t.shape[1] * rs:
        raise _lib.MpvError(f"maxsim search: the rows of {name} must be evenly spaced across items (strides {t.stride()})")
    return t.shape[1], rs


def _maxsim_desc(q, g, k, scale, slices, g_dtype=torch.bfloat16):
    """mpv_maxsim_search_desc over bf16 features; each side is [items, dim] or [items, group, dim], at most one side grouped > 1"""
    _need_cuda(q, g)
    (qg, q_rs), (gg, g_rs) = _maxsim_side("queries", q), _maxsim_side("gallery", g, g_dtype)
    if q.shape[-1] != g.shape[-1]:
        raise _lib.MpvError(f"maxsim search: feature widths differ ({q.shape[-1]} vs {g.shape[-1]})")
    d = _lib.MaxSimSearchDesc()
    d.queries, d.gallery, d.q_rs, d.g_rs = q.data_ptr(), g.data_ptr(), q_rs, g_rs
    d.nq, d.ng, d.q_group, d.g_group, d.dim, d.k, d.slices = q.shape[0], g.shape[0], qg, gg, q.shape[-1], k, slices
    d.scale = 1.0 if scale is None else float(scale)
    return d


def maxsim_topk(q, g, k, scale=None, slices=0):
    """-> (vals fp32 [Nq, k], idx int64 [Nq, k]): the k gallery items with the largest scale * max over the group's rows of <a, b>
    per query item, descending, ties to the lower item, (-inf, -1) beyond Ng.  q, g: bf16 [items, dim] or [items, group, dim], at
    most one of them with group > 1; the result does not depend on `slices` (include/mpv.h: mpv_maxsim_topk)."""
    return _search_topk("maxsim_topk", _maxsim_desc(q, g, k, scale, slices), q, k)


def maxsim_rank(q, g, target, slices=0):
    """-> rank int32 [Nq]: the best rank among the query item's target items (target int64 [Nq] or [Nq, n_t], -1 = unused slot) under
    the query-max score and the order rule of maxsim_topk; Ng for a query with no valid target (include/mpv.h: mpv_maxsim_rank)."""
    return _search_rank("maxsim_rank", _maxsim_desc(q, g, 0, None, slices), q, target, queries="query items")


def maxsim_topk_q8(q, codes, g_scale, k, scale=None, slices=0):
    """maxsim_topk over a gallery of e4m3 codes uint8 [Ng, group, D] or [Ng, D] with g_scale fp32 [Ng, group] or [Ng] (one per row,
    applied before the max over the group); queries bf16 with one row per item -- grouped queries are refused, that direction stays
    on bf16 indexes.  For power-of-two scales bit for bit maxsim_topk on deq(codes) * g_scale (include/mpv.h: mpv_maxsim_topk_q8)."""
    d = _maxsim_desc(q, codes, k, scale, slices, g_dtype=torch.uint8)
    return _search_topk("maxsim_topk_q8", d, q, k, g_scale=_code_scales("maxsim_topk_q8", codes, g_scale))


def maxsim_rank_q8(q, codes, g_scale, target, slices=0):
    """maxsim_rank over a gallery of e4m3 codes (maxsim_topk_q8; include/mpv.h: mpv_maxsim_rank_q8)"""
    d = _maxsim_desc(q, codes, 0, None, slices, g_dtype=torch.uint8)
    return _search_rank("maxsim_rank_q8", d, q, target, queries="query items", g_scale=_code_scales("maxsim_rank_q8", codes, g_scale))


# ---------------------------------------------------------------------------------------------- LoRA products (csrc/lora.hip)
LORA_RANKS = (8, 16, 32, 64)


def _ld(t, ld):
    return int(ld) if ld is not None else int(t.stride(0))


def lora_down(x, w, R, C, r, *, w_rank_major, scale=1.0, out=None, ldx=None, ldw=None, ldt=None):
    """t[R, r] = bf16(scale * x[R, C] w(C, r)); w(c, j) = w[j, c] if w_rank_major ([r, C]: lora_A) else w[c, j] ([C, r]: lora_B).
    Leading dimensions default to the tensors' row strides (include/mpv.h: mpv_lora_down)."""
    _need_cuda(x, w, out)
    if out is None:
        out = torch.empty((R, r), dtype=torch.bfloat16, device=x.device)
    check(_lib.lib().mpv_lora_down(x.data_ptr(), _ld(x, ldx), w.data_ptr(), _ld(w, ldw), int(w_rank_major), out.data_ptr(), _ld(out, ldt),
                                   R, C, r, float(scale), _stream()), "mpv_lora_down")
    return out


def lora_up_add(t, w, y, R, N, r, *, w_rank_major, scale=1.0, ldt=None, ldw=None, ldy=None):
    """y[R, N] = bf16(fp32(y) + scale * t[R, r] w(N, r)^T) in place; w(n, j) = w[j, n] if w_rank_major ([r, N]) else w[n, j] ([N, r])
    (include/mpv.h: mpv_lora_up_add)."""
    _need_cuda(t, w, y)
    check(_lib.lib().mpv_lora_up_add(t.data_ptr(), _ld(t, ldt), w.data_ptr(), _ld(w, ldw), int(w_rank_major), y.data_ptr(), _ld(y, ldy),
                                     R, N, r, float(scale), _stream()), "mpv_lora_up_add")
    return y


def lora_wgrad(t, x, R, C, r, *, g_rank_major, scale=1.0, out=None, ldt=None, ldx=None, ldg=None):
    """g(C, r) = bf16(scale * t[R, r]^T x[R, C]), written [r, C] (g_rank_major) or [C, r]; fixed-order reduction, no atomics
    (include/mpv.h: mpv_lora_wgrad)."""
    _need_cuda(t, x, out)
    if out is None:
        out = torch.empty((r, C) if g_rank_major else (C, r), dtype=torch.bfloat16, device=x.device)
    wsn = _lib.lib().mpv_lora_wgrad_workspace_size(R, C, r)
    ws = workspace(wsn, x.device)
    check(_lib.lib().mpv_lora_wgrad(t.data_ptr(), _ld(t, ldt), x.data_ptr(), _ld(x, ldx), out.data_ptr(), _ld(out, ldg), int(g_rank_major),
                                    R, C, r, float(scale), ws.data_ptr(), ws.numel(), _stream()), "mpv_lora_wgrad")
    return out
