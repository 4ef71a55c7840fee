/* mpv.h -- C ABI of libmpv_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * mPLUG-Video pre-train hot path.
 *
 * The reference (X-PLUG/Youku-mPLUG) has no FFI/plugin layer: its hot path reaches native code
 * only through PyTorch/cuBLAS/cuDNN, megatron_util's fused CUDA kernels and DeepSpeed's
 * FusedAdam.  Each entry point below names the reference call site(s) whose native work it
 * replaces (paths relative to the reference repo root).  The Python host side
 * (youku-mplug_amd/) binds these with ctypes; see INTEGRATION.md for the binding a reference
 * maintainer would add.
 *
 * Conventions
 *  - All tensor pointers are device pointers owned by the caller (PyTorch); bf16 unless noted.
 *    The library never allocates user-visible memory: scratch is passed in (workspace + size,
 *    with a *_workspace_size query).
 *  - Every call takes the hipStream_t to launch on and is asynchronous.
 *  - Return 0 on success, negative MPV_E_* otherwise; mpv_last_error() returns a thread-local
 *    message.  Nothing aborts.
 *  - Re-entrant; no global mutable state besides the thread-local error string.
 *  - Row maps: logical row r lives at physical row (r / group) * stride + (r % group) + offset;
 *    group == 0 means identity.  They address the token rows of the [B,T,1+N,D] ViT stream
 *    (one cls slot per frame) and the abstractor's K/V buffer with its extra bias-kv token.
 */
#ifndef MPV_H_
#define MPV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mpv_stream_t; /* == hipStream_t */

#define MPV_OK 0
#define MPV_E_SHAPE (-1)
#define MPV_E_ALIGN (-2)
#define MPV_E_ARCH (-3)
#define MPV_E_HIP (-4)
#define MPV_E_ARG (-5)

#define MPV_ACT_NONE 0
#define MPV_ACT_GELU_ERF 1  /* nn.GELU, models/vision_transformer.py:94,99 */
#define MPV_ACT_GELU_TANH 2 /* megatron bias_gelu_impl, models/modeling_distributed_gpt3.py:586-588 */
#define MPV_ACT_RELU 3      /* nn.ReLU of cls_head, models/distributed_gpt3.py:526-530, 1081-1085 */
#define MPV_ACT_DERIV 4     /* act_bwd only: act_bwd_z already HOLDS act'(z) (a forward launch with preact_deriv wrote it): the
                               backward epilogue is one multiply.  The GELU' polynomial then runs in the forward epilogue, which
                               is bound by its two stores and has the VALU slots free, instead of in the dgrad epilogue, which it
                               bound (fc2-dgrad x GELU' at K = 768: 33 vs 26 us per round of tiles, r04) */

/* Dropout seeds.  Every `seed` argument / field of this header is a 64-bit value.  A seed with bit 63 CLEAR is the seed itself.
 * A seed with bit 63 SET (MPV_SEED_FROM_DEVICE(ptr)) carries in its low 63 bits the device address of a uint64_t that holds the
 * seed; the kernel reads it when it RUNS.  Kernel arguments are frozen when a training step is captured into a HIP graph: the
 * indirect form is what lets each replay draw fresh masks (the host rewrites the 8 bytes before launching the graph).  Both forms
 * of the same value produce the same masks. */
#define MPV_SEED_FROM_DEVICE(ptr) ((uint64_t)(uintptr_t)(ptr) | (1ull << 63))

int mpv_version(void);
const char* mpv_last_error(void);
/* 0 if the current device is gfx950, MPV_E_ARCH otherwise */
int mpv_check_device(void);
/* the same test on a gcnArchName string (hipDeviceProp_t::gcnArchName, e.g. "gfx950:sramecc+:xnack-"): 0 / MPV_E_ARCH / MPV_E_ARG */
int mpv_check_arch_name(const char* gcn_arch_name);

/* ------------------------------------------------------------------------------------------
 * GEMM: C[M,N] = epilogue(sum_k A(m,k) B(n,k)), bf16 in, fp32 accumulate (v_mfma_f32_16x16x32_bf16 in the 256x256 kernel, 32x32x16 in the 128x128 fallback).
 * transA=0: A is [M][K] (lda); transA=1: A is [K][M].  transB=0: B is [N][K] (nn.Linear
 * weight); transB=1: B is [K][N].  (0,0)=forward, (0,1)=dgrad, (1,1)=wgrad (split-K inside).
 * N, the leading dimensions and the contiguous extent of A (K, or M when transA) are multiples of 8; a wgrad's K is ANY length >= 1, odd included.
 * Replaces: F.linear / nn.Linear (models/vision_transformer.py:104,108,175,205,250),
 * nn.MultiheadAttention projections (:353), visual_fc (models/distributed_gpt3.py:111,136),
 * mpu.Column/RowParallelLinear + LM head (models/modeling_distributed_gpt3.py:562,573,843,852,
 * 1348), bias_gelu (:586-588), bias_dropout_add (:953-979), and their autograd backward. */
typedef struct mpv_gemm_epilogue {
  int a_group, a_stride, a_offset; /* row map on A rows (transA=0 only)                     */
  int c_group, c_stride, c_offset; /* row map on C / residual / preact rows                  */
  int k_group, k_stride, k_offset; /* row map on the reduction rows (transposed operands)    */
  const void* bias;                /* bf16 [N] or NULL (16-byte aligned for the 256x256 kernel, which fetches a tile's slice by
                                      LDS-DMA; any other alignment is taken by the 128x128 kernel) */
  int act;                         /* MPV_ACT_*: y = act(bf16(acc + bias))                    */
  void* preact_out;                /* optional bf16 copy of (acc + bias) before act (ldc)     */
  const void* residual;            /* optional bf16 [.,N] added last (leading dim ldr): C = bf16(v + residual) with v the epilogue's value
                                      so far -- bf16(acc + bias) without an activation.  EXCEPT the small-M forward kernel (M <= 16, the
                                      decode steps): without an activation it adds the residual to the fp32 (acc + bias) and rounds once */
  int64_t ldr;
  const void* act_bwd_z; /* optional bf16 z [M][ldz]: multiply by act'(z) (GELU backward)    */
  int64_t ldz;
  int act_bwd;     /* MPV_ACT_* selecting act' for act_bwd_z                                  */
  float dropout_p; /* dropout on (acc + bias) before the residual add                         */
  uint64_t seed, offset;
  const float* alpha_dev; /* optional device scalar multiplier                                */
  float alpha;            /* host scalar multiplier (0 -> 1)                                  */
  int out_f32;            /* C is fp32 (no epilogue besides alpha / accumulate)               */
  int accumulate;         /* C += result: bf16(bf16(result) + C_old) for a bf16 C on every path, the split-K reduce included */
  void* colsum_out;       /* wgrad only: bf16 [M] = column sums of A over the (mapped) reduction rows,
                             i.e. the bias gradient that goes with dW = dY^T X, fused into the same pass */
  int tile_hint;          /* 0: the library picks the tile kernel per problem; 128 / 256 pin the 128x128 or the
                             256x256 eight-phase kernel where it applies, 192 / 160 its 192- and 160-row tile variants
                             (tests and measurements)                                                          */
  void* row_tap_out;      /* optional bf16 [ceil(M / row_tap_group)][N] (forward / dgrad on the tile kernels; with any epilogue, a
                             bias-only one included): rows m with m % row_tap_group == 0 ALSO store
                             bf16(acc * alpha + bias) -- before activation / dropout / residual -- at row m / group.
                             The ViT block uses it to take the per-frame cls rows of the spatial projection out of the
                             GEMM whose residual epilogue writes x + proj(.) for all rows (vision_transformer.py:263-270) */
  int row_tap_group;
  int split_hint;         /* measurements: > 0 pins the split-K count of a wgrad product (0: the library picks)              */
  int gm_hint;            /* measurements: > 0 pins the m-tiles per n-tile of an XCD's tile walk in the 256x256 kernel       */
  int preact_deriv;       /* with act (GELU kinds) and preact_out: preact_out receives bf16(act'(bf16(acc + bias))) instead of the
                             pre-activation itself -- what the matching dgrad multiplies by (act_bwd = MPV_ACT_DERIV)               */
  int keep_output;        /* cache hint.  0 (default): bf16 output tiles leave as NON-TEMPORAL stores -- a tile is written once, and as
                             plain stores it pushes the operand panels its neighbours share out of the XCD's L2 (round 5: -1.2 ms per
                             step).  1: plain stores -- for a SMALL output that a latency-bound kernel reads right behind this launch
                             (the decoder's qkv product in front of its attention: 26 vs 34 us per layer)                             */
  float colscale;         /* with colscale_cols > 0 (round 6): output columns n < colscale_cols leave as bf16(bf16(acc + bias) * colscale)  */
  int colscale_cols;      /* -- a second rounding, exactly `q = q * self.scale` on the q third of the packed qkv product
                             (models/vision_transformer.py:175-179): the attention kernels then take q as already scaled
                             (mpv_attn_desc.scale_q_bf16 = 2) and none of the three of them re-scales its q rows per work item.
                             Multiple of 8; bias-only epilogue (no activation / residual / dropout / accumulate / fp32 output)      */
} mpv_gemm_epilogue;

size_t mpv_gemm_workspace_size(int64_t M, int64_t N, int64_t K, int transA, int transB);
int mpv_gemm_bf16(const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                  int64_t ldc, int transA, int transB, const mpv_gemm_epilogue* ep, void* workspace,
                  size_t workspace_bytes, mpv_stream_t stream);

/* Test / measurement hook: the row-band plan mpv_gemm_bf16 uses for an M x N x K forward or dgrad product on a chip of
 * `ncu` compute units (csrc/gemm256.hip: rows are cut into up to three bands of 256-, 192- and 160-row tiles, one launch
 * each, so that no launch ends in a mostly empty round of workgroups).  preact / ext_rows: the epilogue also writes the
 * pre-activation / reads residual or GELU' rows.  out6[2i] = tile rows, out6[2i+1] = m-tiles of band i (row order);
 * returns the number of bands.  Host-only, launches nothing. */
int mpv_gemm_plan_bands(int64_t M, int64_t N, int64_t K, int ncu, int preact, int ext_rows, int* out6);

/* ------------------------------------------------------------------------------------------
 * LayerNorm, fp32 statistics, bf16 in/out.  Replaces LayerNormWithForceFP32
 * (models/vision_transformer.py:69-71) and megatron MixedFusedLayerNorm
 * (models/modeling_distributed_gpt3.py:1002,1016,1131).  x rows use xmap, y rows use ymap. */
int mpv_layernorm_fwd(const void* x, const void* gamma, const void* beta, void* y, float* mean, float* rstd,
                      int64_t rows, int64_t cols, int64_t ldx, int64_t ldy, float eps, int x_group, int x_stride,
                      int x_offset, int y_group, int y_stride, int y_offset, mpv_stream_t stream);
size_t mpv_layernorm_bwd_workspace_size(int64_t cols);
/* accumulate_dparams == MPV_LN_DPARAM_DEFER: the call leaves its per-workgroup dgamma/dbeta partials -- fp32
 * [mpv_layernorm_bwd_partial_rows(rows)][2][cols] at the start of `workspace`, which the caller then owns until the
 * finish -- and launches no reduction; mpv_layernorm_dparam_finish folds the partials of up to 8 such calls in two launches
 * (a ViT block has three LayerNorms: six reduce launches otherwise; it uses the 16 partial rows behind the call's own as
 * scratch, which the workspace size already covers).  dgamma / dbeta only select the mode in the deferred call (non-NULL). */
#define MPV_LN_DPARAM_DEFER 2
int mpv_layernorm_bwd_partial_rows(int64_t rows);
int mpv_layernorm_dparam_finish(const float* const* partials, const int* partial_rows, void* const* dgamma, void* const* dbeta,
                                const int* accumulate, int n, int64_t cols, mpv_stream_t stream);
/* dx[xmap(r)] = (dres ? dres[xmap(r)] : 0) + LNbwd(dy[ymap(r)]); dx may alias dres.
 * dx_drop (optional) = dx * keepmask/(1-p) with element index offset + r*cols + c.
 * dgamma/dbeta (bf16 [cols]) may be NULL (frozen GPT: dgrad only); workspace needed if not. */
int mpv_layernorm_bwd(const void* dy, const void* x, const void* gamma, const float* mean, const float* rstd,
                      const void* dres, void* dx, void* dx_drop, float drop_p, uint64_t seed, uint64_t offset,
                      void* dgamma, void* dbeta, int accumulate_dparams, int64_t rows, int64_t cols, int64_t ldx,
                      int64_t ldy, int x_group, int x_stride, int x_offset, int y_group, int y_stride, int y_offset,
                      void* workspace, size_t workspace_bytes, mpv_stream_t stream);

/* The decoder's residual stream in fp32 (models/modeling_distributed_gpt3.py:1038-1078: h + dropout(sublayer(LN(h)) + bias), twice
 * per layer).  The reference adds in bf16; 48 such roundings over 24 layers are what separates a bf16 run from the fp32 function
 * by 1.2e-2 in the logits (tools/parity_bisect.py), so here the sum lives in fp32:
 *   h_out[hmap(r)] = h_in[hmap(r)] + add[amap(r)]   (fp32; skipped when add == NULL),   y[ymap(r)] = LN(h_out row) in bf16.
 * h_in is fp32 [.,ldh], or bf16 when h_in_bf16 (the first LayerNorm behind the embedding); add is a sublayer output in bf16 with
 * bias and dropout already applied by its GEMM.  mpv_ln_stream_bwd is mpv_layernorm_bwd (no parameter gradients: frozen
 * decoder) with x read from the fp32 stream; dy / dres / dx / dx_drop stay bf16 and share x's row map. */
int mpv_ln_stream_fwd(const void* h_in, int h_in_bf16, const void* add, float* h_out, const void* gamma, const void* beta, void* y,
                      float* mean, float* rstd, int64_t rows, int64_t cols, int64_t ldh, int64_t lda, int64_t ldy, float eps,
                      int h_group, int h_stride, int h_offset, int a_group, int a_stride, int a_offset, int y_group, int y_stride,
                      int y_offset, mpv_stream_t stream);
/* The same with the dropout of `add` applied HERE (round 4): add_dropout_p > 0 drops the added tensor -- element index offset + (row of
 * `add`) * cols + column, the index, threshold and bf16 rounding of mpv_gemm_bf16's dropout epilogue, so that a sublayer's GEMM can store
 * bf16(acc + bias) with a plain epilogue and bias_dropout_add (models/modeling_distributed_gpt3.py:953-979, 1059-1078) completes in the
 * LayerNorm that adds it into the stream: an HBM-bound kernel with idle VALU slots instead of a store-bound epilogue.  Bit-identical to
 * dropping in the GEMM. */
int mpv_ln_stream_fwd_drop(const void* h_in, int h_in_bf16, const void* add, float* h_out, const void* gamma, const void* beta, void* y,
                           float* mean, float* rstd, int64_t rows, int64_t cols, int64_t ldh, int64_t lda, int64_t ldy, float eps,
                           int h_group, int h_stride, int h_offset, int a_group, int a_stride, int a_offset, int y_group, int y_stride,
                           int y_offset, float add_dropout_p, uint64_t seed, uint64_t offset, mpv_stream_t stream);
int mpv_ln_stream_bwd(const void* dy, const float* x, const void* gamma, const float* mean, const float* rstd, const void* dres,
                      void* dx, void* dx_drop, float drop_p, uint64_t seed, uint64_t offset, int64_t rows, int64_t cols, int64_t ldx,
                      int64_t ldy, int x_group, int x_stride, int x_offset, int y_group, int y_stride, int y_offset, mpv_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused attention (scores never materialised), exact two-pass softmax in fp32, MFMA QK^T / PV.
 * Replaces: ViT Attention core (models/vision_transformer.py:179-204: q*scale rounded to bf16,
 * fp32 scores+softmax, bf16 probs), GPT3CoreAttention (models/modeling_distributed_gpt3.py:
 * 757-804: baddbmm + scale/causal-mask(-10000)/softmax + dropout + bmm), nn.MultiheadAttention
 * core of AttentionPool (models/vision_transformer.py:353,371).
 * Element (b,h,row,d) of tensor X lives at X + b*x_bs + h*x_hs + row*x_rs + d. head_dim in
 * {64,80,96}.  lse is fp32 [batch][heads][sq]. */
typedef struct mpv_attn_desc {
  const void *q, *k, *v;
  void* o;
  float* lse;
  int64_t q_bs, q_hs, q_rs, k_bs, k_hs, k_rs, v_bs, v_hs, v_rs, o_bs, o_hs, o_rs;
  int batch, heads, sq, sk, head_dim;
  int causal;       /* key j visible to query i iff j <= i + (sk - sq) */
  float scale;      /* softmax(scale * q.k)                            */
  int scale_q_bf16; /* 1: q' = bf16(q*scale) first (ViT numerics); 2: q IS that q' already (written by the qkv product's
                       colscale epilogue): scores use it as it is, dQ is still the gradient of the UNSCALED q (x scale)  */
  float dropout_p;  /* on the probabilities.  The mask is attention's own convention: probability (b, h, row, key) has the element index
                       offset + ((b * heads + h) * sq + row) * sk + key; its pair's counter (mpv_common.h, mpv_rand_pair) is the ROW's base
                       index plus (key & ~1) -- pairs run along the key axis whatever the parity of the base --, key & 1 picks the low / high
                       16 bits of the pair's word, and the element is kept iff that field >= the 16-bit threshold of dropout_p there */
  uint64_t seed, offset;
} mpv_attn_desc;
int mpv_attn_fwd(const mpv_attn_desc* d, mpv_stream_t stream);
/* dO has o's strides; dq/dk/dv have q/k/v's strides; delta is fp32 scratch [batch][heads][sq]. */
int mpv_attn_bwd(const mpv_attn_desc* d, const void* dO, void* dq, void* dk, void* dv, float* delta,
                 mpv_stream_t stream);

/* Causal attention of continuations against a shared, already computed prefix (evaluation of the ITM / category scoring
 * heads: every candidate of one video shares the query features and the common token prefix, models/distributed_gpt3.py:
 * 1160-1218, 598-657).  n_cont continuations of cont_len rows; continuation c belongs to prefix group c / group_size
 * (n_groups = ceil(n_cont / group_size)).  Query row i of continuation c sits at absolute position prefix_len + i and attends
 * to the prefix_len keys of its group's prefix and to its own keys j <= i: softmax(scale * q.k) with fp32 scores and softmax,
 * no dropout.  Element (c,h,i,d) of q/k/v/o lives at X + c*x_cs + h*x_hs + i*x_rs + d; element (g,h,j,d) of pk/pv at
 * X + g*x_gs + h*x_hs + j*x_rs + d (the prefix pass's qkv rows at column offsets head_dim / 2*head_dim).  head_dim 64 or
 * 80 (anything else: MPV_E_SHAPE).  o is bf16. */
typedef struct mpv_attn_prefix_desc {
  const void *q, *k, *v;     /* continuations */
  const void *pk, *pv;       /* prefixes (may be NULL when prefix_len == 0) */
  void* o;
  int64_t q_cs, q_hs, q_rs, k_cs, k_hs, k_rs, v_cs, v_hs, v_rs;
  int64_t pk_gs, pk_hs, pk_rs, pv_gs, pv_hs, pv_rs;
  int64_t o_cs, o_hs, o_rs;
  int n_cont, group_size, n_groups, heads, cont_len, prefix_len, head_dim;
  float scale;
} mpv_attn_prefix_desc;
int mpv_attn_prefix_fwd(const mpv_attn_prefix_desc* d, mpv_stream_t stream);

/* The same attention for PACKED, ragged continuations (scoring given captions: reference captions have a few to 40 tokens each and
 * every clip its own number of them).  All continuation rows lie end to end in one [rows] array, the continuations of one group
 * next to each other, so a group is one contiguous row range: packed row r, head h, element d of q/k/v/o at X + r*x_rs + h*x_hs +
 * d; element (g,h,j,d) of pk/pv at X + g*x_gs + h*x_hs + j*x_rs + d as above (NULL allowed when prefix_len == 0).
 *   seg_start (device, int32 [rows])          packed index of the first row of the continuation row r belongs to, seg_start[r] <= r
 *   group_row (device, int32 [n_groups + 1])  group g owns rows group_row[g] .. group_row[g+1]-1; group_row[0] == 0,
 *                                             group_row[n_groups] == rows; a continuation never spans two groups
 *   max_group_rows (host)                     the largest group's row count: it sizes the grid, nothing is read back from the device
 * Query row r attends to the prefix_len prefix keys of its group and to its own keys kr with seg_start[r] <= kr <= r: ONE softmax
 * over both sets, fp32 scores and statistics, probabilities rounded to bf16 for the PV product, no dropout, o bf16.  Nothing but
 * o[0 .. rows) is written and nothing behind row `rows` is read.  A row's output is a function of its group's prefix and of its own
 * continuation only, bit for bit (masked keys have probability exactly 0 and stay out of the running max).
 * Refused with a negative code before any launch: NULL pointers; head_dim not 64 or 80; rows, n_groups or heads < 1; prefix_len <
 * 0; max_group_rows outside [1, rows]; rows >= 2^30, n_groups > 65535 or heads > 65535 (the grid's y / z limits: MPV_E_SHAPE, "problem
 * too large", as mpv_attn_prefix_fwd); q/k/v/pk/pv rows not 16-byte or o rows not 8-byte aligned; scale <= 0.  The contents of the
 * two index arrays are the caller's promise: build them with mpv_attn_prefix_packed_layout. */
typedef struct mpv_attn_prefix_packed_desc {
  const void *q, *k, *v;     /* packed continuation rows */
  const void *pk, *pv;       /* prefixes (may be NULL when prefix_len == 0) */
  void* o;
  const int32_t *seg_start, *group_row;
  int64_t q_rs, q_hs, k_rs, k_hs, v_rs, v_hs, o_rs, o_hs;
  int64_t pk_gs, pk_hs, pk_rs, pv_gs, pv_hs, pv_rs;
  int rows, n_groups, heads, prefix_len, head_dim, max_group_rows;
  float scale;
} mpv_attn_prefix_packed_desc;
int mpv_attn_prefix_packed_fwd(const mpv_attn_prefix_packed_desc* d, mpv_stream_t stream);
/* Host only (no device needed): the two index arrays of the packed layout from the continuation lengths cont_len[n_cont] and the
 * number of continuations of every group conts_per_group[n_groups], in packed order.  seg_start_out has room for sum(cont_len)
 * entries, group_row_out for n_groups + 1.  Refused (MPV_E_SHAPE): a length < 1, a group without a continuation, counts that do not
 * sum to n_cont, 2^30 rows or more. */
int mpv_attn_prefix_packed_layout(const int32_t* cont_len, int n_cont, const int32_t* conts_per_group, int n_groups,
                                  int32_t* seg_start_out, int32_t* group_row_out, int* rows_out, int* max_group_rows_out);

/* The packed attention for TRAINING (self-critical caption training: the N sampled captions of a clip are continuations of one
 * prefix, which is then computed once).
 * mpv_attn_prefix_packed_fwd_lse is mpv_attn_prefix_packed_fwd that also stores lse, fp32 [heads][rows]: lse[h][r] = m + log(l) of
 * row r's ONE softmax over [prefix | own visible keys], on the scaled scores.  o is mpv_attn_prefix_packed_fwd's bit for bit (the
 * same kernel body: the same tiles in the same order).  The same refusals with the same codes; lse NULL is a null pointer
 * (MPV_E_ARG), lse not 4-byte aligned MPV_E_ALIGN.  Nothing but o[0 .. rows) and lse[0 .. heads)[0 .. rows) is written. */
int mpv_attn_prefix_packed_fwd_lse(const mpv_attn_prefix_packed_desc* d, float* lse, mpv_stream_t stream);
/* The backward.  dO has o's strides, dq / dk / dv have q / k / v's, dpk / dpv have pk / pv's (group, head, row); all bf16.  lse is what
 * the forward above stored; delta is fp32 scratch [heads][rows] (written, then read).  Per continuation over the keys [its group's
 * prefix | its own rows], key kr visible to row r iff it is a prefix key or seg_start[r] <= kr <= r:
 *   P = exp(scale s - lse) in fp32 (a masked pair: exactly 0),   delta = sum_d dO o from the bf16 o given,   dS = P (dO V^T - delta),
 *   dS rounded to bf16 before the two products it enters, P rounded to bf16 before dV,
 *   dq = scale dS K,   dk = scale dS^T q,   dv = P^T dO   (fp32 accumulation, one rounding to bf16),
 * and a group's dpk / dpv are the sums of the prefix keys' dk / dv over ALL rows of the group.  accumulate_prefix == 0: dpk / dpv are
 * overwritten; 1: they are read and the sum is added in fp32 before the one rounding (the prefix rows' own causal gradient and the
 * continuations' contribution become one tensor).  No atomics: every output element is written by exactly one workgroup, and two
 * runs agree bit for bit.  Nothing behind row `rows` is read; nothing but dq / dk / dv[0 .. rows), rows [0, prefix_len) of every group
 * of dpk / dpv and delta is written; with prefix_len == 0, pk / pv / dpk / dpv may be NULL and are not touched.  group_row and
 * seg_start are clamped to [0, rows] where an address is formed from them.  A continuation's dq / dk / dv and a group's dpk / dpv
 * are functions of that group's prefix and rows only.
 * Refused with a negative code before any launch, in mpv_attn_prefix_packed_fwd's order and wording where they coincide: NULL
 * pointers; head_dim not 64 or 80; rows, n_groups or heads < 1; prefix_len < 0; max_group_rows outside [1, rows]; rows or prefix_len
 * >= 2^30, n_groups > 65535 or heads > 65535; rows of any bf16 tensor not 16-byte aligned (strides or pointers), the index arrays,
 * lse or delta not 4-byte (MPV_E_ALIGN); scale <= 0. */
typedef struct mpv_attn_prefix_packed_bwd_desc {
  const void *q, *k, *v, *o, *dO;    /* packed continuation rows */
  const void *pk, *pv;               /* prefixes */
  const float* lse;
  float* delta;
  void *dq, *dk, *dv;
  void *dpk, *dpv;
  const int32_t *seg_start, *group_row;
  int64_t q_rs, q_hs, k_rs, k_hs, v_rs, v_hs, o_rs, o_hs;
  int64_t pk_gs, pk_hs, pk_rs, pv_gs, pv_hs, pv_rs;
  int rows, n_groups, heads, prefix_len, head_dim, max_group_rows;
  int accumulate_prefix;
  float scale;
} mpv_attn_prefix_packed_bwd_desc;
int mpv_attn_prefix_packed_bwd(const mpv_attn_prefix_packed_bwd_desc* d, mpv_stream_t stream);

/* One decode step's attention for sequences that share a per-group prefix KV cache (lockstep beam search / sampling: the K
 * beams or samples of a clip share the visual prefix and the prompt).  n_seq sequences in groups of group_size consecutive
 * ones: sequence s belongs to group s / group_size (n_groups = ceil(n_seq / group_size); the last group may be short).  Every
 * sequence has ONE query row.  It attends, in this order, to the prefix_len keys of its group's prefix (pk / pv) and to its own
 * own_len keys (k / v; the last of them is the current position's; own_len is the same for every sequence): ONE softmax over
 * the concatenation, softmax(scale * q.k) with fp32 scores and statistics (scale multiplies the fp32 scores; q is not
 * pre-scaled), probabilities rounded to bf16 for the PV product.  Element (s,h,d) of q / o lives at X + s*x_ss + h*x_hs + d,
 * element (s,h,j,d) of k / v at X + s*x_ss + h*x_hs + j*x_rs + d, element (g,h,j,d) of pk / pv at X + g*x_gs + h*x_hs + j*x_rs
 * + d.  Rows of k / v at and beyond own_len are never read.  o is bf16; nothing else is written.  The output of a sequence is a
 * function of its group's prefix and its own rows only, bit for bit: not of n_groups, the group's place or the sequence's place
 * in its group.  head_dim 64 or 80, prefix_len >= 1, 1 <= own_len <= 2048, group_size >= 1 (rows go in tiles of 32); q / k / v /
 * pk / pv rows 16-byte aligned, o rows 8-byte aligned.  Anything else: a negative code before any launch. */
typedef struct mpv_attn_decode_shared_desc {
  const void *q, *k, *v;     /* per sequence */
  const void *pk, *pv;       /* per group */
  void* o;
  int64_t q_ss, q_hs, k_ss, k_hs, k_rs, v_ss, v_hs, v_rs;
  int64_t pk_gs, pk_hs, pk_rs, pv_gs, pv_hs, pv_rs;
  int64_t o_ss, o_hs;
  int n_seq, group_size, n_groups, heads, prefix_len, own_len, head_dim;
  float scale;
} mpv_attn_decode_shared_desc;
int mpv_attn_decode_shared_fwd(const mpv_attn_decode_shared_desc* d, mpv_stream_t stream);
/* The same step for groups whose prefixes differ in length (one lockstep search over prompts of different lengths): group g attends
 * to the first group_prefix_len[g] rows of its prefix (pk / pv + g*x_gs) and to its own_len own rows.  group_prefix_len is a DEVICE
 * array of int32 [n_groups]; d->prefix_len is the host-side upper bound (at most the rows between two groups' prefixes), and
 * 1 <= group_prefix_len[g] <= d->prefix_len is the caller's promise: the kernel clamps into that range, so a bad value cannot leave
 * the group's rows (as mpv_gpt_embed_rows_fwd keeps its positions inside wpe).  Prefix rows at and beyond a group's length are never
 * read.  One kernel body serves both entries (the uniform one passes no array), with the prefix length a per-workgroup value:
 *   with every length equal to d->prefix_len the output is mpv_attn_decode_shared_fwd's, bit for bit;
 *   a group's output is, bit for bit, that of mpv_attn_decode_shared_fwd run on that group alone with prefix_len = its length.
 * Refused: what mpv_attn_decode_shared_fwd refuses, and a NULL array.  Nothing is read back from the device. */
int mpv_attn_decode_shared_ragged_fwd(const mpv_attn_decode_shared_desc* d, const int32_t* group_prefix_len, mpv_stream_t stream);
/* The same step for groups that ALSO differ in how many own rows they hold (clips that entered a running loop at different times:
 * generation.sample_inflight_loop): group g attends to the first group_prefix_len[g] rows of its prefix and to the first
 * group_own_len[g] own rows of each of its sequences.  group_own_len is a DEVICE array of int32 [n_groups]; d->own_len (1 .. 2048) is
 * the host-side upper bound and the kernel clamps into [0, d->own_len].  A group of own length 0 is IDLE: its workgroups read no key,
 * no q and no length but their own, and write zeros to the group's o rows.  Own rows at and beyond a group's length are never read.
 * One kernel body serves all three entries, the own length a per-workgroup value next to the prefix length; the steps entry is its
 * own kernel around that body, so the code of the two entries above is what it was:
 *   with every own length equal to d->own_len the output is mpv_attn_decode_shared_ragged_fwd's, bit for bit;
 *   a live group's output is, bit for bit, that of mpv_attn_decode_shared_fwd run on that group alone with its two lengths;
 *   a bad length (negative: idle; beyond d->own_len: d->own_len) touches only its own group.
 * Refused: what mpv_attn_decode_shared_ragged_fwd refuses, and a NULL group_own_len.  Nothing is read back from the device. */
int mpv_attn_decode_shared_steps_fwd(const mpv_attn_decode_shared_desc* d, const int32_t* group_prefix_len, const int32_t* group_own_len,
                                     mpv_stream_t stream);

/* Divided space-time "temporal" attention: T<=16 tokens per (b,n) sequence, many tiny
 * problems (models/vision_transformer.py:247-248 with Attention :169-207).  qkv is the packed
 * [rows][3*D] projection in stream layout; sequence (o,i) (o<n_outer, i<n_inner) has its token
 * t at row o*outer_stride + inner_offset + i + t*t_stride.  out/dout are [rows][D].
 * Numerics: every instance (fp32 rows, bf16 rows, the matrix-core ones below) scores with q' = bf16(q * scale), as the model it
 * replaces does (:179); dq is the gradient of the unscaled q (x scale). */
int mpv_temporal_attn_fwd(const void* qkv, void* out, int n_outer, int64_t outer_stride, int n_inner,
                          int64_t inner_offset, int64_t t_stride, int T, int heads, int head_dim, float scale,
                          mpv_stream_t stream);
int mpv_temporal_attn_bwd(const void* qkv, const void* dout, void* dqkv, int n_outer, int64_t outer_stride,
                          int n_inner, int64_t inner_offset, int64_t t_stride, int T, int heads, int head_dim,
                          float scale, mpv_stream_t stream);

/* The same problem for clips of up to 64 frames, on the matrix cores: 1 <= T <= 64 (T <= 32 runs the 32-token instance, longer
 * clips the 64-token one), head_dim a multiple of 16 up to 96, every operand 16-byte aligned.  Arguments, addressing and numerics
 * as above; token rows t >= T are neither read nor written.  mpv_temporal_attn_fwd / _bwd keep their T <= 16. */
int mpv_temporal_attn_long_fwd(const void* qkv, void* out, int n_outer, int64_t outer_stride, int n_inner,
                               int64_t inner_offset, int64_t t_stride, int T, int heads, int head_dim, float scale,
                               mpv_stream_t stream);
int mpv_temporal_attn_long_bwd(const void* qkv, const void* dout, void* dqkv, int n_outer, int64_t outer_stride,
                               int n_inner, int64_t inner_offset, int64_t t_stride, int T, int heads, int head_dim,
                               float scale, mpv_stream_t stream);

/* What mpv_attn_fwd (role 0) / mpv_attn_bwd (role 1: its dQ launch, 2: its dK/dV launch) would launch for `d`, without
 * launching: the kernel instance as written in csrc/attention.hip, its grid, block and dynamic LDS bytes, and the most LDS
 * that instance is ever asked for (its opt-in limit).  Host only -- no device needed, nothing is dereferenced but `d` and
 * `out`; the refusals of mpv_attn_fwd apply.  For tests and tools: the launch paths do not go through it.
 * mpv_temporal_attn_plan_describe: the same for mpv_temporal_attn_fwd (bwd = 0) / _bwd (bwd = 1);
 * mpv_temporal_attn_long_plan_describe: for mpv_temporal_attn_long_fwd / _bwd. */
typedef struct mpv_attn_plan_info {
  const char* variant;   /* static storage */
  unsigned grid_x, grid_y;
  int block;
  int lds_bytes, lds_limit;
} mpv_attn_plan_info;
int mpv_attn_plan_describe(const mpv_attn_desc* d, int role, mpv_attn_plan_info* out);
int mpv_temporal_attn_plan_describe(int n_outer, int n_inner, int T, int heads, int head_dim, int bwd, mpv_attn_plan_info* out);
int mpv_temporal_attn_long_plan_describe(int n_outer, int n_inner, int T, int heads, int head_dim, int bwd, mpv_attn_plan_info* out);

/* ------------------------------------------------------------------------------------------
 * Patch-embed fold: video [B,3,T,H,W] bf16 -> im2col rows (b,t,ph,pw) x (c,i,j) padded to kpad
 * columns (models/vision_transformer.py:546-548,392-398; models/eva_vit.py:197-203 for P=14). */
int mpv_im2col_patches(const void* video, void* cols, int B, int C, int T, int H, int W, int P, int kpad,
                       mpv_stream_t stream);
/* Token assembly: X[b,t,0] = cls + pos[0]; X[b,t,1+n] = patch[(b,t,n)] + pos[1+n] + temporal[t]
 * (models/vision_transformer.py:555-565) into the [B,T,1+N,D] stream. */
int mpv_vit_embed_assemble_fwd(const void* patch, const void* cls_token, const void* pos_embed,
                               const void* temporal_embed, void* x, int B, int T, int N, int D, mpv_stream_t stream);
/* dpatch [B*T*N, D], dcls [D], dpos [1+N, D], dtemporal [T, D] from dx [B,T,1+N,D]. */
int mpv_vit_embed_assemble_bwd(const void* dx, void* dpatch, void* dcls, void* dpos, void* dtemporal, int B, int T,
                               int N, int D, mpv_stream_t stream);
/* cls merge after spatial attention (models/vision_transformer.py:263-270): for every b,
 * m = mean_t a[b,t,0,:];  y[b,t,0,:] = xt[b,t,0,:] + m.  Token rows: y = xt + a (all rows). */
int mpv_vit_cls_merge_fwd(const void* xt, const void* a, void* y, int B, int T, int N1, int D, mpv_stream_t stream);
/* backward: dxt = dy (all rows); da[token rows] = dy; da[b,t,0] = (sum_t' dy[b,t',0]) / T. */
/* The same merge without the full-tensor passes: after a GEMM with residual = xt and a row tap of group N1
 * (y = xt + a everywhere, tap = a on the cls rows), fix the cls slots in place: y[b,t,0] = xt[b,t,0] + bf16(mean_t' tap[b,t']). */
int mpv_vit_cls_fix_fwd(const void* xt, const void* tap, void* y, int B, int T, int N1, int D, mpv_stream_t stream);
/* Backward in place: saved[b,t] = dy[b,t,0] (bf16 [B*T][D], to be copied back with mpv_copy_rows once the projection's
 * gradients are done), then dy[b,t,0] = bf16(mean_t' dy[b,t',0]); token rows are untouched. */
int mpv_vit_cls_merge_bwd_inplace(void* dy, void* saved, int B, int T, int N1, int D, mpv_stream_t stream);
int mpv_vit_cls_merge_bwd(const void* dy, void* da, int B, int T, int N1, int D, mpv_stream_t stream);

/* copy `rows` rows of `cols` bf16 between row-mapped buffers */
int mpv_copy_rows(const void* src, void* dst, int64_t rows, int64_t cols, int64_t lds, int64_t ldd, int s_group,
                  int s_stride, int s_offset, int d_group, int d_stride, int d_offset, mpv_stream_t stream);
/* out[c] = sum_r in[map(r)][c] (bf16 in, fp32 accumulate, bf16 out, optional accumulate):
 * bias gradients and broadcast-parameter gradients. */
size_t mpv_colsum_workspace_size(int64_t cols);
int mpv_colsum(const void* in, void* out, int64_t rows, int64_t cols, int64_t ld, int group, int stride, int offset,
               int accumulate, void* workspace, size_t workspace_bytes, mpv_stream_t stream);
/* out = a + b (bf16, n elements); used for gradient joins */
int mpv_add(const void* a, const void* b, void* out, int64_t n, mpv_stream_t stream);
/* acc (fp32) += g (bf16), n elements: the gradient-accumulation window sum (DeepSpeed's bf16 optimizer keeps it in fp32,
 * run_pretrain_distributed_gpt3.py:46-53 with --update_freq); mpv_f32_to_bf16 rounds the window sum once at the boundary */
int mpv_accum_f32(float* acc, const void* g, int64_t n, int first, mpv_stream_t stream);
/* dst[0..n) <- words[0..n) (32-bit, n <= 32), the values travelling BY VALUE in the launch: the host's way to hand per-step
 * scalars (MPV_SEED_FROM_DEVICE seeds, mpv_adamw_step_grouped_dev's hyper_dev) to the device without a host buffer that must
 * outlive an asynchronous copy.  Stream-ordered like every other entry point. */
int mpv_store_words(void* dst, const uint32_t* words, int n, mpv_stream_t stream);
int mpv_f32_to_bf16(const float* src, void* dst, int64_t n, mpv_stream_t stream);
/* n independent bf16 copies dst[i][0:count[i]] = src[i][0:count[i]] in ONE launch (host arrays of device pointers): the
 * q / v halves of the packed qkv bias (models/vision_transformer.py:173) of every attention of the tower, and the
 * q_bias / v_bias gradients out of the packed bias-gradient of the qkv weight-gradient products */
int mpv_copy_segments(const void* const* src, void* const* dst, const int64_t* count, int n, mpv_stream_t stream);
/* Finishing step of the composed temporal_attn.proj + temporal_fc backward (models/vision_transformer.py:199-200, 250;
 * Wc = Wf Wp): dWf = bf16(float(dWc Wp^T) + d(bc) bp^T) and d(bp) = Wf^T d(bc), all operands bf16 [D,D] / [D]. */
int mpv_vit_compose_bwd_finish(const void* dwc_wpT, const void* dbc, const void* bp, const void* wf, void* dwf, void* dbp, int D,
                               mpv_stream_t stream);
/* The composed temporal projection of EVERY block of the tower in one launch each (round 6; the [D, D] products of a block depend on
 * parameters and on per-block reduced gradients only, so the 12 blocks' worth goes out together: Wc and bc at the head of the step,
 * dWf / dWp / d(bp) at the end of the tower's backward -- 5 launches per step instead of 60).  Pointer tables are HOST arrays of
 * `batch` device pointers (copied by value into the launches; any batch, 16 problems per launch).
 *   mpv_vit_compose_bias_batched:       bc[b] = bf16(Wf[b] bp[b] + bf[b])             (models/vision_transformer.py:199-200, 250)
 *   mpv_vit_compose_bwd_finish_batched: mpv_vit_compose_bwd_finish for every b
 *   mpv_gemm_bf16_batched:              C[b] = A[b] op B[b], mpv_gemm_bf16's operand forms (transA / transB), ONE shape, plain epilogue
 *                                       (bf16 out, no bias); replaces torch.bmm-shaped loops over blocks, which the reference does not
 *                                       have (it runs proj and temporal_fc as two token-row products, :199-200, 250). */
int mpv_vit_compose_bias_batched(const void* const* wf, const void* const* bp, const void* const* bf, void* const* bc, int batch, int D,
                                 mpv_stream_t stream);
int mpv_vit_compose_bwd_finish_batched(const void* const* dwc_wpT, const void* const* dbc, const void* const* bp, const void* const* wf,
                                       void* const* dwf, void* const* dbp, int batch, int D, mpv_stream_t stream);
int mpv_gemm_bf16_batched(const void* const* A, const void* const* B, void* const* C, int batch, int64_t M, int64_t N, int64_t K,
                          int64_t lda, int64_t ldb, int64_t ldc, int transA, int transB, mpv_stream_t stream);
/* Labels and loss weights of the L text positions behind the Q query slots (models/distributed_gpt3.py:142-159,
 * 348-351; the masked mean of models/modeling_distributed_gpt3.py:1615-1617 as per-position weights):
 * labels[b][l] = ids[b][l+1] (ids[b][1] at l = L-1), weights[b][l] = attention_mask[b][l+1] / sum(attention_mask[:,1:])
 * with positions l < prompt_len[b] (optional) zeroed, weights[b][L-1] = 0. */
int mpv_caption_targets(const int64_t* ids, const int64_t* attention_mask, const int64_t* prompt_len, int B, int L,
                        int64_t* labels, float* weights, mpv_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GPT-3 embedding front: h[b,s,:] = (s < Q ? query[b,s,:] : wte[ids[b,s-Q],:]) + wpe[s,:], then
 * dropout (models/distributed_gpt3.py:155-156; models/modeling_distributed_gpt3.py:640-666). */
int mpv_gpt_embed_fwd(const void* query, const int64_t* ids, const void* wte, const void* wpe, void* h, int B,
                      int Q, int L, int H, float dropout_p, uint64_t seed, uint64_t offset, mpv_stream_t stream);
/* Packed rows of the same front in evaluation (no dropout, no query rows): out[r,:] = wte[ids[r],:] + wpe[pos[r],:], one bf16
 * rounding as above.  ids int64 [rows], pos int32 [rows] (device); wpe has max_positions rows and 0 <= pos[r] < max_positions is the
 * caller's promise (the host knows the positions and checks them: ops.gpt_embed_rows_fwd).  The kernel keeps that promise from
 * becoming a read outside wpe: a position outside the table reads its nearest row instead.  Refused: rows < 1, H not a multiple of
 * 8, max_positions < 1, NULL pointers. */
int mpv_gpt_embed_rows_fwd(const int64_t* ids, const int32_t* pos, const void* wte, const void* wpe, void* out, int rows, int H,
                           int max_positions, mpv_stream_t stream);
/* dquery[b,q,:] = dh[b,q,:] * keepmask/(1-p) */
int mpv_gpt_embed_bwd(const void* dh, void* dquery, int B, int Q, int L, int H, float dropout_p, uint64_t seed,
                      uint64_t offset, mpv_stream_t stream);
/* The same dropout mask applied to the gradient of EVERY row of the embedding output: dfull[rows, H] = dropout_mask * dh (rows = B * S).
 * A trainable decoder (freeze_text_decoder: false, models/distributed_gpt3.py:91-93) needs it for the word- and position-embedding
 * gradients (GPT3Embedding, models/modeling_distributed_gpt3.py:640-666). */
int mpv_gpt_embed_bwd_full(const void* dh, void* dfull, int64_t rows, int H, float dropout_p, uint64_t seed, uint64_t offset,
                           mpv_stream_t stream);

/* Masked cross-entropy over bf16 logits in fp32 (models/modeling_distributed_gpt3.py:1352-1359,
 * 1615-1617): losses[r] = lse(logits[r]) - logits[r][labels[r]];  if dlogits != NULL it is
 * filled with (softmax - onehot) * weight[r] (weight = loss_mask / sum(loss_mask)), may alias
 * logits.  loss_sum (fp32 scalar) receives sum_r losses[r]*weight[r], reduced in a fixed order
 * (deterministic; needs `losses`). */
int mpv_cross_entropy(const void* logits, const int64_t* labels, const float* weight, float* losses, float* loss_sum,
                      void* dlogits, int64_t rows, int64_t vocab, int64_t ld, mpv_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ITC retrieval head (models/distributed_gpt3.py:938-980).
 * F.normalize(dim=-1) forward/backward (:947,960); norm is fp32 [rows] (saved for backward). */
int mpv_l2norm_fwd(const void* x, void* y, float* norm, int64_t rows, int64_t cols, float eps, mpv_stream_t stream);
int mpv_l2norm_bwd(const void* dy, const void* x, const float* norm, void* dx, int64_t rows, int64_t cols,
                   mpv_stream_t stream);
/* dst[r] = src[idx[r]] (last-valid-token pooling of the text hidden state, :958-959) */
int mpv_gather_rows(const void* src, const int64_t* idx, void* dst, int64_t rows, int64_t cols, int64_t ld,
                    mpv_stream_t stream);
/* dst[idx[r]] = src[r], idx distinct, dst rows of stride ld (backward of that pooling where the decoder input
 * carries gradient: the prompt pass of cls_head, models/distributed_gpt3.py:583-585, 1149-1151) */
int mpv_scatter_rows(const void* src, const int64_t* idx, void* dst, int64_t rows, int64_t cols, int64_t ld,
                     mpv_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Generation (KV-cache decode, models/modeling_distributed_gpt3.py:1620-1886).  The forward kernels above serve
 * prefill and the single-row decode steps (mpv_attn_fwd with sq = 1 over the cached keys); two helpers:
 * dst[r][0:cols] = src[idx[r]][0:cols] with row pitches lds / ldd: the beam re-order of a layer's KV cache
 * (InferenceParams.swap_key_value_dict :1459-1473). */
int mpv_gather_rows_ld(const void* src, const int64_t* idx, void* dst, int64_t rows, int64_t cols, int64_t lds, int64_t ldd,
                       mpv_stream_t stream);
/* out_val[r][j], out_idx[r][j] = the j-th largest of log_softmax(logits[r]) + add[r] (add optional), fp32 statistics over
 * bf16 logits, ties broken towards the lower index; k <= 64.  Serves beam_search (:1790-1805: log_softmax, + scores,
 * sort, top 2*beam) and greedy sample (:1411-1413, k = 1). */
size_t mpv_logprob_topk_workspace_size(int64_t rows, int k);
int mpv_logprob_topk(const void* logits, const float* add, int64_t rows, int64_t vocab, int64_t ld, int k, float* out_val,
                     int64_t* out_idx, void* workspace, size_t workspace_bytes, mpv_stream_t stream);
/* One incremental decoder forward over per-layer KV caches, all launches issued from C (one FFI call per step):
 * appends the n = Q + L new positions of every sequence (query [batch*Q][hidden] rows first, then wte[tokens]) at
 * cache rows [pos0, pos0 + n), attends causally over rows [0, pos0 + n) and writes the logits of the LAST new position
 * of every sequence to logits [batch][vocab] (bf16).  kv_cache[l] = [batch][max_len][3*hidden] bf16 in the decoder's
 * head-interleaved q|k|v row format (models/modeling_distributed_gpt3.py:895-902).  Weight tables are host arrays of
 * device pointers.  Covers :640-666, :868-938 (KV memory), :1034-1078, :1184, :1348-1350. */
typedef struct mpv_gpt_layer_weights {
  const void *ln1_w, *ln1_b, *qkv_w, *qkv_b, *dense_w, *dense_b, *ln2_w, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} mpv_gpt_layer_weights;
typedef struct mpv_gpt_weights {
  int layers, hidden, heads, ffn, vocab;
  float ln_eps;
  const mpv_gpt_layer_weights* layer;
  const void *wte, *wpe, *lnf_w, *lnf_b;
  int max_positions; /* rows of wpe (max_position_embeddings); 0 = unchecked */
} mpv_gpt_weights;
size_t mpv_gpt_decode_workspace_size(const mpv_gpt_weights* w, int batch, int n_new);
int mpv_gpt_decode_step(const mpv_gpt_weights* w, void* const* kv_cache, int batch, int max_len, int pos0, const void* query,
                        int Q, const int64_t* tokens, int L, void* workspace, size_t workspace_bytes, void* logits,
                        mpv_stream_t stream);
/* mpv_gpt_decode_step for ONE new token per sequence against a per-group shared prefix: n_seq = n_groups * fan sequences,
 * sequence s continues the prefix of group s / fan.  prefix_cache[l] = [n_groups][prefix_len][3*hidden] (what a prefill through
 * mpv_gpt_decode_step at batch n_groups, max_len = prefix_len, pos0 = 0 leaves), suffix_cache[l] = [n_seq][suffix_max][3*hidden],
 * both in the decoder's q|k|v row format.  The token sits at suffix position t (absolute position prefix_len + t, which must
 * lie inside the position embedding): its qkv row is written to suffix row s*suffix_max + t, the attention is
 * mpv_attn_decode_shared_fwd with own_len = t + 1, the rest of the layer and the LM head are those of mpv_gpt_decode_step.
 * logits [n_seq][vocab] bf16.  The workspace is that of a batch n_seq, one-position step. */
size_t mpv_gpt_decode_shared_workspace_size(const mpv_gpt_weights* w, int n_seq);
int mpv_gpt_decode_step_shared(const mpv_gpt_weights* w, void* const* prefix_cache, void* const* suffix_cache, int n_groups, int fan,
                               int prefix_len, int suffix_max, int t, const int64_t* tokens, void* workspace,
                               size_t workspace_bytes, void* logits, mpv_stream_t stream);
/* mpv_gpt_decode_step_shared over groups whose prefixes differ in length: prefix_cache[l] = [n_groups][prefix_stride][3*hidden],
 * group g's prefix being its first group_prefix_len[g] rows (DEVICE int32 [n_groups], 1 <= length <= max_prefix_len <= prefix_stride:
 * the caller's promise, clamped on the device); max_prefix_len (host) serves the position-table check max_prefix_len + t <
 * max_positions.  Sequence s sits at absolute position group_prefix_len[s / fan] + t: the driver forms these positions on the
 * device inside its workspace, embeds through mpv_gpt_embed_rows_fwd and attends through mpv_attn_decode_shared_ragged_fwd;
 * everything else -- suffix cache, workspace, the rest of the layer, the LM head, logits -- is mpv_gpt_decode_step_shared's. */
int mpv_gpt_decode_step_shared_ragged(const mpv_gpt_weights* w, void* const* prefix_cache, void* const* suffix_cache, int n_groups, int fan,
                                      int prefix_stride, const int32_t* group_prefix_len, int max_prefix_len, int suffix_max, int t,
                                      const int64_t* tokens, void* workspace, size_t workspace_bytes, void* logits, mpv_stream_t stream);
/* mpv_gpt_decode_step_shared_ragged over groups that sit at different suffix positions (a finished clip's slot was given to the next
 * clip while the others went on): group_t is a DEVICE int32 [n_groups] in place of the host t, max_t (host) the largest position any
 * group may hold -- it serves the checks max_t < suffix_max, max_t < 2048 and max_prefix_len + max_t < max_positions.  Group g's
 * sequences sit at suffix position group_t[g], absolute position group_prefix_len[g] + group_t[g] (formed on the device).  A group
 * with group_t[g] < 0 (or beyond max_t: the caller's broken promise stays inside the group) is IDLE: its rows flow through the
 * products as padding, embedded at position group_prefix_len[g]; its attention is the idle case of mpv_attn_decode_shared_steps_fwd;
 * its logits are unspecified but finite for finite weights; NOTHING of it is written into the suffix cache.
 * The qkv product writes dense rows into the workspace (through the identity row map: the product is the ragged step's in
 * everything but its addresses, so the same kernel serves it), one launch per layer places row s at suffix row s*suffix_max +
 * group_t[g], and q is read from the dense rows.  With every group_t[g] equal to t the logits and the suffix cache are
 * mpv_gpt_decode_step_shared_ragged's at t, bit for bit; a live group's logits are those of the same group stepped where all groups
 * sit at its position.  Workspace: mpv_gpt_decode_shared_steps_workspace_size (the shared step's plus the dense qkv rows).
 * Refused: what mpv_gpt_decode_step_shared_ragged refuses (with max_t for t), a NULL group_t, hidden % 8 != 0. */
size_t mpv_gpt_decode_shared_steps_workspace_size(const mpv_gpt_weights* w, int n_seq);
int mpv_gpt_decode_step_shared_steps(const mpv_gpt_weights* w, void* const* prefix_cache, void* const* suffix_cache, int n_groups, int fan,
                                     int prefix_stride, const int32_t* group_prefix_len, int max_prefix_len, int suffix_max,
                                     const int32_t* group_t, int max_t, const int64_t* tokens, void* workspace, size_t workspace_bytes,
                                     void* logits, mpv_stream_t stream);
/* mpv_gpt_decode_step at pos0 = 0 (a prefill) for prompts of different lengths, right-padded to L tokens behind their real ones:
 * the LM head runs on row last_row[b] (DEVICE int64 [batch], an index inside sequence b's n = Q + L new rows, clamped into them) of
 * every sequence, fetched through mpv_gather_rows, instead of on row n - 1.  Causal attention leaves the rows up to last_row[b]
 * exactly those of a prefill of the unpadded prompt; the pad rows' KV is written to the cache and is for the caller never to read
 * (mpv_gpt_decode_step_shared_ragged does not).  Refused: what mpv_gpt_decode_step refuses, and a NULL last_row. */
int mpv_gpt_prefill_ragged(const mpv_gpt_weights* w, void* const* kv_cache, int batch, int max_len, const void* query, int Q,
                           const int64_t* tokens, int L, const int64_t* last_row, void* workspace, size_t workspace_bytes, void* logits,
                           mpv_stream_t stream);
/* beam re-order of all layers: dst[l][j] = src[l][idx[j]] for the first `rows` cached positions */
int mpv_kv_reorder(void* const* src, void* const* dst, int layers, const int64_t* idx, int batch, int max_len, int rows,
                   int hidden, mpv_stream_t stream);
/* beam re-order of the suffix cache of the steps entries, where every clip has written its own number of suffix rows: src and dst
 * are two caches [layers][n_groups * fan * suffix_max][3 * hidden] bf16 (contiguous, 16-byte aligned, different), and ONE launch
 * over all layers does, for sequence j of clip g = j / fan,  dst[l][j][0:r) = src[l][idx[j]][0:r)  with r = clamp(group_rows[g], 0,
 * max_rows).  idx is DEVICE int64 [n_groups * fan] (mpv_beam_advance_steps' src_row: it never leaves the clip; an entry outside
 * [0, n_groups * fan) moves nothing), group_rows DEVICE int32 [n_groups], max_rows (host) the largest count any clip may hold.
 * Copies are 16 bytes wide.  A clip with r = 0 (a free slot, or one installed in this iteration) moves nothing; rows at or behind r
 * are not written.  With every count equal to t the written region is mpv_gather_rows_ld's over (layer, sequence) with t rows.
 * Refused: a NULL pointer, src == dst, hidden % 8 != 0, max_rows outside [0, suffix_max], a misaligned cache, layers > 65535. */
int mpv_kv_suffix_reorder_steps(const void* src, void* dst, int layers, int n_groups, int fan, int suffix_max, const int64_t* idx,
                                const int32_t* group_rows, int max_rows, int hidden, mpv_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * FP8 decoder weights (weight-only, opt-in, the decode steps of the frozen decoder; csrc/gemm_w8.hip).  Numeric contract:
 *   format   OCP e4m3fn (gfx950's native FP8, not fnuz), one fp32 scale per output row of a [N, K] nn.Linear weight (bf16 in).
 *   scale    row n: amax = max_k |w[n,k]|; e = the smallest integer with amax <= 448 * 2^e -- from frexp(amax) = (f, x):
 *            e = x - 9 if f <= 0.875, else x - 8; a zero row has e = 0 (e is never below -126); scale[n] = 2^e.
 *   codes    code[n,k] = RNE_e4m3(w[n,k] * 2^-e).  Nothing saturates and no NaN code is produced (finite weights).
 *   product  C[m,n] = bf16(epi(scale[n] * sum_k A[m,k] * deq(code[n,k]))), A bf16, fp32 accumulation; deq is exact for all 254
 *            finite codes, subnormals included.  epi: bias, GELU-tanh on the bf16-rounded pre-activation, residual with ldr, the
 *            output row map c_group / c_stride / c_offset; any other epilogue field set: MPV_E_ARG.
 * The scales are powers of two, so deq(code) * scale is a bf16 number: the quantised decoder IS a bf16 model, the one with those
 * weights loaded, and the FP8 entries compute its function -- kernel error and quantisation error are separate questions.  (The
 * rounding of a weight to e4m3 is about 2.7 % relative L2 noise per product, computed on the CPU for Gaussian rows; the bf16
 * gates of this project are 1e-2.  What that costs in caption quality has NOT been measured -- no trained checkpoint exists
 * here; running the unchanged bf16 stack on DistributedGPT3.dequantized_state_dict() measures exactly that.)
 *
 * mpv_quantize_rows_e4m3: codes [N][K] uint8 (dense), scale [N] fp32 from w [N][ldw] bf16.  K % 16 == 0, ldw % 8 == 0.
 * mpv_gemm_w8: 1 <= M <= 512, N % 8 == 0, K % 16 == 0 (a 16-byte chunk is 16 codes), anything else MPV_E_SHAPE with C untouched.
 *   The codes are streamed once per product straight into registers, turned into bf16 MFMA operands there, and multiplied into
 *   16-row blocks of A held by the same workgroup (A is re-read from L2: from a few dozen rows on that traffic, not the weight, is
 *   what the product costs).  Shapes with K >= 4096 and N <= 4096 split K over 16 waves whose registers hold 8 row blocks: such a
 *   product goes out in launches of 128 rows.  The K-summation order of an
 *   output element depends on (N, K) only: row m of a 160-row call is bit-identical to the same row computed alone.  No atomics.
 * mpv_gemm_w8_tiled: the same contract, shapes, epilogues and refusals, built for 97-512 rows (any M in [1, 512] is computed).  A
 *   workgroup owns up to 128 rows x 64 columns over all of K: it stages its A tile through LDS in K-steps of 128 (coalesced
 *   16-byte loads, shared by its four waves), each wave keeps the codes of its own 16 columns in registers, four K-steps of
 *   loads are in flight.  An output element is one accumulator chain over ascending k: row m of a 512-row call is bit-identical to that row in
 *   a 97-row or a 1-row call of this entry (NOT to mpv_gemm_w8, whose order differs; both are within the 1e-2 gate of the fp32
 *   product).  K is not split over workgroups, so the workspace (which may be null) is not used and cannot change a result.
 * mpv_gpt_embed_w8_fwd: mpv_gpt_embed_fwd (no dropout) of the bf16 model above -- token rows are deq(code) * scale of the tied
 *   embedding's codes, query rows are copied, the position rows are added in fp32. */
int mpv_quantize_rows_e4m3(const void* w, int64_t N, int64_t K, int64_t ldw, void* codes, float* scale, mpv_stream_t stream);
int mpv_gemm_w8(const void* A, const void* codes, const float* scale, void* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                int64_t ldw, int64_t ldc, const mpv_gemm_epilogue* ep, mpv_stream_t stream);
int mpv_gemm_w8_tiled(const void* A, const void* codes, const float* scale, void* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                      int64_t ldw, int64_t ldc, const mpv_gemm_epilogue* ep, void* workspace, size_t workspace_bytes, mpv_stream_t stream);
int mpv_gpt_embed_w8_fwd(const void* query, const int64_t* ids, const void* wte_codes, const float* wte_scale, const void* wpe, void* h,
                         int B, int Q, int L, int H, mpv_stream_t stream);
/* mpv_gpt_embed_rows_fwd (per-row positions, clamped into wpe's max_positions rows; same refusals) with the token rows read as
 * deq(code) * scale from the tied embedding's codes: mpv_gpt_embed_w8_fwd's conversion, bit for bit. */
int mpv_gpt_embed_rows_w8_fwd(const int64_t* ids, const int32_t* pos, const void* wte_codes, const float* wte_scale, const void* wpe,
                              void* out, int rows, int H, int max_positions, mpv_stream_t stream);
/* The decode steps on FP8 weights: mpv_gpt_decode_step / mpv_gpt_decode_step_shared with the token embedding read from the tied
 * embedding's codes and every weight product of
 *   at most MPV_W8_MAX_ROWS rows                          going to mpv_gemm_w8 on q8's codes,
 *   MPV_W8_MAX_ROWS + 1 .. MPV_W8_TILED_MAX_ROWS rows     going to mpv_gemm_w8_tiled on q8's codes (the lockstep steps: 32 x 5 rows),
 *   more rows (a many-clip prefill)                       going to mpv_gemm_bf16 on w's ORIGINAL bf16 weights.
 * So "the quantised decoder is exactly the bf16 model dequantized_state_dict() returns" holds for a state whose products all stay
 * within MPV_W8_TILED_MAX_ROWS rows; a larger prefill runs the original weights behind the dequantised embedding, which no single
 * state dict reproduces.  Everything else (norms, attention, biases, position embedding, workspace) is w's.  q8->layers must
 * equal w->layers. */
#define MPV_W8_MAX_ROWS 96 /* measured (profiles/decode_w8.json): the largest row count at which the FP8 product is not slower than
                              mpv_gemm_bf16 on most of the 1.3B decoder's four layer shapes */
#define MPV_W8_TILED_MAX_ROWS 512 /* measured (profiles/decode_w8.json): the largest of 128, 160, 256, 384, 512 rows up to which the
                                     1.3B decoder's step sum on the codes is below the bf16 one by more than the run-to-run spread */
typedef struct mpv_gpt_layer_weights_q8 {
  const void *qkv_q, *qkv_s, *dense_q, *dense_s, *fc1_q, *fc1_s, *fc2_q, *fc2_s; /* codes uint8 [N][K], scales fp32 [N] */
} mpv_gpt_layer_weights_q8;
typedef struct mpv_gpt_weights_q8 {
  int layers;
  const mpv_gpt_layer_weights_q8* layer;
  const void *wte_q, *wte_s; /* the tied embedding / LM head: codes [vocab][hidden], scales [vocab] */
} mpv_gpt_weights_q8;
int mpv_gpt_decode_step_q8(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* kv_cache, int batch, int max_len,
                           int pos0, const void* query, int Q, const int64_t* tokens, int L, void* workspace, size_t workspace_bytes,
                           void* logits, mpv_stream_t stream);
int mpv_gpt_decode_step_shared_q8(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* prefix_cache,
                                  void* const* suffix_cache, int n_groups, int fan, int prefix_len, int suffix_max, int t,
                                  const int64_t* tokens, void* workspace, size_t workspace_bytes, void* logits, mpv_stream_t stream);
/* The ragged step and prefill on FP8 weights: the row-count dispatch above, the token rows through mpv_gpt_embed_rows_w8_fwd. */
int mpv_gpt_decode_step_shared_ragged_q8(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* prefix_cache,
                                         void* const* suffix_cache, int n_groups, int fan, int prefix_stride,
                                         const int32_t* group_prefix_len, int max_prefix_len, int suffix_max, int t, const int64_t* tokens,
                                         void* workspace, size_t workspace_bytes, void* logits, mpv_stream_t stream);
int mpv_gpt_decode_step_shared_steps_q8(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* prefix_cache,
                                        void* const* suffix_cache, int n_groups, int fan, int prefix_stride, const int32_t* group_prefix_len,
                                        int max_prefix_len, int suffix_max, const int32_t* group_t, int max_t, const int64_t* tokens,
                                        void* workspace, size_t workspace_bytes, void* logits, mpv_stream_t stream);
int mpv_gpt_prefill_ragged_q8(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* kv_cache, int batch, int max_len,
                              const void* query, int Q, const int64_t* tokens, int L, const int64_t* last_row, void* workspace,
                              size_t workspace_bytes, void* logits, mpv_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Lockstep beam search over a batch of clips (caption evaluation, generation.beam_search_batched_loop): ONE launch advances the
 * beam state of `batch` clips x `beams` (K) beams by one position, doing per clip exactly what one iteration of the reference's
 * beam_search does on the host (models/modeling_distributed_gpt3.py:1793-1840 with BeamHypotheses.add / is_done, :1908-1960).
 * Input: cand_val fp32 / cand_idx int64 [batch*K][2K] -- what mpv_logprob_topk writes for k = 2K with add = scores (row b*K + j
 *   is beam j of clip b) -- the state below, `pos` (the token column this step fills), `cur_len` (positions generated so far,
 *   this one included: the done test's length) and `first` (non-zero: only beam 0 of every clip is read, :1793-1795).
 * State (device arrays, struct of arrays): tokens_in / tokens_out int64 [batch][K][row_len], two different tables that the caller
 *   swaps after every call; scores fp32 [batch][K]; the hypothesis store hyp_score fp64 [batch][K], hyp_order int32 [batch][K]
 *   (insertion counter), hyp_tokens int64 [batch][K][row_len], hyp_count / hyp_next int32 [batch], worst fp64 [batch] (initially
 *   1e9), done int32 [batch].
 * Output: src_row int64 [batch*K] = b*K + source beam (never leaves the clip: it feeds the KV re-order as it is) and next_tok
 *   int64 [batch*K].
 * Per clip: the candidates are ordered by value descending, then beam * vocab + token ascending, and the first 2K are walked.
 *   The stop token at rank >= K is skipped; at rank < K it adds tokens_in[beam] (the whole row) to the store with the score
 *   double(value) / row_len (length penalty 1.0 over the ROW length, sic): added when count < K or score > worst; then the lowest
 *   score goes, ties to the earliest inserted, and worst becomes the lowest that stays.  Any other token becomes the next beam
 *   until there are K.  Done test: count == K && worst >= double(best candidate value) / cur_len.  Otherwise tokens_out[j] =
 *   tokens_in[source beam of j] with the new token at `pos`, scores[j] = its value.  fp64 arithmetic on the fp32 inputs: the
 *   scores are those of the host loop's Python floats bit for bit.
 * A clip that is done, or becomes done in this call, is frozen: tokens_out gets its tokens_in rows unchanged, src_row is the
 *   identity, next_tok the stop token, scores stay; once done, nothing else of its state is written again.
 * Limits: beams in [1, 8], row_len in [1, 2048], 0 <= pos < row_len; a descriptor outside them is refused with a negative code
 *   before any launch.  One wave per clip, no atomics; a clip's result depends neither on `batch` nor on its place in it. */
typedef struct mpv_beam_advance_desc {
  const float* cand_val;
  const int64_t* cand_idx;
  const int64_t* tokens_in;
  int64_t* tokens_out;
  float* scores;
  double* hyp_score;
  int32_t* hyp_order;
  int64_t* hyp_tokens;
  int32_t *hyp_count, *hyp_next;
  double* worst;
  int32_t* done;
  int64_t *src_row, *next_tok;
  int batch, beams, row_len, vocab, pos, cur_len, first;
  int64_t stop_token;
} mpv_beam_advance_desc;
int mpv_beam_advance(const mpv_beam_advance_desc* d, mpv_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Diverse (group) beam search in lockstep (generation.beam_search_batched_loop with beam_groups > 1; Vijayakumar et al., "Diverse
 * Beam Search"): ONE launch advances `batch` clips x `groups` (G) groups x `beams` (K', the beams PER GROUP) by one position.  A
 * (clip, group) pair is a clip of mpv_beam_advance: every state array is the one described there with batch * G pseudo-clips,
 * pseudo-clip b*G + g being group g of clip b -- tokens_in / tokens_out int64 [batch][G][K'][row_len], scores fp32 [batch][G][K'],
 * hyp_score fp64 / hyp_order int32 [batch][G][K'], hyp_tokens int64 [batch][G][K'][row_len], hyp_count / hyp_next int32, worst
 * fp64 and done int32 [batch][G]; src_row / next_tok int64 [batch*G*K'].
 * Input: cand_val fp32 / cand_idx int64 [batch*G*K'][m] with m = 2K' + (G-1)K' -- what mpv_logprob_topk writes for k = m with
 *   add = scores -- and pos, cur_len, first, stop_token as in mpv_beam_advance; diversity_penalty (lambda, fp32).
 * Per clip the groups are processed in the order g = 0 .. G-1:
 *   A group whose done flag is set is frozen exactly as a done clip of mpv_beam_advance: rows copied to tokens_out, identity
 *   src_row, the stop token, nothing else written; it contributes nothing to the groups after it.
 *   Otherwise let c(t) be the number of next beams emitted in THIS call by the groups < g of this clip whose new token is t: only
 *   real next-beam slots count (not a slot left over with the stop token), a frozen group and one that becomes done in this call
 *   do not count, and two beams with the same token count twice.  Every candidate value v becomes v' = v - lambda * c(token), two
 *   separately rounded fp32 operations (fp32 product, then fp32 difference: no contraction); with c = 0, v' is v bit for bit.
 *   Group g then runs exactly one iteration of mpv_beam_advance's contract on its K' beams with the values v': order by v'
 *   descending, then (beam in group) * vocab + token ascending, the first 2K' walked; the stop token at rank >= K' skipped, at
 *   rank < K' added to the group's store with the score double(v') / row_len; eviction and worst as there; done test count == K'
 *   && worst >= double(best v') / cur_len; `first` reads beam 0 of the group only.  scores receive the penalised values v' (the
 *   usual definition): from the second group on the search score is not a model likelihood.  src_row = row0 + source beam with
 *   row0 the first row of the (clip, group): it never leaves the group, so it feeds the KV re-order as it is.
 * The definition is over the whole vocabulary: with every row's full log-probability vector penalised and sorted the result is the
 *   same, because at most (G-1)K' distinct tokens are penalised, lambda >= 0 and the rounding is monotone, so a row's penalised
 *   first 2K' lie inside its unpenalised first 2K' + (G-1)K' under the common tie rule, lower token first.
 * With groups = 1 every state array and output equals mpv_beam_advance's on the same input, bit for bit, whatever lambda is:
 * mpv_beam_advance is the groups = 1 case of one kernel.
 * Limits: beams in [1, 8], groups in [1, 8], groups * beams <= 16, diversity_penalty finite and >= 0, and everything
 *   mpv_beam_advance refuses (row_len in [1, 2048], 0 <= pos < row_len, batch / vocab / cur_len >= 1, a NULL pointer, tokens_in ==
 *   tokens_out); a descriptor outside them is refused with a negative code before any launch, the outputs untouched.
 * One wave per clip, the clip's groups one after the other inside it, the tokens of the earlier groups in LDS; no atomics; a
 *   clip's result depends neither on `batch` nor on its place in it. */
typedef struct mpv_beam_advance_groups_desc {
  const float* cand_val;
  const int64_t* cand_idx;
  const int64_t* tokens_in;
  int64_t* tokens_out;
  float* scores;
  double* hyp_score;
  int32_t* hyp_order;
  int64_t* hyp_tokens;
  int32_t *hyp_count, *hyp_next;
  double* worst;
  int32_t* done;
  int64_t *src_row, *next_tok;
  int batch, beams, row_len, vocab, pos, cur_len, first, groups;
  float diversity_penalty;
  int64_t stop_token;
} mpv_beam_advance_groups_desc;
int mpv_beam_advance_groups(const mpv_beam_advance_groups_desc* d, mpv_stream_t stream);
/* mpv_beam_advance_groups (groups = 1: mpv_beam_advance) for clips that sit at different generation steps -- a finished clip's slot
 * was given to the next clip while the others went on (generation.beam_inflight_loop).  clip_prompt_len and clip_step are DEVICE
 * int32 [d->batch], one value per real clip (not per (clip, group)); the token table is LEFT-aligned, clip c's prompt in columns
 * [0, clip_prompt_len[c]).  For clip c with s = clip_step[c] the call uses pos = clamp(clip_prompt_len[c], 0, row_len) + s,
 * cur_len = s + 1 and first = (s == 0) for all of the clip's groups; d->pos, d->cur_len and d->first are ignored and not checked.
 * A clip with s < 0 (a free slot) or pos >= row_len is FROZEN with all its groups: rows copied to tokens_out, identity src_row, the
 * stop token in next_tok; nothing else is written -- done included -- and neither a candidate nor the done flag is read.
 * Contract: a clip at step s is, bit for bit in every state array and output, the uniform entry (mpv_beam_advance_groups, or
 * mpv_beam_advance at groups = 1) on that clip alone with pos = prompt_len + s, cur_len = s + 1, first = (s == 0); with one common
 * step the call is the uniform entry on the whole batch.  The same kernel body, compiled with one more flag; a workgroup reads its
 * clip's two values once (they are wave-uniform).  One entry serves the plain and the group search.
 * Refused before any launch, the outputs untouched: what mpv_beam_advance_groups refuses except the pos / cur_len checks, and a NULL
 * clip_prompt_len or clip_step. */
int mpv_beam_advance_steps(const mpv_beam_advance_groups_desc* d, const int32_t* clip_prompt_len, const int32_t* clip_step,
                           mpv_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Sampled generation in lockstep (generation.sample_batched_loop): ONE launch draws the next token of `rows` sequences and does the
 * bookkeeping of one iteration of the reference's sample loop (models/modeling_distributed_gpt3.py:1689-1728).  The filters follow
 * :1369-1441; the tie order that the reference leaves to an unstable sort is fixed here.  One sampling step of row r:
 * Input: logits row r of a bf16 [rows][ld] matrix, first `vocab` columns; temperature T > 0; exactly one of plain (top_k == 0,
 *   top_p == 0), greedy (top_k == 1), top-k (top_k > 1), top-p (0 < top_p <= 1).  NaN logits are not supported.
 * Probabilities: z_i = float(l_i) / T, p_i proportional to exp(z_i - max z), fp32.  A logit of -inf has probability 0 and is never
 *   a member of the kept set (it is not counted in out_kept and cannot be drawn).  -0 and +0 are one value.
 * Greedy: the arg-max, lowest index among ties (the rule of mpv_logprob_topk).
 * Top-k (k > 1): every i with l_i >= the k-th largest logit stays; ties with the k-th value all stay (the reference's
 *   `logits < kth` mask).
 * Top-p: order by (logit descending, index ascending); with c_j the inclusive cumulative probability in that order, entry j stays
 *   iff j == 0 or c_{j-1} <= top_p (the reference's right-shifted `cumulative > top_p` mask).  top_p == 1 keeps everything.
 * Draw: u in [0, 1); the token is the smallest index i, in VOCABULARY-INDEX order, of the kept set with
 *   sum_{kept j <= i} p_j > u * sum_{kept} p_j; if no index qualifies, the last kept index.  (Index order: a plain prefix scan,
 *   independent of any sort.)
 * The uniform: u = (h >> 8) * 2^-24 with h the 32-bit hash mpv_rand_pair of csrc/mpv_common.h for the seed `seed` and the counter
 *   (uint64(pos) << 32) | uint32(stream_id[r]); stream_id is a per-row int64 array of the caller's choice, NULL = the row index.  A
 *   row's token depends on (its logits, T, the filter, seed, pos, stream_id[r]) only -- neither on `rows` nor on the row's place in
 *   the launch.  u_override (fp32 [rows], optional) replaces the hash; the generation loop does not use it.
 * Clamp: with vocab_size > 0 the token is clamped to [0, vocab_size - 1] (the reference's padded-vocabulary clamp); 0 = no clamp.
 * A row whose every logit is -inf yields token 0, kept count 0, kept mass 0.
 * Bookkeeping, per row: started = prompt_len[r] <= pos; if started, tokens[r][pos] = token, otherwise the prompt token stays
 *   (teacher forcing); next_tok[r] = tokens[r][pos] after that; done[r] |= started && terminated(token), with termination_mode
 *   0: token == termination_id; 1 (stop_on_eol): token is 628 or 198; 2 (stop_on_double_eol): 628, or 198 with tokens[r][pos - 1]
 *   == 198 (pos == 0 has no previous token).  n_done (one int32) receives the number of rows whose done flag is set after the call.
 *   tokens is int64 [rows][row_len], updated in place: a row writes only its own column `pos`.
 * Optional outputs (NULL = not wanted): out_kept int32 [rows] the size of the kept set, out_mass fp32 [rows] its mass as a fraction
 *   of the total, out_token int64 [rows] the (clamped) sampled token before the started / teacher-forcing logic.
 * Refused with a negative code before any launch: vocab not a multiple of 8 or outside [8, 65536]; ld < vocab or ld % 8 != 0;
 *   logits not 16-byte aligned; T <= 0 or not finite; top_k > 1 or top_k == 1 together with top_p > 0; top_k < 0 or > vocab;
 *   top_p < 0 or > 1; pos outside [0, row_len); a termination_mode other than 0, 1, 2; a NULL logits / tokens / prompt_len / done /
 *   next_tok / n_done.
 * One workgroup per row, the row read once; fixed-order reductions and no floating-point atomics: the same inputs give the same
 *   outputs, bit for bit, on every run. */
typedef struct mpv_sample_advance_desc {
  const void* logits;
  const int64_t* stream_id;
  const float* u_override;
  const int64_t* prompt_len;
  int64_t* tokens;
  int32_t* done;
  int64_t* next_tok;
  int32_t* n_done;
  int32_t* out_kept;
  float* out_mass;
  int64_t* out_token;
  int64_t ld;
  uint64_t seed;
  int64_t termination_id;
  int rows, vocab, row_len, pos, top_k, vocab_size, termination_mode;
  float temperature, top_p;
} mpv_sample_advance_desc;
int mpv_sample_advance(const mpv_sample_advance_desc* d, mpv_stream_t stream);
/* The same step for rows whose prompts differ in length (one lockstep loop over prompts of different lengths, the table
 * left-aligned: row r's prompt sits at columns [0, prompt_len[r])).  The descriptor is the same; d->pos is the generation STEP
 * t >= 0, not a column, and row r works on its own column c_r = clamp(prompt_len[r], 0, row_len) + t, a per-workgroup value that
 * the row's workgroup reads once.  One kernel body serves both entries.
 * Row r with c_r < row_len is started (there is no teacher forcing here: c_r lies behind the prompt): it draws with the counter
 *   (uint64(c_r) << 32) | uint32(stream_id[r]), writes tokens[r][c_r] and next_tok[r]; termination mode 2 looks at tokens[r][c_r - 1]
 *   (c_r == 0 has no previous token).
 * Row r with c_r >= row_len is FROZEN (its budget has ended, or its length was bad): no logit is read, no token is written,
 *   done[r] = 1 (the row counts in n_done), next_tok[r] = tokens[r][row_len - 1], and the optional outputs get token 0, kept 0, mass 0.
 * Invariants:
 *   a row's result depends on its own logits, tokens[r][c_r - 1], done[r], prompt_len[r], t and the scalars only -- neither on
 *     `rows` nor on the row's place in the launch;
 *   a row of a ragged launch equals, bit for bit, mpv_sample_advance run on that row alone at pos = c_r (with a prompt_len <= c_r);
 *     with every prompt_len equal to p the launch equals mpv_sample_advance at pos = p + t, n_done included;
 *   a bad prompt_len[r] (negative: taken as 0; beyond row_len: frozen) touches only row r.
 * Refused: what mpv_sample_advance refuses (prompt_len must not be NULL), and t outside [0, row_len). */
int mpv_sample_advance_ragged(const mpv_sample_advance_desc* d, mpv_stream_t stream);
/* The same step for rows that ALSO differ in their generation step (rows of clips that entered a running loop at different times).
 * The descriptor is the same and d->pos is ignored; row_step is a DEVICE int32 [rows].  Row r works on column
 * c_r = clamp(prompt_len[r], 0, row_len) + row_step[r].  A row with row_step[r] < 0 or c_r >= row_len is FROZEN exactly as above: no
 * logit read, no token written, done[r] = 1, counted in n_done.  Bit for bit: with every row_step[r] == t the launch equals
 * mpv_sample_advance_ragged at step t; a row equals mpv_sample_advance run on that row alone at pos = c_r.
 * Refused: what mpv_sample_advance_ragged refuses except a d->pos out of range, and a NULL row_step. */
int mpv_sample_advance_steps(const mpv_sample_advance_desc* d, const int32_t* row_step, mpv_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Generation constraints in lockstep (generation.LogitsConstraints): ONE launch edits one step's logits in place, before
 * mpv_sample_advance or mpv_logprob_topk reads them, from the loop's own device token table -- the CTRL repetition penalty, the
 * no-repeat n-gram ban, the minimum length and a list of banned ids.  They act on the RAW logits (before temperature, filter and
 * log_softmax).
 * Input: logits bf16 [rows][ld], 16-byte aligned, the first `vocab` columns are the row; tokens int64 [rows][row_len] (the token
 *   table of mpv_sample_advance, or the one of mpv_beam_advance seen as [batch*K][row_len]); prompt_len int64 [rows], or NULL: then
 *   every row has the prompt length prompt_len_all; eos_ids int64 [n_eos], n_eos in [0, 8]; banned_ids int64 [n_banned], n_banned
 *   in [0, 1024] (both device arrays); pos, the token column this step fills; penalty > 0 (1 = off); ngram 0 (off) or 1 .. 8;
 *   min_new_tokens >= 0; include_prompt 0 / 1; ban_value, -inf or finite and negative, stored rounded to bf16.
 * Row r: with prompt_len[r] > pos the row is teacher-forced and is left untouched, bit for bit.  Otherwise the history is
 *   h = tokens[r][start : pos], start = include_prompt ? 0 : prompt_len[r], of length m, and g = pos - prompt_len[r] tokens have
 *   been generated.  History tokens outside [0, vocab) are ignored everywhere (they never form an address), except that they take
 *   part in the n-gram comparison like any other value.
 * 1. Repetition penalty (penalty != 1): every DISTINCT in-range token v of h is penalised once, however often it occurs:
 *   x = float(logits[v]) becomes bf16_rne(x < 0 ? x * penalty : x / penalty), one fp32 multiply or IEEE-correct divide.
 * 2. No-repeat n-gram: ngram == 1 bans every token of h.  ngram = n >= 2, when m >= n: with s = h[m-n+1 : m], for every i in
 *   [0, m-n] with h[i : i+n-1] == s the token h[i+n-1] is banned, if it is in range.
 * 3. Minimum length: while g < min_new_tokens every in-range id of eos_ids is banned.
 * 4. Every in-range id of banned_ids is banned, always.
 * A banned logit becomes ban_value; the ban wins over the penalty.  No other logit is read or written: not the columns >= vocab,
 *   not the bf16 next to an edited one (2-byte stores).  A row's result depends on its own logits, its history and the scalars only
 *   -- neither on `rows` nor on the row's place in the launch -- and every edited logit has one writer rule: the result does not
 *   depend on thread timing.  If every logit of a row ends up banned, the readers' own rules apply (mpv_sample_advance: token 0).
 * ban_value: mpv_sample_advance defines -inf as probability 0, never kept: the value for sampling.  mpv_logprob_topk takes
 *   exp(v - max) per vocabulary slice, and a slice that is -inf throughout is exp(NaN): beam search passes the lowest finite bf16
 *   (-0x1.fep127) instead, which goes through both of its kernels as an exact zero probability.
 * Refused with a negative code before any launch, logits untouched: a NULL logits / tokens; vocab not a multiple of 8 or outside
 *   [8, 65536]; ld < vocab or ld % 8 != 0; logits not 16-byte aligned; rows < 1; row_len outside [1, 2048]; pos outside [0, row_len);
 *   penalty <= 0 or not finite; ngram outside [0, 8]; min_new_tokens < 0; include_prompt other than 0 / 1; n_eos or n_banned outside
 *   its range, or positive with a NULL array; a ban_value that is NaN, +inf or >= 0.  A descriptor with everything off (penalty 1,
 *   ngram 0, no banned id, min_new_tokens 0 or no eos id) launches nothing and returns 0.
 * One workgroup per row, the history in LDS; the work follows the history (O(m n) + the O(m^2) first-occurrence test + distinct
 *   tokens x listed ids), never the vocabulary.  No atomics, no floating-point reductions. */
typedef struct mpv_logits_constrain_desc {
  void* logits;
  const int64_t* tokens;
  const int64_t* prompt_len;
  const int64_t* eos_ids;
  const int64_t* banned_ids;
  int64_t ld;
  int64_t prompt_len_all;
  int rows, vocab, row_len, pos, n_eos, n_banned, ngram, min_new_tokens, include_prompt;
  float penalty, ban_value;
} mpv_logits_constrain_desc;
int mpv_logits_constrain(const mpv_logits_constrain_desc* d, mpv_stream_t stream);
/* The same edit for rows whose prompts differ in length (the left-aligned table of mpv_sample_advance_ragged).  The descriptor is
 * the same; d->pos is the generation STEP t >= 0, prompt_len must not be NULL (prompt_len_all is ignored), and row r works on its
 * own column c_r = clamp(prompt_len[r], 0, row_len) + t, a per-workgroup value read once.  One kernel body serves both entries.
 * Row r with c_r < row_len: the history is tokens[r][start : c_r], start = include_prompt ? 0 : prompt_len[r], and g = t tokens
 *   have been generated.  The table has no padding, so include_prompt = 1 sees exactly the row's prompt.
 * Row r with c_r >= row_len is frozen: its logits stay untouched, bit for bit.
 * Invariants: a row's result depends on its own logits, its history, prompt_len[r], t and the scalars only -- neither on `rows`
 *   nor on the row's place in the launch; a row of a ragged launch equals, bit for bit, mpv_logits_constrain run on that row alone
 *   at pos = c_r with that prompt_len; a bad prompt_len[r] (negative: 0; beyond row_len: frozen) touches only row r.
 * Refused: what mpv_logits_constrain refuses, a NULL prompt_len, and t outside [0, row_len). */
int mpv_logits_constrain_ragged(const mpv_logits_constrain_desc* d, mpv_stream_t stream);
/* ... and for rows that also differ in their step (mpv_sample_advance_steps): d->pos is ignored, row r works on column
 * c_r = clamp(prompt_len[r], 0, row_len) + row_step[r] (DEVICE int32 [rows]) with g = row_step[r] generated tokens.  A row with
 * row_step[r] < 0 or c_r >= row_len is frozen: its logits stay untouched.  Bit for bit the ragged entry when every row_step[r] == t,
 * and mpv_logits_constrain on that row alone at pos = c_r.  Refused: as the ragged entry except d->pos, and a NULL row_step. */
int mpv_logits_constrain_steps(const mpv_logits_constrain_desc* d, const int32_t* row_step, mpv_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Guided decoding (generation.Guidance; classifier-free guidance, also known as contrastive decoding): ONE launch rewrites one step's
 * CONDITIONAL logits in place from the UNCONDITIONAL ones of a second branch that ran in lockstep behind a "null" video, before
 * mpv_logits_constrain, mpv_logits_trie_mask, mpv_sample_advance, mpv_sample_score or mpv_logprob_topk sees them.
 * Input: cond bf16 [rows][ld_c], edited in place; uncond bf16 [rows][ld_u], read only and left bit for bit (it may live in the same
 *   allocation as cond, on other rows); both 16-byte aligned, the first `vocab` columns are the row; scale_m1 = float(guidance_scale
 *   - 1), computed on the host; plaus_log = log(alpha) computed on the host, <= 0, -inf = off; ban_value, -inf or finite and negative,
 *   stored rounded to bf16.  The inputs are the raw, finite logits.
 * Row r: m_c = max_v float(cond[r][v]) and m_u = max_v float(uncond[r][v]) over v < vocab -- exact and order-free; a maximum that is a
 *   zero counts as +0.  Then for every v < vocab
 *     c = float(cond[r][v]) - m_c,  u = float(uncond[r][v]) - m_u,  g = c + scale_m1 * (c - u),  cond[r][v] = bf16_rne(g)
 *   where each subtract, the multiply and the add is ONE IEEE fp32 operation: the multiply and the add are not contracted into a
 *   fused one.  guidance_scale = 1 (scale_m1 = 0) therefore yields the centred conditional logits, guidance_scale = 0 the centred
 *   unconditional ones up to rounding.
 * Plausibility (plaus_log > -inf): a token with c < plaus_log -- p_cond(v) < alpha * max p_cond -- becomes ban_value instead.  The
 *   arg-max of cond has c = 0 >= plaus_log and always survives.
 * Columns >= vocab of either matrix are neither read nor written.  A row's result depends on its own two rows and the scalars only --
 *   neither on `rows` nor on the row's place in the launch -- and every column has one writer: the result does not depend on thread
 *   timing.  No atomics.  A non-finite element follows IEEE through the stated operations and is not otherwise defined; NaN is excluded.
 * ban_value: -inf for mpv_sample_advance, the lowest finite bf16 in front of mpv_logprob_topk, as for mpv_logits_constrain.
 * Refused with a negative code before any launch, logits untouched: what mpv_logits_constrain refuses about pointers, vocab, ld,
 *   alignment and rows, applied to both matrices (a NULL cond / uncond; vocab not a multiple of 8 or outside [8, 65536]; ld_c or ld_u
 *   < vocab or not a multiple of 8; cond or uncond not 16-byte aligned; rows < 1); a scale_m1 that is not finite or < -1; plaus_log > 0
 *   or NaN; a ban_value that is NaN, +inf or >= 0.
 * One workgroup per row; the row pair is loaded once in 16-byte chunks and kept in registers across the maximum, so the launch moves
 *   3 * rows * vocab * 2 bytes. */
typedef struct mpv_logits_guide_desc {
  void* cond;
  const void* uncond;
  int64_t ld_c, ld_u;
  int rows, vocab;
  float scale_m1, plaus_log, ban_value;
} mpv_logits_guide_desc;
int mpv_logits_guide(const mpv_logits_guide_desc* d, mpv_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Closed-vocabulary generation (generation.PhraseTrie, LogitsConstraints.allowed_phrases): ONE launch keeps, in one step's logits,
 * only the tokens that continue the row's generated history along a trie of allowed phrases, after mpv_logits_constrain (a ban
 * still wins) and before mpv_sample_advance or mpv_logprob_topk reads them.  The state of the walk is the loop's own token table.
 * The trie is four DEVICE arrays in CSR form, node 0 the root: child_begin int32 [n_nodes + 1]; child_tok int32 [n_edges], strictly
 *   ascending inside each node's run [child_begin[u], child_begin[u + 1]); child_node int32 [n_edges], the node an edge leads to;
 *   terminal int32 [n_nodes], the index of the phrase that ends at the node, or -1.
 * Input: logits bf16 [rows][ld], 16-byte aligned, the first `vocab` columns are the row; tokens int64 [rows][row_len]; prompt_len
 *   int64 [rows], or NULL: then every row has the prompt length prompt_len_all; eos_ids int64 [n_eos] (device), 1 <= n_eos <= 8;
 *   pos, the token column this step fills; ban_value, -inf or finite and negative, stored rounded to bf16; node_out int32 [rows]
 *   (device) or NULL.
 * Row r at column c = pos:
 * 1. prompt_len[r] > c (teacher-forced): the row is left untouched, bit for bit, and node_out[r] = -2.
 * 2. Otherwise the history is tokens[r][prompt_len[r] : c], the generated tokens only (a negative prompt_len counts as 0).  The walk
 *   starts at the root; every token must be a child of the current node.  A token that is not a child makes the row DEAD: an
 *   out-of-range token, a termination id (no phrase holds one) and anything behind a termination id.
 * 3. A live row at node u allows the child tokens of u and, when terminal[u] >= 0, every in-range id of eos_ids.
 * 4. A dead row allows the in-range ids of eos_ids only: a row that left the trie ends at once.
 * 5. Every column in [0, vocab) that is not allowed becomes ban_value; every allowed column keeps its bits; columns >= vocab are
 *   neither read nor written.  node_out[r] = u for a live row, -1 for a dead one.
 * Invariants: a row's result depends on its own logits, its history, its lengths and the scalars only -- neither on `rows` nor on
 *   the row's place in the launch; every column has one writer; the result does not depend on thread timing; no atomics.
 * ban_value: -inf for mpv_sample_advance, the lowest finite bf16 in front of mpv_logprob_topk, as for mpv_logits_constrain.
 * Refused with a negative code before any launch, logits untouched: what mpv_logits_constrain refuses about logits / vocab / ld /
 *   rows / row_len / pos; n_eos outside [1, 8] or a NULL eos_ids; a NULL trie array; n_nodes < 1; a ban_value that is NaN or >= 0.
 * One workgroup per row: the history goes through LDS, a wave walks it with a 64-ary search of every node's sorted child run, and
 *   the row is written once in 16-byte chunks; a chunk is loaded only when the child run says it holds an allowed token.  Indices read
 *   from the trie arrays are checked against n_nodes / n_edges before they become addresses. */
typedef struct mpv_logits_trie_desc {
  void* logits;
  const int64_t* tokens;
  const int64_t* prompt_len;
  const int64_t* eos_ids;
  const int32_t* child_begin;
  const int32_t* child_tok;
  const int32_t* child_node;
  const int32_t* terminal;
  int32_t* node_out;
  int64_t ld;
  int64_t prompt_len_all;
  int rows, vocab, row_len, pos, n_eos, n_nodes, n_edges;
  float ban_value;
} mpv_logits_trie_desc;
int mpv_logits_trie_mask(const mpv_logits_trie_desc* d, mpv_stream_t stream);
/* The same mask for a LEFT-ALIGNED table of prompts of different lengths: d->pos is the generation STEP t >= 0, prompt_len must not
 * be NULL, and row r works on its own column c_r = clamp(prompt_len[r], 0, row_len) + t.  A row with c_r >= row_len is frozen: its
 * logits stay untouched and node_out[r] = -2.  A row equals, bit for bit, mpv_logits_trie_mask on that row alone at pos = c_r.
 * Refused: what mpv_logits_trie_mask refuses, a NULL prompt_len, and t outside [0, row_len). */
int mpv_logits_trie_mask_ragged(const mpv_logits_trie_desc* d, mpv_stream_t stream);
/* ... and for rows that also differ in their step: d->pos is ignored, row r works on column c_r = clamp(prompt_len[r], 0, row_len) +
 * row_step[r] (DEVICE int32 [rows]).  A row with row_step[r] < 0 or c_r >= row_len is frozen.  Bit for bit the ragged entry when every
 * row_step[r] == t.  Refused: as the ragged entry except d->pos, and a NULL row_step. */
int mpv_logits_trie_mask_steps(const mpv_logits_trie_desc* d, const int32_t* row_step, mpv_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Pairwise overlap counts between caption candidates (generation.consensus_utility / consensus_choice: the consensus, or
 * minimum-Bayes-risk, choice among a clip's samples or beams): for every ordered pair of every group, the length of the longest
 * common subsequence and the clipped n-gram matches of the orders 1 .. 4, over TOKEN IDS.
 * Tables: tok_a int64 [rows_a][ld_a] and tok_b int64 [rows_b][ld_b] (device), of which the first width_a / width_b columns are the
 *   row (ld >= width).  The same table may be passed twice (a clip's samples against each other); two tables serve "candidates
 *   against references".  start_x int32 [rows_x] (device): the first generated column of the row, in [0, width_x]; rows of one call
 *   may differ in it.  begin_x int32 [groups + 1] (device): CSR, group g holds the rows [begin_x[g], begin_x[g + 1]) of side x,
 *   begin_x[0] = 0, begin_x[groups] = rows_x, non-decreasing: a group may have 0 rows on either side.
 * Candidate: row r's candidate is tok[r][start[r] : e], e the column of the first `term` at or behind start[r], or width when there
 *   is none.  A `term` in front of start[r] (inside the prompt) does not end it.  Its length is at most
 *   MPV_CAPTION_OVERLAP_MAX_LEN: a row with width - start[r] above that is refused.
 * Outputs (device): len_a int32 [rows_a], len_b int32 [rows_b], the candidates' lengths; counts int32 [pairs][5] with pairs =
 *   sum_g nA_g * nB_g: group g's nA_g x nB_g pairs row-major (a outer, b inner) from row pair_begin[g] on.  pair_begin int64
 *   [groups + 1] (device) holds the running sums, pair_begin[0] = 0.  counts[p] = { LCS(a, b), m1, m2, m3, m4 }, m_n = sum over the
 *   distinct n-grams g of min(count_a(g), count_b(g)); an order longer than either candidate gives 0.  All five are symmetric in
 *   (a, b).
 * Host copies: host_start_a / host_start_b / host_begin_a / host_begin_b / host_pair_begin are the same five arrays in HOST memory;
 *   the refusals below are decided on them, so that nothing is launched over a bad layout.  The kernels read the device arrays and
 *   clamp what they read, so that even arrays that differ from the host copies cannot make them read outside the tables or hang.
 * Invariants: a pair has one writer; no atomics; the outputs depend on the pair's two candidates only and not on thread timing;
 *   no column at or beyond width_x is read.  No limit on the rows of a group or on the number of groups (pairs / 64 < 2^31).
 * When tok_b, start_b, len_b, ld_b, width_b and rows_b equal side a's, the lengths are computed once.
 * Refused with a negative code before any launch: a NULL descriptor or pointer (MPV_E_ARG); groups < 1, negative rows or widths,
 *   ld < width (MPV_E_SHAPE); a begin that does not start at 0, end at rows or is not monotone, a start outside [0, width], a
 *   pair_begin that is not the running sum of nA_g * nB_g (MPV_E_ARG); width - start above MPV_CAPTION_OVERLAP_MAX_LEN
 *   (MPV_E_SHAPE). */
#define MPV_CAPTION_OVERLAP_MAX_LEN 255
#define MPV_CAPTION_OVERLAP_COUNTS 5
typedef struct mpv_caption_overlap_desc {
  const int64_t* tok_a;
  const int64_t* tok_b;
  const int32_t* start_a;
  const int32_t* start_b;
  const int32_t* begin_a;
  const int32_t* begin_b;
  const int64_t* pair_begin;
  int32_t* len_a;
  int32_t* len_b;
  int32_t* counts;
  const int32_t* host_start_a;
  const int32_t* host_start_b;
  const int32_t* host_begin_a;
  const int32_t* host_begin_b;
  const int64_t* host_pair_begin;
  int64_t ld_a;
  int64_t ld_b;
  int64_t term;
  int rows_a, rows_b, width_a, width_b, groups;
} mpv_caption_overlap_desc;
int mpv_caption_overlap(const mpv_caption_overlap_desc* d, mpv_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * CIDEr of caption candidates against references (generation.CiderStats; DistributedGPT3_Caption.forward_scst's reward and the
 * caption entry point's corpus metric): the reference scorer's compute_cider over TOKEN IDS with corpus statistics from a table.
 * Tables, starts, CSR offsets, pair order, candidate definition, host copies and the 255-token limit are mpv_caption_overlap's:
 *   side a holds the candidates, side b the references, group g's nA_g x nB_g pairs lie row-major from pair_begin[g] on.
 * Corpus table (device): table_keys uint64 [table_capacity], table_idf fp64 [table_capacity], open addressing with linear probing.
 *   Key of an n-gram (n = 1 .. 4) of ids t_0 .. t_{n-1}: sum_i (t_i + 1) << (16 * i) -- exact for ids in [0, 65534], the order is
 *   implied by the highest non-zero field, 0 is the empty slot.  table_capacity is a power of two; the slot of a key is the
 *   splitmix64 finaliser of the key (x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31)
 *   masked by table_capacity - 1 -- ONE function in the library, which the kernel's probe and the host entries at the end of this
 *   section share --, then the following slots, wrapping, up to the first empty one.  table_idf[slot] = log_ref_len - log(max(1, df)), taken in fp64 on the host; a key that is not in
 *   the table weighs log_ref_len (df = 0).  The device takes no logarithm.  A probe gives up after table_capacity slots: a table
 *   without an empty slot cannot hang the kernel.
 * Arithmetic, per pair (c, r) and order n, all in fp64: vec_x[g] = count_x(g) * idf(g) over the distinct n-grams g of x;
 *   norm_x = sqrt(sum_g vec_x[g]^2); val = sum over the distinct g of c of min(vec_c[g], vec_r[g]) * vec_r[g]; val /= norm_c *
 *   norm_r when both are non-zero; val *= exp(-(len_c - len_r)^2 / (2 sigma^2)).  The reference scorer measures a length in
 *   bigrams (len - 1, and 0 for an empty caption): the difference is the same for all non-empty captions, and every value that
 *   involves an empty caption is 0 whatever the penalty.
 * Outputs (device, fp64): pair [pairs][4] = val of the orders 1 .. 4; score [rows_a] = 10 * mean_n(sum_r pair[c][r][n] / nB_g),
 *   0.0 for the candidates of a group without references.
 * Invariants: every value has one writer; no atomics; every sum runs in an order that is a function of the two captions alone (a
 *   lane's positions ascending, then a fixed butterfly over the lanes; the references of a candidate ascending): a pair's four
 *   values and a candidate's score are bit-identical whatever else is in the call.  No column at or beyond width_x is read.
 * Workspace: mpv_caption_cider_workspace_size(d) bytes (read from the host copies: the rows' keys and weights per position and
 *   order, their norms and lengths), 8-byte aligned.
 * Refused with a negative code before any launch: what mpv_caption_overlap refuses; a NULL table or output; table_capacity that is
 *   no power of two or below 2; a log_ref_len that is negative or not finite; sigma that is not positive and finite; a NULL,
 *   misaligned or too small workspace. */
#define MPV_CAPTION_CIDER_ORDERS 4
typedef struct mpv_caption_cider_desc {
  const int64_t* tok_a;
  const int64_t* tok_b;
  const int32_t* start_a;
  const int32_t* start_b;
  const int32_t* begin_a;
  const int32_t* begin_b;
  const int64_t* pair_begin;
  const uint64_t* table_keys;
  const double* table_idf;
  double* pair;
  double* score;
  const int32_t* host_start_a;
  const int32_t* host_start_b;
  const int32_t* host_begin_a;
  const int32_t* host_begin_b;
  const int64_t* host_pair_begin;
  int64_t ld_a;
  int64_t ld_b;
  int64_t term;
  int64_t table_capacity;
  double log_ref_len;
  double sigma;
  int rows_a, rows_b, width_a, width_b, groups;
} mpv_caption_cider_desc;
size_t mpv_caption_cider_workspace_size(const mpv_caption_cider_desc* d);
int mpv_caption_cider(const mpv_caption_cider_desc* d, void* workspace, size_t workspace_bytes, mpv_stream_t stream);
/* The corpus table on the HOST, with the slot rule above: fill inserts n distinct non-zero keys with their values into
 * table_keys / table_idf (both zeroed here first; capacity a power of two > n) -> 0, or a negative code; lookup -> the slot of
 * `key`, or -1 when it is absent (key 0 is never present). */
int mpv_cider_table_fill(const uint64_t* keys, const double* idf, int64_t n, uint64_t* table_keys, double* table_idf, int64_t capacity);
int64_t mpv_cider_table_lookup(const uint64_t* table_keys, int64_t capacity, uint64_t key);
/* ------------------------------------------------------------------------------------------
 * Sequence scores of sampled generation in lockstep (generation.SampleScores): ONE launch, right after mpv_sample_advance, records
 * the model's log-probability of the token that call wrote into column `pos` -- log_softmax of the RAW logits the sampler read
 * (after mpv_logits_constrain edited them, if it did).  Temperature, top-k and top-p are ignored by design: the score is the
 * model's under the constraints, not the proposal's.
 * Input: logits bf16 [rows][ld], 16-byte aligned, the first `vocab` columns are the row, exactly what mpv_sample_advance read this
 *   step; tokens int64 [rows][row_len] AFTER mpv_sample_advance wrote column pos; prompt_len int64 [rows]; done int32 [rows], the
 *   sampler's flags AFTER its call.  State, owned by the scoring: live int32 [rows] (initially 1), token_logprob fp32
 *   [rows][row_len] (initially 0), sum_logprob fp32 [rows] (initially 0), count int32 [rows] (initially 0).
 * Row r: with prompt_len[r] > pos (teacher-forced) or live[r] == 0 (terminated in an earlier call: the sampler lets such a row go
 *   on drawing until the chunk ends) nothing of the row is read except those two words, and nothing is written.  Otherwise, with
 *   t = tokens[r][pos], x_i = float(logits[r][i]) for i < vocab, m = max x_i and S = sum exp(x_i - m) in fp32, where a logit of
 *   -inf contributes 0:  lp = x_t - (m + log S).  If x_t is -inf, lp = -inf explicitly, whatever the rest of the row is (the
 *   all-banned row, where the sampler emits token 0, included): never NaN.  If t is outside [0, vocab), lp = NaN (the loop cannot
 *   produce that; it makes misuse loud).  Then, by one thread: token_logprob[r][pos] = lp; sum_logprob[r] += lp; count[r] += 1;
 *   live[r] = done[r] ? 0 : 1.  The terminating token itself is scored, every position behind it is not.
 * NaN and +inf logits are not supported, as in mpv_sample_advance.  Columns at and beyond vocab are never read.
 * A row's result depends on its own logits, its token and its own state only -- neither on `rows` nor on the row's place in the
 *   launch.  The reductions run in a fixed order, without floating-point atomics: the same inputs give the same bits on every run.
 * Refused with a negative code before any launch, every output untouched: a NULL pointer; vocab not a multiple of 8 or outside
 *   [8, 65536]; ld < vocab or ld % 8 != 0; logits not 16-byte aligned; rows < 1; row_len outside [1, 2048]; pos outside [0, row_len).
 * One workgroup per row, the row read once with 16-byte loads and held in registers (max, then sum); no scratch. */
typedef struct mpv_sample_score_desc {
  const void* logits;
  const int64_t* tokens;
  const int64_t* prompt_len;
  const int32_t* done;
  int32_t* live;
  float* token_logprob;
  float* sum_logprob;
  int32_t* count;
  int64_t ld;
  int rows, vocab, row_len, pos;
} mpv_sample_score_desc;
int mpv_sample_score(const mpv_sample_score_desc* d, mpv_stream_t stream);
/* The same record for rows whose prompts differ in length, right after mpv_sample_advance_ragged.  The descriptor is the same;
 * d->pos is the generation STEP t >= 0 and row r scores the token at its own column c_r = clamp(prompt_len[r], 0, row_len) + t
 * (a per-workgroup value read once) into token_logprob[r][c_r].  One kernel body serves both entries.
 * A row with c_r >= row_len (frozen) or live[r] == 0 (dead) reads nothing else and writes nothing: logits and state stay bit for bit.
 * Invariants: a row's result depends on its own logits, its token, its state, prompt_len[r] and t only -- neither on `rows` nor on
 *   the row's place in the launch; a row of a ragged launch equals, bit for bit, mpv_sample_score run on that row alone at
 *   pos = c_r; a bad prompt_len[r] (negative: 0; beyond row_len: frozen) touches only row r.
 * Refused: what mpv_sample_score refuses (prompt_len must not be NULL), and t outside [0, row_len). */
int mpv_sample_score_ragged(const mpv_sample_score_desc* d, mpv_stream_t stream);
/* ... and for rows that also differ in their step, right after mpv_sample_advance_steps: d->pos is ignored, row r scores the token at
 * column c_r = clamp(prompt_len[r], 0, row_len) + row_step[r] (DEVICE int32 [rows]).  A row with row_step[r] < 0 or c_r >= row_len
 * (frozen) or live[r] == 0 writes nothing.  Bit for bit the ragged entry when every row_step[r] == t, and mpv_sample_score on that
 * row alone at pos = c_r.  Refused: as the ragged entry except d->pos, and a NULL row_step. */
int mpv_sample_score_steps(const mpv_sample_score_desc* d, const int32_t* row_step, mpv_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Device-side video input transform (configs' video_pretrain/train/test transforms,
 * dataset/__init__.py:60-85): the decoder's uint8 clip [T][H][W][3] -> crop (i, j, h, w) ->
 * torch.nn.functional.interpolate to out_h x out_w (mode 0 nearest / 1 bilinear / 2 bicubic, align_corners=False:
 * dataset/video_utils/functional.py:51-72, 95-112) -> .long() truncation -> optional horizontal flip
 * (video_transforms.py:933-936) -> /255 and (x - mean) / std (volume_transforms.py:40-42, functional.py:125-136) ->
 * bf16, written as planes: element (c, t, y, x) at out[c*c_stride + t*t_stride + y*out_w + x] (a [B,3,T,H,W] batch slot).
 * mean3 / std3 are host arrays.  (TemporalConsistentRandomAugment is cv2-based and not part of this entry point.) */
int mpv_video_resized_crop_normalize(const uint8_t* clip, int T, int H, int W, int crop_i, int crop_j, int crop_h, int crop_w,
                                     int out_h, int out_w, int mode, int flip, const float* mean3, const float* std3, void* out,
                                     int64_t c_stride, int64_t t_stride, mpv_stream_t stream);

/* The clip-consistent RandAugment of the loaders (dataset/video_utils/randaugment_video.py; dataset/__init__.py:65-66,75-76) on the
 * device, on uint8 clips [T][H][W][3].  mpv_video_resized_crop_u8 is mpv_video_resized_crop_normalize stopped at the point where
 * the augmentation takes over: the .long() value as uint8 with numpy's wrapping cast (randaugment_video.py:343), [T][oh][ow][3].
 * mpv_video_aug_pointwise: op 0 = contrast_func (:120-130; the per-frame luminance mean needs sums_ws, 3 * T uint64), op 1 =
 * brightness_func (:133-139), in place.  mpv_video_aug_sharpness: sharpness_func (:142-160; cv2.filter2D restated), out of place.
 * mpv_video_aug_warp_affine: cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT) with the INVERTED 2 x 3 matrix (the host inverts as
 * opencv does) -- shear_x/y :163-167,:198-202, translate_x/y :170-187, rotate :67-75 -- out of place.  mpv_video_u8_normalize:
 * ClipToTensor + Normalize (dataset/__init__.py:68-69) into the [3][T][H][W] slot of the batch.  Bit-exact against
 * oracle/augment.py; what that restatement pins is stated in its header (opencv itself is not available to compare with). */
int mpv_video_resized_crop_u8(const uint8_t* clip, int T, int H, int W, int crop_i, int crop_j, int crop_h, int crop_w, int out_h,
                              int out_w, int mode, int flip, uint8_t* out, mpv_stream_t stream);
int mpv_video_aug_pointwise(uint8_t* frames, int T, int H, int W, int op, double factor, uint64_t* sums_ws, mpv_stream_t stream);
int mpv_video_aug_sharpness(const uint8_t* in, uint8_t* out, int T, int H, int W, double factor, mpv_stream_t stream);
int mpv_video_aug_warp_affine(const uint8_t* in, uint8_t* out, int T, int H, int W, const double* inverse_matrix6, const uint8_t* fill3,
                              mpv_stream_t stream);
int mpv_video_u8_normalize(const uint8_t* frames, int T, int H, int W, const float* mean3, const float* std3, void* out,
                           int64_t c_stride, int64_t t_stride, mpv_stream_t stream);
/* Soft-target contrastive cross-entropy over fp32 similarities sim[rows][cols] (:966-978):
 * targets[i][j] = [row_ids[i]==col_ids[j]] / count_i; losses[i] = -sum_j log_softmax(sim_i)[j] targets[i][j];
 * dsim (bf16, optional) = (softmax - targets) * scale; dts[i] (optional) = sum_j dsim[i][j] * sim[i][j]. */
int mpv_soft_target_ce(const float* sim, const int64_t* row_ids, const int64_t* col_ids, float scale, float* losses,
                       void* dsim, float* dts, int64_t rows, int64_t cols, mpv_stream_t stream);
/* Image-text contrastive head of the pre-train model (use_contrastive, models/distributed_gpt3.py:168-212): the similarity of a
 * clip and a title is the MAX over the clip's Q query features.
 * mpv_maxsim_fwd: A bf16 [R][Q][E], T bf16 [C][E] (both L2-normalised rows, E % 8 == 0, 16-byte aligned);
 *   sim fp32 = alpha * max_q <A[r][q], T[c]> (the max is taken before the scale; alpha = *alpha_dev, or 1 when NULL) and
 *   arg int32 = that q, ties to the lowest q (deterministic).  trans = 0: sim / arg are [R][C]; trans = 1: [C][R].
 *   i2t: A = v [B][Q][E], T = t_all [WB][E]; t2i: A = v_all [WB][Q][E], T = t [B][E], trans = 1 (sim_t2i [B][WB]).
 * mpv_maxsim_route: the max's backward as a dense operand: G bf16 [R*Q][C], G[r*Q + q][c] = dsim(r, c) * [arg(r, c) == q], with
 *   dsim bf16 and arg in mpv_maxsim_fwd's layout (trans as there); C % 8 == 0.  Every element written once, no atomics.
 *   dA = alpha G T and dT = alpha G^T A are then plain mpv_gemm_bf16 products.
 * mpv_smoothed_ce: F.cross_entropy(sim, target, label_smoothing=eps) per row over fp32 sim[rows][cols], int64 target[rows]:
 *   targets[i][j] = (1 - eps) [j == target[i]] + eps / cols; losses[i] = -sum_j log_softmax(sim_i)[j] targets[i][j];
 *   dsim (bf16, optional) = (softmax - targets) * scale; dts[i] (optional) = sum_j dsim[i][j] * sim[i][j] (the temp gradient,
 *   as in mpv_soft_target_ce). */
int mpv_maxsim_fwd(const void* A, const void* T, const float* alpha_dev, float* sim, int* arg, int64_t R, int64_t Q, int64_t C,
                   int64_t E, int trans, mpv_stream_t stream);
int mpv_maxsim_route(const void* dsim, const int* arg, void* G, int64_t R, int64_t Q, int64_t C, int trans, mpv_stream_t stream);
int mpv_smoothed_ce(const float* sim, const int64_t* target, float eps, float scale, float* losses, void* dsim, float* dts,
                    int64_t rows, int64_t cols, mpv_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Retrieval search (evaluation / serving of the ITC model: downstream/run_retrieval_distributed_gpt3.py:245-339 builds both full
 * score matrices and argsorts every row on the host; these calls return the k best rows, or the rank of the wanted rows,
 * without the matrix).  queries bf16 [nq][dim], gallery bf16 [ng][dim], row strides q_rs / g_rs in elements (multiples of 8,
 * base pointers 16-byte aligned); dim a multiple of 32 in [32, 1024]; nq <= 65535 * 32; ng <= 2^31 - 1.  Scores are
 * <q, g> in fp32 (bf16 MFMA, fp32 accumulation).
 * Order rule (both calls): row g comes before row h iff s(g) > s(h), or s(g) == s(h) and g < h -- a total order, so results do
 * not depend on `slices` (gallery slices per query tile, each a workgroup; 0 = choose so that a single query fills the chip).
 * NaN scores are ordered after everything and never returned.
 * mpv_sim_topk: vals fp32 [nq][k], idx int64 [nq][k], k in [1, 32]: the k first rows by the rule with s = scale * <q, g>
 *   (scale = 1.0f for the plain product), in that order; when ng < k the tail is (-inf, -1).
 * mpv_sim_rank: target int64 [nq][n_targets] (n_targets in [1, 32]; an entry outside [0, ng) is an unused slot); rank int32 [nq] =
 *   min over the query's targets t of #{g : g comes before t} (ng when the query has no target); scale is not applied.
 *   The target scores come from the code path that scores the stream, so s(g) > s(t) compares like with like.
 * Workspaces: *_workspace_size(d[, n_targets]) bytes (0 for a descriptor the call would refuse), 4-byte aligned. */
typedef struct mpv_sim_search_desc {
  const void *queries, *gallery;
  int64_t q_rs, g_rs;
  int64_t nq, ng;
  int dim, k, slices;
  float scale;
} mpv_sim_search_desc;
size_t mpv_sim_topk_workspace_size(const mpv_sim_search_desc* d);
int mpv_sim_topk(const mpv_sim_search_desc* d, float* vals, int64_t* idx, void* workspace, size_t workspace_bytes, mpv_stream_t stream);
size_t mpv_sim_rank_workspace_size(const mpv_sim_search_desc* d, int n_targets);
int mpv_sim_rank(const mpv_sim_search_desc* d, const int64_t* target, int n_targets, int32_t* rank, void* workspace,
                 size_t workspace_bytes, mpv_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Query-max retrieval search (zero-shot evaluation / serving of the pre-train model's contrastive head, use_contrastive,
 * models/distributed_gpt3.py:178-202): mpv_sim_topk / mpv_sim_rank over ITEMS that are groups of rows.  Neither the
 * [nq][ng][group] products nor an [nq][ng] matrix reach memory.
 * queries / gallery: bf16 rows, L2-normalised by the caller, base pointers 16-byte aligned, row strides q_rs / g_rs in elements
 *   (multiples of 8, at least dim).  nq / ng count ITEMS: item i of a side is its rows i * group .. i * group + group - 1.
 * Score: s(i, j) = max over the rows a of query item i and the rows b of gallery item j of <a, b> (bf16 MFMA, fp32 accumulation);
 *   the max is taken before any scale, as in mpv_maxsim_fwd.
 * Groups: q_group and g_group are in [1, 1024], no multiple of anything, and at most ONE of them exceeds 1 (title -> clip:
 *   g_group = Q; clip -> title: q_group = Q; both 1: mpv_sim_topk / mpv_sim_rank bit for bit).
 * dim: a multiple of 32 in [32, 1024].  k in [1, 32], n_targets in [1, 32]; nq * q_group and ng * g_group <= 2^31 - 1.
 * Order rule, ties, slices: those of mpv_sim_topk / mpv_sim_rank, over items, not rows: item g comes before item h iff
 *   s(g) > s(h), or s(g) == s(h) and g < h -- a total order; `slices` (0 = choose) only cuts the work and the outputs are
 *   bit-identical for every value of it.
 * NaN: a NaN product never wins a max over finite ones; an item whose score is NaN (all its products are) is never returned,
 *   beats nothing, and as a target counts as no target.
 * mpv_maxsim_topk: vals fp32 [nq][k], idx int64 [nq][k]: the k first items by the rule with s = scale * s(i, j), in that order;
 *   when ng < k the tail is (-inf, -1).  No atomics.
 * mpv_maxsim_rank: target int64 [nq][n_targets] (an entry outside [0, ng) is an unused slot); rank int32 [nq] = min over the
 *   query item's targets t of #{g : g comes before t}, ng when it has no valid target; scale is not applied.  The target scores
 *   come from the staging and MFMA path that scores the stream (a max over bit-identical products is bit-identical), so
 *   s(g) > s(t) compares like with like.  Counts are added with integer atomics (order-independent).
 * Refusals: a descriptor the call would refuse makes *_workspace_size return 0 and the call return a negative code before any
 *   launch; a workspace that is too small is MPV_E_ARG.  Workspaces are 4-byte aligned. */
typedef struct mpv_maxsim_search_desc {
  const void *queries, *gallery;
  int64_t q_rs, g_rs;
  int64_t nq, ng;
  int q_group, g_group;
  int dim, k, slices;
  float scale;
} mpv_maxsim_search_desc;
size_t mpv_maxsim_topk_workspace_size(const mpv_maxsim_search_desc* d);
int mpv_maxsim_topk(const mpv_maxsim_search_desc* d, float* vals, int64_t* idx, void* workspace, size_t workspace_bytes,
                    mpv_stream_t stream);
size_t mpv_maxsim_rank_workspace_size(const mpv_maxsim_search_desc* d, int n_targets);
int mpv_maxsim_rank(const mpv_maxsim_search_desc* d, const int64_t* target, int n_targets, int32_t* rank, void* workspace,
                    size_t workspace_bytes, mpv_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Searches over an FP8 gallery (opt-in; half the index bytes; csrc/search_common.h ScCodeStage).  The four searches above with
 * the GALLERY stored as e4m3 codes.  Numeric contract:
 *   format   OCP e4m3fn codes, one byte per element, and one fp32 scale per gallery ROW (g_scale: ng entries for mpv_sim_*_q8,
 *            ng * g_group for mpv_maxsim_*_q8, row order) -- what mpv_quantize_rows_e4m3 writes ("FP8 decoder weights" above).
 *   desc     the descriptors above, unchanged: d->gallery points to the codes, g_rs is counted in CODES, is a multiple of 16 and
 *            at least dim, and the base pointer is 16-byte aligned (a 16-byte chunk is 16 codes).  Queries stay bf16.
 *   score    s(row) = g_scale[row] * sum_k q[k] * deq(code[row][k]).  The sum is the bf16-MFMA / fp32 chain the bf16 entry runs on
 *            that row (the codes become bf16 on the way into the LDS stage, deq is exact; same chunk order, same instruction,
 *            accumulator zeroed at the same point); the product with the scale is taken in fp32 before any comparison and before
 *            any max over a group; for top-k d->scale is applied after that, as above.
 *   equality for scales that are powers of two every output -- values, indices, ranks, for every value of `slices` -- equals, bit
 *            for bit, the matching bf16 entry called on the bf16 gallery deq(code) * g_scale (a bf16 number: the FP8 index IS a
 *            bf16 index, kernel error and quantisation error are separate questions).  Domain: a multiplication by a power of
 *            two commutes with fp32 addition as long as no partial sum is subnormal (or overflows), so the claim holds where the
 *            partial sums of both chains stay normal or zero.  Rows of mpv_quantize_rows_e4m3 from unit-norm features have
 *            exponents around -11; their partial sums are nowhere near 2^-126.
 *   rules    order rule, tie rule, NaN rules and refusal style of the bf16 entries.  The codes 0x7F and 0xFF convert to NaN and
 *            behave as a NaN bf16 element does there.
 * Refused (negative code, *_q8_workspace_size 0, before any launch) beyond what the bf16 entries refuse: a null g_scale; a gallery
 * that is not 16-byte aligned or a g_rs that is not a multiple of 16; for mpv_maxsim_*_q8 a q_group above 1 -- in that direction
 * the gallery is the LDS-resident side and the index is titles, 512 bytes each at dim 256: out of scope, such indexes stay bf16.
 * What the rounding to e4m3 does to rankings of TRAINED features has not been measured (no checkpoint or data set exists here). */
size_t mpv_sim_topk_q8_workspace_size(const mpv_sim_search_desc* d, const float* g_scale);
int mpv_sim_topk_q8(const mpv_sim_search_desc* d, const float* g_scale, float* vals, int64_t* idx, void* workspace,
                    size_t workspace_bytes, mpv_stream_t stream);
size_t mpv_sim_rank_q8_workspace_size(const mpv_sim_search_desc* d, const float* g_scale, int n_targets);
int mpv_sim_rank_q8(const mpv_sim_search_desc* d, const float* g_scale, const int64_t* target, int n_targets, int32_t* rank,
                    void* workspace, size_t workspace_bytes, mpv_stream_t stream);
size_t mpv_maxsim_topk_q8_workspace_size(const mpv_maxsim_search_desc* d, const float* g_scale);
int mpv_maxsim_topk_q8(const mpv_maxsim_search_desc* d, const float* g_scale, float* vals, int64_t* idx, void* workspace,
                       size_t workspace_bytes, mpv_stream_t stream);
size_t mpv_maxsim_rank_q8_workspace_size(const mpv_maxsim_search_desc* d, const float* g_scale, int n_targets);
int mpv_maxsim_rank_q8(const mpv_maxsim_search_desc* d, const float* g_scale, const int64_t* target, int n_targets, int32_t* rank,
                       void* workspace, size_t workspace_bytes, mpv_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Searches with per-row priors (filtering, weighting, hubness correction; csrc/search_common.h ScPrior).  mpv_sim_topk / mpv_sim_rank
 * and their *_q8 forms with one fp32 additive term per GALLERY row: g_prior, ng entries, 4-byte aligned.  The descriptor is unchanged;
 * the q8 entries take g_scale, then g_prior.
 *   score    s'(q, g) = fl(fl(scale * s(q, g)) + g_prior[g]).  s(q, g) is exactly what the plain entry computes (for codes,
 *            fl(g_scale[g] * acc) first); the multiplication and the addition are two separately rounded fp32 operations, never a
 *            fused multiply-add, so a plain fp32 restatement reproduces s' bit for bit from the accumulator.
 *   rank     scale IS applied in mpv_sim_rank_prior*, unlike mpv_sim_rank: with an additive term the order depends on it.  The target
 *            scores go through the stream's own code path, the multiply and the add included.
 *   -inf     a row whose s' is NaN or -inf is not eligible: it is never returned, beats nothing, and as a target counts as no
 *            target.  A term of -inf is therefore a filter.  A row with s' = +inf is ordinary (first, by index).  A query with fewer
 *            than k eligible rows gets the (-inf, -1) tail.
 *   rules    order rule, tie rule, `slices` independence, workspace conventions and refusal style of the plain entries; the q8
 *            entries equal the bf16 ones on deq(code) * g_scale bit for bit under the conditions stated above.
 * Refused (negative code, *_workspace_size 0, before any launch) beyond what the plain entry refuses: a null or misaligned g_prior.
 *
 * mpv_sim_bank_lse: lse fp32 [ng], lse[g] = log sum_{b < nb} exp(beta * <bank_b, gallery_g>), the products being the bf16-MFMA /
 *   fp32 ones of the searches.  With g_prior = -lse and scale = beta the searches above return the inverted-softmax (QB-Norm; with
 *   the test queries as the bank, dual-softmax) scores beta * s(q, g) - lse[g].  bank bf16 [nb][dim], gallery bf16 [ng][dim] (or
 *   codes, for *_q8, with g_scale), row strides and alignment as in the search descriptors; nb, ng in [1, 2^31 - 1]; dim a
 *   multiple of 32 in [32, 1024]; beta finite (any size: the sum is kept against a running max, nothing overflows).
 *   lse[g] is a function of (bank, beta, gallery row g) alone, bit for bit: the same whether the row is scored alone or among
 *   others, at whatever position, for whatever ng, however often.  No atomics; the bank is not cut into slices.  A NaN product
 *   makes that row's lse NaN.  The q8 entry is bit for bit the bf16 entry on the rows bf16(deq(code) * g_scale).
 *   The workspace is not used (its size is a nominal 256 bytes, 0 for a descriptor the call would refuse); it may be null. */
size_t mpv_sim_topk_prior_workspace_size(const mpv_sim_search_desc* d, const float* g_prior);
int mpv_sim_topk_prior(const mpv_sim_search_desc* d, const float* g_prior, float* vals, int64_t* idx, void* workspace,
                       size_t workspace_bytes, mpv_stream_t stream);
size_t mpv_sim_rank_prior_workspace_size(const mpv_sim_search_desc* d, const float* g_prior, int n_targets);
int mpv_sim_rank_prior(const mpv_sim_search_desc* d, const float* g_prior, const int64_t* target, int n_targets, int32_t* rank,
                       void* workspace, size_t workspace_bytes, mpv_stream_t stream);
size_t mpv_sim_topk_prior_q8_workspace_size(const mpv_sim_search_desc* d, const float* g_scale, const float* g_prior);
int mpv_sim_topk_prior_q8(const mpv_sim_search_desc* d, const float* g_scale, const float* g_prior, float* vals, int64_t* idx,
                          void* workspace, size_t workspace_bytes, mpv_stream_t stream);
size_t mpv_sim_rank_prior_q8_workspace_size(const mpv_sim_search_desc* d, const float* g_scale, const float* g_prior, int n_targets);
int mpv_sim_rank_prior_q8(const mpv_sim_search_desc* d, const float* g_scale, const float* g_prior, const int64_t* target,
                          int n_targets, int32_t* rank, void* workspace, size_t workspace_bytes, mpv_stream_t stream);
typedef struct mpv_sim_bank_desc {
  const void *bank, *gallery;
  int64_t b_rs, g_rs;
  int64_t nb, ng;
  int dim;
  float beta;
} mpv_sim_bank_desc;
size_t mpv_sim_bank_lse_workspace_size(const mpv_sim_bank_desc* d);
int mpv_sim_bank_lse(const mpv_sim_bank_desc* d, float* lse, void* workspace, size_t workspace_bytes, mpv_stream_t stream);
size_t mpv_sim_bank_lse_q8_workspace_size(const mpv_sim_bank_desc* d, const float* g_scale);
int mpv_sim_bank_lse_q8(const mpv_sim_bank_desc* d, const float* g_scale, float* lse, void* workspace, size_t workspace_bytes,
                        mpv_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer (DeepSpeed FusedAdam + global-norm clip, run_pretrain_distributed_gpt3.py:137;
 * math of optim/adamw.py:66-115; torch.nn.utils.clip_grad_norm_ semantics, utils.py:308).
 * sumsq (fp32 scalar, pre-zeroed) += sum g^2 over n bf16 gradients -- BIT-REPRODUCIBLE since round 6: per-workgroup partial sums in
 * `workspace` (mpv_grad_sumsq_workspace_size() bytes), added up in a fixed order by a second launch (the clip coefficient, hence every
 * update of a clipped step, hangs on the last bits of this scalar; an atomicAdd per workgroup made them depend on arrival order). */
size_t mpv_grad_sumsq_workspace_size(void);
int mpv_grad_sumsq(const void* grad, int64_t n, float* sumsq, void* workspace, size_t workspace_bytes, mpv_stream_t stream);
/* One AdamW step over a flat range: master/m/v fp32, grad bf16, param bf16 written back.
 * clip coefficient = min(1, max_norm / (sqrt(*sumsq) * inv_world ... ) computed in-kernel from
 * the device scalar; grad_scale multiplies g first (1/world for averaged all-reduce sums). */
int mpv_adamw_step(void* param_bf16, float* master, float* exp_avg, float* exp_avg_sq, const void* grad_bf16,
                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   float grad_scale, const float* sumsq, float max_norm, mpv_stream_t stream);

/* Grouped AdamW over a flat buffer laid out in backward-completion order (so data-parallel
 * gradient buckets are contiguous slices): tile_group[i] (device, uint8) is the parameter-group
 * id (0..ngroups-1; >= 8 = skip) of the i-th 256-element tile; lrs/wds are HOST arrays of the
 * per-group learning rate (lr_schedule * lr_scale, run_pretrain_distributed_gpt3.py:88-96) and
 * weight decay (optim/optim_factory.py:219-265). */
int mpv_adamw_step_grouped(void* param_bf16, float* master, float* exp_avg, float* exp_avg_sq, const void* grad_bf16,
                           int64_t n, const uint8_t* tile_group, const float* lrs, const float* wds, int ngroups,
                           float beta1, float beta2, float eps, int step, float grad_scale, const float* sumsq,
                           float max_norm, mpv_stream_t stream);

/* The same step with every STEP-DEPENDENT hyper-parameter read from device memory at kernel run time: hyper_dev[18] =
 * { lr[8], weight_decay[8], 1 / (1 - beta1^step), 1 / sqrt(1 - beta2^step) }, as written by mpv_adamw_hyper_pack (host; the
 * bias corrections are computed exactly as mpv_adamw_step_grouped computes them, so both entry points update bit-identically).
 * Kernel arguments are frozen when a training step is captured into a HIP graph; with this entry point a replay applies the
 * learning rate of ITS step (the host rewrites the 72 bytes before each replay). */
int mpv_adamw_hyper_pack(const float* lrs, const float* wds, int ngroups, float beta1, float beta2, int step, float* out18);
int mpv_adamw_step_grouped_dev(void* param_bf16, float* master, float* exp_avg, float* exp_avg_sq, const void* grad_bf16,
                               int64_t n, const uint8_t* tile_group, const float* hyper_dev, float beta1, float beta2, float eps,
                               float grad_scale, const float* sumsq, float max_norm, mpv_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * LoRA: the low-rank products of an adapter W + s B A on a frozen nn.Linear (lora_A [r, in], lora_B [out, r]); DESIGN.md section 36.
 * The reference has no adapters: this is the middle setting between its freeze_text_decoder: true and false
 * (models/distributed_gpt3.py:91-93).  bf16 operands, fp32 accumulation on the matrix cores, ONE bf16 rounding per output element.
 * r is 8, 16, 32 or 64 (r = 8 is padded in registers, never in memory); C and N are multiples of 8; R >= 1 is any row count.
 * Every leading dimension is given (multiples of 8, pointers 16-byte aligned): qkv and its slices are pitched.
 * w(c, j) = w[j * ldw + c] when w_rank_major ([r, in]: lora_A), w[c * ldw + j] otherwise ([out, r]: lora_B); g likewise.
 * All scalars by value, no host synchronisation, no allocation: the launches are capturable.
 *
 * mpv_lora_down:   t[i, j] = bf16(scale * sum_c x[i, c] w(c, j)), i < R, j < r.  Streams x once.
 * mpv_lora_up_add: y[i, n] = bf16(fp32(y[i, n]) + scale * sum_j t[i, j] w(n, j)) in place, i < R, n < N; one read and one write
 *                  of y, rows >= R and columns >= N are never touched.
 * In both, the bits of row i do not depend on R (the reduction order of a row is a function of C / r alone).
 * mpv_lora_wgrad:  g(c, j) = bf16(scale * sum_i t[i, j] x[i, c]), written [r, C] (g_rank_major) or [C, r].  Row slices are reduced
 *                  through fp32 partials in the workspace (mpv_lora_wgrad_workspace_size bytes) in a fixed order, without
 *                  floating-point atomics: two calls give the same bits. */
int mpv_lora_down(const void* x, int64_t ldx, const void* w, int64_t ldw, int w_rank_major, void* t, int64_t ldt, int64_t R, int64_t C,
                  int r, float scale, mpv_stream_t stream);
int mpv_lora_up_add(const void* t, int64_t ldt, const void* w, int64_t ldw, int w_rank_major, void* y, int64_t ldy, int64_t R, int64_t N,
                    int r, float scale, mpv_stream_t stream);
size_t mpv_lora_wgrad_workspace_size(int64_t R, int64_t C, int r);
int mpv_lora_wgrad(const void* t, int64_t ldt, const void* x, int64_t ldx, void* g, int64_t ldg, int g_rank_major, int64_t R, int64_t C,
                   int r, float scale, void* workspace, size_t workspace_bytes, mpv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPV_H_ */
