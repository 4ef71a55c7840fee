// decode.hip -- host-side driver of one incremental decoder forward (prefill or a single-token decode step) over the
// per-layer KV caches: every launch of the step is issued from here, so generation costs one FFI call per step instead
// of ~170 (the step is launch-bound otherwise: ~5 rows of work per kernel).  Pure orchestration of the C-ABI kernels.
// Reference: models/modeling_distributed_gpt3.py:640-666 (embedding), :868-938 + :1034-1078 (layer with
// InferenceParams KV memory), :1184 (final LN), :1348-1350 (tied LM head).
#include <math.h>

#include "../../include/mpv.h"
#include "mpv_common.h"

// The two index vectors the ragged entries form on the device (nothing is read back):
//   positions  pos[s] = clamp(group_prefix_len[s / fan], 1, max_prefix_len) + t      the position row of sequence s' new token
//   last rows  idx[b] = b * n + clamp(last_row[b], 0, n - 1)                         the row of sequence b the LM head runs on
__global__ void ragged_positions_kernel(const int32_t* __restrict__ glen, int32_t* __restrict__ pos, int n_seq, int fan, int max_plen, int t) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n_seq) pos[s] = min(max(glen[s / fan], 1), max_plen) + t;
}
__global__ void ragged_last_rows_kernel(const int64_t* __restrict__ last_row, int64_t* __restrict__ idx, int batch, int n) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < batch) idx[b] = (int64_t)b * n + min(max(last_row[b], (int64_t)0), (int64_t)(n - 1));
}

// The steps entries (every group at its own suffix position group_t[g]; a group outside [0, max_t] is idle) form two vectors:
//   positions  pos[s] = clamp(group_prefix_len[g], 1, max_prefix_len) + (live ? group_t[g] : 0)      g = s / fan; idle: a valid row
//   own rows   own[g] = live ? group_t[g] + 1 : 0                                                     the attention's group_own_len
// and place the dense qkv rows of a layer: row s goes to suffix row s * suffix_max + own[g] - 1, an idle group's rows nowhere.
__global__ void steps_index_kernel(const int32_t* __restrict__ glen, const int32_t* __restrict__ group_t, int32_t* __restrict__ pos,
                                   int32_t* __restrict__ own, int n_seq, int fan, int max_plen, int max_t) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  const int g = s / fan, t = group_t[g];
  const bool live = t >= 0 && t <= max_t;
  pos[s] = min(max(glen[g], 1), max_plen) + (live ? t : 0);
  if (s == g * fan) own[g] = live ? t + 1 : 0;
}
__global__ void steps_scatter_kernel(const uint4* __restrict__ qkv, const int32_t* __restrict__ own, uint4* __restrict__ suffix, long long n_seq,
                                     int fan, long long suffix_max, int vecs) {      // vecs: 16-byte pieces of a 3H row
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_seq * vecs; i += (long long)gridDim.x * blockDim.x) {
    const long long s = i / vecs;
    const int o = own[s / fan];                                                      // 0 .. max_t + 1 <= suffix_max (steps_index_kernel)
    if (o > 0) suffix[(s * suffix_max + (o - 1)) * vecs + (i - s * vecs)] = qkv[i];
  }
}

// The beam re-order of the steps entries' suffix cache, all layers in one launch: sequence j of clip g = j / fan continues from the
// first r = clamp(group_rows[g], 0, max_rows) suffix rows of sequence idx[j]; rows at or behind r, and all rows of a clip with r = 0,
// are not written.  An idx[j] outside [0, n_seq) moves nothing (the advance never produces one).
__global__ void steps_reorder_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const int64_t* __restrict__ idx,
                                     const int32_t* __restrict__ group_rows, long long n_seq, int fan, long long suffix_max, int max_rows,
                                     int vecs) {                                        // vecs: 16-byte pieces of a 3H row
  const long long j = blockIdx.x, l = blockIdx.y, from = idx[j];                        // one workgroup per (sequence, layer)
  const int r = min(max(group_rows[j / fan], 0), max_rows);                            // max_rows <= suffix_max (the entry's check)
  if (r == 0 || from < 0 || from >= n_seq) return;
  const uint4* s = src + (l * n_seq + from) * suffix_max * vecs;
  uint4* d = dst + (l * n_seq + j) * suffix_max * vecs;
  for (int i = threadIdx.x; i < r * vecs; i += blockDim.x) d[i] = s[i];
}

extern "C" int mpv_kv_suffix_reorder_steps(const void* src, void* dst, int layers, int n_groups, int fan, int suffix_max, const int64_t* idx,
                                           const int32_t* group_rows, int max_rows, int hidden, hipStream_t stream) {
  const char* who = "mpv_kv_suffix_reorder_steps";
  MPV_REQUIRE(src && dst && idx && group_rows, MPV_E_ARG, "%s: null pointer", who);
  MPV_REQUIRE(src != dst, MPV_E_ARG, "%s: src and dst must be different caches", who);
  MPV_REQUIRE(layers >= 1 && n_groups >= 1 && fan >= 1 && suffix_max >= 1 && hidden >= 8 && hidden % 8 == 0, MPV_E_SHAPE,
              "%s: bad shape layers=%d n_groups=%d fan=%d suffix_max=%d hidden=%d (hidden %% 8 == 0)", who, layers, n_groups, fan, suffix_max, hidden);
  MPV_REQUIRE(max_rows >= 0 && max_rows <= suffix_max, MPV_E_SHAPE, "%s: max_rows (%d) must be in [0, suffix_max = %d]", who, max_rows, suffix_max);
  MPV_REQUIRE((uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0, MPV_E_ARG, "%s: the caches must be 16-byte aligned", who);
  if (max_rows == 0) return MPV_OK;
  const int vecs = 3 * hidden / 8;
  const long long n_seq = (long long)n_groups * fan;
  MPV_REQUIRE(layers <= 65535 && n_seq <= 0x7fffffffLL && (long long)max_rows * vecs <= 0x7fffffffLL, MPV_E_SHAPE,
              "%s: layers=%d, %lld sequences or %d rows of %d hidden exceed the launch", who, layers, n_seq, max_rows, hidden);
  hipLaunchKernelGGL(steps_reorder_kernel, dim3((unsigned)n_seq, (unsigned)layers), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, idx,
                     group_rows, n_seq, fan, (long long)suffix_max, max_rows, vecs);
  return mpv_check_launch(who);
}

static inline char* carve(char*& p, size_t bytes) {
  char* r = p;
  p += (bytes + 255) / 256 * 256;
  return r;
}

extern "C" size_t mpv_gpt_decode_workspace_size(const mpv_gpt_weights* w, int batch, int n_new) {
  const size_t R = (size_t)batch * n_new;
  return 4 * (R * w->hidden * 2 + 256) + (R * w->ffn * 2 + 256) + 2 * ((size_t)batch * w->hidden * 2 + 256) +
         mpv_gemm_workspace_size(R, w->ffn, w->hidden, 0, 0);
}

// One weight product of a step, C[M, N] = epi(A[M, K] W[N, K]^T) with dense operands: on the bf16 weight, or -- in the _q8 entries
// (codes != nullptr) for at most MPV_W8_TILED_MAX_ROWS rows -- on its e4m3 codes (include/mpv.h, "FP8 decoder weights").
struct Products {
  void* gws;
  size_t gws_bytes;
  hipStream_t stream;
  int operator()(const void* A, const void* w_bf16, const void* codes, const void* scale, void* C, int64_t M, int64_t N, int64_t K,
                 const mpv_gemm_epilogue* ep) const {
    if (codes && M <= MPV_W8_MAX_ROWS) return mpv_gemm_w8(A, codes, (const float*)scale, C, M, N, K, K, K, N, ep, stream);
    if (codes && M <= MPV_W8_TILED_MAX_ROWS)
      return mpv_gemm_w8_tiled(A, codes, (const float*)scale, C, M, N, K, K, K, N, ep, gws, gws_bytes, stream);
    return mpv_gemm_bf16(A, w_bf16, C, M, N, K, K, K, N, 0, 0, ep, gws, gws_bytes, stream);
  }
};
static const mpv_gpt_layer_weights_q8 NO_Q8_LAYER = {};

// what follows the attention in a layer: dense + residual, LN2, fc1 + GELU, fc2 + residual (the layer output lands in h)
static int layer_tail(const mpv_gpt_weights* w, const mpv_gpt_layer_weights* lw, const mpv_gpt_layer_weights_q8* lq, int64_t R, void* h,
                      void* x, void* ctx, void* h1, void* g, const Products& product) {
  const int H = w->hidden, F4 = w->ffn;
  hipStream_t stream = product.stream;
  mpv_gemm_epilogue e1 = {};
  e1.bias = lw->dense_b; e1.residual = h; e1.ldr = H;
  int rc = product(ctx, lw->dense_w, lq->dense_q, lq->dense_s, h1, R, H, H, &e1);
  if (rc) return rc;
  rc = mpv_layernorm_fwd(h1, lw->ln2_w, lw->ln2_b, x, nullptr, nullptr, R, H, H, H, w->ln_eps, 0, 0, 0, 0, 0, 0, stream);
  if (rc) return rc;
  mpv_gemm_epilogue e2 = {};
  e2.bias = lw->fc1_b; e2.act = MPV_ACT_GELU_TANH;
  rc = product(x, lw->fc1_w, lq->fc1_q, lq->fc1_s, g, R, F4, H, &e2);
  if (rc) return rc;
  mpv_gemm_epilogue e3 = {};
  e3.bias = lw->fc2_b; e3.residual = h1; e3.ldr = H;
  // the layer input `h` was last read by the dense GEMM (as its residual): its buffer takes the layer output
  return product(g, lw->fc2_w, lq->fc2_q, lq->fc2_s, h, R, H, F4, &e3);
}

// final LN + tied LM head on one row per sequence
static int lm_head(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, const void* lastrow, void* xf, int batch, void* logits,
                   const Products& product) {
  const int H = w->hidden;
  const int rc = mpv_layernorm_fwd(lastrow, w->lnf_w, w->lnf_b, xf, nullptr, nullptr, batch, H, H, H, w->ln_eps, 0, 0, 0, 0, 0, 0,
                                   product.stream);
  if (rc) return rc;
  return product(xf, w->wte, q8 ? q8->wte_q : nullptr, q8 ? q8->wte_s : nullptr, logits, batch, w->vocab, H, nullptr);
}

// the token / query rows of a step plus their position rows: from the bf16 embedding, or from the tied embedding's codes
static int embed(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, const void* query, const int64_t* tokens, int pos0, void* h,
                 int batch, int Q, int L, hipStream_t stream) {
  const void* wpe = (const char*)w->wpe + (size_t)pos0 * w->hidden * 2;
  if (q8) return mpv_gpt_embed_w8_fwd(query, tokens, q8->wte_q, (const float*)q8->wte_s, wpe, h, batch, Q, L, w->hidden, stream);
  return mpv_gpt_embed_fwd(query, tokens, w->wte, wpe, h, batch, Q, L, w->hidden, 0.f, 0, 0, stream);
}

static int check_q8(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, const char* who) {
  MPV_REQUIRE(w && q8, MPV_E_ARG, "%s: null pointer", who);
  MPV_REQUIRE(q8->layers == w->layers && q8->layer && q8->wte_q && q8->wte_s, MPV_E_ARG, "%s: the FP8 table has %d layers, the decoder %d",
              who, q8->layers, w->layers);
  for (int li = 0; li < w->layers; ++li) {
    const mpv_gpt_layer_weights_q8* l = &q8->layer[li];
    MPV_REQUIRE(l->qkv_q && l->qkv_s && l->dense_q && l->dense_s && l->fc1_q && l->fc1_s && l->fc2_q && l->fc2_s, MPV_E_ARG,
                "%s: null codes or scales in layer %d", who, li);
  }
  return MPV_OK;
}

// the body of mpv_gpt_decode_step, mpv_gpt_decode_step_q8 (q8 == nullptr: the bf16 step) and of the ragged prefills (last_row !=
// nullptr: the LM head runs on row last_row[b] of sequence b's n new rows instead of on row n - 1)
static int decode_step(const char* who,
                       const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* kv_cache, int batch, int max_len, int pos0,
                       const void* query, int Q, const int64_t* tokens, int L, void* workspace, size_t workspace_bytes, void* logits,
                       hipStream_t stream, const int64_t* last_row = nullptr) {
  MPV_REQUIRE(w && kv_cache && workspace && logits, MPV_E_ARG, "%s: null pointer", who);
  const int n = Q + L, H = w->hidden, np = w->heads, hn = H / np, F4 = w->ffn;
  MPV_REQUIRE(batch > 0 && n > 0 && pos0 >= 0 && pos0 + n <= max_len, MPV_E_SHAPE,
              "%s: positions [%d, %d) do not fit max_len %d", who, pos0, pos0 + n, max_len);
  MPV_REQUIRE(w->max_positions <= 0 || pos0 + n <= w->max_positions, MPV_E_SHAPE,
              "%s: positions [%d, %d) run past the %d rows of the position embedding", who, pos0, pos0 + n, w->max_positions);
  MPV_REQUIRE(workspace_bytes >= mpv_gpt_decode_workspace_size(w, batch, n), MPV_E_ARG, "%s: workspace too small", who);
  const int64_t R = (int64_t)batch * n;
  char* p = (char*)workspace;
  void* h = carve(p, R * H * 2);
  void* x = carve(p, R * H * 2);
  void* ctx = carve(p, R * H * 2);
  void* h1 = carve(p, R * H * 2);
  void* g = carve(p, R * F4 * 2);
  void* last = carve(p, (size_t)batch * H * 2);
  void* xf = carve(p, (size_t)batch * H * 2);
  const Products product = {p, workspace_bytes - (size_t)(p - (char*)workspace), stream};
  int rc = embed(w, q8, query, tokens, pos0, h, batch, Q, L, stream);
  if (rc) return rc;
  for (int li = 0; li < w->layers; ++li) {
    const mpv_gpt_layer_weights* lw = &w->layer[li];
    const mpv_gpt_layer_weights_q8* lq = q8 ? &q8->layer[li] : &NO_Q8_LAYER;
    char* c = (char*)kv_cache[li];
    rc = mpv_layernorm_fwd(h, lw->ln1_w, lw->ln1_b, x, nullptr, nullptr, R, H, H, H, w->ln_eps, 0, 0, 0, 0, 0, 0, stream);
    if (rc) return rc;
    mpv_gemm_epilogue ep = {};
    ep.bias = lw->qkv_b;
    ep.c_group = n; ep.c_stride = max_len; ep.c_offset = pos0;                 // the new rows land in the cache
    rc = product(x, lw->qkv_w, lq->qkv_q, lq->qkv_s, c, R, 3 * H, H, &ep);
    if (rc) return rc;
    mpv_attn_desc d = {};
    d.q = c + (size_t)pos0 * 3 * H * 2;
    d.k = c + (size_t)hn * 2;
    d.v = c + (size_t)2 * hn * 2;
    d.o = ctx;
    d.q_bs = d.k_bs = d.v_bs = (int64_t)max_len * 3 * H;
    d.q_hs = d.k_hs = d.v_hs = 3 * hn;
    d.q_rs = d.k_rs = d.v_rs = 3 * H;
    d.o_bs = (int64_t)n * H; d.o_hs = hn; d.o_rs = H;
    d.batch = batch; d.heads = np; d.sq = n; d.sk = pos0 + n; d.head_dim = hn;
    d.causal = 1;
    d.scale = 1.0f / sqrtf((float)hn);
    rc = mpv_attn_fwd(&d, stream);
    if (rc) return rc;
    rc = layer_tail(w, lw, lq, R, h, x, ctx, h1, g, product);
    if (rc) return rc;
  }
  const void* lastrow = h;
  if (last_row) {   // LM head on the caller's row of every sequence; x is free behind the last layer and takes the row indices
    hipLaunchKernelGGL(ragged_last_rows_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, stream, last_row, (int64_t*)x, batch, n);
    rc = mpv_check_launch(who);
    if (rc) return rc;
    rc = mpv_gather_rows(h, (const int64_t*)x, last, batch, H, H, stream);
    if (rc) return rc;
    lastrow = last;
  } else if (n > 1) {   // LM head on the last position of every sequence only
    rc = mpv_copy_rows(h, last, batch, H, H, H, 1, n, n - 1, 0, 0, 0, stream);
    if (rc) return rc;
    lastrow = last;
  }
  return lm_head(w, q8, lastrow, xf, batch, logits, product);
}

extern "C" int mpv_gpt_decode_step(const mpv_gpt_weights* w, void* const* kv_cache, int batch, int max_len, int pos0,
                                   const void* query, int Q, const int64_t* tokens, int L, void* workspace,
                                   size_t workspace_bytes, void* logits, hipStream_t stream) {
  return decode_step("mpv_gpt_decode_step",
                     w, nullptr, kv_cache, batch, max_len, pos0, query, Q, tokens, L, workspace, workspace_bytes, logits, stream);
}

extern "C" int mpv_gpt_decode_step_q8(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* kv_cache, int batch,
                                      int max_len, int pos0, const void* query, int Q, const int64_t* tokens, int L, void* workspace,
                                      size_t workspace_bytes, void* logits, hipStream_t stream) {
  const int rc = check_q8(w, q8, "mpv_gpt_decode_step_q8");
  if (rc) return rc;
  return decode_step("mpv_gpt_decode_step_q8",
                     w, q8, kv_cache, batch, max_len, pos0, query, Q, tokens, L, workspace, workspace_bytes, logits, stream);
}

// the prefill of prompts of different lengths (include/mpv.h states the contract)
extern "C" int mpv_gpt_prefill_ragged(const mpv_gpt_weights* w, void* const* kv_cache, int batch, int max_len, const void* query, int Q,
                                      const int64_t* tokens, int L, const int64_t* last_row, void* workspace, size_t workspace_bytes,
                                      void* logits, hipStream_t stream) {
  MPV_REQUIRE(last_row, MPV_E_ARG, "mpv_gpt_prefill_ragged: null last_row");
  return decode_step("mpv_gpt_prefill_ragged",
                     w, nullptr, kv_cache, batch, max_len, 0, query, Q, tokens, L, workspace, workspace_bytes, logits, stream, last_row);
}

extern "C" int mpv_gpt_prefill_ragged_q8(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* kv_cache, int batch,
                                         int max_len, const void* query, int Q, const int64_t* tokens, int L, const int64_t* last_row,
                                         void* workspace, size_t workspace_bytes, void* logits, hipStream_t stream) {
  MPV_REQUIRE(last_row, MPV_E_ARG, "mpv_gpt_prefill_ragged_q8: null last_row");
  const int rc = check_q8(w, q8, "mpv_gpt_prefill_ragged_q8");
  if (rc) return rc;
  return decode_step("mpv_gpt_prefill_ragged_q8",
                     w, q8, kv_cache, batch, max_len, 0, query, Q, tokens, L, workspace, workspace_bytes, logits, stream, last_row);
}

// mpv_gpt_decode_step for one token per sequence against a per-group shared prefix cache (include/mpv.h states the contract)
extern "C" size_t mpv_gpt_decode_shared_workspace_size(const mpv_gpt_weights* w, int n_seq) {
  return mpv_gpt_decode_workspace_size(w, n_seq, 1);
}
// ... of the steps entries: the dense qkv rows of a layer on top
extern "C" size_t mpv_gpt_decode_shared_steps_workspace_size(const mpv_gpt_weights* w, int n_seq) {
  return mpv_gpt_decode_workspace_size(w, n_seq, 1) + ((size_t)n_seq * 3 * w->hidden * 2 + 256);
}

// the body of mpv_gpt_decode_step_shared, mpv_gpt_decode_step_shared_q8 (q8 == nullptr: the bf16 step) and of the two ragged steps
// (ragged: group g's prefix is glen[g] <= prefix_len rows long inside its prefix_stride rows; otherwise prefix_stride == prefix_len)
// and of the two steps entries (group_t != nullptr, on top of ragged: group g sits at suffix position group_t[g]; `t` is then the
// host bound max_t.  The qkv product writes dense rows -- through the identity row map, so that it is the ragged step's product
// in everything but its addresses -- which steps_scatter_kernel places in the suffix cache; q is read from the dense rows)
static int decode_step_shared(const char* who,
                              const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* prefix_cache, void* const* suffix_cache,
                              int n_groups, int fan, int prefix_len, int suffix_max, int t, const int64_t* tokens, void* workspace,
                              size_t workspace_bytes, void* logits, hipStream_t stream, bool ragged = false, const int32_t* glen = nullptr,
                              int prefix_stride = 0, bool steps = false, const int32_t* group_t = nullptr) {
  if (!ragged) prefix_stride = prefix_len;
  MPV_REQUIRE(!ragged || glen, MPV_E_ARG, "%s: null group_prefix_len", who);
  MPV_REQUIRE(!steps || group_t, MPV_E_ARG, "%s: null group_t", who);
  MPV_REQUIRE(prefix_stride >= prefix_len, MPV_E_SHAPE, "%s: max_prefix_len %d exceeds the prefix_stride %d", who,
              prefix_len, prefix_stride);
  MPV_REQUIRE(w && prefix_cache && suffix_cache && tokens && workspace && logits, MPV_E_ARG, "%s: null pointer", who);
  MPV_REQUIRE(n_groups > 0 && fan > 0 && (int64_t)n_groups * fan < (1ll << 31) && prefix_len > 0, MPV_E_SHAPE,
              "%s: empty problem (n_groups %d, fan %d, prefix_len %d)", who, n_groups, fan, prefix_len);
  MPV_REQUIRE(t >= 0 && t < suffix_max && t < 2048, MPV_E_SHAPE,
              "%s: suffix position %d does not fit suffix_max %d (and the attention's 2048 own rows)", who, t, suffix_max);
  MPV_REQUIRE(w->max_positions <= 0 || prefix_len + t < w->max_positions, MPV_E_SHAPE,
              "%s: position %d runs past the %d rows of the position embedding", who, prefix_len + t, w->max_positions);
  const int n_seq = n_groups * fan, H = w->hidden, np = w->heads, hn = H / np, F4 = w->ffn;
  MPV_REQUIRE(workspace_bytes >= (steps ? mpv_gpt_decode_shared_steps_workspace_size(w, n_seq) : mpv_gpt_decode_shared_workspace_size(w, n_seq)),
              MPV_E_ARG, "%s: workspace too small", who);
  MPV_REQUIRE(!steps || H % 8 == 0, MPV_E_SHAPE, "%s: hidden %d must be a multiple of 8", who, H);
  const int64_t R = n_seq;
  char* p = (char*)workspace;
  void* h = carve(p, R * H * 2);
  void* x = carve(p, R * H * 2);
  void* ctx = carve(p, R * H * 2);
  void* h1 = carve(p, R * H * 2);
  void* g = carve(p, R * F4 * 2);
  void* pos = carve(p, (size_t)n_seq * H * 2);           // (the `last` rows of the general step: one position needs no copy; the
                                                         // ragged step keeps its n_seq int32 positions there)
  void* xf = carve(p, (size_t)n_seq * H * 2);
  char* qkv = steps ? carve(p, (size_t)n_seq * 3 * H * 2) : nullptr;                  // the steps entries' dense qkv rows
  int32_t* own = (int32_t*)pos + n_seq;                                             // ... and their n_groups own lengths, behind the positions
  const Products product = {p, workspace_bytes - (size_t)(p - (char*)workspace), stream};
  int rc;
  if (ragged) {
    if (steps)
      hipLaunchKernelGGL(steps_index_kernel, dim3((unsigned)((n_seq + 255) / 256)), dim3(256), 0, stream, glen, group_t, (int32_t*)pos, own, n_seq,
                         fan, prefix_len, t);
    else
      hipLaunchKernelGGL(ragged_positions_kernel, dim3((unsigned)((n_seq + 255) / 256)), dim3(256), 0, stream, glen, (int32_t*)pos, n_seq, fan,
                         prefix_len, t);
    rc = mpv_check_launch(who);
    if (rc) return rc;
    const int rows_wpe = w->max_positions > 0 ? w->max_positions : prefix_len + t + 1;
    rc = q8 ? mpv_gpt_embed_rows_w8_fwd(tokens, (const int32_t*)pos, q8->wte_q, (const float*)q8->wte_s, w->wpe, h, n_seq, H, rows_wpe, stream)
            : mpv_gpt_embed_rows_fwd(tokens, (const int32_t*)pos, w->wte, w->wpe, h, n_seq, H, rows_wpe, stream);
  } else {
    rc = embed(w, q8, nullptr, tokens, prefix_len + t, h, n_seq, 0, 1, stream);
  }
  if (rc) return rc;
  for (int li = 0; li < w->layers; ++li) {
    const mpv_gpt_layer_weights* lw = &w->layer[li];
    const mpv_gpt_layer_weights_q8* lq = q8 ? &q8->layer[li] : &NO_Q8_LAYER;
    char* pc = (char*)prefix_cache[li];
    char* sc = (char*)suffix_cache[li];
    rc = mpv_layernorm_fwd(h, lw->ln1_w, lw->ln1_b, x, nullptr, nullptr, R, H, H, H, w->ln_eps, 0, 0, 0, 0, 0, 0, stream);
    if (rc) return rc;
    mpv_gemm_epilogue ep = {};
    ep.bias = lw->qkv_b;
    ep.c_group = 1; ep.c_stride = suffix_max; ep.c_offset = t;                // row s lands at suffix row s*suffix_max + t
    if (steps) ep.c_stride = 1, ep.c_offset = 0;                              // ... at dense row s: the identity, through the same row map
    rc = product(x, lw->qkv_w, lq->qkv_q, lq->qkv_s, steps ? qkv : sc, R, 3 * H, H, &ep);
    if (rc) return rc;
    if (steps) {
      const int vecs = 3 * H / 8;
      const long long blocks = ((long long)n_seq * vecs + 255) / 256;
      hipLaunchKernelGGL(steps_scatter_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, (const uint4*)qkv, own,
                         (uint4*)sc, (long long)n_seq, fan, (long long)suffix_max, vecs);
      rc = mpv_check_launch(who);
      if (rc) return rc;
    }
    mpv_attn_decode_shared_desc d = {};
    d.q = steps ? qkv : sc + (size_t)t * 3 * H * 2;
    d.k = sc + (size_t)hn * 2;
    d.v = sc + (size_t)2 * hn * 2;
    d.pk = pc + (size_t)hn * 2;
    d.pv = pc + (size_t)2 * hn * 2;
    d.o = ctx;
    d.q_ss = d.k_ss = d.v_ss = (int64_t)suffix_max * 3 * H;
    if (steps) d.q_ss = 3 * H;
    d.pk_gs = d.pv_gs = (int64_t)prefix_stride * 3 * H;
    d.q_hs = d.k_hs = d.v_hs = d.pk_hs = d.pv_hs = 3 * hn;
    d.k_rs = d.v_rs = d.pk_rs = d.pv_rs = 3 * H;
    d.o_ss = H; d.o_hs = hn;
    d.n_seq = n_seq; d.group_size = fan; d.n_groups = n_groups; d.heads = np;
    d.prefix_len = prefix_len; d.own_len = t + 1; d.head_dim = hn;
    d.scale = 1.0f / sqrtf((float)hn);
    rc = steps    ? mpv_attn_decode_shared_steps_fwd(&d, glen, own, stream)
         : ragged ? mpv_attn_decode_shared_ragged_fwd(&d, glen, stream)
                  : mpv_attn_decode_shared_fwd(&d, stream);
    if (rc) return rc;
    rc = layer_tail(w, lw, lq, R, h, x, ctx, h1, g, product);
    if (rc) return rc;
  }
  return lm_head(w, q8, h, xf, n_seq, logits, product);
}

extern "C" int mpv_gpt_decode_step_shared(const mpv_gpt_weights* w, void* const* prefix_cache, void* const* suffix_cache, int n_groups,
                                          int fan, int prefix_len, int suffix_max, int t, const int64_t* tokens, void* workspace,
                                          size_t workspace_bytes, void* logits, hipStream_t stream) {
  return decode_step_shared("mpv_gpt_decode_step_shared",
                            w, nullptr, prefix_cache, suffix_cache, n_groups, fan, prefix_len, suffix_max, t, tokens, workspace,
                            workspace_bytes, logits, stream);
}

extern "C" int mpv_gpt_decode_step_shared_q8(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* prefix_cache,
                                             void* const* suffix_cache, int n_groups, int fan, int prefix_len, int suffix_max, int t,
                                             const int64_t* tokens, void* workspace, size_t workspace_bytes, void* logits,
                                             hipStream_t stream) {
  const int rc = check_q8(w, q8, "mpv_gpt_decode_step_shared_q8");
  if (rc) return rc;
  return decode_step_shared("mpv_gpt_decode_step_shared_q8",
                            w, q8, prefix_cache, suffix_cache, n_groups, fan, prefix_len, suffix_max, t, tokens, workspace,
                            workspace_bytes, logits, stream);
}

extern "C" int mpv_gpt_decode_step_shared_ragged(const mpv_gpt_weights* w, void* const* prefix_cache, void* const* suffix_cache, int n_groups,
                                                 int fan, int prefix_stride, const int32_t* group_prefix_len, int max_prefix_len,
                                                 int suffix_max, int t, const int64_t* tokens, void* workspace, size_t workspace_bytes,
                                                 void* logits, hipStream_t stream) {
  return decode_step_shared("mpv_gpt_decode_step_shared_ragged",
                            w, nullptr, prefix_cache, suffix_cache, n_groups, fan, max_prefix_len, suffix_max, t, tokens, workspace,
                            workspace_bytes, logits, stream, true, group_prefix_len, prefix_stride);
}

extern "C" int mpv_gpt_decode_step_shared_ragged_q8(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* prefix_cache,
                                                    void* const* suffix_cache, int n_groups, int fan, int prefix_stride,
                                                    const int32_t* group_prefix_len, int max_prefix_len, int suffix_max, int t,
                                                    const int64_t* tokens, void* workspace, size_t workspace_bytes, void* logits,
                                                    hipStream_t stream) {
  const int rc = check_q8(w, q8, "mpv_gpt_decode_step_shared_ragged_q8");
  if (rc) return rc;
  return decode_step_shared("mpv_gpt_decode_step_shared_ragged_q8",
                            w, q8, prefix_cache, suffix_cache, n_groups, fan, max_prefix_len, suffix_max, t, tokens, workspace,
                            workspace_bytes, logits, stream, true, group_prefix_len, prefix_stride);
}

extern "C" int mpv_gpt_decode_step_shared_steps(const mpv_gpt_weights* w, void* const* prefix_cache, void* const* suffix_cache, int n_groups,
                                                int fan, int prefix_stride, const int32_t* group_prefix_len, int max_prefix_len, int suffix_max,
                                                const int32_t* group_t, int max_t, const int64_t* tokens, void* workspace,
                                                size_t workspace_bytes, void* logits, hipStream_t stream) {
  return decode_step_shared("mpv_gpt_decode_step_shared_steps",
                            w, nullptr, prefix_cache, suffix_cache, n_groups, fan, max_prefix_len, suffix_max, max_t, tokens, workspace,
                            workspace_bytes, logits, stream, true, group_prefix_len, prefix_stride, true, group_t);
}

extern "C" int mpv_gpt_decode_step_shared_steps_q8(const mpv_gpt_weights* w, const mpv_gpt_weights_q8* q8, void* const* prefix_cache,
                                                   void* const* suffix_cache, int n_groups, int fan, int prefix_stride,
                                                   const int32_t* group_prefix_len, int max_prefix_len, int suffix_max,
                                                   const int32_t* group_t, int max_t, const int64_t* tokens, void* workspace,
                                                   size_t workspace_bytes, void* logits, hipStream_t stream) {
  const int rc = check_q8(w, q8, "mpv_gpt_decode_step_shared_steps_q8");
  if (rc) return rc;
  return decode_step_shared("mpv_gpt_decode_step_shared_steps_q8",
                            w, q8, prefix_cache, suffix_cache, n_groups, fan, max_prefix_len, suffix_max, max_t, tokens, workspace,
                            workspace_bytes, logits, stream, true, group_prefix_len, prefix_stride, true, group_t);
}

// InferenceParams.swap_key_value_dict (:1459-1473) for every layer: dst[l][j] = src[l][idx[j]], first `rows` positions
extern "C" int mpv_kv_reorder(void* const* src, void* const* dst, int layers, const int64_t* idx, int batch, int max_len, int rows,
                              int hidden, hipStream_t stream) {
  MPV_REQUIRE(src && dst && idx, MPV_E_ARG, "mpv_kv_reorder: null pointer");
  const int64_t pitch = (int64_t)max_len * 3 * hidden;
  for (int l = 0; l < layers; ++l) {
    const int rc = mpv_gather_rows_ld(src[l], idx, dst[l], batch, (int64_t)rows * 3 * hidden, pitch, pitch, stream);
    if (rc) return rc;
  }
  return MPV_OK;
}
