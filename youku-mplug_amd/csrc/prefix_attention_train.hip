// prefix_attention_train.hip -- packed shared-prefix attention for TRAINING: the forward of prefix_attention.hip with its softmax
// statistics kept, and the backward.  (Self-critical caption training samples N captions per clip on a shared prefix; the training
// pass over them runs every clip's prefix once and the N samples as packed continuations: DESIGN.md section 32.)
//
//   mpv_attn_prefix_packed_fwd_lse   the kernel body of mpv_attn_prefix_packed_fwd (prefix_stream.h: prefix_fwd_body, same tiles in the
//                                    same order: o agrees bit for bit) which also stores lse[h][r] = m + log(l) of the row's ONE softmax
//                                    over [prefix | own visible keys], on the scaled scores.
//   mpv_attn_prefix_packed_bwd       two kernels, no atomics: every output element is written by exactly one workgroup.
//
// The backward, per continuation over the keys [its group's prefix | its own rows]:  P = exp(scale s - lse) in fp32,
// delta = sum_d dO o (the bf16 o given), dS = P (dO V^T - delta), dS and P rounded to bf16 before the products they enter,
// dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO; a group's dPK / dPV are the sums over all rows of the group.  A masked pair has
// P = 0 exactly (no exp is taken of it), so it contributes an exact zero everywhere.
//
// pptrain_dq_kernel is shaped like the forward: 128 query rows of a (group, head) per workgroup, a query row per lane
// (prefix_tile.h's S^T = K Q^T orientation), q and dO fragments in registers, K / V chunks streamed through LDS -- first the prefix,
// then the own keys the workgroup can see.  Per 32-key tile: S^T = K Q^T and dP^T = V dO^T (A operand: the LDS rows; B: the
// registers), dS^T in the accumulator layout, rounded into the B operand of dQ^T += K^T dS^T (A: the transposing LDS read of the K
// chunk) -- the forward's PV product with K in V's place.  It also stores delta for the second kernel.
//
// pptrain_dkv_kernel is the same machine with the roles swapped: 128 KEY rows per workgroup, a key per lane, k and v fragments in
// registers, Q / dO chunks (and their rows' lse, delta and seg_start: 3 x 64 words beside each chunk) streamed through LDS.  Per
// 32-query tile: S = Q K^T, dP = dO V^T, then dV^T += dO^T P and dK^T += Q^T dS.  The first ceil(prefix_len / 128) workgroups (x)
// of a (group, head) own prefix key tiles and stream ALL query rows of the group; the others own tiles of the group's own keys and
// stream the rows from the tile's first key to the end of the last continuation that has a key in the tile -- found by walking
// seg_start in chunk steps until seg_start[row] lies behind the tile (no further index array).  Key kr is visible to row r iff
// seg_start[r] <= kr <= r.
#include "prefix_stream.h"

namespace {

struct TrainArgs {
  const bf16 *q, *k, *v, *o, *dO, *pk, *pv;
  const float* lse;
  float* delta;
  bf16 *dq, *dk, *dv, *dpk, *dpv;
  const int32_t *seg_start, *group_row;
  long long q_hs, q_rs, k_hs, k_rs, v_hs, v_rs, o_hs, o_rs;
  long long pk_gs, pk_hs, pk_rs, pv_gs, pv_hs, pv_rs;
  int rows, plen, accumulate;
  float scale;
};

constexpr int SIDE_WORDS = 3 * PCH;                     // lse | delta | seg_start of a chunk's 64 rows
constexpr int NO_ROW = 0x7fffffff;                      // seg_start of a staged row behind the stream's last: visible to no key

template <int HD>
__global__ __launch_bounds__(PTHREADS, 2) void pptrain_fwd_kernel(const PrefixArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * PCHUNK];     // [buf][K|V]
  prefix_fwd_body<HD, true, true>(p, smem);
}

// this lane's 8-element pieces of row `rp` (already offset by the lane's half): the B-operand fragments of a 32-row tile
template <int NS>
__device__ __forceinline__ void load_frags(bf16x8 (&f)[NS], const bf16* rp, bool ok) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    union { i32x4 i; bf16x8 b; } u;
    u.i = *(const i32x4*)(rp + s * 16);                  // HD is a multiple of 16: every d-step lies inside the row
    if (!ok) u.i = i32x4{0, 0, 0, 0};
    f[s] = u.b;
  }
}

template <int NDT>
__device__ __forceinline__ void zero_acc(f32x16 (&a)[NDT]) {
#pragma unroll
  for (int d = 0; d < NDT; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) a[d][e] = 0.f;
}

// acc^T (column d = dt*32 + accumulator row, this lane's row of the output) x mul (+ what is there, if `add`) -> bf16 row
template <int HD>
__device__ __forceinline__ void store_row(bf16* row, const f32x16 (&acc)[(HD + 31) / 32], float mul, bool add, int lane) {
#pragma unroll
  for (int d = 0; d < (HD + 31) / 32; ++d)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int col = d * 32 + 8 * q4 + 4 * (lane >> 5);
      if (col < HD) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[d][4 * q4 + e] * mul;
        if (add) v += cvt4(*(const bf16x4*)(row + col));      // fp32 sum, one rounding
        *(bf16x4*)(row + col) = cvt4(v);
      }
    }
}

// ------------------------------------------------------------------------------------------------------------------ dQ
template <int HD>
__global__ __launch_bounds__(PTHREADS, 2) void pptrain_dq_kernel(const TrainArgs p) {
  constexpr int NS = HD / 16;
  constexpr int NDT = (HD + 31) / 32;
  __shared__ __attribute__((aligned(16))) char smem[4 * PCHUNK];     // [buf][K|V]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.z, h = blockIdx.y;
  // what the index arrays promise is clamped to the rows there are
  const int g0 = max(0, min(p.group_row[g], p.rows)), g1 = max(g0, min(p.group_row[g + 1], p.rows));
  const int blk_r0 = g0 + blockIdx.x * PROWS;
  if (blk_r0 >= g1) return;                              // (a group smaller than the largest): uniform over the workgroup
  const int wq0 = blk_r0 + wave * 32;
  const int r = wq0 + (lane & 31);                       // this lane's query row
  const int rc = min(r, g1 - 1);
  const bool active = wq0 < g1, mine = r < g1;
  auto first_key = [&](int row) { return max(g0, min(p.seg_start[row], row)); };
  const int row_first_key = first_key(rc);

  bf16x8 qf[NS], dof[NS];
  float delta = 0.f;
  {
    const long long off = (long long)rc * p.o_rs + (long long)h * p.o_hs + (lane >> 5) * 8;
    load_frags<NS>(qf, p.q + (long long)rc * p.q_rs + (long long)h * p.q_hs + (lane >> 5) * 8, mine);
    load_frags<NS>(dof, p.dO + off, mine);
    bf16x8 of[NS];
    load_frags<NS>(of, p.o + off, mine);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const f32x8 a = cvt8(dof[s]), b = cvt8(of[s]);
#pragma unroll
      for (int e = 0; e < 8; ++e) delta = fmaf(a[e], b[e], delta);
    }
    delta += __shfl_xor(delta, 32, 64);                  // the two half-waves hold the two halves of every d-step
  }
  const float lse = mine ? p.lse[(long long)h * p.rows + r] : 0.f;
  if (mine && lane < 32) p.delta[(long long)h * p.rows + r] = delta;
  const float sc = p.scale;
  f32x16 acc[NDT];
  zero_acc<NDT>(acc);

  auto tile = [&](auto visible) {
    return [&, visible](const char* kl, const char* vl, int kt, int key0) {
      f32x16 s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
      for (int st = 0; st < NS; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pfrag_rows(kl, kt, st, lane), qf[st], s, 0, 0, 0);
#pragma unroll
      for (int st = 0; st < NS; ++st) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pfrag_rows(vl, kt, st, lane), dof[st], dp, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float pr = visible(key0 + pacc_row(e, lane)) ? __expf(s[e] * sc - lse) : 0.f;
        s[e] = pr * (dp[e] - delta);
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 dsf = pacc_to_frag(s, ks);
#pragma unroll
        for (int d = 0; d < NDT; ++d)
          acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pfrag_cols(kl, kt, ks, d, lane), dsf, acc[d], 0, 0, 0);
      }
    };
  };

  // ---------------- phase 1: the group's prefix, dense for every row
  if (p.plen > 0) {
    const int last = p.plen - 1;
    const KeyStream ks = {p.pk + (long long)g * p.pk_gs + (long long)h * p.pk_hs, p.pv + (long long)g * p.pv_gs + (long long)h * p.pv_hs,
                          p.pk_rs, p.pv_rs, 0, 0, 0, 0, last, 0, last};
    stream_tiles<HD, false>(smem, ks, tid, active, tile([&](int key) { return key <= last; }));
  }
  // ---------------- phase 2: own keys, visible iff in the row's own continuation and not behind the row
  {
    const KeyStream ks = {p.k + (long long)h * p.k_hs, p.v + (long long)h * p.v_hs, p.k_rs, p.v_rs, 0, 0, 0,
                          __builtin_amdgcn_readfirstlane(first_key(blk_r0)), min(g1, blk_r0 + PROWS) - 1,
                          __builtin_amdgcn_readfirstlane(first_key(min(wq0, g1 - 1))), min(wq0 + 31, g1 - 1)};
    stream_tiles<HD, false>(smem, ks, tid, active, tile([&](int key) { return key >= row_first_key && key <= rc; }));
  }
  if (mine) store_row<HD>(p.dq + (long long)r * p.q_rs + (long long)h * p.q_hs, acc, sc, false, lane);
}

// ------------------------------------------------------------------------------------------------------------------ dK, dV
template <int HD>
__global__ __launch_bounds__(PTHREADS, 2) void pptrain_dkv_kernel(const TrainArgs p) {
  constexpr int NS = HD / 16;
  constexpr int NDT = (HD + 31) / 32;
  __shared__ __attribute__((aligned(16))) char smem[4 * PCHUNK];     // [buf][Q|dO]
  __shared__ __attribute__((aligned(16))) float side[2 * SIDE_WORDS];   // [buf][lse | delta | seg_start]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.z, h = blockIdx.y;
  const int g0 = max(0, min(p.group_row[g], p.rows)), g1 = max(g0, min(p.group_row[g + 1], p.rows));
  const int npt = (p.plen + PROWS - 1) / PROWS;          // prefix key tiles come first in x
  const bool pre = (int)blockIdx.x < npt;
  const int t0 = pre ? blockIdx.x * PROWS : g0 + ((int)blockIdx.x - npt) * PROWS;      // the tile's first key
  const int kend = pre ? p.plen : g1;                    // one behind the last key there is
  if (t0 >= kend || g0 >= g1) return;                    // uniform over the workgroup
  const int t1 = min(t0 + PROWS, kend) - 1;              // the tile's last key
  const int wk0 = t0 + wave * 32;
  const int kr = wk0 + (lane & 31);                      // this lane's key row
  const int krc = min(kr, kend - 1);
  const bool active = wk0 < kend, mine = kr < kend;
  const long long koff = pre ? (long long)g * p.pk_gs + (long long)h * p.pk_hs + (long long)krc * p.pk_rs
                             : (long long)h * p.k_hs + (long long)krc * p.k_rs;
  const long long voff = pre ? (long long)g * p.pv_gs + (long long)h * p.pv_hs + (long long)krc * p.pv_rs
                             : (long long)h * p.v_hs + (long long)krc * p.v_rs;
  bf16x8 kf[NS], vf[NS];
  load_frags<NS>(kf, (pre ? p.pk : p.k) + koff + (lane >> 5) * 8, mine);
  load_frags<NS>(vf, (pre ? p.pv : p.v) + voff + (lane >> 5) * 8, mine);

  // the query rows [first, last] streamed: the whole group for a prefix tile; for an own tile from its first key to the end (rounded up
  // to chunk steps, inside the group) of the last continuation with a key in it -- seg_start does not decrease along the rows
  const int first = pre ? g0 : t0;
  int last = pre ? g1 - 1 : t1;
  if (!pre)
    while (last + 1 < g1 && __builtin_amdgcn_readfirstlane(p.seg_start[last + 1]) <= t1) last = min(last + PCH, g1 - 1);
  // wave-uniform skips: a tile of rows that lie before this wave's keys, or whose first row starts a continuation behind them
  const int skip_before = pre ? first : wk0;
  const int skip_seg = pre ? NO_ROW - 1 : min(wk0 + 31, kend - 1);

  const float sc = p.scale;
  f32x16 dka[NDT], dva[NDT];
  zero_acc<NDT>(dka);
  zero_acc<NDT>(dva);

  const bf16* qb = p.q + (long long)h * p.q_hs;
  const bf16* dob = p.dO + (long long)h * p.o_hs;
  const float* lseb = p.lse + (long long)h * p.rows;
  const float* delb = p.delta + (long long)h * p.rows;
  KeyStage<HD, false> sq_, sd_;
  float s_lse = 0.f, s_del = 0.f;
  int s_seg = NO_ROW;
  auto issue = [&](int row0) {
    sq_.issue(qb, tid, row0, last, 0, 0, p.q_rs);
    sd_.issue(dob, tid, row0, last, 0, 0, p.o_rs);
    if (tid < PCH) {
      const int row = row0 + tid;
      const bool ok = row <= last;
      s_lse = ok ? lseb[row] : 0.f;
      s_del = ok ? delb[row] : 0.f;
      s_seg = ok ? p.seg_start[row] : NO_ROW;
    }
  };
  auto commit = [&](int buf) {
    sq_.commit(smem + buf * 2 * PCHUNK, tid);
    sd_.commit(smem + buf * 2 * PCHUNK + PCHUNK, tid);
    if (tid < PCH) {
      float* sd = side + buf * SIDE_WORDS;
      sd[tid] = s_lse;
      sd[PCH + tid] = s_del;
      ((int*)sd)[2 * PCH + tid] = s_seg;
    }
  };

  const int nchunk = (last - first) / PCH + 1;
  issue(first);
  commit(0);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    const int cur = c & 1;
    if (c + 1 < nchunk) issue(first + (c + 1) * PCH);
    const char* ql = smem + cur * 2 * PCHUNK;
    const char* dol = ql + PCHUNK;
    const float* sd = side + cur * SIDE_WORDS;
    if (active) {
#pragma unroll 1
      for (int qt = 0; qt < 2; ++qt) {
        const int row0 = first + c * PCH + qt * 32;
        if (row0 > last || row0 + 31 < skip_before) continue;
        if (__builtin_amdgcn_readfirstlane(((const int*)sd)[2 * PCH + qt * 32]) > skip_seg) continue;
        f32x16 s, dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
        for (int st = 0; st < NS; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pfrag_rows(ql, qt, st, lane), kf[st], s, 0, 0, 0);
#pragma unroll
        for (int st = 0; st < NS; ++st) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pfrag_rows(dol, qt, st, lane), vf[st], dp, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = qt * 32 + pacc_row(e, lane);     // the query row's place in the chunk
          const int row = first + c * PCH + i, seg = ((const int*)sd)[2 * PCH + i];
          const bool vis = pre ? seg != NO_ROW : (seg <= kr && kr <= row);
          const float pr = vis ? __expf(s[e] * sc - sd[i]) : 0.f;
          dp[e] = pr * (dp[e] - sd[PCH + i]);
          s[e] = pr;
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 pf = pacc_to_frag(s, ks), dsf = pacc_to_frag(dp, ks);
#pragma unroll
          for (int d = 0; d < NDT; ++d) {
            dva[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pfrag_cols(dol, qt, ks, d, lane), pf, dva[d], 0, 0, 0);
            dka[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pfrag_cols(ql, qt, ks, d, lane), dsf, dka[d], 0, 0, 0);
          }
        }
      }
    }
    if (c + 1 < nchunk) commit(cur ^ 1);
    __syncthreads();
  }

  if (mine) {
    const bool add = pre && p.accumulate;
    store_row<HD>((pre ? p.dpk : p.dk) + koff, dka, sc, add, lane);
    store_row<HD>((pre ? p.dpv : p.dv) + voff, dva, 1.0f, add, lane);
  }
}

}  // namespace

extern "C" int mpv_attn_prefix_packed_fwd_lse(const mpv_attn_prefix_packed_desc* d, float* lse, hipStream_t stream) {
  const char* name = "mpv_attn_prefix_packed_fwd_lse";
  PrefixArgs a;
  dim3 grid;
  if (const int rc = prefix_fwd_args(name, ", the index arrays and lse 4-byte", d, true, lse, a, grid)) return rc;
  if (d->head_dim == 64)
    hipLaunchKernelGGL((pptrain_fwd_kernel<64>), grid, dim3(PTHREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((pptrain_fwd_kernel<80>), grid, dim3(PTHREADS), 0, stream, a);
  return mpv_check_launch(name);
}

extern "C" int mpv_attn_prefix_packed_bwd(const mpv_attn_prefix_packed_bwd_desc* d, hipStream_t stream) {
  const char* name = "mpv_attn_prefix_packed_bwd";
  MPV_REQUIRE(d && d->q && d->k && d->v && d->o && d->dO && d->lse && d->delta && d->dq && d->dk && d->dv && d->seg_start &&
                  d->group_row && (d->prefix_len == 0 || (d->pk && d->pv && d->dpk && d->dpv)),
              MPV_E_ARG, "%s: null pointer", name);
  MPV_REQUIRE(d->head_dim == 64 || d->head_dim == 80, MPV_E_SHAPE, "%s: head_dim %d is not supported (64: the 1.3B decoder, 80: 2.7B)",
              name, d->head_dim);
  MPV_REQUIRE(d->rows >= 1 && d->n_groups >= 1 && d->heads >= 1 && d->prefix_len >= 0, MPV_E_SHAPE,
              "%s: empty problem (rows %d, n_groups %d, heads %d, prefix_len %d)", name, d->rows, d->n_groups, d->heads, d->prefix_len);
  MPV_REQUIRE(d->max_group_rows >= 1 && d->max_group_rows <= d->rows, MPV_E_SHAPE, "%s: max_group_rows %d must lie in [1, rows %d]", name,
              d->max_group_rows, d->rows);
  const long long own_tiles = ((long long)d->max_group_rows + PROWS - 1) / PROWS, pre_tiles = ((long long)d->prefix_len + PROWS - 1) / PROWS;
  MPV_REQUIRE(d->rows < (1 << 30) && d->prefix_len < (1 << 30) && d->n_groups <= 65535 && d->heads <= 65535, MPV_E_SHAPE,
              "%s: problem too large", name);
  TrainArgs a = {};
  a.q = (const bf16*)d->q; a.k = (const bf16*)d->k; a.v = (const bf16*)d->v; a.o = (const bf16*)d->o; a.dO = (const bf16*)d->dO;
  a.pk = (const bf16*)d->pk; a.pv = (const bf16*)d->pv;
  a.lse = d->lse; a.delta = d->delta;
  a.dq = (bf16*)d->dq; a.dk = (bf16*)d->dk; a.dv = (bf16*)d->dv; a.dpk = (bf16*)d->dpk; a.dpv = (bf16*)d->dpv;
  a.seg_start = d->seg_start; a.group_row = d->group_row;
  a.q_hs = d->q_hs; a.q_rs = d->q_rs; a.k_hs = d->k_hs; a.k_rs = d->k_rs; a.v_hs = d->v_hs; a.v_rs = d->v_rs; a.o_hs = d->o_hs; a.o_rs = d->o_rs;
  a.pk_gs = d->pk_gs; a.pk_hs = d->pk_hs; a.pk_rs = d->pk_rs; a.pv_gs = d->pv_gs; a.pv_hs = d->pv_hs; a.pv_rs = d->pv_rs;
  a.rows = d->rows; a.plen = d->prefix_len; a.accumulate = d->accumulate_prefix != 0; a.scale = d->scale;
  const long long st[] = {a.q_hs, a.q_rs, a.k_hs, a.k_rs, a.v_hs, a.v_rs, a.o_hs, a.o_rs, a.pk_gs, a.pk_hs, a.pk_rs, a.pv_gs, a.pv_hs, a.pv_rs};
  bool al = true;
  for (long long s : st) al = al && (s % 8 == 0);
  MPV_REQUIRE(al, MPV_E_ALIGN, "%s: strides must keep q/k/v/o/dO/pk/pv rows and the gradients' 16-byte aligned", name);
  MPV_REQUIRE((((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.o | (uintptr_t)a.dO | (uintptr_t)a.pk | (uintptr_t)a.pv |
                (uintptr_t)a.dq | (uintptr_t)a.dk | (uintptr_t)a.dv | (uintptr_t)a.dpk | (uintptr_t)a.dpv) & 15) == 0 &&
                  (((uintptr_t)a.seg_start | (uintptr_t)a.group_row | (uintptr_t)a.lse | (uintptr_t)a.delta) & 3) == 0,
              MPV_E_ALIGN, "%s: q/k/v/o/dO/pk/pv and the gradients must be 16-byte aligned, the index arrays, lse and delta 4-byte", name);
  MPV_REQUIRE(a.scale > 0.f, MPV_E_ARG, "%s: scale must be positive", name);
  const dim3 block(PTHREADS);
  const dim3 grid_q((unsigned)own_tiles, (unsigned)d->heads, (unsigned)d->n_groups);
  const dim3 grid_kv((unsigned)(pre_tiles + own_tiles), (unsigned)d->heads, (unsigned)d->n_groups);
  if (d->head_dim == 64) {
    hipLaunchKernelGGL((pptrain_dq_kernel<64>), grid_q, block, 0, stream, a);
    hipLaunchKernelGGL((pptrain_dkv_kernel<64>), grid_kv, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL((pptrain_dq_kernel<80>), grid_q, block, 0, stream, a);
    hipLaunchKernelGGL((pptrain_dkv_kernel<80>), grid_kv, block, 0, stream, a);
  }
  return mpv_check_launch(name);
}
