// prefix_packed_attention.hip -- causal attention of PACKED, ragged continuations against per-group shared prefixes (evaluation only).
//
// The problem of prefix_attention.hip without its two uniformities: continuations have their own lengths, and groups their own
// numbers of continuations.  All continuation rows lie end to end in one [rows] array (the continuations of one group next to each
// other, so a group is one contiguous row range), and two small index arrays describe the packing:
//   seg_start[r]   packed index of the first row of the continuation row r belongs to (seg_start[r] <= r)
//   group_row[g]   first packed row of group g (group_row[n_groups] == rows)
// Query row r attends to the prefix_len prefix keys of its group and to its own keys kr with seg_start[r] <= kr <= r: one softmax
// over both sets.
//
// Layout: a workgroup = 4 waves = 128 consecutive packed rows of one (group, head) -- prefix_attention.hip's stacking is simply
// the packed order here.  Phase 1 streams the group's prefix (dense for every row); phase 2 streams the packed own keys from
// seg_start[first row of the tile] (a continuation may straddle a tile: the second tile starts in the first) to the tile's last
// row, masked by the two integer compares above.  Tile arithmetic: prefix_tile.h (S^T = K Q^T on mfma_f32_32x32x16_bf16, online
// softmax in fp32, probabilities rounded to bf16 for the PV product, one division at the end).  A masked key is a true no-op:
// its score is -inf before the running max and its probability exp(-inf) = 0 exactly, so a row's result depends on its group's
// prefix, on its own continuation and on nothing else.
#include <string.h>

#include "mpv_common.h"
#include "prefix_tile.h"
#include "../../include/mpv.h"

namespace {

constexpr int KCH = 64;                 // key rows per LDS chunk
constexpr int KCHUNK = KCH * PROWB;
constexpr int KWAVES = 4;
constexpr int KROWS = KWAVES * 32;      // packed query rows per workgroup
constexpr int KTHREADS = KWAVES * 64;

struct PackedArgs {
  const bf16 *q, *k, *v, *pk, *pv;
  bf16* o;
  const int32_t *seg_start, *group_row;
  long long q_rs, q_hs, k_rs, k_hs, v_rs, v_hs, o_rs, o_hs;
  long long pk_gs, pk_hs, pk_rs, pv_gs, pv_hs, pv_rs;
  int plen, hd;
  float scale;
};

// A deliberate copy of prefix_attention.hip's SegStage (and, in the kernel below, of that kernel's prefix phase and chunk loop) without the
// per-segment division: that file is to compile as it does, so the staging code is restated here as prefix_tile.h restates its tile.
// 64 key rows x HD columns -> registers -> LDS; row kr of the stream lives at base + kr * rs.  Rows past `last` and columns past
// hd are zeros (the PV product multiplies them by exact-zero probabilities; zeros keep it finite), and are never read.
template <int HD>
struct RowStage {
  static constexpr int CPR = (HD + 31) / 32 * 4;       // 16-byte chunks per (padded) row
  static constexpr int NLOAD = (KCH * CPR + KTHREADS - 1) / KTHREADS;   // 2 (hd 64) or 3 (hd 80) b128 per thread
  i32x4 r[NLOAD];

  __device__ __forceinline__ void issue(const bf16* base, int tid, int row0, int last, long long rs, int hd) {
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) {
      const int c = tid + KTHREADS * i;
      const int row = c / CPR, cc = c - row * CPR;
      const int kr = row0 + row;
      const bool ok = (c < KCH * CPR) && (kr <= last) && (cc * 8 < hd);
      i32x4 x = i32x4{0, 0, 0, 0};
      if (ok) x = *(const i32x4*)(base + (long long)kr * rs + cc * 8);
      r[i] = x;
    }
  }
  __device__ __forceinline__ void commit(char* lds, int tid) {
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) {
      const int c = tid + KTHREADS * i;
      const int row = c / CPR, cc = c - row * CPR;
      if (c < KCH * CPR) *(i32x4*)(lds + row * PROWB + cc * 16) = r[i];
    }
  }
};

template <int HD>
__global__ __launch_bounds__(KTHREADS, 2) void attn_prefix_packed_fwd_kernel(const PackedArgs p) {
  constexpr int NS = HD / 16;
  constexpr int NDT = (HD + 31) / 32;
  __shared__ __attribute__((aligned(16))) char smem[4 * KCHUNK];     // [buf][K|V]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.z, h = blockIdx.y;
  const int g0 = p.group_row[g], g1 = p.group_row[g + 1];     // packed rows [g0, g1) of this group
  const int blk_r0 = g0 + blockIdx.x * KROWS;                 // first packed row of this tile
  if (blk_r0 >= g1) return;                                   // (a group smaller than the largest): uniform over the workgroup
  const int wq0 = blk_r0 + wave * 32;
  const int r = wq0 + (lane & 31);                            // this lane's packed query row
  const int rc = min(r, g1 - 1);
  const int row_first_key = p.seg_start[rc];                  // first packed own key visible to row r

  bf16x8 qf[NS];
  {
    const bf16* rp = p.q + (long long)rc * p.q_rs + (long long)h * p.q_hs + (lane >> 5) * 8;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      union { i32x4 i; bf16x8 b; } u;
      u.i = *(const i32x4*)(rp + s * 16);                     // HD is a multiple of 16: every d-step lies inside the row
      if (!(r < g1)) u.i = i32x4{0, 0, 0, 0};
      qf[s] = u.b;
    }
  }
  const float sc = p.scale;
  float m = -INFINITY, l = 0.f;
  f32x16 oacc[NDT];
#pragma unroll
  for (int d = 0; d < NDT; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;

  RowStage<HD> sk_, sv_;
  // ---------------- phase 1: the group's prefix, dense for every row
  if (p.plen > 0) {
    const bf16* kb = p.pk + (long long)g * p.pk_gs + (long long)h * p.pk_hs;
    const bf16* vb = p.pv + (long long)g * p.pv_gs + (long long)h * p.pv_hs;
    const int last = p.plen - 1;
    const int nchunk = (p.plen + KCH - 1) / KCH;
    sk_.issue(kb, tid, 0, last, p.pk_rs, p.hd);
    sv_.issue(vb, tid, 0, last, p.pv_rs, p.hd);
    sk_.commit(smem, tid);
    sv_.commit(smem + KCHUNK, tid);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
      const int cur = c & 1;
      if (c + 1 < nchunk) {
        sk_.issue(kb, tid, (c + 1) * KCH, last, p.pk_rs, p.hd);
        sv_.issue(vb, tid, (c + 1) * KCH, last, p.pv_rs, p.hd);
      }
      const char* kl = smem + cur * 2 * KCHUNK;
      {
#pragma unroll 1
        for (int kt = 0; kt < 2; ++kt) {
          const int key0 = c * KCH + kt * 32;
          if (key0 > last) continue;
          ptile_update<HD>(kl, kl + KCHUNK, kt, key0, qf, sc, m, l, oacc, lane, [&](int key) { return key <= last; });
        }
      }
      if (c + 1 < nchunk) {
        sk_.commit(smem + (cur ^ 1) * 2 * KCHUNK, tid);
        sv_.commit(smem + (cur ^ 1) * 2 * KCHUNK + KCHUNK, tid);
      }
      __syncthreads();
    }
  }

  // ---------------- phase 2: own keys, visible iff in the row's own continuation and not behind the row
  {
    const bf16* kb = p.k + (long long)h * p.k_hs;
    const bf16* vb = p.v + (long long)h * p.v_hs;
    const int kb0 = __builtin_amdgcn_readfirstlane(p.seg_start[blk_r0]);       // first own key any row of the tile sees
    const int last = min(g1, blk_r0 + KROWS) - 1;                               // ... and the last (< rows: nothing behind is read)
    const int nchunk = (last - kb0) / KCH + 1;
    const int wk0 = __builtin_amdgcn_readfirstlane(p.seg_start[min(wq0, g1 - 1)]);   // this wave's key window (wave-uniform skips)
    const int wk1 = min(wq0 + 31, g1 - 1);
    sk_.issue(kb, tid, kb0, last, p.k_rs, p.hd);
    sv_.issue(vb, tid, kb0, last, p.v_rs, p.hd);
    sk_.commit(smem, tid);
    sv_.commit(smem + KCHUNK, tid);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
      const int cur = c & 1;
      if (c + 1 < nchunk) {
        sk_.issue(kb, tid, kb0 + (c + 1) * KCH, last, p.k_rs, p.hd);
        sv_.issue(vb, tid, kb0 + (c + 1) * KCH, last, p.v_rs, p.hd);
      }
      const char* kl = smem + cur * 2 * KCHUNK;
      if (wq0 < g1) {
#pragma unroll 1
        for (int kt = 0; kt < 2; ++kt) {
          const int key0 = kb0 + c * KCH + kt * 32;
          if (key0 > wk1 || key0 + 31 < wk0) continue;
          ptile_update<HD>(kl, kl + KCHUNK, kt, key0, qf, sc, m, l, oacc, lane,
                           [&](int key) { return key >= row_first_key && key <= rc; });
        }
      }
      if (c + 1 < nchunk) {
        sk_.commit(smem + (cur ^ 1) * 2 * KCHUNK, tid);
        sv_.commit(smem + (cur ^ 1) * 2 * KCHUNK + KCHUNK, tid);
      }
      __syncthreads();
    }
  }

  if (r < g1) {
    const float inv_l = 1.0f / l;                        // l >= 1: the row sees at least its own key
    bf16* orow = p.o + (long long)r * p.o_rs + (long long)h * p.o_hs;
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int col = d * 32 + 8 * q4 + 4 * (lane >> 5);
        if (col < p.hd) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = oacc[d][4 * q4 + e] * inv_l;
          *(bf16x4*)(orow + col) = cvt4(v);
        }
      }
  }
}

}  // namespace

extern "C" int mpv_attn_prefix_packed_layout(const int32_t* cont_len, int n_cont, const int32_t* conts_per_group, int n_groups,
                                             int32_t* seg_start_out, int32_t* group_row_out, int* rows_out,
                                             int* max_group_rows_out) {
  MPV_REQUIRE(cont_len && conts_per_group && seg_start_out && group_row_out && rows_out && max_group_rows_out, MPV_E_ARG,
              "mpv_attn_prefix_packed_layout: null pointer");
  MPV_REQUIRE(n_cont >= 1 && n_groups >= 1, MPV_E_SHAPE, "mpv_attn_prefix_packed_layout: empty problem (n_cont %d, n_groups %d)",
              n_cont, n_groups);
  long long conts = 0, total = 0;
  for (int g = 0; g < n_groups; ++g) {
    MPV_REQUIRE(conts_per_group[g] >= 1, MPV_E_SHAPE, "mpv_attn_prefix_packed_layout: group %d has no continuation (%d)", g,
                (int)conts_per_group[g]);
    conts += conts_per_group[g];
  }
  MPV_REQUIRE(conts == n_cont, MPV_E_SHAPE, "mpv_attn_prefix_packed_layout: the groups hold %lld continuations, n_cont is %d", conts,
              n_cont);
  for (int c = 0; c < n_cont; ++c) {
    MPV_REQUIRE(cont_len[c] >= 1, MPV_E_SHAPE, "mpv_attn_prefix_packed_layout: continuation %d has length %d (must be >= 1)", c,
                (int)cont_len[c]);
    total += cont_len[c];
    MPV_REQUIRE(total < (1ll << 30), MPV_E_SHAPE, "mpv_attn_prefix_packed_layout: more than 2^30 rows");
  }
  int row = 0, c = 0, max_rows = 0;
  for (int g = 0; g < n_groups; ++g) {
    group_row_out[g] = row;
    for (int i = 0; i < conts_per_group[g]; ++i, ++c) {
      const int first = row;
      for (int j = 0; j < cont_len[c]; ++j) seg_start_out[row++] = first;
    }
    if (row - group_row_out[g] > max_rows) max_rows = row - group_row_out[g];
  }
  group_row_out[n_groups] = row;
  *rows_out = row;
  *max_group_rows_out = max_rows;
  return MPV_OK;
}

extern "C" int mpv_attn_prefix_packed_fwd(const mpv_attn_prefix_packed_desc* d, hipStream_t stream) {
  MPV_REQUIRE(d && d->q && d->k && d->v && d->o && d->seg_start && d->group_row && (d->prefix_len == 0 || (d->pk && d->pv)),
              MPV_E_ARG, "mpv_attn_prefix_packed_fwd: null pointer");
  MPV_REQUIRE(d->head_dim == 64 || d->head_dim == 80, MPV_E_SHAPE,
              "mpv_attn_prefix_packed_fwd: head_dim %d is not supported (64: the 1.3B decoder, 80: 2.7B)", d->head_dim);
  MPV_REQUIRE(d->rows >= 1 && d->n_groups >= 1 && d->heads >= 1 && d->prefix_len >= 0, MPV_E_SHAPE,
              "mpv_attn_prefix_packed_fwd: empty problem (rows %d, n_groups %d, heads %d, prefix_len %d)", d->rows, d->n_groups,
              d->heads, d->prefix_len);
  MPV_REQUIRE(d->max_group_rows >= 1 && d->max_group_rows <= d->rows, MPV_E_SHAPE,
              "mpv_attn_prefix_packed_fwd: max_group_rows %d must lie in [1, rows %d]", d->max_group_rows, d->rows);
  MPV_REQUIRE(d->rows < (1 << 30) && d->n_groups <= 65535 && d->heads <= 65535, MPV_E_SHAPE,
              "mpv_attn_prefix_packed_fwd: problem too large");
  const int64_t st[] = {d->q_rs, d->q_hs, d->k_rs, d->k_hs, d->v_rs, d->v_hs, d->pk_gs, d->pk_hs, d->pk_rs, d->pv_gs, d->pv_hs, d->pv_rs};
  bool al = true;
  for (int64_t s : st) al = al && (s % 8 == 0);
  MPV_REQUIRE(al && d->o_rs % 4 == 0 && d->o_hs % 4 == 0, MPV_E_ALIGN,
              "mpv_attn_prefix_packed_fwd: strides must keep q/k/v/pk/pv rows 16-byte and o rows 8-byte aligned");
  MPV_REQUIRE((((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->pk | (uintptr_t)d->pv) & 15) == 0 &&
                  ((uintptr_t)d->o & 7) == 0 && (((uintptr_t)d->seg_start | (uintptr_t)d->group_row) & 3) == 0,
              MPV_E_ALIGN, "mpv_attn_prefix_packed_fwd: q/k/v/pk/pv must be 16-byte aligned, o 8-byte, the index arrays 4-byte");
  MPV_REQUIRE(d->scale > 0.f, MPV_E_ARG, "mpv_attn_prefix_packed_fwd: scale must be positive");
  PackedArgs a;
  a.q = (const bf16*)d->q;
  a.k = (const bf16*)d->k;
  a.v = (const bf16*)d->v;
  a.pk = (const bf16*)d->pk;
  a.pv = (const bf16*)d->pv;
  a.o = (bf16*)d->o;
  a.seg_start = d->seg_start;
  a.group_row = d->group_row;
  a.q_rs = d->q_rs; a.q_hs = d->q_hs;
  a.k_rs = d->k_rs; a.k_hs = d->k_hs;
  a.v_rs = d->v_rs; a.v_hs = d->v_hs;
  a.o_rs = d->o_rs; a.o_hs = d->o_hs;
  a.pk_gs = d->pk_gs; a.pk_hs = d->pk_hs; a.pk_rs = d->pk_rs;
  a.pv_gs = d->pv_gs; a.pv_hs = d->pv_hs; a.pv_rs = d->pv_rs;
  a.plen = d->prefix_len;
  a.hd = d->head_dim;
  a.scale = d->scale;
  const dim3 grid((unsigned)((d->max_group_rows + KROWS - 1) / KROWS), (unsigned)d->heads, (unsigned)d->n_groups);
  if (d->head_dim == 64)
    hipLaunchKernelGGL(attn_prefix_packed_fwd_kernel<64>, grid, dim3(KTHREADS), 0, stream, a);
  else
    hipLaunchKernelGGL(attn_prefix_packed_fwd_kernel<80>, grid, dim3(KTHREADS), 0, stream, a);
  return mpv_check_launch("mpv_attn_prefix_packed_fwd");
}
