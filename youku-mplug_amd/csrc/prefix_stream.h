// prefix_stream.h -- what the shared-prefix attention kernels of prefix_attention.hip (evaluation: attn_prefix_fwd_kernel) and of
// prefix_attention_train.hip (training: the forward that keeps its statistics, and the backward) have in common: the workgroup shape,
// the staging of 64-row chunks through LDS, the chunk loop, the forward's kernel body and the host-side tests of the forward entries.
//
// Layout: a workgroup = 4 waves = 128 consecutive rows of one (group, head), so that every chunk brought into LDS serves all of them.
// A chunk is 64 rows of TWO streamed tensors (K and V for the forward and dQ, Q and dO for dK/dV) at the 208-byte pitch of
// prefix_tile.h, double-buffered: 4 x 64 x 208 bytes.
#pragma once

#include <string.h>

#include "mpv_common.h"
#include "prefix_tile.h"
#include "../../include/mpv.h"

namespace {

constexpr int PCH = 64;                 // streamed rows per LDS chunk
constexpr int PCHUNK = PCH * PROWB;
constexpr int PWAVES = 4;
constexpr int PROWS = PWAVES * 32;      // rows per workgroup
constexpr int PTHREADS = PWAVES * 64;

struct PrefixArgs {
  const bf16 *q, *k, *v, *pk, *pv;
  bf16* o;
  const int32_t *seg_start, *group_row;                              // packed only
  long long q_hs, q_rs, k_hs, k_rs, v_hs, v_rs, o_hs, o_rs;
  long long q_cs, k_cs, v_cs, o_cs;                                  // uniform only
  long long pk_gs, pk_hs, pk_rs, pv_gs, pv_hs, pv_rs;
  int n_cont, group_size, lc;                                        // uniform only
  int plen;
  float scale;
  float* lse;                                                        // the training forward only: fp32 [heads][lse_hs]
  long long lse_hs;
};

// A stream of key rows [first, last] and this wave's window [wk0, wk1] into it (tiles outside the window are skipped).  Row kr lives
// at k + kr * k_rs, or with segments (SEG: rows of `seg` each, segment strides k_ss / v_ss) at k + (kr / seg) * k_ss + (kr % seg) * k_rs.
struct KeyStream {
  const bf16 *k, *v;
  long long k_rs, v_rs, k_ss, v_ss;
  int seg, first, last, wk0, wk1;
};

// 64 key rows x HD columns -> registers -> LDS.  Rows past `last` and the columns that pad HD to a multiple of 32 are zeros (the PV
// product multiplies them by exact-zero probabilities; zeros keep it finite); rows past `last` are never read from memory.
template <int HD, bool SEG>
struct KeyStage {
  static constexpr int CPR = (HD + 31) / 32 * 4;       // 16-byte chunks per (padded) row
  static constexpr int NLOAD = (PCH * CPR + PTHREADS - 1) / PTHREADS;   // 2 (hd 64) or 3 (hd 80) b128 per thread
  i32x4 r[NLOAD];

  __device__ __forceinline__ void issue(const bf16* base, int tid, int row0, int last, int seg, long long seg_stride, long long rs) {
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) {
      const int c = tid + PTHREADS * i;
      const int row = c / CPR, cc = c - row * CPR;
      const int kr = row0 + row;
      const bool ok = (c < PCH * CPR) && (kr <= last) && (cc * 8 < HD);
      i32x4 x = i32x4{0, 0, 0, 0};
      if (ok) {
        if constexpr (SEG) {
          const int sg = kr / seg;
          x = *(const i32x4*)(base + sg * seg_stride + (long long)(kr - sg * seg) * rs + cc * 8);
        } else {
          x = *(const i32x4*)(base + (long long)kr * rs + cc * 8);
        }
      }
      r[i] = x;
    }
  }
  __device__ __forceinline__ void commit(char* lds, int tid) {
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) {
      const int c = tid + PTHREADS * i;
      const int row = c / CPR, cc = c - row * CPR;
      if (c < PCH * CPR) *(i32x4*)(lds + row * PROWB + cc * 16) = r[i];
    }
  }
};

// The chunk loop: stream ks through the two LDS buffers (the next chunk's global loads in flight under this chunk's tiles) and hand
// every 32-key tile inside this wave's window to tile(k chunk, v chunk, tile of the chunk, its first key).  Every wave stages; only an
// `active` one (it has rows) computes.
template <int HD, bool SEG, class Tile>
__device__ __forceinline__ void stream_tiles(char* smem, const KeyStream& ks, int tid, bool active, Tile tile) {
  KeyStage<HD, SEG> sk_, sv_;
  const int nchunk = (ks.last - ks.first) / PCH + 1;
  sk_.issue(ks.k, tid, ks.first, ks.last, ks.seg, ks.k_ss, ks.k_rs);
  sv_.issue(ks.v, tid, ks.first, ks.last, ks.seg, ks.v_ss, ks.v_rs);
  sk_.commit(smem, tid);
  sv_.commit(smem + PCHUNK, tid);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    const int cur = c & 1;
    if (c + 1 < nchunk) {
      sk_.issue(ks.k, tid, ks.first + (c + 1) * PCH, ks.last, ks.seg, ks.k_ss, ks.k_rs);
      sv_.issue(ks.v, tid, ks.first + (c + 1) * PCH, ks.last, ks.seg, ks.v_ss, ks.v_rs);
    }
    const char* kl = smem + cur * 2 * PCHUNK;
    if (active) {
#pragma unroll 1
      for (int kt = 0; kt < 2; ++kt) {
        const int key0 = ks.first + c * PCH + kt * 32;
        if (key0 > ks.wk1 || key0 + 31 < ks.wk0) continue;
        tile(kl, kl + PCHUNK, kt, key0);
      }
    }
    if (c + 1 < nchunk) {
      sk_.commit(smem + (cur ^ 1) * 2 * PCHUNK, tid);
      sv_.commit(smem + (cur ^ 1) * 2 * PCHUNK + PCHUNK, tid);
    }
    __syncthreads();
  }
}

// The forward's use of it: every tile updates this wave's rows (prefix_tile.h).
template <int HD, bool SEG, class Visible>
__device__ __forceinline__ void stream_phase(char* smem, const KeyStream& ks, int tid, int lane, bool active,
                                             const bf16x8 (&qf)[HD / 16], float sc, float& m, float& l, f32x16 (&oacc)[(HD + 31) / 32],
                                             Visible visible) {
  stream_tiles<HD, SEG>(smem, ks, tid, active, [&](const char* kl, const char* vl, int kt, int key0) {
    ptile_update<HD>(kl, vl, kt, key0, qf, sc, m, l, oacc, lane, visible);
  });
}

// The forward's kernel body (prefix_attention.hip's header tells the layout and the two phases).  LSE: also store the row's softmax
// statistic m + log(l) of the scaled scores -- the same tiles in the same order, so o does not depend on it.
template <int HD, bool PACKED, bool LSE>
__device__ __forceinline__ void prefix_fwd_body(const PrefixArgs& p, char* smem) {
  constexpr int NS = HD / 16;
  constexpr int NDT = (HD + 31) / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.z, h = blockIdx.y;
  // rows [g0, g1) of this group, and the continuation its uniform numbering starts from
  const int c0 = PACKED ? 0 : g * p.group_size;
  const int g0 = PACKED ? p.group_row[g] : 0;
  const int g1 = PACKED ? p.group_row[g + 1] : min(p.group_size, p.n_cont - c0) * p.lc;
  const int blk_r0 = g0 + blockIdx.x * PROWS;
  if (blk_r0 >= g1) return;                              // (a group smaller than the largest): uniform over the workgroup
  const int wq0 = blk_r0 + wave * 32;
  const int r = wq0 + (lane & 31);                       // this lane's query row
  const int rc = min(r, g1 - 1);
  const bool active = wq0 < g1;
  // the row map: the first own key a row sees, and a row's place in q / k / v / o given that tensor's strides
  auto first_key = [&](int row) { return PACKED ? p.seg_start[row] : row / p.lc * p.lc; };
  auto row_at = [&](int row, long long cs, long long rs) {
    return PACKED ? (long long)row * rs : (long long)(c0 + row / p.lc) * cs + (long long)(row % p.lc) * rs;
  };
  const int row_first_key = first_key(rc);

  bf16x8 qf[NS];
  {
    const bf16* rp = p.q + row_at(rc, p.q_cs, p.q_rs) + (long long)h * p.q_hs + (lane >> 5) * 8;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      union { i32x4 i; bf16x8 b; } u;
      u.i = *(const i32x4*)(rp + s * 16);                // HD is a multiple of 16: every d-step lies inside the row
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

  // ---------------- phase 1: the group's prefix, dense for every row
  if (p.plen > 0) {
    const int last = p.plen - 1;
    const KeyStream ks = {p.pk + (long long)g * p.pk_gs + (long long)h * p.pk_hs, p.pv + (long long)g * p.pv_gs + (long long)h * p.pv_hs,
                          p.pk_rs, p.pv_rs, 0, 0, 0, 0, last, 0, last};
    stream_phase<HD, false>(smem, ks, tid, lane, active, qf, sc, m, l, oacc, [&](int key) { return key <= last; });
  }

  // ---------------- phase 2: own keys, visible iff in the row's own continuation and not behind the row
  {
    // the first own key any row of the workgroup sees and the last; this wave's window (wave-uniform tile skips)
    const KeyStream ks = {p.k + (long long)c0 * p.k_cs + (long long)h * p.k_hs, p.v + (long long)c0 * p.v_cs + (long long)h * p.v_hs,
                          p.k_rs, p.v_rs, p.k_cs, p.v_cs, p.lc,
                          __builtin_amdgcn_readfirstlane(first_key(blk_r0)), min(g1, blk_r0 + PROWS) - 1,
                          __builtin_amdgcn_readfirstlane(first_key(min(wq0, g1 - 1))), min(wq0 + 31, g1 - 1)};
    stream_phase<HD, !PACKED>(smem, ks, tid, lane, active, qf, sc, m, l, oacc,
                              [&](int key) { return key >= row_first_key && key <= rc; });
  }

  if (r < g1) {
    const float inv_l = 1.0f / l;                        // l >= 1: the row sees at least its own key
    bf16* orow = p.o + row_at(r, p.o_cs, p.o_rs) + (long long)h * p.o_hs;
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int col = d * 32 + 8 * q4 + 4 * (lane >> 5);
        if (col < HD) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = oacc[d][4 * q4 + e] * inv_l;
          *(bf16x4*)(orow + col) = cvt4(v);
        }
      }
    if constexpr (LSE) {
      if (lane < 32) p.lse[(long long)h * p.lse_hs + r] = m + logf(l);      // both half-waves hold the row's (m, l)
    }
  }
}

// An entry's own side of its descriptor: its index pointers, then (map_args) its shape tests, the row map's fields of PrefixArgs,
// the number of rows the kernel indexes (`span`) and the rows of the largest group, which size the grid.
bool map_pointers(const mpv_attn_prefix_desc*) { return true; }
bool map_pointers(const mpv_attn_prefix_packed_desc* d) { return d->seg_start && d->group_row; }

int map_args(const char* name, const mpv_attn_prefix_desc* d, PrefixArgs& a, long long& span, long long& group_rows) {
  MPV_REQUIRE(d->n_cont > 0 && d->group_size > 0 && d->heads > 0 && d->cont_len > 0 && d->prefix_len >= 0, MPV_E_SHAPE,
              "%s: empty problem (n_cont %d, group_size %d, heads %d, cont_len %d, prefix_len %d)", name, d->n_cont,
              d->group_size, d->heads, d->cont_len, d->prefix_len);
  MPV_REQUIRE(d->n_groups == (d->n_cont + d->group_size - 1) / d->group_size, MPV_E_SHAPE,
              "%s: n_groups %d must be ceil(n_cont %d / group_size %d)", name, d->n_groups, d->n_cont, d->group_size);
  a.q_cs = d->q_cs; a.k_cs = d->k_cs; a.v_cs = d->v_cs; a.o_cs = d->o_cs;
  a.n_cont = d->n_cont;
  a.group_size = d->group_size;
  a.lc = d->cont_len;
  span = group_rows = (long long)d->group_size * d->cont_len;
  return MPV_OK;
}

int map_args(const char* name, const mpv_attn_prefix_packed_desc* d, PrefixArgs& a, long long& span, long long& group_rows) {
  MPV_REQUIRE(d->rows >= 1 && d->n_groups >= 1 && d->heads >= 1 && d->prefix_len >= 0, MPV_E_SHAPE,
              "%s: empty problem (rows %d, n_groups %d, heads %d, prefix_len %d)", name, d->rows, d->n_groups,
              d->heads, d->prefix_len);
  MPV_REQUIRE(d->max_group_rows >= 1 && d->max_group_rows <= d->rows, MPV_E_SHAPE,
              "%s: max_group_rows %d must lie in [1, rows %d]", name, d->max_group_rows, d->rows);
  a.seg_start = d->seg_start;
  a.group_row = d->group_row;
  span = d->rows;
  group_rows = d->max_group_rows;
  return MPV_OK;
}

// Everything the forward entries have in common but the launch: the tests (the entry's own shape tests take their place between the
// head_dim test and the grid limits, so the first fault named is the same whichever entry meets it), the copy into PrefixArgs and
// the grid.  `index_arrays` finishes the pointer-alignment message, the one text whose ending is the entry's own.  `lse` (with
// want_lse, the training forward) joins the null-pointer and the alignment test.
template <class Desc>
int prefix_fwd_args(const char* name, const char* index_arrays, const Desc* d, bool want_lse, float* lse, PrefixArgs& a, dim3& grid) {
  MPV_REQUIRE(d && d->q && d->k && d->v && d->o && map_pointers(d) && (d->prefix_len == 0 || (d->pk && d->pv)) && (!want_lse || lse),
              MPV_E_ARG, "%s: null pointer", name);
  MPV_REQUIRE(d->head_dim == 64 || d->head_dim == 80, MPV_E_SHAPE, "%s: head_dim %d is not supported (64: the 1.3B decoder, 80: 2.7B)",
              name, d->head_dim);
  a = PrefixArgs{};
  long long span, group_rows;
  if (const int rc = map_args(name, d, a, span, group_rows)) return rc;
  MPV_REQUIRE(span < (1ll << 30) && d->n_groups <= 65535 && d->heads <= 65535, MPV_E_SHAPE, "%s: problem too large", name);
  a.q = (const bf16*)d->q;
  a.k = (const bf16*)d->k;
  a.v = (const bf16*)d->v;
  a.pk = (const bf16*)d->pk;
  a.pv = (const bf16*)d->pv;
  a.o = (bf16*)d->o;
  a.q_hs = d->q_hs; a.q_rs = d->q_rs;
  a.k_hs = d->k_hs; a.k_rs = d->k_rs;
  a.v_hs = d->v_hs; a.v_rs = d->v_rs;
  a.o_hs = d->o_hs; a.o_rs = d->o_rs;
  a.pk_gs = d->pk_gs; a.pk_hs = d->pk_hs; a.pk_rs = d->pk_rs;
  a.pv_gs = d->pv_gs; a.pv_hs = d->pv_hs; a.pv_rs = d->pv_rs;
  a.plen = d->prefix_len;
  a.scale = d->scale;
  a.lse = want_lse ? lse : nullptr;
  a.lse_hs = span;
  const long long st[] = {a.q_cs, a.q_hs, a.q_rs, a.k_cs, a.k_hs, a.k_rs, a.v_cs, a.v_hs, a.v_rs,
                          a.pk_gs, a.pk_hs, a.pk_rs, a.pv_gs, a.pv_hs, a.pv_rs};
  bool al = true;
  for (long long s : st) al = al && (s % 8 == 0);
  MPV_REQUIRE(al && a.o_cs % 4 == 0 && a.o_hs % 4 == 0 && a.o_rs % 4 == 0, MPV_E_ALIGN,
              "%s: strides must keep q/k/v/pk/pv rows 16-byte and o rows 8-byte aligned", name);
  MPV_REQUIRE((((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.pk | (uintptr_t)a.pv) & 15) == 0 &&
                  ((uintptr_t)a.o & 7) == 0 && (((uintptr_t)a.seg_start | (uintptr_t)a.group_row | (uintptr_t)a.lse) & 3) == 0,
              MPV_E_ALIGN, "%s: q/k/v/pk/pv must be 16-byte aligned, o 8-byte%s", name, index_arrays);
  MPV_REQUIRE(a.scale > 0.f, MPV_E_ARG, "%s: scale must be positive", name);
  grid = dim3((unsigned)((group_rows + PROWS - 1) / PROWS), (unsigned)d->heads, (unsigned)d->n_groups);
  return MPV_OK;
}

}  // namespace
