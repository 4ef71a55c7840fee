// prefix_attention.hip -- causal attention of many continuations against per-group shared, already computed prefixes (evaluation
// only): one kernel body behind two entries that differ in how a query row is numbered and addressed.
//
// The scoring heads run every (video, candidate) pair as its own decoder sequence; the first P rows of all candidates of one
// video are identical (query features + the common token prefix), so their K/V are computed once per video (the prefix pass)
// and each candidate runs only its own rows.  A query row attends to the P prefix keys of its group and to the keys of its own
// continuation that are not behind it: one softmax over both sets.
//
//   mpv_attn_prefix_fwd          UNIFORM: every continuation has Lc rows and every group (but a short last one) group_size
//                                continuations, each at its own address (x_cs).  The rows of a group are numbered as if stacked end
//                                to end from the group's first continuation: row r = local continuation r / Lc, row r % Lc.
//   mpv_attn_prefix_packed_fwd   PACKED: continuations have their own lengths and groups their own numbers of them; all rows lie end
//                                to end in one [rows] array and are numbered by their place in it.  Two index arrays describe the
//                                packing: seg_start[r], the first row of the continuation row r belongs to (seg_start[r] <= r), and
//                                group_row[g], the first row of group g (group_row[n_groups] == rows).
//
// Those two -- where row r's own keys begin, and how a row number becomes an address -- are the whole difference (the `PACKED`
// branches below); in both numberings a group is one contiguous range of rows and a continuation one contiguous range inside it.
//
// Layout: a workgroup = 4 waves = 128 consecutive rows of one (group, head), so that every prefix K/V chunk brought into LDS serves
// all of them -- with continuations of a few rows (category names) per-continuation tiles would leave the MFMA tiles mostly empty.
// Phase 1 streams the prefix (dense for every row); phase 2 streams the own keys the workgroup can see, from the first key of its
// first row's continuation (a continuation may straddle a workgroup edge: the second workgroup's stream starts inside the first's
// rows) to its last row: key kr is visible to row r iff first_key(r) <= kr <= r.  Both phases are stream_phase(); the prefix is
// the stream whose window covers everything.  Tile arithmetic: prefix_tile.h (S^T = K Q^T on mfma_f32_32x32x16_bf16, online softmax
// in fp32, probabilities rounded to bf16 for the PV product, one division at the end).  A masked key is a true no-op: its score is
// -inf before the running max and its probability exp(-inf) = 0 exactly, so a row's result depends on its group's prefix, on its
// own continuation and on nothing else -- and the two entries, which cut a group into the same tiles, agree bit for bit on a
// uniform problem.
#include <string.h>

#include "mpv_common.h"
#include "prefix_tile.h"
#include "../../include/mpv.h"

namespace {

constexpr int PCH = 64;                 // key rows per LDS chunk
constexpr int PCHUNK = PCH * PROWB;
constexpr int PWAVES = 4;
constexpr int PROWS = PWAVES * 32;      // query rows per workgroup
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

// The chunk loop: stream ks through the two LDS buffers (the next chunk's global loads in flight under this chunk's tiles) and
// update this wave's rows with every 32-key tile inside its window.  Every wave stages; only an `active` one (it has rows) computes.
template <int HD, bool SEG, class Visible>
__device__ __forceinline__ void stream_phase(char* smem, const KeyStream& ks, int tid, int lane, bool active,
                                             const bf16x8 (&qf)[HD / 16], float sc, float& m, float& l, f32x16 (&oacc)[(HD + 31) / 32],
                                             Visible visible) {
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
        ptile_update<HD>(kl, kl + PCHUNK, kt, key0, qf, sc, m, l, oacc, lane, visible);
      }
    }
    if (c + 1 < nchunk) {
      sk_.commit(smem + (cur ^ 1) * 2 * PCHUNK, tid);
      sv_.commit(smem + (cur ^ 1) * 2 * PCHUNK + PCHUNK, tid);
    }
    __syncthreads();
  }
}

template <int HD, bool PACKED>
__global__ __launch_bounds__(PTHREADS, 2) void attn_prefix_fwd_kernel(const PrefixArgs p) {
  constexpr int NS = HD / 16;
  constexpr int NDT = (HD + 31) / 32;
  __shared__ __attribute__((aligned(16))) char smem[4 * PCHUNK];     // [buf][K|V]
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
  }
}

// An entry's own side of its descriptor: its index pointers, then (map_args) its shape tests, the row map's fields of PrefixArgs,
// the number of rows the kernel indexes (`span`) and the rows of the largest group, which size the grid.
bool map_pointers(const mpv_attn_prefix_desc*) { return true; }
bool map_pointers(const mpv_attn_prefix_packed_desc* d) { return d->seg_start && d->group_row; }

int map_args(const mpv_attn_prefix_desc* d, PrefixArgs& a, long long& span, long long& group_rows) {
  MPV_REQUIRE(d->n_cont > 0 && d->group_size > 0 && d->heads > 0 && d->cont_len > 0 && d->prefix_len >= 0, MPV_E_SHAPE,
              "mpv_attn_prefix_fwd: empty problem (n_cont %d, group_size %d, heads %d, cont_len %d, prefix_len %d)", d->n_cont,
              d->group_size, d->heads, d->cont_len, d->prefix_len);
  MPV_REQUIRE(d->n_groups == (d->n_cont + d->group_size - 1) / d->group_size, MPV_E_SHAPE,
              "mpv_attn_prefix_fwd: n_groups %d must be ceil(n_cont %d / group_size %d)", d->n_groups, d->n_cont, d->group_size);
  a.q_cs = d->q_cs; a.k_cs = d->k_cs; a.v_cs = d->v_cs; a.o_cs = d->o_cs;
  a.n_cont = d->n_cont;
  a.group_size = d->group_size;
  a.lc = d->cont_len;
  span = group_rows = (long long)d->group_size * d->cont_len;
  return MPV_OK;
}

int map_args(const mpv_attn_prefix_packed_desc* d, PrefixArgs& a, long long& span, long long& group_rows) {
  MPV_REQUIRE(d->rows >= 1 && d->n_groups >= 1 && d->heads >= 1 && d->prefix_len >= 0, MPV_E_SHAPE,
              "mpv_attn_prefix_packed_fwd: empty problem (rows %d, n_groups %d, heads %d, prefix_len %d)", d->rows, d->n_groups,
              d->heads, d->prefix_len);
  MPV_REQUIRE(d->max_group_rows >= 1 && d->max_group_rows <= d->rows, MPV_E_SHAPE,
              "mpv_attn_prefix_packed_fwd: max_group_rows %d must lie in [1, rows %d]", d->max_group_rows, d->rows);
  a.seg_start = d->seg_start;
  a.group_row = d->group_row;
  span = d->rows;
  group_rows = d->max_group_rows;
  return MPV_OK;
}

// Everything the two entries have in common: the tests (the entry's own shape tests take their place between the head_dim test and
// the grid limits, so the first fault named is the same whichever entry meets it), the copy into PrefixArgs and the launch.
// `index_arrays` finishes the pointer-alignment message, the one text whose ending is the entry's own.
template <bool PACKED, class Desc>
int prefix_fwd(const char* name, const char* index_arrays, const Desc* d, hipStream_t stream) {
  MPV_REQUIRE(d && d->q && d->k && d->v && d->o && map_pointers(d) && (d->prefix_len == 0 || (d->pk && d->pv)), MPV_E_ARG,
              "%s: null pointer", name);
  MPV_REQUIRE(d->head_dim == 64 || d->head_dim == 80, MPV_E_SHAPE, "%s: head_dim %d is not supported (64: the 1.3B decoder, 80: 2.7B)",
              name, d->head_dim);
  PrefixArgs a = {};
  long long span, group_rows;
  if (const int rc = map_args(d, a, span, group_rows)) return rc;
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
  const long long st[] = {a.q_cs, a.q_hs, a.q_rs, a.k_cs, a.k_hs, a.k_rs, a.v_cs, a.v_hs, a.v_rs,
                          a.pk_gs, a.pk_hs, a.pk_rs, a.pv_gs, a.pv_hs, a.pv_rs};
  bool al = true;
  for (long long s : st) al = al && (s % 8 == 0);
  MPV_REQUIRE(al && a.o_cs % 4 == 0 && a.o_hs % 4 == 0 && a.o_rs % 4 == 0, MPV_E_ALIGN,
              "%s: strides must keep q/k/v/pk/pv rows 16-byte and o rows 8-byte aligned", name);
  MPV_REQUIRE((((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.pk | (uintptr_t)a.pv) & 15) == 0 &&
                  ((uintptr_t)a.o & 7) == 0 && (((uintptr_t)a.seg_start | (uintptr_t)a.group_row) & 3) == 0,
              MPV_E_ALIGN, "%s: q/k/v/pk/pv must be 16-byte aligned, o 8-byte%s", name, index_arrays);
  MPV_REQUIRE(a.scale > 0.f, MPV_E_ARG, "%s: scale must be positive", name);
  const dim3 grid((unsigned)((group_rows + PROWS - 1) / PROWS), (unsigned)d->heads, (unsigned)d->n_groups);
  if (d->head_dim == 64)
    hipLaunchKernelGGL((attn_prefix_fwd_kernel<64, PACKED>), grid, dim3(PTHREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((attn_prefix_fwd_kernel<80, PACKED>), grid, dim3(PTHREADS), 0, stream, a);
  return mpv_check_launch(name);
}

}  // namespace

extern "C" int mpv_attn_prefix_fwd(const mpv_attn_prefix_desc* d, hipStream_t stream) {
  return prefix_fwd<false>("mpv_attn_prefix_fwd", " aligned", d, stream);
}

extern "C" int mpv_attn_prefix_packed_fwd(const mpv_attn_prefix_packed_desc* d, hipStream_t stream) {
  return prefix_fwd<true>("mpv_attn_prefix_packed_fwd", ", the index arrays 4-byte", d, stream);
}

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
