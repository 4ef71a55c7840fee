// search_common.h -- the one definition of what the fused search kernels share (retrieval_search.hip: mpv_sim_*, maxsim_search.hip:
// mpv_maxsim_*): the 32 x 32 MFMA tile walk (register stage, LDS stage, resident tile), the order rule, the per-lane sorted list
// and the rank-mode bookkeeping in LDS.  Every stream and target-score kernel of both files stages its rows and multiplies them
// through THESE functions -- same operand roles, same k order (chunks of 128 ascending, 16 per MFMA), same instruction -- and an
// MFMA output element is a function of its A row, its B column and the accumulator only.  That is what the bit-identity claims
// of both files (a target's score equals the stream's score of the same row; mpv_maxsim_* with both groups 1 equals mpv_sim_*)
// rest on.  The host-side checks live once in search_common.hip, the slice merge and rank finish kernels in retrieval_search.hip.
#pragma once
#include "mpv_common.h"
#include "fp8_deq.h"

namespace {

constexpr int SC_TILE = 32;             // rows of a tile: resident rows (queries) per workgroup, streamed rows per wave and step
constexpr int SC_WAVES = 4;
constexpr int SC_KC = 128;              // k per staged chunk
constexpr int SC_PITCH = SC_KC + 8;     // bf16 elements: 272 bytes, rows 4 banks apart
constexpr int SC_UNITS = SC_TILE * SC_KC / 8 / 64;   // 16-byte units per lane and chunk (8)
constexpr int SC_NONE = 0x7fffffff;     // index of an empty list entry (at most 2^31 - 1 rows, so no row has it)
constexpr int SC_MAX_K = 32, SC_MAX_T = 32, SC_MAX_SLICES = 4096;
constexpr int SC_MERGE_CACHE = 6144;    // workspace entries per query that the merge kernel keeps in LDS

// Order rule: (v, g) beats (bv, bg) iff v > bv or (v == bv and g < bg).  Indices are distinct, so it is a total order; a NaN
// beats nothing.
__device__ __forceinline__ bool sc_better(float v, int g, float bv, int bg) { return v > bv || (v == bv && g < bg); }

struct ScStage {
  bf16x8 r[SC_UNITS];
};

// 32 rows x 128 k of the streamed side -> registers.  row_of(j) is the row staged as tile row j, or < 0 for a row of zeros.
template <class RowFn>
__device__ __forceinline__ void sc_stage_load(ScStage& st, const bf16* __restrict__ S, long long s_rs, int k0, int D, RowFn row_of,
                                              int lane) {
#pragma unroll
  for (int j = 0; j < SC_UNITS; ++j) {
    const int u = j * 64 + lane, row = u >> 4, k = k0 + (u & 15) * 8;
    const long long gr = row_of(row);
    bf16x8 v = {};
    if (gr >= 0 && k < D) v = *(const bf16x8*)(S + gr * s_rs + k);
    st.r[j] = v;
  }
}
__device__ __forceinline__ void sc_stage_store(const ScStage& st, bf16* buf, int lane) {
#pragma unroll
  for (int j = 0; j < SC_UNITS; ++j) {
    const int u = j * 64 + lane;
    *(bf16x8*)(buf + (u >> 4) * SC_PITCH + (u & 15) * 8) = st.r[j];
  }
}
// ---- the streamed side as e4m3fn codes (the *_q8 entries; include/mpv.h, "Searches over an FP8 gallery") ----------------------
// Only the way INTO the LDS stage differs: a lane loads 16-byte chunks of 16 codes (a 32 x 128 chunk is 4 units per lane, not 8)
// and turns them into bf16 with the exact deq_pair on the way to the stage, so the stage holds what ScStage would have put there
// for the bf16 gallery deq(code) -- same layout, same sc_tile_mma, bit-identical accumulators.  The fp32 scale of tile row j
// travels with the chunk (lane j loads it) and is parked in the 16 spare bytes that SC_PITCH leaves behind row j's 128 elements,
// which neither stage store nor sc_tile_mma touches: it is read back when the tile's scores are finished, after the register
// stage has already moved on to the next tile.
struct ScCodes {
  const uint8_t* c;          // codes, row stride counted in codes (a multiple of 16)
  const float* scale;        // one per row
};
struct ScCodeStage {
  i32x4 r[SC_UNITS / 2];
  float scale;               // of tile row lane & 31
};
template <class RowFn>
__device__ __forceinline__ void sc_stage_load(ScCodeStage& st, ScCodes S, long long s_rs, int k0, int D, RowFn row_of, int lane) {
#pragma unroll
  for (int j = 0; j < SC_UNITS / 2; ++j) {
    const int u = j * 64 + lane, row = u >> 3, k = k0 + (u & 7) * 16;
    const long long gr = row_of(row);
    i32x4 v = {};                                    // code 0 is +0.0
    if (gr >= 0 && k < D) v = *(const i32x4*)(S.c + gr * s_rs + k);
    st.r[j] = v;
  }
  const long long sr = row_of(lane & 31);
  st.scale = sr >= 0 ? S.scale[sr] : 1.f;
}
__device__ __forceinline__ void sc_stage_store(const ScCodeStage& st, bf16* buf, int lane) {
#pragma unroll
  for (int j = 0; j < SC_UNITS / 2; ++j) {
    const int u = j * 64 + lane;
    Frag lo, hi;
    deq_chunk(st.r[j], lo, hi);
    bf16* p = buf + (u >> 3) * SC_PITCH + (u & 7) * 16;
    *(bf16x8*)p = lo.b;
    *(bf16x8*)(p + 8) = hi.b;
  }
  if (lane < SC_TILE) *(float*)(buf + lane * SC_PITCH + SC_KC) = st.scale;
}
// what a kernel stages a source through, and whether its scores carry a row scale
template <class Src>
struct ScSource;
template <>
struct ScSource<const bf16*> {
  using Stage = ScStage;
  static constexpr bool scaled = false, prior = false;
};
template <>
struct ScSource<ScCodes> {
  using Stage = ScCodeStage;
  static constexpr bool scaled = true, prior = false;
};
// ---- a streamed side with one fp32 additive term per row (the *_prior entries; include/mpv.h, "Searches with per-row priors") ----
// Either source above plus `prior`: the term of tile row j travels with the chunk exactly as a code row's scale does (lane j loads
// it) and is parked 4 bytes behind the scale's slot in the 16 spare bytes of the row's pitch.  A row of zeros has the term 0.
template <class Src>
struct ScPrior {
  Src s;
  const float* prior;        // one per row
};
template <class Stage>
struct ScPriorStage {
  Stage s;
  float prior;               // of tile row lane & 31
};
template <class Src, class RowFn>
__device__ __forceinline__ void sc_stage_load(ScPriorStage<typename ScSource<Src>::Stage>& st, ScPrior<Src> S, long long s_rs, int k0,
                                              int D, RowFn row_of, int lane) {
  sc_stage_load(st.s, S.s, s_rs, k0, D, row_of, lane);
  const long long pr = row_of(lane & 31);
  st.prior = pr >= 0 ? S.prior[pr] : 0.f;
}
template <class Stage>
__device__ __forceinline__ void sc_stage_store(const ScPriorStage<Stage>& st, bf16* buf, int lane) {
  sc_stage_store(st.s, buf, lane);
  if (lane < SC_TILE) *(float*)(buf + lane * SC_PITCH + SC_KC + 2) = st.prior;
}
template <class Src>
struct ScSource<ScPrior<Src>> {
  using Stage = ScPriorStage<typename ScSource<Src>::Stage>;
  static constexpr bool scaled = ScSource<Src>::scaled, prior = true;
};
// the term parked with staged tile row `row`
__device__ __forceinline__ float sc_row_prior(const bf16* sbuf, int row) { return *(const float*)(sbuf + row * SC_PITCH + SC_KC + 2); }
// fl(fl(scale * s) + prior): two separately rounded fp32 operations, never contracted into a fused multiply-add, so that a plain
// fp32 restatement reproduces a score bit for bit from its accumulator
__device__ __forceinline__ float sc_prior_score(float s, float scale, float prior) {
#pragma clang fp contract(off)
  const float m = s * scale;
  return m + prior;
}
// A score with a term is eligible iff it is neither NaN nor -inf: -inf is how a row is left out.
__device__ __forceinline__ bool sc_eligible(float v) { return v > -INFINITY; }
// the scale parked with staged tile row `row`
__device__ __forceinline__ float sc_row_scale(const bf16* sbuf, int row) { return *(const float*)(sbuf + row * SC_PITCH + SC_KC); }
// acc[i] *= the scale of its row (sc_tile_mma below: row 8 (i / 4) + 4 (lane / 32) + i % 4), in fp32: the first thing a kernel
// does with a finished tile of codes, before any comparison or max sees a score
__device__ __forceinline__ void sc_scale_acc(f32x16& acc, const bf16* sbuf, int lane) {
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] *= sc_row_scale(sbuf, 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3));
}
// acc[i] += <staged row 8 (i / 4) + 4 (lane / 32) + i % 4, resident row lane & 31> over `ksteps` 16-wide steps
__device__ __forceinline__ void sc_tile_mma(f32x16& acc, const bf16* sbuf, const bf16* rrow, int ksteps, int lane) {
  const bf16* ap = sbuf + (lane & 31) * SC_PITCH + 8 * (lane >> 5);
  const bf16* bp = rrow + 8 * (lane >> 5);
  for (int kk = 0; kk < ksteps; ++kk)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(ap + kk * 16), *(const bf16x8*)(bp + kk * 16), acc, 0, 0, 0);
}
// 32 resident rows (row_of(j), or zeros when < 0) -> LDS at pitch D + 8
template <class RowFn>
__device__ __forceinline__ void sc_load_resident(bf16* rbuf, const bf16* __restrict__ R, long long r_rs, int D, RowFn row_of, int tid,
                                                 int nthreads) {
  const int upr = D >> 3;
  for (int u = tid; u < SC_TILE * upr; u += nthreads) {
    const int row = u / upr, c = (u - row * upr) * 8;
    const long long gr = row_of(row);
    bf16x8 v = {};
    if (gr >= 0) v = *(const bf16x8*)(R + gr * r_rs + c);
    *(bf16x8*)(rbuf + row * (D + 8) + c) = v;
  }
}
// the same from codes: the resident tile holds the bf16 rows bf16(deq(code) * scale) (round to nearest even; exact for the
// power-of-two scales of mpv_quantize_rows_e4m3), so whatever multiplies against it is what the bf16 entry computes on those rows
template <class RowFn>
__device__ __forceinline__ void sc_load_resident(bf16* rbuf, ScCodes R, long long r_rs, int D, RowFn row_of, int tid, int nthreads) {
  const int upr = D >> 4;
  for (int u = tid; u < SC_TILE * upr; u += nthreads) {
    const int row = u / upr, c = (u - row * upr) * 16;
    const long long gr = row_of(row);
    i32x4 v = {};
    float sc = 1.f;
    if (gr >= 0) {
      v = *(const i32x4*)(R.c + gr * r_rs + c);
      sc = R.scale[gr];
    }
    Frag lo, hi;
    deq_chunk(v, lo, hi);
    *(bf16x8*)(rbuf + row * (D + 8) + c) = cvt8(cvt8(lo.b) * sc);
    *(bf16x8*)(rbuf + row * (D + 8) + c + 8) = cvt8(cvt8(hi.b) * sc);
  }
}

// Sorted (descending) list of the k <= KMAX best (value, index) pairs seen by one lane, in registers.  The list sits in the LAST k
// slots, so the k-th entry -- what a candidate has to beat -- is always slot KMAX - 1; the slots before it hold (+inf, -1), which
// nothing beats.  Every loop is unrolled over KMAX with static indices (no scratch); an insertion is 3 VALU ops per slot.
// The kernels write the last k slots out (to LDS, to the workspace) with loops of their own, in the kernel body: reached through a
// function, the same loops make the compiler lay the whole top-k kernel out anew (other register count, other occupancy).
template <int KMAX>
struct TopList {
  float v[KMAX];
  int g[KMAX];
  __device__ __forceinline__ void init(int k) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      v[j] = j < KMAX - k ? INFINITY : -INFINITY;
      g[j] = j < KMAX - k ? -1 : SC_NONE;
    }
  }
  __device__ __forceinline__ bool beats(float cv, int cg) const { return sc_better(cv, cg, v[KMAX - 1], g[KMAX - 1]); }
  // precondition: beats(cv, cg).  Slot j takes its upper neighbour when the candidate belongs above that, the candidate when
  // it belongs exactly here, and stays otherwise; walking up the list, "candidate beats slot j" is the previous step's `up`.
  __device__ __forceinline__ void insert(float cv, int cg) {
    bool below = true;
#pragma unroll
    for (int j = KMAX - 1; j > 0; --j) {
      const bool up = sc_better(cv, cg, v[j - 1], g[j - 1]);
      v[j] = up ? v[j - 1] : (below ? cv : v[j]);
      g[j] = up ? g[j - 1] : (below ? cg : g[j]);
      below = up;
    }
    v[0] = below ? cv : v[0];
    g[0] = below ? cg : g[0];
  }
};

// Rank mode: the targets of the workgroup's 32 queries ([32][n_t]: score, index or -1, count) parked in LDS.  `nq` queries,
// targets valid in [0, ng).  A barrier has to pass before the arrays are read.
struct ScRankLds {
  float* tv;
  int *ti, *cnt;
};
__device__ __forceinline__ ScRankLds sc_rank_park(char* lds, const int64_t* target, const float* tscore, int q0, int nq, int ng,
                                                  int n_t, int tid, int nthreads) {
  ScRankLds r;
  r.tv = (float*)lds;
  r.ti = (int*)(r.tv + SC_TILE * n_t);
  r.cnt = r.ti + SC_TILE * n_t;
  for (int j = tid; j < SC_TILE * n_t; j += nthreads) {
    const int q = q0 + j / n_t;
    long long t = -1;
    if (q < nq) t = target[(long long)q * n_t + (j % n_t)];
    const bool ok = t >= 0 && t < ng;
    r.ti[j] = ok ? (int)t : -1;
    r.tv[j] = ok ? tscore[(long long)q * n_t + (j % n_t)] : 0.f;
    r.cnt[j] = 0;
  }
  return r;
}
// the workgroup's counts -> counts[nq][n_t]: one global integer atomic per (query, target) that counted anything
__device__ __forceinline__ void sc_rank_flush(const int* cnt, int* counts, int q0, int nq, int n_t, int tid, int nthreads) {
  for (int j = tid; j < SC_TILE * n_t; j += nthreads) {
    const int q = q0 + j / n_t;
    if (q < nq && cnt[j] > 0) atomicAdd(&counts[(long long)q * n_t + (j % n_t)], cnt[j]);
  }
}

}  // namespace

// ---- host side, shared by the entry points of both files and internal to the library: search_common.hip ------------------------
#define SC_HIDDEN __attribute__((visibility("hidden")))
// dim, row strides, operand alignment and slice count of a search descriptor (`what` names the entry point in the error text)
SC_HIDDEN int sc_check_desc(const char* what, const void* queries, const void* gallery, int dim, long long q_rs, long long g_rs,
                            int slices);
// what a gallery of e4m3 codes adds to that: the scales exist, g_rs (in codes) is a multiple of 16, the base is 16-byte aligned
SC_HIDDEN int sc_check_codes(const char* what, const void* gallery, long long g_rs, const float* g_scale);
// The workspace of every entry point is two arrays of n 4-byte entries, each padded to 256 bytes.
SC_HIDDEN size_t sc_ws_bytes(size_t n);
SC_HIDDEN int sc_ws_check(const char* what, const void* ws, size_t ws_bytes, size_t n);      // size and alignment
SC_HIDDEN void* sc_ws_upper(void* ws, size_t n);                                               // the second array
// dynamic LDS of a stream kernel: resident tile + one stage per wave + tail; more than 48 KiB needs the opt-in
SC_HIDDEN size_t sc_stream_lds(int D, int waves, size_t tail);
SC_HIDDEN void sc_allow_lds(const void* kernel, size_t lds);
// ---- retrieval_search.hip: launchers of the two kernels both files end with -----------------------------------------------------
// sim_topk_merge_kernel: workspace [slices][nq][k] -> vals, idx [nq][k]
SC_HIDDEN int sc_merge_slices(const char* what, const float* ws_val, const int* ws_idx, float* vals, int64_t* idx, int nq, int k,
                              int slices, hipStream_t stream);
// sim_rank_finish_kernel: rank[q] = smallest count among the valid targets, ng when there is none.  With `tscore` a target whose
// score is NaN is no target (mpv_maxsim_rank); with null every index in [0, ng) counts (mpv_sim_rank).
SC_HIDDEN int sc_rank_finish(const char* what, const int64_t* target, const float* tscore, const int* counts, int* rank, int nq,
                             int n_t, int ng, hipStream_t stream);
