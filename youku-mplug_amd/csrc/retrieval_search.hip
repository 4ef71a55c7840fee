// Retrieval search over L2-normalised feature rows (the ITC model's evaluation, downstream/run_retrieval_distributed_gpt3.py:
// 245-339): similarity + selection fused, the score matrix never reaches memory.
//
//   mpv_sim_topk   the k best gallery rows per query: (scale * <q, g>, g), descending, ties to the LOWER gallery index.
//   mpv_sim_rank   per query the best rank among its target rows; rank(t) = #{g : s(g) > s(t) or (s(g) == s(t) and g < t)}.
//
// One streaming kernel serves both.  A workgroup (4 waves) owns 32 queries and one slice of the gallery.  The query tile is
// copied to LDS once and stays there.  The gallery is walked in super-tiles of 128 rows, wave w taking rows 32 w .. 32 w + 31:
// each wave copies its 32 rows x 128 k chunk with coalesced 16-byte loads into registers one step ahead (the loads of step
// s + 1 are in flight while step s computes), parks it in its own LDS stage (272-byte pitch: conflict-free ds_read_b128) and
// runs v_mfma_f32_32x32x16_bf16 with A = gallery rows, B = queries: a lane ends up with 16 scores of ONE query (lane & 31).
//   top-k: every lane keeps a sorted list of the k best (value, index) pairs it has seen, in registers (TopList: unrolled and
//     predicated, no dynamic indexing).  A score only touches the list when it beats the k-th entry: expected k ln(N / k)
//     insertions per list over a stream of N rows, 3 VALU ops per slot each.  The 8 lists of a query (4 waves x 2 lane
//     halves) are merged at the end, the slice's list goes to the workspace and the merge kernel (one workgroup per query, k
//     rounds of "best entry that is worse than the last one written") combines the slices.
//   rank: the target scores sit in LDS; every score is compared with every target of its query and the counts are added up
//     with integer adds (LDS, then one global atomic add per (query, target) and workgroup): order-independent.
// Order rule: (v, g) beats (bv, bg) iff v > bv or (v == bv and g < bg).  Gallery indices are distinct, so the rule is a total
// order and the result cannot depend on the slice count, the wave that saw a row, or the order of the merges.  NaN scores
// beat nothing and are never returned.
//
// The tile walk (sc_stage_*, sc_tile_mma, sc_load_resident), the order rule, TopList and the rank bookkeeping are defined once,
// in search_common.h, for this file and maxsim_search.hip; the common host checks are in search_common.hip.  The slice merge
// (sim_topk_merge_kernel) and the rank finish (sim_rank_finish_kernel) below serve both files through sc_merge_slices /
// sc_rank_finish.
//
// Self-consistency of s(g) > s(t) in mpv_sim_rank: the target scores are produced by sim_target_kernel, which stages the 32
// target rows of a query tile through the stream's own sc_stage_* / sc_tile_mma -- same operand roles, same k order (chunks
// of 128 ascending, 16 per MFMA), same instruction, accumulator zeroed at the same point -- and reads the diagonal of the
// 32 x 32 tile.  An MFMA output element is a function of its A row, its B column and the accumulator only, so the score of
// target row t is bit-identical to the score the stream computes when it meets row t.
//
// mpv_sim_topk_q8 / mpv_sim_rank_q8 (include/mpv.h, "Searches over an FP8 gallery") are the same two kernel bodies instantiated on
// a gallery of e4m3 codes with one fp32 scale per row (search_common.h, ScCodes / ScCodeStage): the codes become bf16 on the way
// into the LDS stage, so the accumulators are those of the bf16 kernel on deq(code), and the row scale multiplies a finished score
// before anything compares it.
#include "search_common.h"
#include "../../include/mpv.h"

namespace {

constexpr int RS_SUPER = SC_WAVES * SC_TILE;      // gallery rows per workgroup and step

struct RsArgs {
  const bf16 *Q, *G;
  long long q_rs, g_rs;
  int nq, ng, D, k, n_t;
  int per_slice;             // super-tiles per slice
  float scale;
  float* ws_val;             // top-k: [slices][nq][k]
  int* ws_idx;
  const int64_t* target;     // rank: [nq][n_t]
  const float* tscore;       // rank: [nq][n_t]
  int* counts;               // rank: [nq][n_t], zeroed
  const float* g_scale;      // *_q8: G points to e4m3 codes, g_rs counts codes, one scale per gallery row
  const float* g_prior;      // *_prior: one additive term per gallery row; the score is fl(fl(scale * s) + g_prior[g])
};

// The stream, written once over the gallery's source type: bf16 rows (sim_stream_kernel) or e4m3 codes with row scales
// (q8_stream_kernel), which differ in how a chunk reaches the LDS stage and in one fp32 multiplication per finished score.
template <int MODE, int KMAX, class Src>        // MODE 0: top-k (k <= KMAX), 1: rank counts
__device__ __forceinline__ void sim_stream_body(const RsArgs& a, const Src G) {
  extern __shared__ __attribute__((aligned(16))) char rs_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
  const int D = a.D, qpitch = D + 8;
  bf16* qbuf = (bf16*)rs_smem;
  bf16* gbuf = qbuf + SC_TILE * qpitch + wave * (SC_TILE * SC_PITCH);
  char* tail = rs_smem + (size_t)(SC_TILE * qpitch + SC_WAVES * SC_TILE * SC_PITCH) * sizeof(bf16);
  const int q0 = blockIdx.y * SC_TILE, slice = blockIdx.x;
  const long long s_row0 = (long long)slice * a.per_slice * RS_SUPER;
  long long s_end = s_row0 + (long long)a.per_slice * RS_SUPER;
  if (s_end > a.ng) s_end = a.ng;
  const unsigned uend = (unsigned)s_end;
  const int n_super = s_row0 < s_end ? (int)((s_end - s_row0 + RS_SUPER - 1) / RS_SUPER) : 0;

  TopList<KMAX> top;         // top-k: this lane's list (its query is lane & 31; lanes l and l ^ 32 see different rows of it)
  ScRankLds rk = {};         // rank: target scores [32][n_t], target rows, counts, in LDS
  if (MODE == 0)
    top.init(a.k);
  else
    rk = sc_rank_park(tail, a.target, a.tscore, q0, a.nq, a.ng, a.n_t, tid, 64 * SC_WAVES);
  sc_load_resident(qbuf, a.Q, a.q_rs, D, [&](int j) -> long long { return q0 + j < a.nq ? q0 + j : -1; }, tid, 64 * SC_WAVES);

  const int nk = (D + SC_KC - 1) / SC_KC;
  const int nsteps = n_super * nk;
  const bf16* qrow = qbuf + l32 * qpitch;
  typename ScSource<Src>::Stage st;
  long long row0 = s_row0 + wave * SC_TILE;
  auto rows = [&](long long r0) { return [=](int j) -> long long { return r0 + j < s_end ? r0 + j : -1; }; };
  if (nsteps > 0) sc_stage_load(st, G, a.g_rs, 0, D, rows(row0), lane);
  f32x16 acc = {};
  int kc = 0;
  for (int s = 0; s < nsteps; ++s) {
    sc_stage_store(st, gbuf, lane);
    __syncthreads();                                 // stage (and, first time round, queries / targets) visible
    if (s + 1 < nsteps) {                            // next step's rows fly while this one computes
      const bool wrap = kc + 1 == nk;
      sc_stage_load(st, G, a.g_rs, wrap ? 0 : (kc + 1) * SC_KC, D, rows(wrap ? row0 + RS_SUPER : row0), lane);
    }
    if (kc == 0) acc = f32x16{};
    const int kleft = D - kc * SC_KC;
    sc_tile_mma(acc, gbuf, qrow + kc * SC_KC, (kleft < SC_KC ? kleft : SC_KC) >> 4, lane);
    if (kc + 1 == nk) {
      // acc[i] is gallery row base + 8 (i / 4) + i % 4.  Unsigned: the last super-tile of a gallery of 2^31 - 1 rows runs
      // past INT_MAX; such rows fail g < uend and are never used as an index.
      const unsigned base = (unsigned)row0 + 4 * half;
      if constexpr (ScSource<Src>::scaled) sc_scale_acc(acc, gbuf, lane);
      // with a term the score of both modes is fl(fl(scale * s) + term), and a row that ends up at -inf (or NaN) is not there at all
      auto with_prior = [&](float s, int i) { return sc_prior_score(s, a.scale, sc_row_prior(gbuf, 8 * (i >> 2) + 4 * half + (i & 3))); };
      if (MODE == 0) {
        // one insertion site (the list code is 3 ops x KMAX slots): mark the scores that beat the list, then take them one by one
        unsigned m = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if constexpr (ScSource<Src>::prior)
            acc[i] = with_prior(acc[i], i);
          else
            acc[i] *= a.scale;
          const unsigned g = base + 8 * (i >> 2) + (i & 3);
          bool in = g < uend;
          if constexpr (ScSource<Src>::prior) in = in && sc_eligible(acc[i]);      // (-inf, g) would beat the list's filler
          m |= (in && top.beats(acc[i], (int)g)) ? 1u << i : 0u;
        }
        while (m) {                                  // rare once the list has settled
          const int i = __builtin_ctz(m);
          m &= m - 1;
          float v = acc[0];
#pragma unroll
          for (int e = 1; e < 16; ++e) v = i == e ? acc[e] : v;
          const int g = (int)(base + 8 * (i >> 2) + (i & 3));
          if (top.beats(v, g)) top.insert(v, g);          // the threshold may have risen since the marking
        }
      } else {
        if constexpr (ScSource<Src>::prior) {
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[i] = with_prior(acc[i], i);
        }
        for (int t = 0; t < a.n_t; ++t) {
          const int tg = rk.ti[l32 * a.n_t + t];
          const float ts = rk.tv[l32 * a.n_t + t];
          int c = 0;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const unsigned g = base + 8 * (i >> 2) + (i & 3);
            c += (g < uend && sc_better(acc[i], (int)g, ts, tg)) ? 1 : 0;
          }
          if (tg >= 0 && c > 0) atomicAdd(&rk.cnt[l32 * a.n_t + t], c);
        }
      }
      kc = 0;
      row0 += RS_SUPER;
    } else {
      ++kc;
    }
    __syncthreads();                                 // every wave is done with its stage before the next store
  }
  __syncthreads();
  if (MODE == 0) {
    // 8 lists per query (4 waves x 2 halves) -> 1, through LDS ([wave][k][32]) in two rounds: the upper half of each wave hands
    // its list to the lower half, then waves 1-3 hand theirs to wave 0.  A sorted list stops contributing at its first entry
    // that fails.  (The write-out loops stay in the kernel body: search_common.h, TopList.)
    const int k = a.k;
    float* lv = (float*)tail;
    int* li = (int*)(lv + SC_WAVES * k * 32);
    auto put = [&]() {
#pragma unroll
      for (int j = 0; j < KMAX; ++j)
        if (j >= KMAX - k) {
          lv[(wave * k + j - (KMAX - k)) * 32 + l32] = top.v[j];
          li[(wave * k + j - (KMAX - k)) * 32 + l32] = top.g[j];
        }
    };
    auto absorb = [&](int w) {
      for (int j = 0; j < k; ++j) {
        const float cv = lv[(w * k + j) * 32 + l32];
        const int cg = li[(w * k + j) * 32 + l32];
        if (cg == SC_NONE || !top.beats(cv, cg)) break;
        top.insert(cv, cg);
      }
    };
    if (half == 1) put();
    __syncthreads();
    if (half == 0) absorb(wave);
    __syncthreads();
    if (half == 0 && wave > 0) put();
    __syncthreads();
    if (wave == 0 && half == 0) {
      for (int w = 1; w < SC_WAVES; ++w) absorb(w);
      if (q0 + l32 < a.nq) {
        const long long o = ((long long)slice * a.nq + q0 + l32) * k;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
          if (j >= KMAX - k) {
            a.ws_val[o + j - (KMAX - k)] = top.v[j];
            a.ws_idx[o + j - (KMAX - k)] = top.g[j];
          }
      }
    }
  } else {
    sc_rank_flush(rk.cnt, a.counts, q0, a.nq, a.n_t, tid, 64 * SC_WAVES);
  }
}

// The mangled names of the bf16 kernels are what the resource gate of the ISA test knows them by, so they keep their template
// heads; the instances over codes are named apart.
template <int MODE, int KMAX>
__global__ __launch_bounds__(64 * SC_WAVES) void sim_stream_kernel(RsArgs a) {
  sim_stream_body<MODE, KMAX>(a, a.G);
}
template <int MODE, int KMAX>
__global__ __launch_bounds__(64 * SC_WAVES) void q8_stream_kernel(RsArgs a) {
  sim_stream_body<MODE, KMAX>(a, ScCodes{(const uint8_t*)a.G, a.g_scale});
}
// the instances with a per-row term (mpv_sim_*_prior, mpv_sim_*_prior_q8)
template <int MODE, int KMAX>
__global__ __launch_bounds__(64 * SC_WAVES) __attribute__((amdgpu_waves_per_eu(KMAX == 16 ? 3 : 1))) void pri_stream_kernel(RsArgs a) {
  sim_stream_body<MODE, KMAX>(a, ScPrior<const bf16*>{a.G, a.g_prior});
}
template <int MODE, int KMAX>
__global__ __launch_bounds__(64 * SC_WAVES) void pri8_stream_kernel(RsArgs a) {
  sim_stream_body<MODE, KMAX>(a, ScPrior<ScCodes>{ScCodes{(const uint8_t*)a.G, a.g_scale}, a.g_prior});
}

// Scores of the target rows, through the stream's staging and MFMA functions: one wave = 32 queries x target slot t, tile row j
// is the target row of query j, the score is the tile's diagonal.
template <class Src>
__device__ __forceinline__ void sim_target_body(const RsArgs& a, const Src G, float* __restrict__ tscore) {
  extern __shared__ __attribute__((aligned(16))) char rs_smem[];
  const int lane = threadIdx.x, l32 = lane & 31, half = lane >> 5;
  const int D = a.D, qpitch = D + 8;
  bf16* qbuf = (bf16*)rs_smem;
  bf16* gbuf = qbuf + SC_TILE * qpitch;
  const int q0 = blockIdx.y * SC_TILE, t = blockIdx.x;
  sc_load_resident(qbuf, a.Q, a.q_rs, D, [&](int j) -> long long { return q0 + j < a.nq ? q0 + j : -1; }, lane, 64);
  auto rows = [&](int j) -> long long {
    if (q0 + j >= a.nq) return -1;
    const long long g = a.target[(long long)(q0 + j) * a.n_t + t];
    return g >= 0 && g < a.ng ? g : -1;
  };
  const int nk = (D + SC_KC - 1) / SC_KC;
  f32x16 acc = {};
  typename ScSource<Src>::Stage st;
  for (int kc = 0; kc < nk; ++kc) {
    sc_stage_load(st, G, a.g_rs, kc * SC_KC, D, rows, lane);
    __syncthreads();                                 // the previous chunk has been consumed
    sc_stage_store(st, gbuf, lane);
    __syncthreads();
    const int kleft = D - kc * SC_KC;
    sc_tile_mma(acc, gbuf, qbuf + l32 * qpitch + kc * SC_KC, (kleft < SC_KC ? kleft : SC_KC) >> 4, lane);
  }
  // tile row l32 sits in acc[4 (l32 / 8) + l32 % 4] of the lane with half == (l32 / 4) % 2
  const int want = 4 * (l32 >> 3) + (l32 & 3);
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) v = i == want ? acc[i] : v;
  if constexpr (ScSource<Src>::scaled) v *= sc_row_scale(gbuf, l32);
  if constexpr (ScSource<Src>::prior) {
    // the stream's own multiply and add; a target that is not eligible is written as NaN, which the stream never counts
    // against and the finish kernel takes for "no target"
    v = sc_prior_score(v, a.scale, sc_row_prior(gbuf, l32));
    v = sc_eligible(v) ? v : __builtin_nanf("");
  }
  if (half == ((l32 >> 2) & 1) && q0 + l32 < a.nq) tscore[(long long)(q0 + l32) * a.n_t + t] = v;
}
__global__ __launch_bounds__(64) void sim_target_kernel(RsArgs a, float* __restrict__ tscore) { sim_target_body(a, a.G, tscore); }
__global__ __launch_bounds__(64) void q8_target_kernel(RsArgs a, float* __restrict__ tscore) {
  sim_target_body(a, ScCodes{(const uint8_t*)a.G, a.g_scale}, tscore);
}
__global__ __launch_bounds__(64) void pri_target_kernel(RsArgs a, float* __restrict__ tscore) {
  sim_target_body(a, ScPrior<const bf16*>{a.G, a.g_prior}, tscore);
}
__global__ __launch_bounds__(64) void pri8_target_kernel(RsArgs a, float* __restrict__ tscore) {
  sim_target_body(a, ScPrior<ScCodes>{ScCodes{(const uint8_t*)a.G, a.g_scale}, a.g_prior}, tscore);
}

// One workgroup per query: k rounds; round j writes the best workspace entry that the entry written in round j - 1 beats.  The
// slices * k entries are copied to LDS first when they fit (SC_MERGE_CACHE; the host's slice choice keeps them fitting), so a
// round is a scan of LDS plus a workgroup reduction by the order rule -- the same answer whichever thread holds which entry.
__global__ __launch_bounds__(256) void sim_topk_merge_kernel(const float* __restrict__ ws_val, const int* __restrict__ ws_idx,
                                                             float* __restrict__ vals, int64_t* __restrict__ idx, int nq, int k,
                                                             int slices) {
  __shared__ float c_v[SC_MERGE_CACHE];
  __shared__ int c_g[SC_MERGE_CACHE];
  __shared__ float r_v[2][4];
  __shared__ int r_g[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  const int n = slices * k;
  const bool cached = n <= SC_MERGE_CACHE;
  auto entry = [&](int e) { return ((long long)(e / k) * nq + q) * k + (e % k); };
  if (cached)
    for (int e = tid; e < n; e += 256) {
      c_v[e] = ws_val[entry(e)];
      c_g[e] = ws_idx[entry(e)];
    }
  __syncthreads();
  float pv = INFINITY;
  int pg = -1;
  for (int j = 0; j < k; ++j) {
    float bv = -INFINITY;
    int bg = SC_NONE;
    for (int e = tid; e < n; e += 256) {
      const float v = cached ? c_v[e] : ws_val[entry(e)];
      const int g = cached ? c_g[e] : ws_idx[entry(e)];
      if (g != SC_NONE && sc_better(pv, pg, v, g) && sc_better(v, g, bv, bg)) {
        bv = v;
        bg = g;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int og = __shfl_xor(bg, off, 64);
      if (sc_better(ov, og, bv, bg)) {
        bv = ov;
        bg = og;
      }
    }
    if (lane == 0) {
      r_v[j & 1][wave] = bv;
      r_g[j & 1][wave] = bg;
    }
    __syncthreads();                                  // double-buffered by round parity: one barrier per round
    bv = r_v[j & 1][0];
    bg = r_g[j & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (sc_better(r_v[j & 1][w], r_g[j & 1][w], bv, bg)) {
        bv = r_v[j & 1][w];
        bg = r_g[j & 1][w];
      }
    if (tid == 0) {
      vals[(long long)q * k + j] = bg == SC_NONE ? -INFINITY : bv;
      idx[(long long)q * k + j] = bg == SC_NONE ? -1 : bg;
    }
    if (bg == SC_NONE) {                              // fewer than k rows in the gallery: the rest is filler (uniform exit)
      for (int r = j + 1 + tid; r < k; r += 256) {
        vals[(long long)q * k + r] = -INFINITY;
        idx[(long long)q * k + r] = -1;
      }
      break;
    }
    pv = bv;
    pg = bg;
  }
}

__global__ __launch_bounds__(256) void sim_rank_finish_kernel(const int64_t* __restrict__ target, const float* __restrict__ tscore,
                                                              const int* __restrict__ counts, int* __restrict__ rank, int nq, int n_t,
                                                              int ng) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  int best = ng;                                      // no target: worse than every real rank
  for (int t = 0; t < n_t; ++t) {
    const long long g = target[(long long)q * n_t + t];
    const int c = counts[(long long)q * n_t + t];
    const float s = tscore ? tscore[(long long)q * n_t + t] : 0.f;
    if (g >= 0 && g < ng && s == s && c < best) best = c;      // a NaN item is ordered after everything: no target to be found
  }
  rank[q] = best;
}

struct RsPlan {
  int qtiles, slices, per_slice;
};

// What a gallery is searched as: `codes`, e4m3 codes with the row scales g_scale (the *_q8 entries), which adds sc_check_codes to
// the checks; `prior`, with the per-row terms g_prior (the *_prior entries), which have to exist and be 4-byte aligned.
struct RsKind {
  bool codes;
  const float* g_scale;
  bool prior;
  const float* g_prior;
};

int rs_plan(const mpv_sim_search_desc* d, RsPlan* p, const char* what, int topk_k = 0, RsKind kind = {}) {
  const bool codes = kind.codes;
  const float* g_scale = kind.g_scale;
  MPV_REQUIRE(d && d->queries && d->gallery, MPV_E_ARG, "%s: null pointer", what);
  MPV_REQUIRE(d->nq > 0 && d->ng > 0 && d->nq <= 65535ll * SC_TILE /* grid.y */ && d->ng <= 0x7fffffffll, MPV_E_SHAPE,
              "%s: bad shape nq=%lld ng=%lld", what, (long long)d->nq, (long long)d->ng);
  int rc = sc_check_desc(what, d->queries, d->gallery, d->dim, d->q_rs, d->g_rs, d->slices);
  if (rc == MPV_OK && codes) rc = sc_check_codes(what, d->gallery, d->g_rs, g_scale);
  if (rc != MPV_OK) return rc;
  if (kind.prior) {
    MPV_REQUIRE(kind.g_prior, MPV_E_ARG, "%s: null g_prior", what);
    MPV_REQUIRE(((uintptr_t)kind.g_prior & 3) == 0, MPV_E_ALIGN, "%s: g_prior must be 4-byte aligned", what);
  }
  const long long supers = (d->ng + RS_SUPER - 1) / RS_SUPER;
  p->qtiles = (int)((d->nq + SC_TILE - 1) / SC_TILE);
  // 0 = choose: 3 workgroups per CU over the 256 CUs, at least 4 super-tiles (512 rows) each
  long long s = d->slices;
  if (s == 0) {
    s = (768 + p->qtiles - 1) / p->qtiles;
    if (s > (supers + 3) / 4) s = (supers + 3) / 4;
    // top-k: two workgroups fit a CU (registers), so no more than 512 -- a 513th would run alone in a second round -- and no
    // more than the merge kernel caches (SC_MERGE_CACHE entries, k per slice)
    if (topk_k > 0 && s > 512) s = 512;
    if (topk_k > 0 && s > SC_MERGE_CACHE / topk_k) s = SC_MERGE_CACHE / topk_k;
  }
  if (s > supers) s = supers;
  if (s < 1) s = 1;
  p->per_slice = (int)((supers + s - 1) / s);
  p->slices = (int)((supers + p->per_slice - 1) / p->per_slice);      // no empty slice
  return MPV_OK;
}

RsArgs rs_args(const mpv_sim_search_desc* d, const RsPlan& p, RsKind kind) {
  RsArgs a = {};
  a.Q = (const bf16*)d->queries;
  a.G = (const bf16*)d->gallery;
  a.q_rs = d->q_rs;
  a.g_rs = d->g_rs;
  a.nq = (int)d->nq;
  a.ng = (int)d->ng;
  a.D = d->dim;
  a.per_slice = p.per_slice;
  a.scale = 1.0f;
  a.g_scale = kind.g_scale;
  a.g_prior = kind.g_prior;
  return a;
}

// The entry points, each written once for both gallery types (`codes`: the *_q8 form).  `names`: the entry point, then its stages.
size_t rs_topk_ws(const char* what, const mpv_sim_search_desc* d, RsKind kind) {
  RsPlan p;
  if (!d || d->k < 1 || d->k > SC_MAX_K || rs_plan(d, &p, what, d->k, kind) != MPV_OK) return 0;
  return sc_ws_bytes((size_t)p.slices * (size_t)d->nq * d->k);
}

// the top-k stream instance of a kind for list length KMAX
template <int KMAX>
void (*rs_topk_kernel(RsKind kind))(RsArgs) {
  if (kind.prior) return kind.codes ? pri8_stream_kernel<0, KMAX> : pri_stream_kernel<0, KMAX>;
  return kind.codes ? q8_stream_kernel<0, KMAX> : sim_stream_kernel<0, KMAX>;
}

int rs_topk(const char* const names[2], const mpv_sim_search_desc* d, RsKind kind, float* vals, int64_t* idx, void* workspace,
            size_t workspace_bytes, hipStream_t stream) {
  const char* what = names[0];
  RsPlan p;
  MPV_REQUIRE(d, MPV_E_ARG, "%s: null descriptor", what);
  MPV_REQUIRE(d->k >= 1 && d->k <= SC_MAX_K, MPV_E_ARG, "%s: k (%d) must be in [1, %d]", what, d->k, SC_MAX_K);
  int rc = rs_plan(d, &p, what, d->k, kind);
  if (rc != MPV_OK) return rc;
  MPV_REQUIRE(vals && idx && workspace, MPV_E_ARG, "%s: null pointer", what);
  const size_t n = (size_t)p.slices * (size_t)d->nq * d->k;
  rc = sc_ws_check(what, workspace, workspace_bytes, n);
  if (rc != MPV_OK) return rc;
  RsArgs a = rs_args(d, p, kind);
  a.k = d->k;
  a.scale = d->scale;
  a.ws_val = (float*)workspace;
  a.ws_idx = (int*)sc_ws_upper(workspace, n);
  const size_t lds = sc_stream_lds(d->dim, SC_WAVES, (size_t)SC_WAVES * d->k * 32 * 8);
  auto kern = d->k <= 4 ? rs_topk_kernel<4>(kind) : d->k <= 16 ? rs_topk_kernel<16>(kind) : rs_topk_kernel<32>(kind);
  sc_allow_lds((const void*)kern, lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)p.slices, (unsigned)p.qtiles), dim3(64 * SC_WAVES), lds, stream, a);
  rc = mpv_check_launch(what);
  if (rc != MPV_OK) return rc;
  return sc_merge_slices(names[1], a.ws_val, a.ws_idx, vals, idx, a.nq, a.k, p.slices, stream);
}

int rs_rank(const char* const names[3], const mpv_sim_search_desc* d, RsKind kind, const int64_t* target, int n_targets, int32_t* rank,
            void* workspace, size_t workspace_bytes, hipStream_t stream) {
  const char* what = names[0];
  RsPlan p;
  int rc = rs_plan(d, &p, what, 0, kind);
  if (rc != MPV_OK) return rc;
  MPV_REQUIRE(target && rank && workspace, MPV_E_ARG, "%s: null pointer", what);
  MPV_REQUIRE(n_targets >= 1 && n_targets <= SC_MAX_T, MPV_E_ARG, "%s: n_targets (%d) must be in [1, %d]", what, n_targets, SC_MAX_T);
  const size_t n = (size_t)d->nq * n_targets;
  rc = sc_ws_check(what, workspace, workspace_bytes, n);
  if (rc != MPV_OK) return rc;
  RsArgs a = rs_args(d, p, kind);
  if (kind.prior) a.scale = d->scale;                 // with an additive term the order depends on the scale
  a.n_t = n_targets;
  a.target = target;
  float* tscore = (float*)workspace;
  a.tscore = tscore;
  a.counts = (int*)sc_ws_upper(workspace, n);
  if (hipMemsetAsync(a.counts, 0, n * 4, stream) != hipSuccess) {
    mpv_set_error("%s: hipMemsetAsync failed", what);
    return MPV_E_HIP;
  }
  const size_t lds_t = sc_stream_lds(d->dim, 1, 0);
  auto tkern = kind.prior ? (kind.codes ? pri8_target_kernel : pri_target_kernel) : (kind.codes ? q8_target_kernel : sim_target_kernel);
  sc_allow_lds((const void*)tkern, lds_t);
  hipLaunchKernelGGL(tkern, dim3((unsigned)n_targets, (unsigned)p.qtiles), dim3(64), lds_t, stream, a, tscore);
  rc = mpv_check_launch(names[1]);
  if (rc != MPV_OK) return rc;
  const size_t lds = sc_stream_lds(d->dim, SC_WAVES, (size_t)SC_TILE * n_targets * 12);
  auto kern = kind.prior ? (kind.codes ? pri8_stream_kernel<1, 1> : pri_stream_kernel<1, 1>)
                         : (kind.codes ? q8_stream_kernel<1, 1> : sim_stream_kernel<1, 1>);
  sc_allow_lds((const void*)kern, lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)p.slices, (unsigned)p.qtiles), dim3(64 * SC_WAVES), lds, stream, a);
  rc = mpv_check_launch(what);
  if (rc != MPV_OK) return rc;
  // no target scores: a target whose score is NaN still counts as a target here (mpv_maxsim_rank skips it); with a term, a
  // target that is not eligible carries a NaN score (pri_target_kernel) and is no target
  return sc_rank_finish(names[2], target, kind.prior ? tscore : nullptr, a.counts, rank, a.nq, n_targets, a.ng, stream);
}

const char* const RS_TOPK[2] = {"mpv_sim_topk", "mpv_sim_topk (merge)"};
const char* const RS_TOPK_Q8[2] = {"mpv_sim_topk_q8", "mpv_sim_topk_q8 (merge)"};
const char* const RS_RANK[3] = {"mpv_sim_rank", "mpv_sim_rank (target scores)", "mpv_sim_rank (finish)"};
const char* const RS_RANK_Q8[3] = {"mpv_sim_rank_q8", "mpv_sim_rank_q8 (target scores)", "mpv_sim_rank_q8 (finish)"};
const char* const RS_TOPK_PRI[2] = {"mpv_sim_topk_prior", "mpv_sim_topk_prior (merge)"};
const char* const RS_TOPK_PRI8[2] = {"mpv_sim_topk_prior_q8", "mpv_sim_topk_prior_q8 (merge)"};
const char* const RS_RANK_PRI[3] = {"mpv_sim_rank_prior", "mpv_sim_rank_prior (target scores)", "mpv_sim_rank_prior (finish)"};
const char* const RS_RANK_PRI8[3] = {"mpv_sim_rank_prior_q8", "mpv_sim_rank_prior_q8 (target scores)", "mpv_sim_rank_prior_q8 (finish)"};

size_t rs_rank_ws(const char* what, const mpv_sim_search_desc* d, RsKind kind, int n_targets) {
  RsPlan p;                                           // a descriptor the call would refuse: 0
  if (n_targets < 1 || n_targets > SC_MAX_T || rs_plan(d, &p, what, 0, kind) != MPV_OK) return 0;
  return sc_ws_bytes((size_t)d->nq * n_targets);
}

}  // namespace

// the launchers of the two kernels above, for this file and maxsim_search.hip (declared in search_common.h)
int sc_merge_slices(const char* what, const float* ws_val, const int* ws_idx, float* vals, int64_t* idx, int nq, int k, int slices,
                    hipStream_t stream) {
  hipLaunchKernelGGL(sim_topk_merge_kernel, dim3((unsigned)nq), dim3(256), 0, stream, ws_val, ws_idx, vals, idx, nq, k, slices);
  return mpv_check_launch(what);
}

int sc_rank_finish(const char* what, const int64_t* target, const float* tscore, const int* counts, int* rank, int nq, int n_t, int ng,
                   hipStream_t stream) {
  hipLaunchKernelGGL(sim_rank_finish_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, target, tscore, counts, rank, nq,
                     n_t, ng);
  return mpv_check_launch(what);
}

extern "C" size_t mpv_sim_topk_workspace_size(const mpv_sim_search_desc* d) {
  return rs_topk_ws("mpv_sim_topk_workspace_size", d, RsKind{});
}
extern "C" int mpv_sim_topk(const mpv_sim_search_desc* d, float* vals, int64_t* idx, void* workspace, size_t workspace_bytes,
                            hipStream_t stream) {
  return rs_topk(RS_TOPK, d, RsKind{}, vals, idx, workspace, workspace_bytes, stream);
}
extern "C" size_t mpv_sim_rank_workspace_size(const mpv_sim_search_desc* d, int n_targets) {
  if (!d || d->nq <= 0 || n_targets < 1 || n_targets > SC_MAX_T) return 0;
  return sc_ws_bytes((size_t)d->nq * n_targets);
}
extern "C" int mpv_sim_rank(const mpv_sim_search_desc* d, const int64_t* target, int n_targets, int32_t* rank, void* workspace,
                            size_t workspace_bytes, hipStream_t stream) {
  return rs_rank(RS_RANK, d, RsKind{}, target, n_targets, rank, workspace, workspace_bytes, stream);
}

// ---- the same searches over e4m3 codes (include/mpv.h, "Searches over an FP8 gallery") ------------------------------------------
extern "C" size_t mpv_sim_topk_q8_workspace_size(const mpv_sim_search_desc* d, const float* g_scale) {
  return rs_topk_ws("mpv_sim_topk_q8_workspace_size", d, RsKind{true, g_scale});
}
extern "C" int mpv_sim_topk_q8(const mpv_sim_search_desc* d, const float* g_scale, float* vals, int64_t* idx, void* workspace,
                               size_t workspace_bytes, hipStream_t stream) {
  return rs_topk(RS_TOPK_Q8, d, RsKind{true, g_scale}, vals, idx, workspace, workspace_bytes, stream);
}
extern "C" size_t mpv_sim_rank_q8_workspace_size(const mpv_sim_search_desc* d, const float* g_scale, int n_targets) {
  return rs_rank_ws("mpv_sim_rank_q8_workspace_size", d, RsKind{true, g_scale}, n_targets);
}
extern "C" int mpv_sim_rank_q8(const mpv_sim_search_desc* d, const float* g_scale, const int64_t* target, int n_targets, int32_t* rank,
                               void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return rs_rank(RS_RANK_Q8, d, RsKind{true, g_scale}, target, n_targets, rank, workspace, workspace_bytes, stream);
}

// ---- the same searches with a per-row additive term (include/mpv.h, "Searches with per-row priors") ------------------------------
extern "C" size_t mpv_sim_topk_prior_workspace_size(const mpv_sim_search_desc* d, const float* g_prior) {
  return rs_topk_ws("mpv_sim_topk_prior_workspace_size", d, RsKind{false, nullptr, true, g_prior});
}
extern "C" int mpv_sim_topk_prior(const mpv_sim_search_desc* d, const float* g_prior, float* vals, int64_t* idx, void* workspace,
                                  size_t workspace_bytes, hipStream_t stream) {
  return rs_topk(RS_TOPK_PRI, d, RsKind{false, nullptr, true, g_prior}, vals, idx, workspace, workspace_bytes, stream);
}
extern "C" size_t mpv_sim_rank_prior_workspace_size(const mpv_sim_search_desc* d, const float* g_prior, int n_targets) {
  return rs_rank_ws("mpv_sim_rank_prior_workspace_size", d, RsKind{false, nullptr, true, g_prior}, n_targets);
}
extern "C" int mpv_sim_rank_prior(const mpv_sim_search_desc* d, const float* g_prior, const int64_t* target, int n_targets,
                                  int32_t* rank, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return rs_rank(RS_RANK_PRI, d, RsKind{false, nullptr, true, g_prior}, target, n_targets, rank, workspace, workspace_bytes, stream);
}
extern "C" size_t mpv_sim_topk_prior_q8_workspace_size(const mpv_sim_search_desc* d, const float* g_scale, const float* g_prior) {
  return rs_topk_ws("mpv_sim_topk_prior_q8_workspace_size", d, RsKind{true, g_scale, true, g_prior});
}
extern "C" int mpv_sim_topk_prior_q8(const mpv_sim_search_desc* d, const float* g_scale, const float* g_prior, float* vals,
                                     int64_t* idx, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return rs_topk(RS_TOPK_PRI8, d, RsKind{true, g_scale, true, g_prior}, vals, idx, workspace, workspace_bytes, stream);
}
extern "C" size_t mpv_sim_rank_prior_q8_workspace_size(const mpv_sim_search_desc* d, const float* g_scale, const float* g_prior,
                                                       int n_targets) {
  return rs_rank_ws("mpv_sim_rank_prior_q8_workspace_size", d, RsKind{true, g_scale, true, g_prior}, n_targets);
}
extern "C" int mpv_sim_rank_prior_q8(const mpv_sim_search_desc* d, const float* g_scale, const float* g_prior, const int64_t* target,
                                     int n_targets, int32_t* rank, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return rs_rank(RS_RANK_PRI8, d, RsKind{true, g_scale, true, g_prior}, target, n_targets, rank, workspace, workspace_bytes, stream);
}
