// Query-max retrieval search (zero-shot evaluation / serving of the pre-train model's contrastive head): the score of a title and
// a clip is the MAX over the clip's query features (models/distributed_gpt3.py:178-202, mpv_maxsim_fwd), and selection is fused
// with it as in retrieval_search.hip -- neither the [nq][ng][Q] products nor an [nq][ng] matrix reach memory.
//
//   mpv_maxsim_topk   the k best gallery ITEMS per query item: (scale * s(i, j), j), descending, ties to the LOWER item index.
//   mpv_maxsim_rank   per query item the best rank among its target items.
//   s(i, j) = max over the rows a of query item i and the rows b of gallery item j of <a, b>; one side has one row per item.
//
// Both kernels keep one side RESIDENT in LDS (32 rows, the MFMA's B operand: a lane owns resident row lane & 31) and STREAM the
// other (32 rows x 128 k chunks per wave through registers and a 272-byte-pitch LDS stage, one step ahead, the MFMA's A operand)
// -- through sc_stage_* / sc_tile_mma / sc_load_resident of search_common.h, the one definition that retrieval_search.hip uses
// too.  The grouped side is always the streamed one, so the max over a group is a max over accumulator ROWS, which a lane holds
// itself: no cross-lane reduction beyond the two lane halves.
//   gallery grouped (title -> clip, and group == 1): mxs_gallery_kernel.  A workgroup owns 32 queries; every wave walks its own
//     contiguous run of gallery items.  Groups straddle the 32-row tiles, so a lane carries a running max; the item boundaries
//     are wave-uniform.  Per tile the 32 row scores of a lane's query are put in row order (one exchange between the lane
//     halves), scanned by a segmented running max, and the scores of the items that END in the tile are offered to the lane's
//     sorted list (TopList of search_common.h) or compared with the query's targets.
//   queries grouped (clip -> title): mxs_item_kernel.  A wave owns ONE query item and streams its rows against every resident
//     tile of 32 titles (shared by the workgroup's 4 waves); after the item's last row lane l holds s(item, title 32 t + l).  The
//     item's list lives across the wave (slot j in lane j): the lanes that beat the k-th slot are found with a ballot and
//     inserted one by one with a shift between neighbouring lanes.  Rank counts are ballots + one integer atomic per target.
// Order rule, NaN rule and slice independence are those of retrieval_search.hip: (v, g) beats (bv, bg) iff v > bv or (v == bv
// and g < bg) over ITEM indices; an item's score is computed entirely by one wave, every MFMA output element is a function of
// its A row, its B column and the accumulator only, and a max does not depend on the order of its operands, so no result
// depends on how the work was cut.  The running max starts at NaN and takes any operand over a NaN, so a NaN product never
// wins over a finite one and an item is NaN only when all its products are; such an item beats nothing.
// Target scores of mpv_maxsim_rank come from mxs_item_kernel's target modes: the same staging functions, chunk order (128 k
// ascending, 16 per MFMA), operand roles and accumulator reset as the stream that later meets the same rows, hence bit-identical
// products, and a max over bit-identical elements is bit-identical.  With both groups 1 the products are those of
// retrieval_search.hip's kernels for the same reason -- one definition of the tile walk -- and the max is over one element, so
// mpv_maxsim_* equals mpv_sim_* bit for bit.  The slices are merged by sim_topk_merge_kernel and the ranks finished by
// sim_rank_finish_kernel (retrieval_search.hip), which both files launch.
//
// mpv_maxsim_topk_q8 / mpv_maxsim_rank_q8 (include/mpv.h, "Searches over an FP8 gallery"): the gallery-grouped direction over e4m3
// codes with one fp32 scale per row -- mxs_gallery_kernel's body and mode 3 of mxs_item_kernel's instantiated on the code stage of
// search_common.h; the scale multiplies a row's score before the max over the group.  Grouped queries are refused there: the
// gallery would be the resident side, which is bf16 only.
#include "search_common.h"
#include "../../include/mpv.h"

namespace {

constexpr int MX_MAX_GROUP = 1024;

// running max that starts at NaN: any operand replaces a NaN, a NaN operand replaces nothing
__device__ __forceinline__ float mx_nanmax(float run, float x) { return (x > run || run != run) ? x : run; }

struct MxArgs {
  const bf16 *S, *R;         // streamed (grouped) rows, resident rows
  long long s_rs, r_rs;
  int ns, nr;                // streamed ITEMS, resident rows
  int G, D, k, n_t;
  int per_unit;              // gallery kernel: items per wave;  item kernel: resident tiles per slice
  int tiles;                 // streamed 32-row tiles per unit (gallery kernel) / per item (item kernel)
  int n_items_q;             // query items (rows of the outputs)
  float scale;
  float* ws_val;             // top-k: [slices][nq][k]
  int* ws_idx;
  const int64_t* target;     // rank: [nq][n_t]
  const float* tscore;       // rank: [nq][n_t]
  int* counts;               // rank: [nq][n_t], zeroed
  const float* s_scale;      // *_q8: S points to e4m3 codes, s_rs counts codes, one scale per streamed row
};

// ---------------------------------------------------------------------------------------------------------------------------
// Gallery grouped (or no group at all).  grid (query tiles, slices); wave w of slice s is unit 4 s + w and owns the items
// unit * per_unit .. + per_unit - 1, i.e. a contiguous run of rows that starts on an item boundary.
// Written once over the streamed side's source type: bf16 rows (mxs_gallery_kernel) or e4m3 codes with row scales
// (q8_gallery_kernel; search_common.h, ScCodeStage).
template <int MODE, int KMAX, class Src>        // MODE 0: top-k (k <= KMAX), 1: rank counts
__device__ __forceinline__ void mxs_gallery_body(const MxArgs& a, const Src S) {
  extern __shared__ __attribute__((aligned(16))) char mx_smem[];
  const int tid = threadIdx.x, lane = tid & 63, l32 = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = a.D, rpitch = D + 8, G = a.G;
  bf16* rbuf = (bf16*)mx_smem;
  bf16* sbuf = rbuf + SC_TILE * rpitch + wave * (SC_TILE * SC_PITCH);
  char* tail = mx_smem + (size_t)(SC_TILE * rpitch + SC_WAVES * SC_TILE * SC_PITCH) * sizeof(bf16);
  const int q0 = blockIdx.x * SC_TILE, slice = blockIdx.y;
  long long it_lo = ((long long)slice * SC_WAVES + wave) * a.per_unit;
  if (it_lo > a.ns) it_lo = a.ns;
  long long it_hi = it_lo + a.per_unit;
  if (it_hi > a.ns) it_hi = a.ns;
  const long long row_lo = it_lo * G, row_hi = it_hi * G;

  TopList<KMAX> top;         // top-k: this lane's list for query lane & 31 (both lane halves keep the same list)
  ScRankLds rk = {};         // rank: target scores [32][n_t], target items, counts, in LDS
  if (MODE == 0)
    top.init(a.k);
  else
    rk = sc_rank_park(tail, a.target, a.tscore, q0, a.nr, a.ns, a.n_t, tid, 64 * SC_WAVES);
  sc_load_resident(rbuf, a.R, a.r_rs, D, [&](int j) -> long long { return q0 + j < a.nr ? q0 + j : -1; }, tid, 64 * SC_WAVES);

  const int nk = (D + SC_KC - 1) / SC_KC;
  const int nsteps = a.tiles * nk;                     // the same for every wave: the barriers below are uniform
  const bf16* rrow = rbuf + l32 * rpitch;
  typename ScSource<Src>::Stage st;
  long long trow = row_lo;                             // first row of the tile in flight
  auto rows = [&](long long r0) { return [=](int j) -> long long { return r0 + j < row_hi ? r0 + j : -1; }; };
  sc_stage_load(st, S, a.s_rs, 0, D, rows(trow), lane);
  f32x16 acc = {};
  float run = __builtin_nanf("");                      // max over the rows seen so far of the item in progress
  int item = (int)it_lo, pos = 0;                      // that item, and how many of its rows have been seen
  int kc = 0;
  for (int s = 0; s < nsteps; ++s) {
    sc_stage_store(st, sbuf, lane);
    __syncthreads();
    if (s + 1 < nsteps) {
      const bool wrap = kc + 1 == nk;
      sc_stage_load(st, S, a.s_rs, wrap ? 0 : (kc + 1) * SC_KC, D, rows(wrap ? trow + SC_TILE : trow), lane);
    }
    if (kc == 0) acc = f32x16{};
    const int kleft = D - kc * SC_KC;
    sc_tile_mma(acc, sbuf, rrow + kc * SC_KC, (kleft < SC_KC ? kleft : SC_KC) >> 4, lane);
    if (kc + 1 == nk) {
      // r[j] = score of tile row j: acc[i] of the lane with half h is row 8 (i / 4) + 4 h + i % 4
      if constexpr (ScSource<Src>::scaled) sc_scale_acc(acc, sbuf, lane);
      float r[32];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float mine = acc[i], other = __shfl_xor(mine, 32, 64);
        r[8 * (i >> 2) + (i & 3)] = half == 0 ? mine : other;
        r[8 * (i >> 2) + 4 + (i & 3)] = half == 0 ? other : mine;
      }
      // segmented running max in row order; r[j] becomes the item's score where an item ends (bit j of `ends`, wave-uniform)
      unsigned ends = 0;
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        if (trow + j < row_hi) {
          run = mx_nanmax(run, r[j]);
          r[j] = run;
          if (++pos == G) {
            ends |= 1u << j;
            pos = 0;
            run = __builtin_nanf("");
          }
        }
      }
      if (MODE == 0) {
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
          r[j] *= a.scale;
          const int g = item + __builtin_popcount(ends & ((1u << j) - 1u));
          m |= ((ends >> j & 1u) && top.beats(r[j], g)) ? 1u << j : 0u;
        }
        while (m) {                                    // one insertion site; rare once the list has settled
          const int j = __builtin_ctz(m);
          m &= m - 1;
          float v = r[0];
#pragma unroll
          for (int e = 1; e < 32; ++e) v = j == e ? r[e] : v;
          const int g = item + __builtin_popcount(ends & ((1u << j) - 1u));
          if (top.beats(v, g)) top.insert(v, g);
        }
      } else {
        for (int t = 0; t < a.n_t; ++t) {
          const int tg = rk.ti[l32 * a.n_t + t];
          const float ts = rk.tv[l32 * a.n_t + t];
          int c = 0;
#pragma unroll
          for (int j = 0; j < 32; ++j) {
            const int g = item + __builtin_popcount(ends & ((1u << j) - 1u));
            c += ((ends >> j & 1u) && sc_better(r[j], g, ts, tg)) ? 1 : 0;
          }
          if (half == 0 && tg >= 0 && c > 0) atomicAdd(&rk.cnt[l32 * a.n_t + t], c);
        }
      }
      item += __builtin_popcount(ends);
      kc = 0;
      trow += SC_TILE;
    } else {
      ++kc;
    }
    __syncthreads();
  }
  __syncthreads();
  if (MODE == 0) {
    // 4 lists per query (one per wave; the two lane halves hold the same one) -> 1 through LDS ([wave][k][32])
    const int k = a.k;
    float* lv = (float*)tail;
    int* li = (int*)(lv + SC_WAVES * k * 32);
    if (half == 0 && wave > 0) {
#pragma unroll
      for (int j = 0; j < KMAX; ++j)
        if (j >= KMAX - k) {
          lv[(wave * k + j - (KMAX - k)) * 32 + l32] = top.v[j];
          li[(wave * k + j - (KMAX - k)) * 32 + l32] = top.g[j];
        }
    }
    __syncthreads();
    if (wave == 0 && half == 0) {
      for (int w = 1; w < SC_WAVES; ++w)
        for (int j = 0; j < k; ++j) {
          const float cv = lv[(w * k + j) * 32 + l32];
          const int cg = li[(w * k + j) * 32 + l32];
          if (cg == SC_NONE || !top.beats(cv, cg)) break;
          top.insert(cv, cg);
        }
      if (q0 + l32 < a.nr) {
        const long long o = ((long long)slice * a.nr + q0 + l32) * k;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
          if (j >= KMAX - k) {
            a.ws_val[o + j - (KMAX - k)] = top.v[j];
            a.ws_idx[o + j - (KMAX - k)] = top.g[j];
          }
      }
    }
  } else {
    sc_rank_flush(rk.cnt, a.counts, q0, a.nr, a.n_t, tid, 64 * SC_WAVES);
  }
}

// The bf16 kernels keep the names and template heads the resource gate of the ISA test knows; the instances over codes are named
// apart (retrieval_search.hip does the same).
template <int MODE, int KMAX>
__global__ __launch_bounds__(64 * SC_WAVES) void mxs_gallery_kernel(MxArgs a) {
  mxs_gallery_body<MODE, KMAX>(a, a.S);
}
template <int MODE, int KMAX>
__global__ __launch_bounds__(64 * SC_WAVES) void q8_gallery_kernel(MxArgs a) {
  mxs_gallery_body<MODE, KMAX>(a, ScCodes{(const uint8_t*)a.S, a.s_scale});
}

// ---------------------------------------------------------------------------------------------------------------------------
// One wave per streamed item.  MODE 0 / 1: top-k / rank counts of query item blockIdx.x * waves + wave over the resident tiles
// of slice blockIdx.y (grid (ceil(nq / 4), slices), 4 waves).  MODE 2 / 3 (one wave): the target scores of mpv_maxsim_rank.
//   2: queries grouped -- streamed item = query item blockIdx.x, resident row j = its target title j;  tscore[item][j].
//   3: gallery grouped -- streamed item = target (blockIdx.y) of query blockIdx.x, resident row 0 = that query; tscore[q][t].
// Over codes only MODE 3 exists (q8_item_kernel): with queries grouped the gallery is the resident side, which stays bf16.
template <int MODE, class Src>
__device__ __forceinline__ void mxs_item_body(const MxArgs& a, const Src S, float* __restrict__ tscore_out) {
  extern __shared__ __attribute__((aligned(16))) char mx_smem[];
  const int tid = threadIdx.x, lane = tid & 63, l32 = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nthreads = blockDim.x, nwaves = nthreads >> 6;
  const int D = a.D, rpitch = D + 8, G = a.G;
  bf16* rbuf = (bf16*)mx_smem;
  bf16* sbuf = rbuf + SC_TILE * rpitch + wave * (SC_TILE * SC_PITCH);
  const int n_tt = (a.nr + SC_TILE - 1) / SC_TILE;

  long long sit;             // the streamed item of this wave, < 0: none (the wave still takes part in the barriers)
  int tt_lo = 0, tt_hi = 1;
  if (MODE <= 1) {
    sit = (long long)blockIdx.x * nwaves + wave;
    if (sit >= a.ns) sit = -1;
    tt_lo = blockIdx.y * a.per_unit;
    tt_hi = tt_lo + a.per_unit < n_tt ? tt_lo + a.per_unit : n_tt;
  } else if (MODE == 2) {
    sit = blockIdx.x;
  } else {
    const long long t = a.target[(long long)blockIdx.x * a.n_t + blockIdx.y];
    sit = t >= 0 && t < a.ns ? t : -1;
  }
  const long long srow0 = sit * G;

  float lv = -INFINITY;      // MODE 0: slot `lane` of the item's sorted list (lanes 0 .. k - 1)
  int lg = SC_NONE;
  const int nk = (D + SC_KC - 1) / SC_KC;
  const int nsteps = a.tiles * nk;
  const bf16* rrow = rbuf + l32 * rpitch;
  auto rows = [&](int tl) { return [=](int j) -> long long { return sit >= 0 && tl * SC_TILE + j < G ? srow0 + tl * SC_TILE + j : -1; }; };

  for (int tt = tt_lo; tt < tt_hi; ++tt) {
    // the last barrier of the previous tile's loop has passed: nobody reads the resident tile any more
    if (MODE <= 1) {
      sc_load_resident(rbuf, a.R, a.r_rs, D, [&](int j) -> long long { return tt * SC_TILE + j < a.nr ? (long long)tt * SC_TILE + j : -1; },
                       tid, nthreads);
    } else if (MODE == 2) {
      sc_load_resident(rbuf, a.R, a.r_rs, D, [&](int j) -> long long {
        if (j >= a.n_t) return -1;
        const long long t = a.target[sit * a.n_t + j];
        return t >= 0 && t < a.nr ? t : -1;
      }, tid, nthreads);
    } else {
      sc_load_resident(rbuf, a.R, a.r_rs, D, [&](int j) -> long long { return j == 0 ? (long long)blockIdx.x : -1; }, tid, nthreads);
    }
    typename ScSource<Src>::Stage st;
    sc_stage_load(st, S, a.s_rs, 0, D, rows(0), lane);
    f32x16 acc = {};
    float run = __builtin_nanf("");
    int kc = 0, tl = 0;
    for (int s = 0; s < nsteps; ++s) {
      sc_stage_store(st, sbuf, lane);
      __syncthreads();                                 // stage and resident tile visible
      if (s + 1 < nsteps) {
        const bool wrap = kc + 1 == nk;
        sc_stage_load(st, S, a.s_rs, wrap ? 0 : (kc + 1) * SC_KC, D, rows(wrap ? tl + 1 : tl), lane);
      }
      if (kc == 0) acc = f32x16{};
      const int kleft = D - kc * SC_KC;
      sc_tile_mma(acc, sbuf, rrow + kc * SC_KC, (kleft < SC_KC ? kleft : SC_KC) >> 4, lane);
      if (kc + 1 == nk) {
        if constexpr (ScSource<Src>::scaled) sc_scale_acc(acc, sbuf, lane);
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (tl * SC_TILE + 8 * (i >> 2) + 4 * half + (i & 3) < G) run = mx_nanmax(run, acc[i]);
        kc = 0;
        ++tl;
      } else {
        ++kc;
      }
      __syncthreads();                                 // every wave is done with its stage and, at the end, the resident tile
    }
    const float score = mx_nanmax(run, __shfl_xor(run, 32, 64));    // s(item, resident row lane & 31)
    const int title = tt * SC_TILE + l32;
    const bool valid = half == 0 && sit >= 0 && title < a.nr;
    if (MODE == 0) {
      const float v = score * a.scale;
      float kv = __shfl(lv, a.k - 1, 64);
      int kg = __shfl(lg, a.k - 1, 64);
      unsigned long long m = __ballot(valid && sc_better(v, title, kv, kg));
      while (m) {                                      // wave-uniform
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        const float cv = __shfl(v, b, 64);
        const int cg = tt * SC_TILE + b;
        if (sc_better(cv, cg, kv, kg)) {
          const float pv = __shfl_up(lv, 1, 64);
          const int pg = __shfl_up(lg, 1, 64);
          const bool up = lane > 0 && sc_better(cv, cg, pv, pg), here = sc_better(cv, cg, lv, lg);
          lv = up ? pv : (here ? cv : lv);
          lg = up ? pg : (here ? cg : lg);
          kv = __shfl(lv, a.k - 1, 64);
          kg = __shfl(lg, a.k - 1, 64);
        }
      }
    } else if (MODE == 1) {
      for (int t = 0; t < a.n_t; ++t) {
        long long tg = -1;
        float ts = 0.f;
        if (sit >= 0) {
          tg = a.target[sit * a.n_t + t];
          ts = a.tscore[sit * a.n_t + t];
        }
        const bool ok = tg >= 0 && tg < a.nr;
        const int c = __builtin_popcountll(__ballot(valid && ok && sc_better(score, title, ts, (int)tg)));
        if (lane == 0 && ok && c > 0) atomicAdd(&a.counts[sit * a.n_t + t], c);
      }
    } else if (MODE == 2) {
      if (half == 0 && l32 < a.n_t) tscore_out[sit * a.n_t + l32] = score;
    } else {
      if (lane == 0) tscore_out[(long long)blockIdx.x * a.n_t + blockIdx.y] = sit >= 0 ? score : 0.f;
    }
  }
  if (MODE == 0 && sit >= 0 && lane < a.k) {
    const long long o = ((long long)blockIdx.y * a.ns + sit) * a.k + lane;
    a.ws_val[o] = lv;
    a.ws_idx[o] = lg;
  }
}
template <int MODE>
__global__ __launch_bounds__(64 * SC_WAVES) void mxs_item_kernel(MxArgs a, float* __restrict__ tscore_out) {
  mxs_item_body<MODE>(a, a.S, tscore_out);
}
__global__ __launch_bounds__(64 * SC_WAVES) void q8_item_kernel(MxArgs a, float* __restrict__ tscore_out) {
  mxs_item_body<3>(a, ScCodes{(const uint8_t*)a.S, a.s_scale}, tscore_out);
}

struct MxPlan {
  bool by_item;              // queries grouped: mxs_item_kernel
  int slices, per_unit, tiles;
};

// `codes`: the gallery is e4m3 codes with the row scales g_scale (the *_q8 entries): sc_check_codes, and no grouped queries
int mx_plan(const mpv_maxsim_search_desc* d, MxPlan* p, const char* what, int topk_k = 0, bool codes = false,
            const float* g_scale = nullptr) {
  MPV_REQUIRE(d && d->queries && d->gallery, MPV_E_ARG, "%s: null pointer", what);
  MPV_REQUIRE(d->q_group >= 1 && d->q_group <= MX_MAX_GROUP && d->g_group >= 1 && d->g_group <= MX_MAX_GROUP, MPV_E_SHAPE,
              "%s: groups (%d, %d) must be in [1, %d]", what, d->q_group, d->g_group, MX_MAX_GROUP);
  MPV_REQUIRE(d->q_group == 1 || d->g_group == 1, MPV_E_SHAPE, "%s: only one of q_group (%d) and g_group (%d) may exceed 1", what,
              d->q_group, d->g_group);
  MPV_REQUIRE(d->nq > 0 && d->ng > 0 && d->nq <= 0x7fffffffll / d->q_group && d->ng <= 0x7fffffffll / d->g_group, MPV_E_SHAPE,
              "%s: bad shape nq=%lld x %d ng=%lld x %d (rows per side <= 2^31 - 1)", what, (long long)d->nq, d->q_group, (long long)d->ng,
              d->g_group);
  int rc = sc_check_desc(what, d->queries, d->gallery, d->dim, d->q_rs, d->g_rs, d->slices);
  if (rc == MPV_OK && codes) rc = sc_check_codes(what, d->gallery, d->g_rs, g_scale);
  if (rc != MPV_OK) return rc;
  MPV_REQUIRE(!codes || d->q_group == 1, MPV_E_SHAPE,
              "%s: q_group (%d) must be 1 over a gallery of codes (with grouped queries the gallery is the resident side: bf16 only)", what,
              d->q_group);
  p->by_item = d->q_group > 1;
  long long s = d->slices;
  if (!p->by_item) {
    // units of work are waves: slices * 4 of them share the gallery's items.  0 = choose: 3 workgroups per CU over the 256 CUs,
    // at least 512 gallery rows per workgroup
    const long long qtiles = (d->nq + SC_TILE - 1) / SC_TILE, rows = d->ng * d->g_group;
    const long long max_s = (d->ng + SC_WAVES - 1) / SC_WAVES;
    if (s == 0) {
      s = (768 + qtiles - 1) / qtiles;
      if (s > (rows + 511) / 512) s = (rows + 511) / 512;
      if (topk_k > 0 && s > 512) s = 512;
      if (topk_k > 0 && s > SC_MERGE_CACHE / topk_k) s = SC_MERGE_CACHE / topk_k;
    }
    if (s > max_s) s = max_s;
    if (s < 1) s = 1;
    const long long per = (d->ng + s * SC_WAVES - 1) / (s * SC_WAVES);
    p->per_unit = (int)per;
    p->slices = (int)((d->ng + per * SC_WAVES - 1) / (per * SC_WAVES));      // no empty slice
    p->tiles = (int)((per * d->g_group + SC_TILE - 1) / SC_TILE);
  } else {
    const long long groups = (d->nq + SC_WAVES - 1) / SC_WAVES, n_tt = (d->ng + SC_TILE - 1) / SC_TILE;
    if (s == 0) {
      s = (768 + groups - 1) / groups;
      if (topk_k > 0 && s > SC_MERGE_CACHE / topk_k) s = SC_MERGE_CACHE / topk_k;
    }
    if (s > n_tt) s = n_tt;
    if (s < 1) s = 1;
    p->per_unit = (int)((n_tt + s - 1) / s);
    p->slices = (int)((n_tt + p->per_unit - 1) / p->per_unit);
    p->tiles = (d->q_group + SC_TILE - 1) / SC_TILE;
  }
  return MPV_OK;
}

MxArgs mx_args(const mpv_maxsim_search_desc* d, const MxPlan& p, const float* g_scale) {
  MxArgs a = {};
  if (p.by_item) {
    a.S = (const bf16*)d->queries, a.s_rs = d->q_rs, a.ns = (int)d->nq, a.G = d->q_group;
    a.R = (const bf16*)d->gallery, a.r_rs = d->g_rs, a.nr = (int)d->ng;
  } else {
    a.S = (const bf16*)d->gallery, a.s_rs = d->g_rs, a.ns = (int)d->ng, a.G = d->g_group;
    a.R = (const bf16*)d->queries, a.r_rs = d->q_rs, a.nr = (int)d->nq;
  }
  a.D = d->dim;
  a.per_unit = p.per_unit;
  a.tiles = p.tiles;
  a.n_items_q = (int)d->nq;
  a.scale = 1.0f;
  a.s_scale = g_scale;                                // codes are always the streamed side (mx_plan)
  return a;
}

// The entry points, each written once for both gallery types (`codes`: the *_q8 form).  `names`: the entry point, then its stages.
size_t mx_topk_ws(const char* what, const mpv_maxsim_search_desc* d, bool codes, const float* g_scale) {
  MxPlan p;
  if (!d || d->k < 1 || d->k > SC_MAX_K || mx_plan(d, &p, what, d->k, codes, g_scale) != MPV_OK) return 0;
  return sc_ws_bytes((size_t)p.slices * (size_t)d->nq * d->k);
}

int mx_topk(const char* const names[2], const mpv_maxsim_search_desc* d, bool codes, const float* g_scale, float* vals, int64_t* idx,
            void* workspace, size_t workspace_bytes, hipStream_t stream) {
  const char* what = names[0];
  MxPlan p;
  MPV_REQUIRE(d, MPV_E_ARG, "%s: null descriptor", what);
  MPV_REQUIRE(d->k >= 1 && d->k <= SC_MAX_K, MPV_E_ARG, "%s: k (%d) must be in [1, %d]", what, d->k, SC_MAX_K);
  int rc = mx_plan(d, &p, what, d->k, codes, g_scale);
  if (rc != MPV_OK) return rc;
  MPV_REQUIRE(vals && idx && workspace, MPV_E_ARG, "%s: null pointer", what);
  const size_t n = (size_t)p.slices * (size_t)d->nq * d->k;
  rc = sc_ws_check(what, workspace, workspace_bytes, n);
  if (rc != MPV_OK) return rc;
  MxArgs a = mx_args(d, p, g_scale);
  a.k = d->k;
  a.scale = d->scale;
  a.ws_val = (float*)workspace;
  a.ws_idx = (int*)sc_ws_upper(workspace, n);
  if (p.by_item) {
    const size_t lds = sc_stream_lds(d->dim, SC_WAVES, 0);
    sc_allow_lds((const void*)mxs_item_kernel<0>, lds);
    hipLaunchKernelGGL(mxs_item_kernel<0>, dim3((unsigned)((d->nq + SC_WAVES - 1) / SC_WAVES), (unsigned)p.slices), dim3(64 * SC_WAVES),
                       lds, stream, a, (float*)nullptr);
  } else {
    const size_t lds = sc_stream_lds(d->dim, SC_WAVES, (size_t)SC_WAVES * d->k * 32 * 8);
    auto kern = d->k <= 4 ? mxs_gallery_kernel<0, 4> : d->k <= 16 ? mxs_gallery_kernel<0, 16> : mxs_gallery_kernel<0, 32>;
    if (codes) kern = d->k <= 4 ? q8_gallery_kernel<0, 4> : d->k <= 16 ? q8_gallery_kernel<0, 16> : q8_gallery_kernel<0, 32>;
    sc_allow_lds((const void*)kern, lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)((d->nq + SC_TILE - 1) / SC_TILE), (unsigned)p.slices), dim3(64 * SC_WAVES), lds, stream, a);
  }
  rc = mpv_check_launch(what);
  if (rc != MPV_OK) return rc;
  return sc_merge_slices(names[1], a.ws_val, a.ws_idx, vals, idx, (int)d->nq, a.k, p.slices, stream);
}

size_t mx_rank_ws(const char* what, const mpv_maxsim_search_desc* d, bool codes, const float* g_scale, int n_targets) {
  MxPlan p;
  if (!d || n_targets < 1 || n_targets > SC_MAX_T || mx_plan(d, &p, what, 0, codes, g_scale) != MPV_OK) return 0;
  return sc_ws_bytes((size_t)d->nq * n_targets);
}

int mx_rank(const char* const names[3], const mpv_maxsim_search_desc* d, bool codes, const float* g_scale, const int64_t* target,
            int n_targets, int32_t* rank, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  const char* what = names[0];
  MxPlan p;
  int rc = mx_plan(d, &p, what, 0, codes, g_scale);
  if (rc != MPV_OK) return rc;
  MPV_REQUIRE(target && rank && workspace, MPV_E_ARG, "%s: null pointer", what);
  MPV_REQUIRE(n_targets >= 1 && n_targets <= SC_MAX_T, MPV_E_ARG, "%s: n_targets (%d) must be in [1, %d]", what, n_targets, SC_MAX_T);
  const size_t n = (size_t)d->nq * n_targets;
  rc = sc_ws_check(what, workspace, workspace_bytes, n);
  if (rc != MPV_OK) return rc;
  MxArgs a = mx_args(d, p, g_scale);
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
  if (p.by_item) {
    sc_allow_lds((const void*)mxs_item_kernel<2>, lds_t);
    hipLaunchKernelGGL(mxs_item_kernel<2>, dim3((unsigned)d->nq), dim3(64), lds_t, stream, a, tscore);
    rc = mpv_check_launch(names[1]);
    if (rc != MPV_OK) return rc;
    const size_t lds = sc_stream_lds(d->dim, SC_WAVES, 0);
    sc_allow_lds((const void*)mxs_item_kernel<1>, lds);
    hipLaunchKernelGGL(mxs_item_kernel<1>, dim3((unsigned)((d->nq + SC_WAVES - 1) / SC_WAVES), (unsigned)p.slices), dim3(64 * SC_WAVES),
                       lds, stream, a, (float*)nullptr);
  } else {
    MxArgs ta = a;                                    // one wave per (query, target): the target item's rows against that query
    ta.tiles = (d->g_group + SC_TILE - 1) / SC_TILE;
    auto tkern = codes ? q8_item_kernel : mxs_item_kernel<3>;
    sc_allow_lds((const void*)tkern, lds_t);
    hipLaunchKernelGGL(tkern, dim3((unsigned)d->nq, (unsigned)n_targets), dim3(64), lds_t, stream, ta, tscore);
    rc = mpv_check_launch(names[1]);
    if (rc != MPV_OK) return rc;
    const size_t lds = sc_stream_lds(d->dim, SC_WAVES, (size_t)SC_TILE * n_targets * 12);
    auto kern = codes ? q8_gallery_kernel<1, 1> : mxs_gallery_kernel<1, 1>;
    sc_allow_lds((const void*)kern, lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)((d->nq + SC_TILE - 1) / SC_TILE), (unsigned)p.slices), dim3(64 * SC_WAVES), lds, stream, a);
  }
  rc = mpv_check_launch(what);
  if (rc != MPV_OK) return rc;
  return sc_rank_finish(names[2], target, tscore, a.counts, rank, (int)d->nq, n_targets, (int)d->ng, stream);
}

const char* const MX_TOPK[2] = {"mpv_maxsim_topk", "mpv_maxsim_topk (merge)"};
const char* const MX_TOPK_Q8[2] = {"mpv_maxsim_topk_q8", "mpv_maxsim_topk_q8 (merge)"};
const char* const MX_RANK[3] = {"mpv_maxsim_rank", "mpv_maxsim_rank (target scores)", "mpv_maxsim_rank (finish)"};
const char* const MX_RANK_Q8[3] = {"mpv_maxsim_rank_q8", "mpv_maxsim_rank_q8 (target scores)", "mpv_maxsim_rank_q8 (finish)"};

}  // namespace

extern "C" size_t mpv_maxsim_topk_workspace_size(const mpv_maxsim_search_desc* d) {
  return mx_topk_ws("mpv_maxsim_topk_workspace_size", d, false, nullptr);
}
extern "C" int mpv_maxsim_topk(const mpv_maxsim_search_desc* d, float* vals, int64_t* idx, void* workspace, size_t workspace_bytes,
                               hipStream_t stream) {
  return mx_topk(MX_TOPK, d, false, nullptr, vals, idx, workspace, workspace_bytes, stream);
}
extern "C" size_t mpv_maxsim_rank_workspace_size(const mpv_maxsim_search_desc* d, int n_targets) {
  return mx_rank_ws("mpv_maxsim_rank_workspace_size", d, false, nullptr, n_targets);
}
extern "C" int mpv_maxsim_rank(const mpv_maxsim_search_desc* d, const int64_t* target, int n_targets, int32_t* rank, void* workspace,
                               size_t workspace_bytes, hipStream_t stream) {
  return mx_rank(MX_RANK, d, false, nullptr, target, n_targets, rank, workspace, workspace_bytes, stream);
}

// ---- the same searches over e4m3 codes, gallery grouped or not (include/mpv.h, "Searches over an FP8 gallery") -------------------
extern "C" size_t mpv_maxsim_topk_q8_workspace_size(const mpv_maxsim_search_desc* d, const float* g_scale) {
  return mx_topk_ws("mpv_maxsim_topk_q8_workspace_size", d, true, g_scale);
}
extern "C" int mpv_maxsim_topk_q8(const mpv_maxsim_search_desc* d, const float* g_scale, float* vals, int64_t* idx, void* workspace,
                                  size_t workspace_bytes, hipStream_t stream) {
  return mx_topk(MX_TOPK_Q8, d, true, g_scale, vals, idx, workspace, workspace_bytes, stream);
}
extern "C" size_t mpv_maxsim_rank_q8_workspace_size(const mpv_maxsim_search_desc* d, const float* g_scale, int n_targets) {
  return mx_rank_ws("mpv_maxsim_rank_q8_workspace_size", d, true, g_scale, n_targets);
}
extern "C" int mpv_maxsim_rank_q8(const mpv_maxsim_search_desc* d, const float* g_scale, const int64_t* target, int n_targets,
                                  int32_t* rank, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return mx_rank(MX_RANK_Q8, d, true, g_scale, target, n_targets, rank, workspace, workspace_bytes, stream);
}
