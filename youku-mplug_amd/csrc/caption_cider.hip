// CIDEr of caption candidates against references on the device: mpv_caption_cider fills, for every (candidate, reference) pair of
// every group (clip), the four per-order similarities of the reference scorer's compute_cider -- tf-idf vectors over the 1..4-grams
// of TOKEN IDS, clipped cosine, Gaussian length penalty -- and every candidate's score 10 * mean_n(sum_r / R).  The corpus statistics
// come from an open-addressing table built on the host (generation.CiderStats); the semantics are stated in include/mpv.h.
//
// Three kernels, plain C++, fp64, no atomics:
//   cc_rows    one wave per ROW of either table, once per call: the caption's length (a ballot over 64 columns at a time), its tokens
//              as 16-bit fields in LDS, the packed key of the four tokens from every position (key of order n = the low n fields).
//              Lane l owns the positions l, l + 64, ...: it counts its key among the row's keys (tf) and in front of it (first
//              occurrence), probes the corpus table for every first occurrence and writes key and vec = tf * idf per position and
//              order to the workspace -- key 0 where the n-gram has occurred before or runs over the caption's end -- and the four
//              norms.  A caption of a few dozen tokens is latency-bound: 30 x 30 key comparisons per row are nothing next to the
//              table probes, which is why they run once per row here and not once per pair.
//   cc_pairs   one wave per PAIR: the reference's keys and weights per order go through LDS (4 x 255 x 16 bytes), every lane looks
//              its candidate positions' keys up among them (all lanes read the same LDS word: a broadcast), accumulates
//              min(vec_c, vec_r) * vec_r and the wave finishes: norms, penalty, four stores.
//   cc_scores  one thread per candidate: the sum over its group's references in ascending order.
// Every sum has an order that is a function of the captions alone -- a lane's positions ascending, then the xor butterfly 32, 16, ..,
// 1 over the lanes (an addition is commutative: every lane ends with the same bits) -- so a pair's values do not depend on what else
// is in the call.  Lengths are measured in tokens; the reference scorer measures them in bigrams (len - 1): the difference of two
// non-empty captions is the same, and every value that involves an empty caption is 0 whatever the penalty.
// Every loop is bounded by a length clamped to [0, min(255, width - start, P)] in the kernel itself (P: the workspace's positions per
// row) and a probe by the table's capacity: bad data can neither hang a kernel nor make it touch a column at or beyond the width of
// its table or a workspace slot of another row.
#include <math.h>
#include <string.h>

#include "mpv_common.h"
#include "../../include/mpv.h"

namespace {

constexpr int CC_LANES = 64, CC_MAX_LEN = MPV_CAPTION_OVERLAP_MAX_LEN, CC_ORD = MPV_CAPTION_CIDER_ORDERS, CC_CHUNKS = 4, CC_SCORE_THREADS = 256;
static_assert(CC_CHUNKS * CC_LANES > CC_MAX_LEN, "a wave covers a row in CC_CHUNKS steps");

struct cc_ws {          // the workspace: rows = rows_a + rows_b (side a first), P positions per row and order
  uint64_t* key;        // [rows][4][P]  packed n-gram at its first occurrence, else 0
  double* vec;          // [rows][4][P]  tf * idf beside it
  double* norm;         // [rows][4]
  int32_t* len;         // [rows]
  int P;
};

__device__ __forceinline__ int cc_clamp(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }
__device__ __forceinline__ uint64_t cc_mask(int n) { return n == 3 ? ~0ull : (1ull << (16 * (n + 1))) - 1; }      // order n + 1: the low n + 1 fields

__device__ __forceinline__ double cc_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double cc_idf(uint64_t key, const uint64_t* __restrict__ tkeys, const double* __restrict__ tidf, uint64_t mask,
                                         double log_ref_len) {
  uint64_t slot = mpv_mix64(key) & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    const uint64_t k = tkeys[slot];
    if (k == key) return tidf[slot];
    if (k == 0) break;
    slot = (slot + 1) & mask;
  }
  return log_ref_len;                                          // not in the corpus: df = 0
}

__global__ __launch_bounds__(CC_LANES) void cc_rows(const int64_t* __restrict__ tok, int64_t ld, const int32_t* __restrict__ start, int rows,
                                                    int width, int64_t term, int row_base, const uint64_t* __restrict__ tkeys,
                                                    const double* __restrict__ tidf, uint64_t tmask, double log_ref_len, cc_ws ws) {
  __shared__ uint16_t field[CC_CHUNKS * CC_LANES + 4];         // id + 1 per position, 0 from the caption's end on
  __shared__ uint64_t full[CC_CHUNKS * CC_LANES];              // the four fields from every position on
  const int lane = threadIdx.x, r = blockIdx.x;
  if (r >= rows) return;                                       // (wave-uniform)
  const int s = cc_clamp(start[r], 0, width);
  const int nmax = min(min(width - s, CC_MAX_LEN), ws.P);
  const int64_t* __restrict__ p = tok + (int64_t)r * ld + s;

  int64_t mine[CC_CHUNKS];
#pragma unroll
  for (int c = 0; c < CC_CHUNKS; ++c) {
    const int pos = c * CC_LANES + lane;
    mine[c] = pos < nmax ? p[pos] : term;                      // the columns behind the row end it (nmax <= 255: position 255 always does)
  }
  int len = nmax;
#pragma unroll
  for (int c = CC_CHUNKS - 1; c >= 0; --c) {
    const unsigned long long hit = __ballot(mine[c] == term);
    if (hit) len = c * CC_LANES + __ffsll((long long)hit) - 1;
  }
  len = min(len, nmax);
#pragma unroll
  for (int c = 0; c < CC_CHUNKS; ++c) {
    const int pos = c * CC_LANES + lane;
    field[pos] = pos < len ? (uint16_t)(mine[c] + 1) : (uint16_t)0;
  }
  if (lane < 4) field[CC_CHUNKS * CC_LANES + lane] = 0;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CC_CHUNKS; ++c) {
    const int pos = c * CC_LANES + lane;
    full[pos] = (uint64_t)field[pos] | (uint64_t)field[pos + 1] << 16 | (uint64_t)field[pos + 2] << 32 | (uint64_t)field[pos + 3] << 48;
  }
  __syncthreads();

  const int64_t row = (int64_t)row_base + r;
  uint64_t* __restrict__ wk = ws.key + row * CC_ORD * ws.P;
  double* __restrict__ wv = ws.vec + row * CC_ORD * ws.P;
  double acc[CC_ORD] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < CC_CHUNKS; ++c) {
    const int i = c * CC_LANES + lane;
    if (i >= len) continue;
    const uint64_t fi = full[i];
    int tf[CC_ORD] = {0, 0, 0, 0}, before[CC_ORD] = {0, 0, 0, 0};
    for (int j = 0; j < len; ++j) {
      const uint64_t x = fi ^ full[j];                         // an n-gram that fits at i has n non-zero fields: it equals only n-grams that fit at j
#pragma unroll
      for (int n = 0; n < CC_ORD; ++n) {
        const int eq = (x & cc_mask(n)) == 0;
        tf[n] += eq;
        before[n] += eq & (j < i);
      }
    }
#pragma unroll
    for (int n = 0; n < CC_ORD; ++n) {
      uint64_t key = 0;
      double vec = 0.0;
      if (i + n < len && before[n] == 0) {                     // the first occurrence of an n-gram that fits
        key = fi & cc_mask(n);
        vec = (double)tf[n] * cc_idf(key, tkeys, tidf, tmask, log_ref_len);
        acc[n] += vec * vec;
      }
      wk[n * ws.P + i] = key;
      wv[n * ws.P + i] = vec;
    }
  }
#pragma unroll
  for (int n = 0; n < CC_ORD; ++n) {
    const double total = cc_wave_sum(acc[n]);
    if (lane == 0) ws.norm[row * CC_ORD + n] = sqrt(total);
  }
  if (lane == 0) ws.len[row] = len;
}

__global__ __launch_bounds__(CC_LANES) void cc_pairs(mpv_caption_cider_desc d, cc_ws ws, int64_t pairs) {
  __shared__ uint64_t rk[CC_ORD * CC_MAX_LEN];
  __shared__ double rv[CC_ORD * CC_MAX_LEN];
  const int lane = threadIdx.x;
  const int64_t p = blockIdx.x;
  if (p >= pairs) return;                                      // (wave-uniform, as everything up to the loads)
  double* __restrict__ out = d.pair + p * CC_ORD;

  // ---- the pair's group: the last g with pair_begin[g] <= p (an empty group shares its offset with the next one)
  int lo = 0, hi = d.groups;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (d.pair_begin[mid] <= p) lo = mid; else hi = mid;
  }
  const int64_t local = p - d.pair_begin[lo];
  const int a0 = d.begin_a[lo], b0 = d.begin_b[lo];
  const int nb = d.begin_b[lo + 1] - b0;
  int64_t ra = -1, rb = -1;
  if (local >= 0 && nb > 0) {
    const int64_t ia = local / nb;
    ra = a0 + ia;
    rb = b0 + (local - ia * nb);
  }
  if (ra < 0 || ra >= d.rows_a || rb < 0 || rb >= d.rows_b) {  // (the host has checked its copies: belt and braces)
    if (lane < CC_ORD) out[lane] = 0.0;
    return;
  }
  const int64_t row_a = ra, row_b = (int64_t)d.rows_a + rb;
  const int cap = min(CC_MAX_LEN, ws.P);
  const int la = cc_clamp(ws.len[row_a], 0, cap), lb = cc_clamp(ws.len[row_b], 0, cap);
  const uint64_t* __restrict__ ka = ws.key + row_a * CC_ORD * ws.P;
  const double* __restrict__ va = ws.vec + row_a * CC_ORD * ws.P;
  const uint64_t* __restrict__ kb = ws.key + row_b * CC_ORD * ws.P;
  const double* __restrict__ vb = ws.vec + row_b * CC_ORD * ws.P;

#pragma unroll
  for (int n = 0; n < CC_ORD; ++n)
    for (int j = lane; j < lb - n; j += CC_LANES) {
      rk[n * CC_MAX_LEN + j] = kb[n * ws.P + j];
      rv[n * CC_MAX_LEN + j] = vb[n * ws.P + j];
    }
  __syncthreads();

  double acc[CC_ORD] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < CC_CHUNKS; ++c) {
    const int i = c * CC_LANES + lane;
#pragma unroll
    for (int n = 0; n < CC_ORD; ++n) {
      if (i + n >= la) continue;
      const uint64_t k = ka[n * ws.P + i];
      if (k == 0) continue;                                    // counted at its first occurrence
      const double vc = va[n * ws.P + i];
      double vr = 0.0;                                         // an n-gram the reference does not hold
      for (int j = 0; j < lb - n; ++j)
        if (rk[n * CC_MAX_LEN + j] == k) {
          vr = rv[n * CC_MAX_LEN + j];
          break;
        }
      acc[n] += fmin(vc, vr) * vr;
    }
  }
  const double dl = (double)(la - lb);
  const double penalty = exp(-(dl * dl) / (2.0 * d.sigma * d.sigma));
#pragma unroll
  for (int n = 0; n < CC_ORD; ++n) {
    double val = cc_wave_sum(acc[n]);
    const double nc = ws.norm[row_a * CC_ORD + n], nr = ws.norm[row_b * CC_ORD + n];
    if (nc != 0.0 && nr != 0.0) val /= nc * nr;
    val *= penalty;
    if (lane == 0) out[n] = val;
  }
}

__global__ __launch_bounds__(CC_SCORE_THREADS) void cc_scores(mpv_caption_cider_desc d) {
  const int r = blockIdx.x * CC_SCORE_THREADS + threadIdx.x;
  if (r >= d.rows_a) return;
  int lo = 0, hi = d.groups;                                   // the last g with begin_a[g] <= r: an empty group shares its offset with the next one
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (d.begin_a[mid] <= r) lo = mid; else hi = mid;
  }
  const int ia = r - d.begin_a[lo];
  const int nb = d.begin_b[lo + 1] - d.begin_b[lo];
  double score = 0.0;
  if (nb > 0 && ia >= 0 && r < d.begin_a[lo + 1]) {
    const double* __restrict__ v = d.pair + (d.pair_begin[lo] + (int64_t)ia * nb) * CC_ORD;
    double sum[CC_ORD] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < nb; ++j)
#pragma unroll
      for (int n = 0; n < CC_ORD; ++n) sum[n] += v[(int64_t)j * CC_ORD + n];
    score = 10.0 * ((((sum[0] + sum[1]) + sum[2]) + sum[3]) / CC_ORD / (double)nb);
  }
  d.score[r] = score;
}

// one side's HOST copies: begin is a CSR over [0, rows], every start leaves a candidate of at most CC_MAX_LEN columns
int check_side(const char* side, const int32_t* begin, const int32_t* start, int groups, int rows, int width) {
  MPV_REQUIRE(begin[0] == 0 && begin[groups] == rows, MPV_E_ARG, "mpv_caption_cider: begin_%s must run from 0 to rows_%s = %d (got %d .. %d)",
              side, side, rows, begin[0], begin[groups]);
  for (int g = 0; g < groups; ++g)
    MPV_REQUIRE(begin[g] <= begin[g + 1], MPV_E_ARG, "mpv_caption_cider: begin_%s is not monotone at group %d (%d > %d)", side, g, begin[g],
                begin[g + 1]);
  for (int r = 0; r < rows; ++r) {
    MPV_REQUIRE(start[r] >= 0 && start[r] <= width, MPV_E_ARG, "mpv_caption_cider: start_%s[%d] = %d outside [0, width_%s = %d]", side, r,
                start[r], side, width);
    MPV_REQUIRE(width - start[r] <= CC_MAX_LEN, MPV_E_SHAPE, "mpv_caption_cider: row %d of %s can hold a candidate of %d tokens (at most %d)",
                r, side, width - start[r], CC_MAX_LEN);
  }
  return MPV_OK;
}

// positions per row of the workspace: the longest candidate either table can hold (host copies), at least 1
int positions(const mpv_caption_cider_desc* d) {
  int P = 1;
  for (int r = 0; r < d->rows_a; ++r) P = max(P, min(d->width_a - d->host_start_a[r], CC_MAX_LEN));
  for (int r = 0; r < d->rows_b; ++r) P = max(P, min(d->width_b - d->host_start_b[r], CC_MAX_LEN));
  return P;
}

size_t ws_bytes(int64_t rows, int P) {
  const size_t per_row = (size_t)CC_ORD * P * (sizeof(uint64_t) + sizeof(double)) + CC_ORD * sizeof(double);
  return ((size_t)rows * (per_row + sizeof(int32_t)) + 7) / 8 * 8;
}

bool power_of_two(int64_t x) { return x >= 2 && (x & (x - 1)) == 0; }

}  // namespace

extern "C" size_t mpv_caption_cider_workspace_size(const mpv_caption_cider_desc* d) {
  if (!d || d->rows_a < 0 || d->rows_b < 0 || (d->rows_a > 0 && !d->host_start_a) || (d->rows_b > 0 && !d->host_start_b)) return 0;
  return max(ws_bytes((int64_t)d->rows_a + d->rows_b, positions(d)), (size_t)8);
}

extern "C" int mpv_caption_cider(const mpv_caption_cider_desc* d, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  MPV_REQUIRE(d, MPV_E_ARG, "mpv_caption_cider: null descriptor");
  MPV_REQUIRE(d->tok_a && d->tok_b && d->start_a && d->start_b && d->begin_a && d->begin_b && d->pair_begin && d->pair && d->score, MPV_E_ARG,
              "mpv_caption_cider: null pointer");
  MPV_REQUIRE(d->table_keys && d->table_idf, MPV_E_ARG, "mpv_caption_cider: null pointer (corpus table)");
  MPV_REQUIRE(d->host_start_a && d->host_start_b && d->host_begin_a && d->host_begin_b && d->host_pair_begin, MPV_E_ARG,
              "mpv_caption_cider: null pointer (host copy)");
  MPV_REQUIRE(d->groups >= 1 && d->rows_a >= 0 && d->rows_b >= 0, MPV_E_SHAPE, "mpv_caption_cider: groups (%d) must be positive, rows (%d, %d) not negative",
              d->groups, d->rows_a, d->rows_b);
  MPV_REQUIRE(d->width_a >= 0 && d->width_b >= 0 && d->ld_a >= d->width_a && d->ld_b >= d->width_b, MPV_E_SHAPE,
              "mpv_caption_cider: widths (%d, %d) must not be negative and the row strides (%lld, %lld) at least the widths", d->width_a, d->width_b,
              (long long)d->ld_a, (long long)d->ld_b);
  MPV_REQUIRE(power_of_two(d->table_capacity), MPV_E_ARG, "mpv_caption_cider: table_capacity = %lld is no power of two >= 2",
              (long long)d->table_capacity);
  MPV_REQUIRE(isfinite(d->log_ref_len) && d->log_ref_len >= 0.0, MPV_E_ARG, "mpv_caption_cider: log_ref_len = %g must be finite and not negative",
              d->log_ref_len);
  MPV_REQUIRE(isfinite(d->sigma) && d->sigma > 0.0, MPV_E_ARG, "mpv_caption_cider: sigma = %g must be finite and positive", d->sigma);
  int rc = check_side("a", d->host_begin_a, d->host_start_a, d->groups, d->rows_a, d->width_a);
  if (rc != MPV_OK) return rc;
  rc = check_side("b", d->host_begin_b, d->host_start_b, d->groups, d->rows_b, d->width_b);
  if (rc != MPV_OK) return rc;
  MPV_REQUIRE(d->host_pair_begin[0] == 0, MPV_E_ARG, "mpv_caption_cider: pair_begin must start at 0");
  for (int g = 0; g < d->groups; ++g) {
    const int64_t na = d->host_begin_a[g + 1] - d->host_begin_a[g], nb = d->host_begin_b[g + 1] - d->host_begin_b[g];
    MPV_REQUIRE(d->host_pair_begin[g + 1] - d->host_pair_begin[g] == na * nb, MPV_E_ARG,
                "mpv_caption_cider: pair_begin of group %d spans %lld pairs for %lld x %lld rows", g,
                (long long)(d->host_pair_begin[g + 1] - d->host_pair_begin[g]), (long long)na, (long long)nb);
  }
  const int64_t pairs = d->host_pair_begin[d->groups];
  MPV_REQUIRE(pairs <= 0x7fffffffLL, MPV_E_SHAPE, "mpv_caption_cider: %lld pairs are more than one grid holds", (long long)pairs);
  const int64_t rows = (int64_t)d->rows_a + d->rows_b;
  const int P = positions(d);
  const size_t need = ws_bytes(rows, P);
  MPV_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= need, MPV_E_ARG,
              "mpv_caption_cider: workspace of %zu bytes at %p (needs %zu, 8-byte aligned)", workspace_bytes, workspace, need);

  cc_ws ws;
  ws.P = P;
  ws.key = (uint64_t*)workspace;
  ws.vec = (double*)(ws.key + rows * CC_ORD * P);
  ws.norm = ws.vec + rows * CC_ORD * P;
  ws.len = (int32_t*)(ws.norm + rows * CC_ORD);
  const uint64_t tmask = (uint64_t)d->table_capacity - 1;
  if (d->rows_a > 0)
    hipLaunchKernelGGL(cc_rows, dim3((unsigned)d->rows_a), dim3(CC_LANES), 0, stream, d->tok_a, d->ld_a, d->start_a, d->rows_a, d->width_a, d->term, 0,
                       d->table_keys, d->table_idf, tmask, d->log_ref_len, ws);
  if (d->rows_b > 0)
    hipLaunchKernelGGL(cc_rows, dim3((unsigned)d->rows_b), dim3(CC_LANES), 0, stream, d->tok_b, d->ld_b, d->start_b, d->rows_b, d->width_b, d->term,
                       d->rows_a, d->table_keys, d->table_idf, tmask, d->log_ref_len, ws);
  if (pairs > 0) hipLaunchKernelGGL(cc_pairs, dim3((unsigned)pairs), dim3(CC_LANES), 0, stream, *d, ws, pairs);
  if (d->rows_a > 0)
    hipLaunchKernelGGL(cc_scores, dim3((unsigned)((d->rows_a + CC_SCORE_THREADS - 1) / CC_SCORE_THREADS)), dim3(CC_SCORE_THREADS), 0, stream, *d);
  return mpv_check_launch("mpv_caption_cider");
}

extern "C" int mpv_cider_table_fill(const uint64_t* keys, const double* idf, int64_t n, uint64_t* table_keys, double* table_idf, int64_t capacity) {
  MPV_REQUIRE(table_keys && table_idf && (n == 0 || (keys && idf)), MPV_E_ARG, "mpv_cider_table_fill: null pointer");
  MPV_REQUIRE(n >= 0 && power_of_two(capacity) && capacity > n, MPV_E_ARG,
              "mpv_cider_table_fill: capacity = %lld must be a power of two above the %lld entries", (long long)capacity, (long long)n);
  memset(table_keys, 0, (size_t)capacity * sizeof(uint64_t));
  memset(table_idf, 0, (size_t)capacity * sizeof(double));
  const uint64_t mask = (uint64_t)capacity - 1;
  for (int64_t e = 0; e < n; ++e) {
    MPV_REQUIRE(keys[e] != 0, MPV_E_ARG, "mpv_cider_table_fill: key %lld is 0 (the empty slot)", (long long)e);
    uint64_t slot = mpv_mix64(keys[e]) & mask;
    while (table_keys[slot] != 0) {                              // (capacity > n: an empty slot exists)
      MPV_REQUIRE(table_keys[slot] != keys[e], MPV_E_ARG, "mpv_cider_table_fill: key %lld occurs twice", (long long)e);
      slot = (slot + 1) & mask;
    }
    table_keys[slot] = keys[e];
    table_idf[slot] = idf[e];
  }
  return MPV_OK;
}

extern "C" int64_t mpv_cider_table_lookup(const uint64_t* table_keys, int64_t capacity, uint64_t key) {
  if (!table_keys || !power_of_two(capacity) || key == 0) return -1;
  const uint64_t mask = (uint64_t)capacity - 1;
  uint64_t slot = mpv_mix64(key) & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    if (table_keys[slot] == key) return (int64_t)slot;
    if (table_keys[slot] == 0) return -1;
    slot = (slot + 1) & mask;
  }
  return -1;
}
