// Pairwise overlap counts between caption candidates on the device: mpv_caption_overlap fills, for every ordered pair (a, b) of every
// group (clip), the five integers [LCS(a, b), m1, m2, m3, m4] -- the length of the longest common subsequence and the clipped n-gram
// matches m_n = sum over the distinct n-grams g of min(count_a(g), count_b(g)) -- over token ids.  They are what a consensus
// (minimum-Bayes-risk) choice under ROUGE-L or an n-gram F needs; the utilities themselves are fp64 on the host
// (generation.consensus_utility).  The semantics are stated in include/mpv.h.
//
// Two kernels, plain integer C++, no atomics, no barrier:
//   co_lengths  one thread per row: the candidate's length, the distance from start[row] to the first `term` at or behind it (or to the
//               table's width).  A `term` in front of start[row] -- inside the prompt -- is never looked at.
//   co_pairs    one LANE per pair, one wave per workgroup, a grid over 64-pair tiles of the flattened pair list; a lane finds its group
//               by a binary search of the pair offsets.  The two candidates are read from global memory (a chunk's table is a few
//               hundred KB: it stays in L2, a row's tokens in the vector cache).
//     LCS       the textbook DP over ONE rolling row of uint8 cells (a count is at most 255) in LDS: cell j of lane l lives at byte
//               j * 64 + l, so the 64 lanes' cells of a column are 64 adjacent bytes -- 16 banks, four lanes per dword, no two dwords in
//               one bank.  255 columns x 64 lanes = 16 320 bytes per wave: ten waves fit a CU's 160 KiB.
//     n-grams   m_n = #{ i : e_n(i) < c_n(i) } with e_n(i) the number of EARLIER positions of a holding the n-gram that starts at i
//               and c_n(i) the number of positions of b holding it: occurrence number e (0-based) of a gram of a is matched iff b holds
//               more than e of it, which sums to min(count_a, count_b) per gram.  One scan per position serves the four orders: a scan
//               compares first tokens only and extends a hit to at most four tokens.
// Every loop is bounded by a length that is clamped to [0, min(255, width - start)] in the kernel itself, whatever the arrays hold:
// bad data cannot hang the kernel or make it read a column at or beyond the width of its table.  A pair has one writer; the outputs
// do not depend on thread timing.
#include "mpv_common.h"
#include "../../include/mpv.h"

namespace {

constexpr int CO_LANES = 64, CO_MAX_LEN = MPV_CAPTION_OVERLAP_MAX_LEN, CO_LEN_THREADS = 256;

__device__ __forceinline__ int co_clamp(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

__global__ __launch_bounds__(CO_LEN_THREADS) void co_lengths(const int64_t* __restrict__ tok, int64_t ld, const int32_t* __restrict__ start,
                                                             int rows, int width, int64_t term, int32_t* __restrict__ len) {
  const int r = blockIdx.x * CO_LEN_THREADS + threadIdx.x;
  if (r >= rows) return;
  const int s = co_clamp(start[r], 0, width);
  const int n = min(width - s, CO_MAX_LEN);
  const int64_t* p = tok + (int64_t)r * ld + s;
  int l = 0;
  while (l < n && p[l] != term) ++l;
  len[r] = l;
}

__global__ __launch_bounds__(CO_LANES) void co_pairs(mpv_caption_overlap_desc d, int64_t pairs) {
  __shared__ uint8_t cell[CO_MAX_LEN * CO_LANES];
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * CO_LANES + lane;
  if (p >= pairs) return;                                      // (no barrier below)

  // ---- the pair's group: the last g with pair_begin[g] <= p (an empty group shares its offset with the next one)
  int lo = 0, hi = d.groups;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (d.pair_begin[mid] <= p) lo = mid; else hi = mid;
  }
  const int64_t local = p - d.pair_begin[lo];
  const int a0 = d.begin_a[lo], b0 = d.begin_b[lo];
  const int nb = d.begin_b[lo + 1] - b0;
  if (local < 0 || nb <= 0) return;
  const int64_t ia = local / nb;
  const int64_t ra = a0 + ia, rb = b0 + (local - ia * nb);
  if (ra < 0 || ra >= d.rows_a || rb < 0 || rb >= d.rows_b) return;      // (the host has checked its copies: belt and braces)

  const int sa = co_clamp(d.start_a[ra], 0, d.width_a), sb = co_clamp(d.start_b[rb], 0, d.width_b);
  const int la = co_clamp(d.len_a[ra], 0, min(d.width_a - sa, CO_MAX_LEN));
  const int lb = co_clamp(d.len_b[rb], 0, min(d.width_b - sb, CO_MAX_LEN));
  const int64_t* __restrict__ A = d.tok_a + ra * d.ld_a + sa;
  const int64_t* __restrict__ B = d.tok_b + rb * d.ld_b + sb;

  // ---- the longest common subsequence: one rolling row, cell j = LCS(a[:i + 1], b[:j + 1])
  for (int j = 0; j < lb; ++j) cell[j * CO_LANES + lane] = 0;
  int lcs = 0;
  for (int i = 0; i < la; ++i) {
    const int64_t ai = A[i];
    int diag = 0, left = 0;
    for (int j = 0; j < lb; ++j) {
      const int up = cell[j * CO_LANES + lane];
      const int v = ai == B[j] ? diag + 1 : max(up, left);
      cell[j * CO_LANES + lane] = (uint8_t)v;
      diag = up;
      left = v;
    }
    lcs = left;
  }

  // ---- the clipped n-gram matches of the orders 1 .. 4
  int m1 = 0, m2 = 0, m3 = 0, m4 = 0;
  for (int i = 0; i < la; ++i) {
    const int64_t ai = A[i];
    const int avail = min(4, la - i);                           // the longest gram that starts at i
    int e1 = 0, e2 = 0, e3 = 0, e4 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    for (int k = 0; k < i; ++k) {
      if (A[k] != ai) continue;
      int ml = 1;
      while (ml < avail && A[k + ml] == A[i + ml]) ++ml;       // k + ml < i + ml < la
      e1 += 1; e2 += ml >= 2; e3 += ml >= 3; e4 += ml >= 4;
    }
    for (int k = 0; k < lb; ++k) {
      if (B[k] != ai) continue;
      const int lim = min(avail, lb - k);
      int ml = 1;
      while (ml < lim && B[k + ml] == A[i + ml]) ++ml;
      c1 += 1; c2 += ml >= 2; c3 += ml >= 3; c4 += ml >= 4;
    }
    m1 += e1 < c1; m2 += e2 < c2; m3 += e3 < c3; m4 += e4 < c4; // an order longer than what is left of a: e = c = 0
  }

  int32_t* out = d.counts + p * MPV_CAPTION_OVERLAP_COUNTS;
  out[0] = lcs; out[1] = m1; out[2] = m2; out[3] = m3; out[4] = m4;
}

// one side's HOST copies: begin is a CSR over [0, rows], every start leaves a candidate of at most CO_MAX_LEN columns
int check_side(const char* side, const int32_t* begin, const int32_t* start, int groups, int rows, int width) {
  MPV_REQUIRE(begin[0] == 0 && begin[groups] == rows, MPV_E_ARG, "mpv_caption_overlap: begin_%s must run from 0 to rows_%s = %d (got %d .. %d)",
              side, side, rows, begin[0], begin[groups]);
  for (int g = 0; g < groups; ++g)
    MPV_REQUIRE(begin[g] <= begin[g + 1], MPV_E_ARG, "mpv_caption_overlap: begin_%s is not monotone at group %d (%d > %d)", side, g, begin[g],
                begin[g + 1]);
  for (int r = 0; r < rows; ++r) {
    MPV_REQUIRE(start[r] >= 0 && start[r] <= width, MPV_E_ARG, "mpv_caption_overlap: start_%s[%d] = %d outside [0, width_%s = %d]", side, r,
                start[r], side, width);
    MPV_REQUIRE(width - start[r] <= CO_MAX_LEN, MPV_E_SHAPE, "mpv_caption_overlap: row %d of %s can hold a candidate of %d tokens (at most %d)",
                r, side, width - start[r], CO_MAX_LEN);
  }
  return MPV_OK;
}

}  // namespace

extern "C" int mpv_caption_overlap(const mpv_caption_overlap_desc* d, hipStream_t stream) {
  MPV_REQUIRE(d, MPV_E_ARG, "mpv_caption_overlap: null descriptor");
  MPV_REQUIRE(d->tok_a && d->tok_b && d->start_a && d->start_b && d->begin_a && d->begin_b && d->pair_begin && d->len_a && d->len_b && d->counts,
              MPV_E_ARG, "mpv_caption_overlap: null pointer");
  MPV_REQUIRE(d->host_start_a && d->host_start_b && d->host_begin_a && d->host_begin_b && d->host_pair_begin, MPV_E_ARG,
              "mpv_caption_overlap: null pointer (host copy)");
  MPV_REQUIRE(d->groups >= 1 && d->rows_a >= 0 && d->rows_b >= 0, MPV_E_SHAPE, "mpv_caption_overlap: groups (%d) must be positive, rows (%d, %d) not negative",
              d->groups, d->rows_a, d->rows_b);
  MPV_REQUIRE(d->width_a >= 0 && d->width_b >= 0 && d->ld_a >= d->width_a && d->ld_b >= d->width_b, MPV_E_SHAPE,
              "mpv_caption_overlap: widths (%d, %d) must not be negative and the row strides (%lld, %lld) at least the widths", d->width_a, d->width_b,
              (long long)d->ld_a, (long long)d->ld_b);
  int rc = check_side("a", d->host_begin_a, d->host_start_a, d->groups, d->rows_a, d->width_a);
  if (rc != MPV_OK) return rc;
  rc = check_side("b", d->host_begin_b, d->host_start_b, d->groups, d->rows_b, d->width_b);
  if (rc != MPV_OK) return rc;
  MPV_REQUIRE(d->host_pair_begin[0] == 0, MPV_E_ARG, "mpv_caption_overlap: pair_begin must start at 0");
  for (int g = 0; g < d->groups; ++g) {
    const int64_t na = d->host_begin_a[g + 1] - d->host_begin_a[g], nb = d->host_begin_b[g + 1] - d->host_begin_b[g];
    MPV_REQUIRE(d->host_pair_begin[g + 1] - d->host_pair_begin[g] == na * nb, MPV_E_ARG,
                "mpv_caption_overlap: pair_begin of group %d spans %lld pairs for %lld x %lld rows", g,
                (long long)(d->host_pair_begin[g + 1] - d->host_pair_begin[g]), (long long)na, (long long)nb);
  }
  const int64_t pairs = d->host_pair_begin[d->groups];
  const int64_t tiles = (pairs + CO_LANES - 1) / CO_LANES;
  MPV_REQUIRE(tiles <= 0x7fffffffLL, MPV_E_SHAPE, "mpv_caption_overlap: %lld pairs are more than one grid holds", (long long)pairs);

  if (d->rows_a > 0)
    hipLaunchKernelGGL(co_lengths, dim3((unsigned)((d->rows_a + CO_LEN_THREADS - 1) / CO_LEN_THREADS)), dim3(CO_LEN_THREADS), 0, stream, d->tok_a,
                       d->ld_a, d->start_a, d->rows_a, d->width_a, d->term, d->len_a);
  const bool same = d->tok_b == d->tok_a && d->start_b == d->start_a && d->len_b == d->len_a && d->rows_b == d->rows_a && d->width_b == d->width_a &&
                    d->ld_b == d->ld_a;                        // A is B: one table, its lengths once
  if (d->rows_b > 0 && !same)
    hipLaunchKernelGGL(co_lengths, dim3((unsigned)((d->rows_b + CO_LEN_THREADS - 1) / CO_LEN_THREADS)), dim3(CO_LEN_THREADS), 0, stream, d->tok_b,
                       d->ld_b, d->start_b, d->rows_b, d->width_b, d->term, d->len_b);
  if (pairs > 0) hipLaunchKernelGGL(co_pairs, dim3((unsigned)tiles), dim3(CO_LANES), 0, stream, *d, pairs);
  return mpv_check_launch("mpv_caption_overlap");
}
