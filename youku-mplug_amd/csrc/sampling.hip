// Sampled generation on the device: mpv_sample_advance does, for every sequence of a batch, what ONE iteration of
// generation.sample_loop does with a chain of torch calls -- temperature, the top-k / top-p filter of
// models/modeling_distributed_gpt3.py:1369-1441, the draw, the teacher-forcing write into the token table and the termination
// bookkeeping (:1689-1728) -- in one launch.  The semantics (tie rules, draw order, the uniform) are stated in include/mpv.h.
//
// One workgroup of 1024 threads per row; nothing is shared between rows, so a row's token depends neither on `rows` nor on its
// place in the launch.  The row (at most 65536 bf16) is read from memory ONCE, with 16-byte loads, and stays on the CU: thread t
// holds the eight logits of vector v = c * 1024 + t for c = 0 .. 7 (a wave reads 1 KiB per instruction), as 16-bit order-preserving
// keys in LDS (128 KiB, each thread re-reads only its own 16-byte slots: conflict-free, no barrier) and as fp32 probabilities in
// 64 registers -- keys and probabilities together do not fit the 128 registers of a 1024-thread workgroup.  No sort:
//   1. max key (integer), p_i = exp2((l_i - max) * log2(e) / T), total mass S.
//   2. the cutoff key: a bisection over the 16-bit keys whose probe is a block-wide count (top-k: the k-th largest key) or a
//      block-wide sum of p over the keys above the probe (top-p: the smallest key with mass above it <= top_p * S).
//   3. entries equal to the cutoff key share one p*: top-p keeps tie number r (index order) iff M_gt + r p* <= top_p S, which is
//      a count n_keep and a prefix rank; top-k keeps all of them; greedy is cutoff = max key, n_keep = 1.
//   4. the draw: prefix sums of the kept p in index order, in three levels -- the 128 segments of 512 consecutive elements (one
//      wave x one vector slot), the 64 lanes of the segment that holds the crossing, the 8 elements of that lane.
// Every sum runs in a fixed order (lane-local in element order, xor butterfly / Hillis-Steele across the lanes of a wave, wave
// partials through LDS in wave order); there is no floating-point atomic anywhere, so the outputs are bit-reproducible.  The one
// atomic is the integer add that counts the done rows.
//
// The ragged entry (mpv_sample_advance_ragged: prompts of different lengths in one lockstep loop) is the same kernel body with the
// token column a per-workgroup value, c_r = clamp(prompt_len[r], 0, row_len) + step, read once by the row's workgroup; a row whose
// column lies behind the table is frozen and leaves before the first barrier.  The column is a template parameter's business: the
// uniform instantiation (sa_rows<sample_advance_kernel>) reads d.pos as before and contains nothing of the ragged one
// (sa_rows<sa_ragged_entry>).  The steps entry (mpv_sample_advance_steps: rows that entered a running loop at different times,
// sa_rows<sa_steps_entry>) reads the step per row as well, from row_step[r]; a negative step freezes the row.
#include "mpv_common.h"
#include "../../include/mpv.h"

#include <limits.h>
#include <math.h>
#include <type_traits>

namespace {

constexpr int SA_THREADS = 1024, SA_WAVES = SA_THREADS / 64, SA_SLOTS = 8, SA_SEGS = SA_SLOTS * SA_WAVES;
constexpr int SA_MAX_VOCAB = SA_THREADS * SA_SLOTS * 8;
constexpr unsigned SA_KEY_NEG_INF = 0x007fu;             // key of -inf: every finite logit and +inf lie above it

// order-preserving 16-bit key of a bf16 (-0 is +0: equal logits must get equal keys)
__device__ __forceinline__ unsigned sa_key(unsigned b) {
  b = b == 0x8000u ? 0u : b;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ float sa_logit(unsigned key) {
  const unsigned b = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);
  return __uint_as_float(b << 16);
}
__device__ __forceinline__ unsigned sa_get(const uint4& v, int e) {
  const unsigned w = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w;
  return (e & 1) ? w >> 16 : w & 0xffffu;
}

// slot c of this thread's keys; the compiler barrier keeps the eight reads of an unrolled pass from being hoisted together (32
// registers beside the 64 of p would spill); four waves per SIMD cover the LDS latency instead
__device__ __forceinline__ uint4 sa_slot(const uint4* row_keys, int c, int tid) {
  asm volatile("" ::: "memory");
  return row_keys[c * SA_THREADS + tid];
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_scan_i(int v, int lane) {          // inclusive
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    v += lane >= o ? t : 0;
  }
  return v;
}
__device__ __forceinline__ float wave_scan_f(float v, int lane) {       // inclusive, fixed order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    v += lane >= o ? t : 0.f;
  }
  return v;
}

// Block-wide reductions over the 16 waves: wave partials (identical in every lane) go through one of two LDS buffers and are
// combined in wave order by every thread, so every thread holds the same bits.  The buffer alternates from call to call: one
// barrier per call is enough (a wave can write a buffer again only two calls later, behind a barrier that every reader of the
// earlier call has passed).
struct SaReduce {
  int* buf;      // [2][SA_WAVES]
  int phase;
  __device__ __forceinline__ int* slot() {
    phase ^= 1;
    return buf + phase * SA_WAVES;
  }
  __device__ __forceinline__ float sum_f(float v, int wave) {
    int* s = slot();
    s[wave] = __float_as_int(wave_sum(v));
    __syncthreads();
    float r = 0.f;
#pragma unroll
    for (int w = 0; w < SA_WAVES; ++w) r += __int_as_float(s[w]);
    return r;
  }
  __device__ __forceinline__ int sum_i(int v, int wave) {
    int* s = slot();
    s[wave] = wave_sum_i(v);
    __syncthreads();
    int r = 0;
#pragma unroll
    for (int w = 0; w < SA_WAVES; ++w) r += s[w];
    return r;
  }
  __device__ __forceinline__ int max_i(int v, int wave) {
    int* s = slot();
    s[wave] = wave_max_i(v);
    __syncthreads();
    int r = s[0];
#pragma unroll
    for (int w = 1; w < SA_WAVES; ++w) r = max(r, s[w]);
    return r;
  }
};

// wave 0: x[0 .. 127] -> exclusive prefix ex[] and inclusive prefix in[] in segment order (lane l takes entries 2l, 2l + 1)
__device__ __forceinline__ void sa_seg_scan_i(const int* x, int* ex, int lane) {
  const int a = x[2 * lane], b = x[2 * lane + 1];
  const int incl = wave_scan_i(a + b, lane);
  ex[2 * lane] = incl - a - b;
  ex[2 * lane + 1] = incl - b;
}
__device__ __forceinline__ void sa_seg_scan_f(const float* x, float* ex, float* in, int lane) {
  const float a = x[2 * lane], b = x[2 * lane + 1];
  const float incl = wave_scan_f(a + b, lane);
  float before = __shfl_up(incl, 1, 64);
  before = lane ? before : 0.f;
  ex[2 * lane] = before;
  ex[2 * lane + 1] = before + a;
  in[2 * lane] = before + a;
  in[2 * lane + 1] = incl;
}

// The kernel is a template over an entry tag.  The uniform entry's tag carries the kernel's name of old, so that its symbol still
// contains it (the resource checks and profiles look the uniform kernel up by that name) and the ragged one's does not.
struct sample_advance_kernel {};      // mpv_sample_advance: every row at column d.pos
struct sa_ragged_entry {};            // mpv_sample_advance_ragged: row r at its own column
struct sa_steps_entry {};             // mpv_sample_advance_steps: row r at its own column AND its own step row_step[r]

template <class Entry>
__global__ __launch_bounds__(SA_THREADS) void sa_rows(mpv_sample_advance_desc d, float exp_scale, const int32_t* __restrict__ row_step) {
  constexpr bool STEPS = std::is_same<Entry, sa_steps_entry>::value;       // (row_step is read by this instantiation only)
  constexpr bool RAGGED = std::is_same<Entry, sa_ragged_entry>::value || STEPS;
  __shared__ uint4 row_keys[SA_SLOTS * SA_THREADS];      // 128 KiB: slot c of thread t at [c * 1024 + t]; a thread reads only what it wrote
  __shared__ int red_buf[2 * SA_WAVES];
  __shared__ int seg_cnt[SA_SEGS], seg_cnt_ex[SA_SEGS];
  __shared__ float seg_mass[SA_SEGS], seg_mass_ex[SA_SEGS], seg_mass_in[SA_SEGS];
  __shared__ int pick_seg, pick_tok;
  __shared__ float pick_kept;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long row = blockIdx.x;
  const int vocab = d.vocab;
  SaReduce red{red_buf, 0};

  // ---- the token column of this row: d.pos, or (ragged) the row's own prompt length + the step d.pos
  int pos = d.pos;
  if (RAGGED) {
    const long long pl = d.prompt_len[row];
    const int step = STEPS ? row_step[row] : d.pos;
    const long long col = (pl < 0 ? 0 : pl > d.row_len ? d.row_len : pl) + step;
    if (col >= d.row_len || (STEPS && step < 0)) {       // block-uniform: frozen (the budget has ended, a bad length, an idle row); no logits read
      if (tid == 0) {
        if (d.out_token) d.out_token[row] = 0;
        if (d.out_kept) d.out_kept[row] = 0;
        if (d.out_mass) d.out_mass[row] = 0.f;
        d.next_tok[row] = d.tokens[row * d.row_len + d.row_len - 1];
        d.done[row] = 1;
        atomicAdd(d.n_done, 1);
      }
      return;
    }
    pos = (int)col;
  }

  if (tid < SA_SEGS) seg_cnt[tid] = 0, seg_mass[tid] = 0.f;
  if (tid == 0) pick_seg = -1, pick_tok = 0;

  // ---- the row, once: keys; a vector slot past the vocabulary holds key 0 (below -inf) and p = 0
  const bf16* lrow = (const bf16*)d.logits + row * d.ld;
  int kmax = 0;
#pragma unroll
  for (int c = 0; c < SA_SLOTS; ++c) {
    const int base = (c * SA_THREADS + tid) * 8;
    uint4 raw = make_uint4(0, 0, 0, 0);
    const bool have = base < vocab;                      // vocab % 8 == 0: a vector is inside the row or outside it
    if (have) raw = *(const uint4*)(lrow + base);
    unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned lo = have ? sa_key(w[j] & 0xffffu) : 0u, hi = have ? sa_key(w[j] >> 16) : 0u;
      kmax = max(kmax, (int)max(lo, hi));
      w[j] = lo | (hi << 16);
    }
    row_keys[c * SA_THREADS + tid] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  kmax = red.max_i(kmax, wave);

  int token = 0, n_kept = 0;
  float mass = 0.f;
  if (kmax > (int)SA_KEY_NEG_INF) {                      // block-uniform; a row of -inf only: token 0, nothing kept
    // ---- 1. probabilities and the total mass
    const float lmax = sa_logit((unsigned)kmax);
    float p[SA_SLOTS][8];
    float part = 0.f;
#pragma unroll
    for (int c = 0; c < SA_SLOTS; ++c) {
      const uint4 kv = sa_slot(row_keys, c, tid);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned k = sa_get(kv, e);
        p[c][e] = k > SA_KEY_NEG_INF ? __builtin_amdgcn_exp2f((sa_logit(k) - lmax) * exp_scale) : 0.f;
        part += p[c][e];
      }
    }
    const float S = red.sum_f(part, wave);

    // ---- 2. the cutoff key and how many of its entries stay
    unsigned cut = SA_KEY_NEG_INF;                       // plain, top_p == 1: everything above -inf
    int n_keep = INT_MAX;
    if (d.top_k == 1) {
      cut = (unsigned)kmax;
      n_keep = 1;
    } else if (d.top_k > 1) {                            // the largest key with at least k entries at or above it
      int lo = (int)SA_KEY_NEG_INF, hi = kmax;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        int n = 0;
#pragma unroll
        for (int c = 0; c < SA_SLOTS; ++c) {
          const uint4 kv = sa_slot(row_keys, c, tid);
#pragma unroll
          for (int e = 0; e < 8; ++e) n += (int)sa_get(kv, e) >= mid ? 1 : 0;
        }
        if (red.sum_i(n, wave) >= d.top_k) lo = mid; else hi = mid - 1;
      }
      cut = (unsigned)lo;
    } else if (d.top_p > 0.f && d.top_p < 1.f) {         // the smallest key with mass above it <= top_p * S
      const float P = d.top_p * S;
      auto mass_above = [&](int key) {
        float g = 0.f;
#pragma unroll
        for (int c = 0; c < SA_SLOTS; ++c) {
          const uint4 kv = sa_slot(row_keys, c, tid);
#pragma unroll
          for (int e = 0; e < 8; ++e) g += (int)sa_get(kv, e) > key ? p[c][e] : 0.f;
        }
        return red.sum_f(g, wave);
      };
      int lo = (int)SA_KEY_NEG_INF, hi = kmax;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (mass_above(mid) <= P) hi = mid; else lo = mid + 1;
      }
      cut = (unsigned)lo;
      const float m_gt = mass_above(lo);
      int n = 0;
#pragma unroll
      for (int c = 0; c < SA_SLOTS; ++c) {
        const uint4 kv = sa_slot(row_keys, c, tid);
#pragma unroll
        for (int e = 0; e < 8; ++e) n += sa_get(kv, e) == cut ? 1 : 0;
      }
      const int n_tie = red.sum_i(n, wave);
      const float p_star = cut > SA_KEY_NEG_INF ? __builtin_amdgcn_exp2f((sa_logit(cut) - lmax) * exp_scale) : 0.f;
      if (p_star > 0.f) {                                // tie r stays iff m_gt + r p* <= P
        const float r = fmaxf((P - m_gt) / p_star, 0.f);
        n_keep = r >= (float)n_tie ? n_tie : (int)floorf(r) + 1;
      }
    }

    // ---- 3. ranks of the entries at the cutoff key, in index order: per-segment counts, their prefix
#pragma unroll
    for (int c = 0; c < SA_SLOTS; ++c) {
      if (c * SA_THREADS * 8 >= vocab) continue;         // block-uniform
      const uint4 kv = sa_slot(row_keys, c, tid);
      int n = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) n += sa_get(kv, e) == cut ? 1 : 0;
      n = wave_sum_i(n);
      if (lane == 0) seg_cnt[c * SA_WAVES + wave] = n;
    }
    __syncthreads();
    if (wave == 0) sa_seg_scan_i(seg_cnt, seg_cnt_ex, lane);
    __syncthreads();

    // ---- 4. the kept set (one bit per element), its mass per segment, its size, its last index
    unsigned kept_lo = 0, kept_hi = 0;
    int cnt = 0, last = -1;
#pragma unroll
    for (int c = 0; c < SA_SLOTS; ++c) {
      if (c * SA_THREADS * 8 >= vocab) continue;
      const uint4 kv = sa_slot(row_keys, c, tid);
      int ties = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) ties += sa_get(kv, e) == cut ? 1 : 0;
      int rank = seg_cnt_ex[c * SA_WAVES + wave] + wave_scan_i(ties, lane) - ties;
      float m = 0.f;
      unsigned bits = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned k = sa_get(kv, e);
        bool keep = k > cut;
        if (k == cut) keep = rank < n_keep, ++rank;
        keep = keep && k > SA_KEY_NEG_INF;
        bits |= keep ? 1u << e : 0u;
        m += keep ? p[c][e] : 0.f;
        cnt += keep ? 1 : 0;
        last = keep ? (c * SA_THREADS + tid) * 8 + e : last;
      }
      if (c < 4) kept_lo |= bits << (8 * c); else kept_hi |= bits << (8 * (c - 4));
      const float incl = wave_scan_f(m, lane);
      if (lane == 63) seg_mass[c * SA_WAVES + wave] = incl;
    }
    n_kept = red.sum_i(cnt, wave);
    last = red.max_i(last, wave);                        // (its barrier also publishes seg_mass)

    // ---- 5. the draw
    float u;
    if (d.u_override) {
      u = d.u_override[row];
    } else {
      const long long sid = d.stream_id ? d.stream_id[row] : row;
      u = (float)(mpv_rand_pair(d.seed, ((uint64_t)(uint32_t)pos << 32) | (uint32_t)sid) >> 8) * 0x1p-24f;
    }
    if (wave == 0) {
      sa_seg_scan_f(seg_mass, seg_mass_ex, seg_mass_in, lane);
      const float kept = __shfl(seg_mass_in[2 * lane + 1], 63, 64), target = u * kept;
      const unsigned long long b0 = __ballot(seg_mass_in[2 * lane] > target && seg_mass[2 * lane] > 0.f);
      const unsigned long long b1 = __ballot(seg_mass_in[2 * lane + 1] > target && seg_mass[2 * lane + 1] > 0.f);
      int s0 = b0 ? 2 * (__ffsll((long long)b0) - 1) : SA_SEGS, s1 = b1 ? 2 * (__ffsll((long long)b1) - 1) + 1 : SA_SEGS;
      if (lane == 0) {
        pick_seg = min(s0, s1) < SA_SEGS ? min(s0, s1) : -1;
        pick_kept = kept;
        pick_tok = last;                                 // the fallback: the last kept index
      }
    }
    __syncthreads();
    mass = pick_kept / S;
    const int seg = pick_seg;
#pragma unroll
    for (int c = 0; c < SA_SLOTS; ++c) {
      if (seg != c * SA_WAVES + wave) continue;          // wave-uniform: the one wave and slot that hold the crossing
      const unsigned bits = ((c < 4 ? kept_lo : kept_hi) >> (8 * (c & 3))) & 0xffu;
      const float target = u * pick_kept;
      float m = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) m += (bits >> e) & 1u ? p[c][e] : 0.f;
      const float incl = wave_scan_f(m, lane);           // the same values as in step 4
      float before = __shfl_up(incl, 1, 64);
      before = seg_mass_ex[seg] + (lane ? before : 0.f);
      const unsigned long long cross = __ballot(seg_mass_ex[seg] + incl > target && m > 0.f), any = __ballot(m > 0.f);
      const int owner = cross ? __ffsll((long long)cross) - 1 : 63 - __clzll((long long)any);      // any != 0: the segment has mass
      if (lane == owner) {
        int pick = -1, fallback = -1;
        float run = before;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const bool keep = ((bits >> e) & 1u) && p[c][e] > 0.f;
          run += keep ? p[c][e] : 0.f;
          if (keep) fallback = e;
          if (keep && pick < 0 && run > target) pick = e;
        }
        pick_tok = (c * SA_THREADS + tid) * 8 + (pick >= 0 ? pick : fallback);
      }
    }
    __syncthreads();
    token = pick_tok;
  }

  // ---- the bookkeeping of sample_loop's body (:1689-1728)
  if (tid == 0) {
    long long tok = token;
    if (d.vocab_size > 0) tok = tok < d.vocab_size ? tok : d.vocab_size - 1;
    if (d.out_token) d.out_token[row] = tok;
    if (d.out_kept) d.out_kept[row] = n_kept;
    if (d.out_mass) d.out_mass[row] = mass;
    int64_t* trow = d.tokens + row * d.row_len;
    const bool started = RAGGED || d.prompt_len[row] <= pos;      // ragged: no teacher forcing, the column lies behind the prompt
    if (started) trow[pos] = tok;
    d.next_tok[row] = trow[pos];
    bool term;
    if (d.termination_mode == 2) term = tok == 628 || (tok == 198 && pos > 0 && trow[pos - 1] == 198);
    else if (d.termination_mode == 1) term = tok == 628 || tok == 198;
    else term = tok == d.termination_id;
    const int done = (d.done[row] != 0 || (started && term)) ? 1 : 0;
    d.done[row] = done;
    if (done) atomicAdd(d.n_done, 1);
  }
}

}  // namespace

// the body of the three entries (row_step != nullptr: the steps one, which ignores d->pos); `who` names the entry in the messages
static int launch_sample_advance(const mpv_sample_advance_desc* d, bool ragged, const char* who, hipStream_t stream,
                                 const int32_t* row_step = nullptr, bool steps = false) {
  MPV_REQUIRE(d, MPV_E_ARG, "%s: null descriptor", who);
  MPV_REQUIRE(!steps || row_step, MPV_E_ARG, "%s: null row_step", who);
  MPV_REQUIRE(d->logits && d->tokens && d->prompt_len && d->done && d->next_tok && d->n_done, MPV_E_ARG, "%s: null pointer", who);
  MPV_REQUIRE(d->rows >= 1, MPV_E_SHAPE, "%s: rows (%d) must be positive", who, d->rows);
  MPV_REQUIRE(d->vocab >= 8 && d->vocab <= SA_MAX_VOCAB && d->vocab % 8 == 0, MPV_E_SHAPE, "%s: vocab (%d) must be a multiple of 8 in [8, %d]", who,
              d->vocab, SA_MAX_VOCAB);
  MPV_REQUIRE(d->ld >= d->vocab && d->ld % 8 == 0, MPV_E_SHAPE, "%s: ld (%lld) must be a multiple of 8 and at least vocab (%d)", who,
              (long long)d->ld, d->vocab);
  MPV_REQUIRE(((uintptr_t)d->logits & 15) == 0, MPV_E_ALIGN, "%s: logits must be 16-byte aligned", who);
  MPV_REQUIRE(isfinite(d->temperature) && d->temperature > 0.f, MPV_E_ARG, "%s: temperature (%g) must be finite and positive", who,
              (double)d->temperature);
  MPV_REQUIRE(d->top_k >= 0 && d->top_k <= d->vocab, MPV_E_ARG, "%s: top_k (%d) must be in [0, vocab = %d]", who, d->top_k, d->vocab);
  MPV_REQUIRE(d->top_p >= 0.f && d->top_p <= 1.f, MPV_E_ARG, "%s: top_p (%g) must be in [0, 1]", who, (double)d->top_p);
  MPV_REQUIRE(!(d->top_k > 1 && d->top_p > 0.f), MPV_E_ARG, "%s: cannot set both top-k and top-p samplings", who);
  MPV_REQUIRE(!(d->top_k == 1 && d->top_p > 0.f), MPV_E_ARG, "%s: cannot set both greedy and top-p samplings", who);
  MPV_REQUIRE(d->row_len >= 1 && (steps || (d->pos >= 0 && d->pos < d->row_len)), MPV_E_SHAPE, "%s: %s (%d) must be in [0, row_len = %d)", who,
              ragged ? "step" : "pos", d->pos, d->row_len);
  MPV_REQUIRE(d->termination_mode >= 0 && d->termination_mode <= 2 && d->vocab_size >= 0, MPV_E_ARG,
              "%s: termination_mode (%d) must be 0, 1 or 2 and vocab_size (%d) non-negative", who, d->termination_mode, d->vocab_size);
  if (hipMemsetAsync(d->n_done, 0, sizeof(int32_t), stream) != hipSuccess) {
    mpv_set_error("%s: clearing n_done failed: %s", who, hipGetErrorString(hipGetLastError()));
    return MPV_E_HIP;
  }
  const float exp_scale = (float)(1.4426950408889634 / (double)d->temperature);
  if (steps) hipLaunchKernelGGL(sa_rows<sa_steps_entry>, dim3((unsigned)d->rows), dim3(SA_THREADS), 0, stream, *d, exp_scale, row_step);
  else if (ragged) hipLaunchKernelGGL(sa_rows<sa_ragged_entry>, dim3((unsigned)d->rows), dim3(SA_THREADS), 0, stream, *d, exp_scale, nullptr);
  else hipLaunchKernelGGL(sa_rows<sample_advance_kernel>, dim3((unsigned)d->rows), dim3(SA_THREADS), 0, stream, *d, exp_scale, nullptr);
  return mpv_check_launch(who);
}

extern "C" int mpv_sample_advance_steps(const mpv_sample_advance_desc* d, const int32_t* row_step, hipStream_t stream) {
  return launch_sample_advance(d, true, "mpv_sample_advance_steps", stream, row_step, true);
}

extern "C" int mpv_sample_advance(const mpv_sample_advance_desc* d, hipStream_t stream) {
  return launch_sample_advance(d, false, "mpv_sample_advance", stream);
}

extern "C" int mpv_sample_advance_ragged(const mpv_sample_advance_desc* d, hipStream_t stream) {
  return launch_sample_advance(d, true, "mpv_sample_advance_ragged", stream);
}
