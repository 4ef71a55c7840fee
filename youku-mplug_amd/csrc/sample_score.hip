// Sequence scores of sampled generation on the device: mpv_sample_score records, for every sequence of a lockstep batch, the model's
// log-probability of the token that mpv_sample_advance has just written into column `pos` -- log_softmax over the logits the sampler
// read (after mpv_logits_constrain edited them), not over the tempered or filtered proposal.  The semantics are stated in
// include/mpv.h.
//
// One workgroup of 1024 threads per row; nothing is shared between rows, so a row's score depends neither on `rows` nor on its place
// in the launch.  A row that is teacher-forced or no longer live returns after two scalar reads.  Otherwise the row (at most 65536
// bf16) is read from memory ONCE, with 16-byte loads, into registers: thread t holds the eight logits of vector v = c * 1024 + t for
// c = 0 .. 7 (32 registers).  Two passes over the registers, no online rescaling:
//   1. m = max x_i (exact in any order): lane-local, xor butterfly, the 16 wave maxima through LDS.
//   2. S = sum exp(x_i - m): lane-local in element order, xor butterfly (a + b is commutative: every lane holds the same bits), the 16
//      wave partials through LDS, added in wave order by thread 0.
// Thread 0 then reads the token and its logit (one 2-byte load), forms lp = x_t - (m + log S) and does the bookkeeping.  Every sum runs
// in a fixed order and there is no atomic: the outputs are bit-reproducible.  No scratch.
//
// The ragged entry (mpv_sample_score_ragged) is the same kernel body with the token column a per-workgroup value,
// c_r = clamp(prompt_len[r], 0, row_len) + step; a row whose column lies behind the table is frozen and returns like a dead one.
// The steps entry (mpv_sample_score_steps) reads the step per row as well, from row_step[r]; a negative step freezes the row.
#include "mpv_common.h"
#include "../../include/mpv.h"

#include <math.h>
#include <type_traits>

namespace {

constexpr int SS_THREADS = 1024, SS_WAVES = SS_THREADS / 64, SS_SLOTS = 8;
constexpr int SS_MAX_VOCAB = SS_THREADS * SS_SLOTS * 8, SS_MAX_ROW = 2048;
constexpr unsigned SS_NEG_INF_PAIR = 0xff80ff80u;        // two bf16 -inf: what a vector slot past the vocabulary holds

// The kernel is a template over an entry tag.  The uniform entry's tag carries the kernel's name of old, so that its symbol still
// contains it (the resource checks and profiles look the uniform kernel up by that name) and the ragged one's does not.
struct sample_score_kernel {};        // mpv_sample_score: every row at column d.pos
struct ss_ragged_entry {};            // mpv_sample_score_ragged: row r at its own column
struct ss_steps_entry {};             // mpv_sample_score_steps: row r at its own column AND its own step row_step[r]

template <class Entry>
__global__ __launch_bounds__(SS_THREADS) void ss_rows(mpv_sample_score_desc d, const int32_t* __restrict__ row_step) {
  constexpr bool STEPS = std::is_same<Entry, ss_steps_entry>::value;       // (row_step is read by this instantiation only)
  constexpr bool RAGGED = std::is_same<Entry, ss_ragged_entry>::value || STEPS;
  __shared__ float wave_m[SS_WAVES], wave_s[SS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long row = blockIdx.x;
  int pos = d.pos;
  if (RAGGED) {                                                // the row's own column: its prompt length + the step d.pos
    long long pl = d.prompt_len[row];
    pl = pl < 0 ? 0 : pl > d.row_len ? d.row_len : pl;
    const int step = STEPS ? row_step[row] : d.pos;
    if (pl + step >= d.row_len || (STEPS && step < 0) || d.live[row] == 0) return;   // block-uniform: frozen, or scored to its end already
    pos = (int)pl + step;
  } else if (d.prompt_len[row] > d.pos || d.live[row] == 0) {
    return;                                                    // block-uniform (live is rewritten behind the last barrier only)
  }
  const int vocab = d.vocab;
  const float ninf = -INFINITY;

  // ---- the row, once; a vector is inside the row or outside it (vocab % 8 == 0)
  const bf16* lrow = (const bf16*)d.logits + row * d.ld;
  uint4 raw[SS_SLOTS];
#pragma unroll
  for (int c = 0; c < SS_SLOTS; ++c) {
    const int base = (c * SS_THREADS + tid) * 8;
    raw[c] = make_uint4(SS_NEG_INF_PAIR, SS_NEG_INF_PAIR, SS_NEG_INF_PAIR, SS_NEG_INF_PAIR);
    if (base < vocab) raw[c] = *(const uint4*)(lrow + base);
  }

  // ---- 1. the maximum
  float m = ninf;
#pragma unroll
  for (int c = 0; c < SS_SLOTS; ++c) {
    const unsigned w[4] = {raw[c].x, raw[c].y, raw[c].z, raw[c].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) m = fmaxf(m, fmaxf(__uint_as_float(w[j] << 16), __uint_as_float(w[j] & 0xffff0000u)));
  }
  m = wave_max(m);
  if (lane == 0) wave_m[wave] = m;
  __syncthreads();
  m = wave_m[0];
#pragma unroll
  for (int w = 1; w < SS_WAVES; ++w) m = fmaxf(m, wave_m[w]);

  // ---- 2. the sum of exp(x - m); -inf contributes 0 (also in a row of -inf only, where x - m would be NaN)
  float part = 0.f;
#pragma unroll
  for (int c = 0; c < SS_SLOTS; ++c) {
    const unsigned w[4] = {raw[c].x, raw[c].y, raw[c].z, raw[c].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float lo = __uint_as_float(w[j] << 16), hi = __uint_as_float(w[j] & 0xffff0000u);
      part += lo == ninf ? 0.f : mpv_exp(lo - m);
      part += hi == ninf ? 0.f : mpv_exp(hi - m);
    }
  }
  part = wave_sum(part);
  if (lane == 0) wave_s[wave] = part;
  __syncthreads();

  // ---- the score and the bookkeeping, by one thread
  if (tid == 0) {
    float S = 0.f;
#pragma unroll
    for (int w = 0; w < SS_WAVES; ++w) S += wave_s[w];
    const long long at = row * d.row_len + pos;
    const long long t = d.tokens[at];
    float lp = __builtin_nanf("");                       // a token outside [0, vocab): misuse, made loud
    if (t >= 0 && t < vocab) {
      const float xt = bf2f(lrow[t]);
      lp = xt == ninf ? ninf : xt - (m + logf(S));
    }
    d.token_logprob[at] = lp;
    d.sum_logprob[row] += lp;
    d.count[row] += 1;
    d.live[row] = d.done[row] ? 0 : 1;
  }
}

}  // namespace

// the body of the three entries (row_step != nullptr: the steps one, which ignores d->pos); `who` names the entry in the messages
static int launch_sample_score(const mpv_sample_score_desc* d, bool ragged, const char* who, hipStream_t stream,
                               const int32_t* row_step = nullptr, bool steps = false) {
  MPV_REQUIRE(d, MPV_E_ARG, "%s: null descriptor", who);
  MPV_REQUIRE(!steps || row_step, MPV_E_ARG, "%s: null row_step", who);
  MPV_REQUIRE(d->logits && d->tokens && d->prompt_len && d->done && d->live && d->token_logprob && d->sum_logprob && d->count, MPV_E_ARG,
              "%s: null pointer", who);
  MPV_REQUIRE(d->rows >= 1, MPV_E_SHAPE, "%s: rows (%d) must be positive", who, d->rows);
  MPV_REQUIRE(d->vocab >= 8 && d->vocab <= SS_MAX_VOCAB && d->vocab % 8 == 0, MPV_E_SHAPE, "%s: vocab (%d) must be a multiple of 8 in [8, %d]", who,
              d->vocab, SS_MAX_VOCAB);
  MPV_REQUIRE(d->ld >= d->vocab && d->ld % 8 == 0, MPV_E_SHAPE, "%s: ld (%lld) must be a multiple of 8 and at least vocab (%d)", who,
              (long long)d->ld, d->vocab);
  MPV_REQUIRE(((uintptr_t)d->logits & 15) == 0, MPV_E_ALIGN, "%s: logits must be 16-byte aligned", who);
  MPV_REQUIRE(d->row_len >= 1 && d->row_len <= SS_MAX_ROW, MPV_E_SHAPE, "%s: row_len (%d) must be in [1, %d]", who, d->row_len, SS_MAX_ROW);
  MPV_REQUIRE(steps || (d->pos >= 0 && d->pos < d->row_len), MPV_E_SHAPE, "%s: %s (%d) must be in [0, row_len = %d)", who, ragged ? "step" : "pos",
              d->pos, d->row_len);
  if (steps) hipLaunchKernelGGL(ss_rows<ss_steps_entry>, dim3((unsigned)d->rows), dim3(SS_THREADS), 0, stream, *d, row_step);
  else if (ragged) hipLaunchKernelGGL(ss_rows<ss_ragged_entry>, dim3((unsigned)d->rows), dim3(SS_THREADS), 0, stream, *d, nullptr);
  else hipLaunchKernelGGL(ss_rows<sample_score_kernel>, dim3((unsigned)d->rows), dim3(SS_THREADS), 0, stream, *d, nullptr);
  return mpv_check_launch(who);
}

extern "C" int mpv_sample_score_steps(const mpv_sample_score_desc* d, const int32_t* row_step, hipStream_t stream) {
  return launch_sample_score(d, true, "mpv_sample_score_steps", stream, row_step, true);
}

extern "C" int mpv_sample_score(const mpv_sample_score_desc* d, hipStream_t stream) {
  return launch_sample_score(d, false, "mpv_sample_score", stream);
}

extern "C" int mpv_sample_score_ragged(const mpv_sample_score_desc* d, hipStream_t stream) {
  return launch_sample_score(d, true, "mpv_sample_score_ragged", stream);
}
