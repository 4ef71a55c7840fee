// Generation constraints on the device: mpv_logits_constrain edits one step's logits in place -- CTRL repetition penalty, no-repeat
// n-gram, minimum length (the end tokens stay banned below min_new_tokens) and a banned-id list -- before mpv_sample_advance or
// mpv_logprob_topk reads them, from the lockstep loops' own device token table.  The semantics are stated in include/mpv.h.
//
// One workgroup of 1024 threads per row; nothing is shared between rows.  The work follows the HISTORY, never the vocabulary: the
// row's history (at most 2047 tokens) and the id lists (at most 1024 + 8) are copied to LDS, and only the logits that are edited are
// touched -- one 2-byte load and one 2-byte store each.  Three steps, a barrier between them:
//   1. copy: hist[i] = tokens[r][start + i]; listed[] = banned_ids followed, while the row is below min_new_tokens, by eos_ids.
//   2. hit[i] = "the n-gram that ends at history position i repeats the current suffix" (ngram 1: every position).  O(m n).
//   3. ONE writer per address.  The thread of history position i walks the whole history once: it owns token v = hist[i] iff no
//      earlier position holds v (the first-occurrence test, O(m^2) over the workgroup, LDS broadcast reads), and v is banned iff some
//      position that holds v is a hit or v is listed.  The owner stores ban_value, or reads the logit, applies the penalty and stores
//      it.  The threads of the listed ids store ban_value too: an id that is also in the history gets the same bits from both.
// No address is read by one thread and written by another, and no address receives two different values: the result does not
// depend on thread timing.  No scratch, no atomics, no floating-point reduction.
//
// The ragged entry (mpv_logits_constrain_ragged) is the same kernel body with the token column a per-workgroup value,
// c_r = clamp(prompt_len[r], 0, row_len) + step; a row whose column lies behind the table is frozen and left as it is.  The steps
// entry (mpv_logits_constrain_steps: rows that entered a running loop at different times) reads the step per row as well, from
// row_step[r]; a negative step freezes the row.
#include "mpv_common.h"
#include "../../include/mpv.h"

#include <math.h>
#include <string.h>
#include <type_traits>

namespace {

constexpr int LC_THREADS = 1024, LC_MAX_ROW = 2048, LC_MAX_EOS = 8, LC_MAX_BANNED = 1024, LC_MAX_NGRAM = 8, LC_MAX_VOCAB = 65536;

// The kernel is a template over an entry tag.  The uniform entry's tag carries the kernel's name of old, so that its symbol still
// contains it (the resource checks and profiles look the uniform kernel up by that name) and the ragged one's does not.
struct logits_constrain_kernel {};    // mpv_logits_constrain: every row at column d.pos
struct lc_ragged_entry {};            // mpv_logits_constrain_ragged: row r at its own column
struct lc_steps_entry {};             // mpv_logits_constrain_steps: row r at its own column AND its own step row_step[r]

template <class Entry>
__global__ __launch_bounds__(LC_THREADS) void lc_rows(mpv_logits_constrain_desc d, unsigned ban_bits, const int32_t* __restrict__ row_step) {
  constexpr bool STEPS = std::is_same<Entry, lc_steps_entry>::value;       // (row_step is read by this instantiation only)
  constexpr bool RAGGED = std::is_same<Entry, lc_ragged_entry>::value || STEPS;
  __shared__ long long hist[LC_MAX_ROW];                       // 16 KiB
  __shared__ long long listed[LC_MAX_BANNED + LC_MAX_EOS];     // 8 KiB
  __shared__ unsigned char hit[LC_MAX_ROW];                    // 2 KiB
  const int tid = threadIdx.x;
  const long long row = blockIdx.x;
  long long pl;
  int pos;
  if (RAGGED) {                                                // the row's own column: its prompt length + the step d.pos
    pl = d.prompt_len[row];
    pl = pl < 0 ? 0 : pl > d.row_len ? d.row_len : pl;
    const int step = STEPS ? row_step[row] : d.pos;
    if (pl + step >= d.row_len || (STEPS && step < 0)) return; // block-uniform: a frozen row stays as it is
    pos = (int)pl + step;
  } else {
    pl = d.prompt_len ? d.prompt_len[row] : d.prompt_len_all;
    if (pl > d.pos) return;                                    // block-uniform: a teacher-forced row stays as it is
    pos = d.pos;
  }
  const int start = d.include_prompt || pl < 0 ? 0 : (int)pl;  // 0 <= start <= pos < row_len <= 2048
  const int m = pos - start, n = d.ngram, vocab = d.vocab;
  const int n_list = d.n_banned + ((long long)pos - pl < d.min_new_tokens ? d.n_eos : 0);

  // ---- 1. the history and the id lists
  const int64_t* trow = d.tokens + row * d.row_len + start;
  for (int i = tid; i < m; i += LC_THREADS) hist[i] = trow[i];
  for (int i = tid; i < n_list; i += LC_THREADS) listed[i] = i < d.n_banned ? d.banned_ids[i] : d.eos_ids[i - d.n_banned];
  __syncthreads();

  // ---- 2. history positions that end a repeat of the suffix s = hist[m - n + 1 : m] (out-of-range tokens compare like any other)
  for (int i = tid; i < m; i += LC_THREADS) {
    bool f = n == 1;
    if (n >= 2 && i >= n - 1) {                                // the gram hist[i - n + 1 : i + 1]; i <= m - 1, so m >= n here
      f = true;
      for (int k = 0; k < n - 1; ++k) f = f && hist[i - (n - 1) + k] == hist[m - (n - 1) + k];
    }
    hit[i] = f ? 1 : 0;
  }
  __syncthreads();

  // ---- 3. one writer per edited logit
  unsigned short* lrow = (unsigned short*)d.logits + row * d.ld;
  for (int i = tid; i < m; i += LC_THREADS) {
    const long long v = hist[i];
    if (v < 0 || v >= vocab) continue;                         // never an address
    bool first = true, ban = false;
    for (int j = 0; j < m; ++j) {
      const bool same = hist[j] == v;
      first = first && !(same && j < i);
      ban = ban || (same && hit[j]);
    }
    if (!first) continue;
    for (int j = 0; j < n_list; ++j) ban = ban || listed[j] == v;
    if (ban) {
      lrow[v] = (unsigned short)ban_bits;
    } else if (d.penalty != 1.f) {
      const float x = __uint_as_float((unsigned)lrow[v] << 16);
      const float y = x < 0.f ? x * d.penalty : __fdiv_rn(x, d.penalty);
      lrow[v] = __builtin_bit_cast(unsigned short, f2bf(y));
    }
  }
  for (int i = tid; i < n_list; i += LC_THREADS) {
    const long long v = listed[i];
    if (v >= 0 && v < vocab) lrow[v] = (unsigned short)ban_bits;
  }
}

// round-to-nearest-even bf16 bits of a float that is -inf or finite
unsigned lc_bf16_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, sizeof u);
  if ((u & 0x7f800000u) == 0x7f800000u) return u >> 16;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

}  // namespace

// the body of the three entries (row_step != nullptr: the steps one, which ignores d->pos); `who` names the entry in the messages
static int launch_logits_constrain(const mpv_logits_constrain_desc* d, bool ragged, const char* who, hipStream_t stream,
                                   const int32_t* row_step = nullptr, bool steps = false) {
  MPV_REQUIRE(d, MPV_E_ARG, "%s: null descriptor", who);
  MPV_REQUIRE(!steps || row_step, MPV_E_ARG, "%s: null row_step", who);
  MPV_REQUIRE(d->logits && d->tokens, MPV_E_ARG, "%s: null logits or tokens", who);
  MPV_REQUIRE(!ragged || d->prompt_len, MPV_E_ARG, "%s: null prompt_len", who);
  MPV_REQUIRE(d->rows >= 1, MPV_E_SHAPE, "%s: rows (%d) must be positive", who, d->rows);
  MPV_REQUIRE(d->vocab >= 8 && d->vocab <= LC_MAX_VOCAB && d->vocab % 8 == 0, MPV_E_SHAPE, "%s: vocab (%d) must be a multiple of 8 in [8, %d]", who,
              d->vocab, LC_MAX_VOCAB);
  MPV_REQUIRE(d->ld >= d->vocab && d->ld % 8 == 0, MPV_E_SHAPE, "%s: ld (%lld) must be a multiple of 8 and at least vocab (%d)", who,
              (long long)d->ld, d->vocab);
  MPV_REQUIRE(((uintptr_t)d->logits & 15) == 0, MPV_E_ALIGN, "%s: logits must be 16-byte aligned", who);
  MPV_REQUIRE(d->row_len >= 1 && d->row_len <= LC_MAX_ROW, MPV_E_SHAPE, "%s: row_len (%d) must be in [1, %d]", who, d->row_len, LC_MAX_ROW);
  MPV_REQUIRE(steps || (d->pos >= 0 && d->pos < d->row_len), MPV_E_SHAPE, "%s: %s (%d) must be in [0, row_len = %d)", who, ragged ? "step" : "pos",
              d->pos, d->row_len);
  MPV_REQUIRE(isfinite(d->penalty) && d->penalty > 0.f, MPV_E_ARG, "%s: penalty (%g) must be finite and positive", who, (double)d->penalty);
  MPV_REQUIRE(d->ngram >= 0 && d->ngram <= LC_MAX_NGRAM, MPV_E_ARG, "%s: ngram (%d) must be in [0, %d]", who, d->ngram, LC_MAX_NGRAM);
  MPV_REQUIRE(d->min_new_tokens >= 0, MPV_E_ARG, "%s: min_new_tokens (%d) must not be negative", who, d->min_new_tokens);
  MPV_REQUIRE(d->include_prompt == 0 || d->include_prompt == 1, MPV_E_ARG, "%s: include_prompt (%d) must be 0 or 1", who, d->include_prompt);
  MPV_REQUIRE(d->n_eos >= 0 && d->n_eos <= LC_MAX_EOS && (d->n_eos == 0 || d->eos_ids), MPV_E_ARG,
              "%s: n_eos (%d) must be in [0, %d], with an array when positive", who, d->n_eos, LC_MAX_EOS);
  MPV_REQUIRE(d->n_banned >= 0 && d->n_banned <= LC_MAX_BANNED && (d->n_banned == 0 || d->banned_ids), MPV_E_ARG,
              "%s: n_banned (%d) must be in [0, %d], with an array when positive", who, d->n_banned, LC_MAX_BANNED);
  MPV_REQUIRE(!isnan(d->ban_value) && d->ban_value < 0.f, MPV_E_ARG, "%s: ban_value (%g) must be -inf or a finite negative number", who,
              (double)d->ban_value);
  if (d->penalty == 1.f && d->ngram == 0 && d->n_banned == 0 && (d->min_new_tokens == 0 || d->n_eos == 0)) return MPV_OK;      // everything off
  const unsigned ban_bits = lc_bf16_bits(d->ban_value);
  if (steps) hipLaunchKernelGGL(lc_rows<lc_steps_entry>, dim3((unsigned)d->rows), dim3(LC_THREADS), 0, stream, *d, ban_bits, row_step);
  else if (ragged) hipLaunchKernelGGL(lc_rows<lc_ragged_entry>, dim3((unsigned)d->rows), dim3(LC_THREADS), 0, stream, *d, ban_bits, nullptr);
  else hipLaunchKernelGGL(lc_rows<logits_constrain_kernel>, dim3((unsigned)d->rows), dim3(LC_THREADS), 0, stream, *d, ban_bits, nullptr);
  return mpv_check_launch(who);
}

extern "C" int mpv_logits_constrain_steps(const mpv_logits_constrain_desc* d, const int32_t* row_step, hipStream_t stream) {
  return launch_logits_constrain(d, true, "mpv_logits_constrain_steps", stream, row_step, true);
}

extern "C" int mpv_logits_constrain(const mpv_logits_constrain_desc* d, hipStream_t stream) {
  return launch_logits_constrain(d, false, "mpv_logits_constrain", stream);
}

extern "C" int mpv_logits_constrain_ragged(const mpv_logits_constrain_desc* d, hipStream_t stream) {
  return launch_logits_constrain(d, true, "mpv_logits_constrain_ragged", stream);
}
