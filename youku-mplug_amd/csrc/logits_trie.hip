// Closed-vocabulary generation on the device: mpv_logits_trie_mask keeps, in one step's logits, only the tokens that continue the row's
// generated history along a trie of allowed phrases (generation.PhraseTrie, flattened to CSR arrays), before mpv_sample_advance or
// mpv_logprob_topk reads them.  The semantics are stated in include/mpv.h.
//
// One workgroup of 1024 threads per row; nothing is shared between rows.  Three steps, a barrier between them:
//   1. copy: hist[i] = tokens[r][prompt_len[r] + i], the generated tokens, to LDS.
//   2. walk (wave 0): from the root, one level per history token.  The children of a node are a sorted run of child_tok; the wave
//      narrows the run 64 ways per round (lane i probes the i-th of 64 evenly spaced entries, one ballot says in which piece the token
//      lies) until it holds at most 64 entries, which one load per lane and one ballot decide.  A root of 51200 children takes two
//      rounds and the final look; a single lane's binary search would take sixteen dependent global loads.  Every quantity of the walk
//      is wave-uniform.  The node (or -1: dead) goes to LDS.
//   3. mask: the allowed set is the node's sorted child run, staged in LDS when it holds at most TM_STAGE tokens, plus the termination
//      ids when the node ends a phrase or the row is dead.  A thread owns whole 8-column (16-byte) chunks: a lower bound in the child
//      run says whether the chunk holds an allowed token.  If none, the chunk is stored as eight ban values WITHOUT being loaded; if
//      all eight are allowed it is neither loaded nor stored; otherwise it is loaded, the columns that are not allowed are replaced
//      and it is stored once.  One writer per column, 16-byte accesses only, columns >= vocab never touched.
// No scratch, no atomics, no floating-point arithmetic: the result does not depend on thread timing.
//
// The ragged entry (mpv_logits_trie_mask_ragged) and the steps entry (mpv_logits_trie_mask_steps) are the same kernel body with the
// column a per-workgroup value, exactly as in logits_constrain.hip.
#include "mpv_common.h"
#include "../../include/mpv.h"

#include <math.h>
#include <string.h>
#include <type_traits>

namespace {

constexpr int TM_THREADS = 1024, TM_MAX_ROW = 2048, TM_MAX_EOS = 8, TM_MAX_VOCAB = 65536, TM_STAGE = 4096;

struct logits_trie_mask_kernel {};    // mpv_logits_trie_mask: every row at column d.pos (the symbol carries the name)
struct tm_ragged_entry {};            // mpv_logits_trie_mask_ragged: row r at its own column
struct tm_steps_entry {};             // mpv_logits_trie_mask_steps: row r at its own column AND its own step row_step[r]

// the mask of one row over the sorted allowed run ch[0 : nc) (LDS or global: the address space is the caller's) and eos[0 : n_eos)
template <class Ptr>
__device__ __forceinline__ void tm_mask_row(uint4* __restrict__ lrow, int nchunks, Ptr ch, int nc, const int* eos, int n_eos, unsigned ban2, int tid) {
  const uint4 ban4 = make_uint4(ban2, ban2, ban2, ban2);
  const int lo_tok = nc ? ch[0] : 0x7fffffff, hi_tok = nc ? ch[nc - 1] : -1;
  for (int k = tid; k < nchunks; k += TM_THREADS) {
    const int c0 = k * 8;
    unsigned keep = 0;                                         // bit j: column c0 + j is allowed
    if (c0 + 7 >= lo_tok && c0 <= hi_tok) {
      int lo = 0, hi = nc;                                     // lower bound of c0 in the run
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ch[mid] < c0) lo = mid + 1; else hi = mid;
      }
      for (int j = lo; j < nc; ++j) {
        const unsigned off = (unsigned)(ch[j] - c0);
        if (off >= 8u) break;
        keep |= 1u << off;
      }
    }
    for (int q = 0; q < n_eos; ++q) {
      const unsigned off = (unsigned)(eos[q] - c0);
      if (off < 8u) keep |= 1u << off;
    }
    if (keep == 0xffu) continue;                               // every column allowed: the chunk keeps its bits
    uint4 v = ban4;
    if (keep) {
      const uint4 x = lrow[k];
      const unsigned w[4] = {x.x, x.y, x.z, x.w};
      unsigned o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned m = ((keep >> (2 * j)) & 1u ? 0x0000ffffu : 0u) | ((keep >> (2 * j + 1)) & 1u ? 0xffff0000u : 0u);
        o[j] = (w[j] & m) | (ban2 & ~m);
      }
      v = make_uint4(o[0], o[1], o[2], o[3]);
    }
    lrow[k] = v;
  }
}

template <class Entry>
__global__ __launch_bounds__(TM_THREADS) void tm_rows(mpv_logits_trie_desc d, unsigned ban_bits, const int32_t* __restrict__ row_step) {
  constexpr bool STEPS = std::is_same<Entry, tm_steps_entry>::value;
  constexpr bool RAGGED = std::is_same<Entry, tm_ragged_entry>::value || STEPS;
  __shared__ long long hist[TM_MAX_ROW];                       // 16 KiB
  __shared__ int staged[TM_STAGE];                             // 16 KiB
  __shared__ int eos_in[TM_MAX_EOS];
  __shared__ int sh_node;
  const int tid = threadIdx.x;
  const long long row = blockIdx.x;
  long long pl;
  int pos;
  bool frozen;
  if (RAGGED) {                                                // the row's own column: its prompt length + the step
    pl = d.prompt_len[row];
    pl = pl < 0 ? 0 : pl > d.row_len ? d.row_len : pl;
    const int step = STEPS ? row_step[row] : d.pos;
    frozen = pl + step >= d.row_len || (STEPS && step < 0);
    pos = (int)pl + step;
  } else {
    pl = d.prompt_len ? d.prompt_len[row] : d.prompt_len_all;
    frozen = pl > d.pos;                                       // a teacher-forced row
    pos = d.pos;
  }
  if (frozen) {                                                // block-uniform: the row stays as it is
    if (tid == 0 && d.node_out) d.node_out[row] = -2;
    return;
  }
  const int start = pl < 0 ? 0 : (int)pl;                      // 0 <= start <= pos < row_len <= 2048
  const int m = pos - start, vocab = d.vocab;

  // ---- 1. the generated tokens
  const int64_t* trow = d.tokens + row * d.row_len + start;
  for (int i = tid; i < m; i += TM_THREADS) hist[i] = trow[i];
  __syncthreads();

  // ---- 2. the walk, by wave 0; every index that comes out of the arrays is checked before it becomes an address
  if (tid < 64) {
    int u = 0;
    bool dead = false;
    for (int i = 0; i < m && !dead; ++i) {
      const long long t = hist[i];
      int b = d.child_begin[u], e = d.child_begin[u + 1];
      b = b < 0 ? 0 : b;
      e = e > d.n_edges ? d.n_edges : e;
      if (t < 0 || t >= vocab || b >= e) { dead = true; break; }
      const int tt = (int)t;
      while (e - b > 64) {                                     // 64-ary narrowing of the sorted run
        const int step = (e - b + 63) >> 6;
        const int idx = b + tid * step;
        const int v = idx < e ? d.child_tok[idx] : 0x7fffffff;
        const int cnt = __popcll(__ballot(v <= tt));           // a prefix of the lanes: the run ascends
        if (cnt == 0) { e = b; break; }
        b += (cnt - 1) * step;
        e = b + step < e ? b + step : e;
      }
      const int v = b + tid < e ? d.child_tok[b + tid] : -1;
      const unsigned long long hit = __ballot(v == tt);
      if (!hit) { dead = true; break; }
      u = d.child_node[b + __ffsll((long long)hit) - 1];
      if (u < 0 || u >= d.n_nodes) dead = true;
    }
    if (tid == 0) {
      sh_node = dead ? -1 : u;
      if (d.node_out) d.node_out[row] = dead ? -1 : u;
    }
  }
  if (tid >= 64 && tid < 64 + TM_MAX_EOS) {                    // meanwhile: the termination ids that are columns
    const int q = tid - 64;
    long long v = q < d.n_eos ? d.eos_ids[q] : -1;
    eos_in[q] = v >= 0 && v < vocab ? (int)v : -8;             // -8: no column of any chunk
  }
  __syncthreads();

  // ---- 3. the mask
  const int u = sh_node;
  int b = 0, e = 0;
  bool ends = true;                                            // dead: the termination ids only
  if (u >= 0) {
    b = d.child_begin[u];
    e = d.child_begin[u + 1];
    b = b < 0 ? 0 : b;
    e = e > d.n_edges ? d.n_edges : e;
    e = e < b ? b : e;
    ends = d.terminal[u] >= 0;
  }
  const int nc = e - b, n_eos = ends ? d.n_eos : 0;
  uint4* lrow = (uint4*)((unsigned short*)d.logits + row * d.ld);
  const unsigned ban2 = ban_bits | (ban_bits << 16);
  if (nc <= TM_STAGE) {
    for (int i = tid; i < nc; i += TM_THREADS) staged[i] = d.child_tok[b + i];
    __syncthreads();
    tm_mask_row(lrow, vocab >> 3, (const int*)staged, nc, eos_in, n_eos, ban2, tid);
  } else {
    tm_mask_row(lrow, vocab >> 3, d.child_tok + b, nc, eos_in, n_eos, ban2, tid);
  }
}

// round-to-nearest-even bf16 bits of a float that is -inf or finite
unsigned tm_bf16_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, sizeof u);
  if ((u & 0x7f800000u) == 0x7f800000u) return u >> 16;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

}  // namespace

// the body of the three entries (row_step != nullptr: the steps one, which ignores d->pos); `who` names the entry in the messages
static int launch_logits_trie(const mpv_logits_trie_desc* d, bool ragged, const char* who, hipStream_t stream, const int32_t* row_step = nullptr,
                              bool steps = false) {
  MPV_REQUIRE(d, MPV_E_ARG, "%s: null descriptor", who);
  MPV_REQUIRE(!steps || row_step, MPV_E_ARG, "%s: null row_step", who);
  MPV_REQUIRE(d->logits && d->tokens, MPV_E_ARG, "%s: null logits or tokens", who);
  MPV_REQUIRE(!ragged || d->prompt_len, MPV_E_ARG, "%s: null prompt_len", who);
  MPV_REQUIRE(d->rows >= 1, MPV_E_SHAPE, "%s: rows (%d) must be positive", who, d->rows);
  MPV_REQUIRE(d->vocab >= 8 && d->vocab <= TM_MAX_VOCAB && d->vocab % 8 == 0, MPV_E_SHAPE, "%s: vocab (%d) must be a multiple of 8 in [8, %d]", who,
              d->vocab, TM_MAX_VOCAB);
  MPV_REQUIRE(d->ld >= d->vocab && d->ld % 8 == 0, MPV_E_SHAPE, "%s: ld (%lld) must be a multiple of 8 and at least vocab (%d)", who,
              (long long)d->ld, d->vocab);
  MPV_REQUIRE(((uintptr_t)d->logits & 15) == 0, MPV_E_ALIGN, "%s: logits must be 16-byte aligned", who);
  MPV_REQUIRE(d->row_len >= 1 && d->row_len <= TM_MAX_ROW, MPV_E_SHAPE, "%s: row_len (%d) must be in [1, %d]", who, d->row_len, TM_MAX_ROW);
  MPV_REQUIRE(steps || (d->pos >= 0 && d->pos < d->row_len), MPV_E_SHAPE, "%s: %s (%d) must be in [0, row_len = %d)", who, ragged ? "step" : "pos",
              d->pos, d->row_len);
  MPV_REQUIRE(d->n_eos >= 1 && d->n_eos <= TM_MAX_EOS && d->eos_ids, MPV_E_ARG, "%s: n_eos (%d) must be in [1, %d], with an array", who, d->n_eos,
              TM_MAX_EOS);
  MPV_REQUIRE(d->child_begin && d->child_tok && d->child_node && d->terminal, MPV_E_ARG, "%s: null trie array", who);
  MPV_REQUIRE(d->n_nodes >= 1 && d->n_edges >= 0, MPV_E_ARG, "%s: n_nodes (%d) must be positive and n_edges (%d) not negative", who, d->n_nodes,
              d->n_edges);
  MPV_REQUIRE(!isnan(d->ban_value) && d->ban_value < 0.f, MPV_E_ARG, "%s: ban_value (%g) must be -inf or a finite negative number", who,
              (double)d->ban_value);
  const unsigned ban_bits = tm_bf16_bits(d->ban_value);
  if (steps) hipLaunchKernelGGL(tm_rows<tm_steps_entry>, dim3((unsigned)d->rows), dim3(TM_THREADS), 0, stream, *d, ban_bits, row_step);
  else if (ragged) hipLaunchKernelGGL(tm_rows<tm_ragged_entry>, dim3((unsigned)d->rows), dim3(TM_THREADS), 0, stream, *d, ban_bits, nullptr);
  else hipLaunchKernelGGL(tm_rows<logits_trie_mask_kernel>, dim3((unsigned)d->rows), dim3(TM_THREADS), 0, stream, *d, ban_bits, nullptr);
  return mpv_check_launch(who);
}

extern "C" int mpv_logits_trie_mask(const mpv_logits_trie_desc* d, hipStream_t stream) {
  return launch_logits_trie(d, false, "mpv_logits_trie_mask", stream);
}

extern "C" int mpv_logits_trie_mask_ragged(const mpv_logits_trie_desc* d, hipStream_t stream) {
  return launch_logits_trie(d, true, "mpv_logits_trie_mask_ragged", stream);
}

extern "C" int mpv_logits_trie_mask_steps(const mpv_logits_trie_desc* d, const int32_t* row_step, hipStream_t stream) {
  return launch_logits_trie(d, true, "mpv_logits_trie_mask_steps", stream, row_step, true);
}
