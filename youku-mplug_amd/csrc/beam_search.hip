// Lockstep beam search over a batch of clips (caption evaluation): mpv_beam_advance does, for every clip of the batch, what ONE
// iteration of generation.beam_search_loop does on the host for one clip -- models/modeling_distributed_gpt3.py:1793-1840 (candidate
// order, stop-token handling, next beams) and BeamHypotheses.add / is_done (:1908-1960) -- so that a decode step of B clips x K beams
// needs no host bookkeeping: the step's outputs (source row and new token of every sequence) stay on the device and feed the KV
// re-order and the next decode step.
//
// One workgroup of one wave per clip; nothing is shared between clips, so a clip's result depends neither on the batch size nor
// on its place in the batch.
//   1. rank: the clip's candidates (2K of beam 0 on the first step, K x 2K afterwards; <= 128) are parked in LDS and every lane
//      counts, for its (at most two) candidates, how many come before them under the order rule
//          value descending, then beam * V + token ascending (then position in the input, which only matters for malformed input);
//      that count is the candidate's rank -- a total order, so the ranks are distinct -- and the candidates of rank < 2K write
//      themselves to slot `rank` of the sorted list.  No atomics, no dependence on the order in which lanes run.
//   2. walk: the sorted list is walked in rank order with wave-uniform control flow (every lane holds the same heap state in
//      registers and reads the same LDS words).  The walk is latency work (<= 16 entries); the lanes only differ in the row copies:
//      a stop token of rank < K copies the Lt tokens of its source row into the hypothesis store, lane l taking positions
//      l, l + 64, ...  The heap arithmetic is fp64 on fp32 inputs -- double(value) / Lt, compared with `worst` -- which is what the
//      Python floats of the host loop do, bit for bit (one correctly rounded fp64 division; no pow: length_penalty is 1.0).
//   3. finish: done test, state write-back, and unless the clip is (or has just become) done the K row copies into the other
//      token table with the new token written at `pos`, the new beam scores, src_row and next_tok.
// A done clip is frozen: its rows go to the other token table unchanged (the tables are swapped by the caller after every call),
// it gets identity src_row and the stop token, and nothing else of its state is written.
#include "mpv_common.h"
#include "../../include/mpv.h"

namespace {

constexpr int BA_MAX_K = 8, BA_MAX_LT = 2048, BA_MAX_CAND = BA_MAX_K * 2 * BA_MAX_K;

// candidate (va, ka, ia) comes before (vb, kb, ib)
__device__ __forceinline__ bool ba_before(float va, long long ka, int ia, float vb, long long kb, int ib) {
  return va > vb || (va == vb && (ka < kb || (ka == kb && ia < ib)));
}

__global__ __launch_bounds__(64) void beam_advance_kernel(mpv_beam_advance_desc d) {
  __shared__ float c_val[BA_MAX_CAND];
  __shared__ long long c_key[BA_MAX_CAND];
  __shared__ long long c_tok[BA_MAX_CAND];
  __shared__ float s_val[2 * BA_MAX_K];
  __shared__ int s_beam[2 * BA_MAX_K];
  __shared__ long long s_tok[2 * BA_MAX_K];
  __shared__ float n_val[BA_MAX_K];                      // the next beams: (value, source beam, token)
  __shared__ int n_beam[BA_MAX_K];
  __shared__ long long n_tok[BA_MAX_K];
  const int lane = threadIdx.x, K = d.beams, K2 = 2 * K, Lt = d.row_len;
  const long long b = blockIdx.x, row0 = b * K;
  const int64_t* tin = d.tokens_in + row0 * Lt;
  int64_t* tout = d.tokens_out + row0 * Lt;

  if (d.done[b]) {                                       // frozen: wave-uniform
    for (int j = 0; j < K; ++j)
      for (int t = lane; t < Lt; t += 64) tout[(long long)j * Lt + t] = tin[(long long)j * Lt + t];
    if (lane < K) {
      d.src_row[row0 + lane] = row0 + lane;
      d.next_tok[row0 + lane] = d.stop_token;
    }
    return;
  }

  // ---- 1. rank
  const int n_cand = d.first ? K2 : K * K2;              // the first step reads beam 0 only (:1793-1795)
  for (int i = lane; i < n_cand; i += 64) {
    const long long tok = d.cand_idx[row0 * K2 + i];
    c_val[i] = d.cand_val[row0 * K2 + i];
    c_tok[i] = tok;
    c_key[i] = (long long)(i / K2) * d.vocab + tok;
  }
  __syncthreads();
  for (int i = lane; i < n_cand; i += 64) {
    const float v = c_val[i];
    const long long key = c_key[i];
    int rank = 0;
    for (int j = 0; j < n_cand; ++j) rank += ba_before(c_val[j], c_key[j], j, v, key, i) ? 1 : 0;
    if (rank < K2) {
      s_val[rank] = v;
      s_beam[rank] = i / K2;
      s_tok[rank] = c_tok[i];
    }
  }
  __syncthreads();

  // ---- 2. walk (wave-uniform)
  double hs[BA_MAX_K];
  int ho[BA_MAX_K];
#pragma unroll
  for (int j = 0; j < BA_MAX_K; ++j) {
    hs[j] = j < K ? d.hyp_score[row0 + j] : 0.0;
    ho[j] = j < K ? d.hyp_order[row0 + j] : 0;
  }
  int count = d.hyp_count[b], next = d.hyp_next[b];
  double worst = d.worst[b];
  int64_t* hyp_rows = d.hyp_tokens + row0 * Lt;
  int n_next = 0;
  for (int r = 0; r < K2 && n_next < K; ++r) {
    const float v = s_val[r];
    const int beam = s_beam[r];
    const long long tok = s_tok[r];
    if (tok != d.stop_token) {
      if (lane == 0) {
        n_val[n_next] = v;
        n_beam[n_next] = beam;
        n_tok[n_next] = tok;
      }
      ++n_next;
      continue;
    }
    if (r >= K) continue;                                // :1809-1812
    const double score = (double)v / (double)Lt;         // BeamHypotheses.add: sum_logprobs / len(row) ** 1.0 (:1936)
    if (!(count < K || score > worst)) continue;
    int slot = count;
    if (count < K) {
      ++count;
      worst = score < worst ? score : worst;
    } else {
      // evict the lowest score, ties to the earliest inserted; the new entry is above `worst`, so it is never the one to go
      slot = 0;
      double ls = hs[0];
      int lo = ho[0];
#pragma unroll
      for (int j = 1; j < BA_MAX_K; ++j)
        if (j < K && (hs[j] < ls || (hs[j] == ls && ho[j] < lo))) slot = j, ls = hs[j], lo = ho[j];
      worst = score;                                     // becomes the lowest of what stays (:1942-1944: the second lowest of K + 1)
#pragma unroll
      for (int j = 0; j < BA_MAX_K; ++j)
        if (j < K && j != slot && hs[j] < worst) worst = hs[j];
    }
#pragma unroll
    for (int j = 0; j < BA_MAX_K; ++j)
      if (j == slot) hs[j] = score, ho[j] = next;
    ++next;
    for (int t = lane; t < Lt; t += 64) hyp_rows[(long long)slot * Lt + t] = tin[(long long)beam * Lt + t];
  }

  // ---- 3. finish
  const bool now_done = count == K && worst >= (double)s_val[0] / (double)d.cur_len;      // is_done (:1946-1960)
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < BA_MAX_K; ++j)
      if (j < K) {
        d.hyp_score[row0 + j] = hs[j];
        d.hyp_order[row0 + j] = ho[j];
      }
    d.hyp_count[b] = count;
    d.hyp_next[b] = next;
    d.worst[b] = worst;
    d.done[b] = now_done ? 1 : 0;
  }
  __syncthreads();                                       // n_val / n_beam / n_tok of lane 0
  if (now_done) {
    for (int j = 0; j < K; ++j)
      for (int t = lane; t < Lt; t += 64) tout[(long long)j * Lt + t] = tin[(long long)j * Lt + t];
    if (lane < K) {
      d.src_row[row0 + lane] = row0 + lane;
      d.next_tok[row0 + lane] = d.stop_token;
    }
    return;
  }
  for (int j = 0; j < K; ++j) {
    // fewer than K next beams cannot come out of 2K candidates with distinct tokens per beam; a slot left over keeps its own row
    const bool have = j < n_next;
    const int beam = have ? n_beam[j] : j;
    const long long tok = have ? n_tok[j] : d.stop_token;
    for (int t = lane; t < Lt; t += 64) tout[(long long)j * Lt + t] = t == d.pos ? tok : tin[(long long)beam * Lt + t];
    if (lane == 0) {
      d.scores[row0 + j] = have ? n_val[j] : -INFINITY;
      d.src_row[row0 + j] = row0 + beam;
      d.next_tok[row0 + j] = tok;
    }
  }
}

}  // namespace

extern "C" int mpv_beam_advance(const mpv_beam_advance_desc* d, hipStream_t stream) {
  MPV_REQUIRE(d, MPV_E_ARG, "mpv_beam_advance: null descriptor");
  MPV_REQUIRE(d->beams >= 1 && d->beams <= BA_MAX_K, MPV_E_SHAPE, "mpv_beam_advance: beams (%d) must be in [1, %d]", d->beams, BA_MAX_K);
  MPV_REQUIRE(d->row_len >= 1 && d->row_len <= BA_MAX_LT, MPV_E_SHAPE, "mpv_beam_advance: row_len (%d) must be in [1, %d]", d->row_len,
              BA_MAX_LT);
  MPV_REQUIRE(d->batch >= 1 && d->vocab >= 1 && d->cur_len >= 1 && d->pos >= 0 && d->pos < d->row_len, MPV_E_SHAPE,
              "mpv_beam_advance: bad shape batch=%d vocab=%d cur_len=%d pos=%d (row_len %d)", d->batch, d->vocab, d->cur_len, d->pos,
              d->row_len);
  MPV_REQUIRE(d->cand_val && d->cand_idx && d->tokens_in && d->tokens_out && d->scores && d->hyp_score && d->hyp_order && d->hyp_tokens &&
                  d->hyp_count && d->hyp_next && d->worst && d->done && d->src_row && d->next_tok,
              MPV_E_ARG, "mpv_beam_advance: null pointer");
  MPV_REQUIRE(d->tokens_in != d->tokens_out, MPV_E_ARG, "mpv_beam_advance: tokens_in and tokens_out must be different tables");
  hipLaunchKernelGGL(beam_advance_kernel, dim3((unsigned)d->batch), dim3(64), 0, stream, *d);
  return mpv_check_launch("mpv_beam_advance");
}
