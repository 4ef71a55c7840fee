// Diverse (group) beam search in lockstep over a batch of clips (Vijayakumar et al., "Diverse Beam Search"; num_beam_groups /
// diversity_penalty of the usual generation interfaces): mpv_beam_advance_groups is mpv_beam_advance (csrc/beam_search.hip) for a
// search whose beams are split into G groups of K' beams.  A (clip, group) pair is a clip of mpv_beam_advance's state -- its own
// beams, hypothesis store, worst score and done flag -- and runs exactly one iteration of that contract per call; the one coupling
// is inside a call, between the groups of one clip: group g's candidate values are lowered by lambda times the number of next beams
// that the groups before it have emitted in this call with the candidate's token (the Hamming diversity of the paper).
//
// One workgroup of one wave per CLIP, as there; the clip's groups are walked one after the other inside the wave, because group g
// needs what the groups before it chose.  The tokens they chose sit in LDS (at most G * K' <= 16, with multiplicity), the rest of
// an iteration is the three phases of beam_advance_kernel on a candidate list of m = 2K' + (G-1)K' per beam (DESIGN.md section 21
// says why that many are enough to stand for the whole vocabulary):
//   1. rank: the group's candidates (m of beam 0 on the first step, K' x m afterwards; <= 192) are parked in LDS with their
//      penalised values v' = v - lambda * c, two separately rounded fp32 operations and v itself when c = 0; every lane counts, for
//      its (at most three) candidates, how many come before them under the order rule -- value descending, then (beam in group) *
//      V + token ascending, then position in the input -- and the candidates of rank < 2K' write themselves to the sorted list.
//   2. walk, 3. finish: those of beam_advance_kernel, on K' beams, with wave-uniform control flow (every lane reads the same LDS
//      words and holds the same heap state in registers); the lanes differ only in the row copies.  The next beams a live group
//      emits are appended to the LDS token list; a frozen group, and one that becomes done in this call, appends nothing.
// No atomics; nothing is shared between clips, so a clip's result depends neither on the batch size nor on its place in the batch.
#include "mpv_common.h"
#include "../../include/mpv.h"

namespace {

constexpr int GA_MAX_K = 8, GA_MAX_G = 8, GA_MAX_SEQ = 16, GA_MAX_LT = 2048;
constexpr int GA_MAX_CAND = GA_MAX_K * (2 * GA_MAX_K + GA_MAX_K);      // K' = 8, G = 2: 8 rows of m = 24 (G * K' <= 16 bounds the rest)

// candidate (va, ka, ia) comes before (vb, kb, ib)
__device__ __forceinline__ bool ga_before(float va, long long ka, int ia, float vb, long long kb, int ib) {
  return va > vb || (va == vb && (ka < kb || (ka == kb && ia < ib)));
}

__global__ __launch_bounds__(64) void beam_advance_groups_kernel(mpv_beam_advance_groups_desc d) {
  __shared__ float c_val[GA_MAX_CAND];
  __shared__ long long c_key[GA_MAX_CAND];
  __shared__ long long c_tok[GA_MAX_CAND];
  __shared__ float s_val[2 * GA_MAX_K];
  __shared__ int s_beam[2 * GA_MAX_K];
  __shared__ long long s_tok[2 * GA_MAX_K];
  __shared__ float n_val[GA_MAX_K];                      // the group's next beams: (value, source beam, token)
  __shared__ int n_beam[GA_MAX_K];
  __shared__ long long n_tok[GA_MAX_K];
  __shared__ long long e_tok[GA_MAX_SEQ];                // the tokens of the next beams emitted so far in this call, by this clip
  const int lane = threadIdx.x, K = d.beams, K2 = 2 * K, G = d.groups, M = K2 + (G - 1) * K, Lt = d.row_len;
  const float lambda = d.diversity_penalty;
  int n_emit = 0;                                        // wave-uniform

  for (int g = 0; g < G; ++g) {
    __syncthreads();                                     // the LDS of the group before: e_tok written, c_* / s_* / n_* read
    const long long b = (long long)blockIdx.x * G + g, row0 = b * K;
    const int64_t* tin = d.tokens_in + row0 * Lt;
    int64_t* tout = d.tokens_out + row0 * Lt;

    if (d.done[b]) {                                     // frozen: wave-uniform
      for (int j = 0; j < K; ++j)
        for (int t = lane; t < Lt; t += 64) tout[(long long)j * Lt + t] = tin[(long long)j * Lt + t];
      if (lane < K) {
        d.src_row[row0 + lane] = row0 + lane;
        d.next_tok[row0 + lane] = d.stop_token;
      }
      continue;
    }

    // ---- 1. penalise and rank
    const int n_cand = d.first ? M : K * M;              // the first step reads beam 0 of the group only
    for (int i = lane; i < n_cand; i += 64) {
      const long long tok = d.cand_idx[row0 * M + i];
      const float v = d.cand_val[row0 * M + i];
      int c = 0;
      for (int e = 0; e < n_emit; ++e) c += e_tok[e] == tok ? 1 : 0;
      c_val[i] = c ? __fsub_rn(v, __fmul_rn(lambda, (float)c)) : v;
      c_tok[i] = tok;
      c_key[i] = (long long)(i / M) * d.vocab + tok;
    }
    __syncthreads();
    for (int i = lane; i < n_cand; i += 64) {
      const float v = c_val[i];
      const long long key = c_key[i];
      int rank = 0;
      for (int j = 0; j < n_cand; ++j) rank += ga_before(c_val[j], c_key[j], j, v, key, i) ? 1 : 0;
      if (rank < K2) {
        s_val[rank] = v;
        s_beam[rank] = i / M;
        s_tok[rank] = c_tok[i];
      }
    }
    __syncthreads();

    // ---- 2. walk (wave-uniform)
    double hs[GA_MAX_K];
    int ho[GA_MAX_K];
#pragma unroll
    for (int j = 0; j < GA_MAX_K; ++j) {
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
      if (r >= K) continue;
      const double score = (double)v / (double)Lt;
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
        for (int j = 1; j < GA_MAX_K; ++j)
          if (j < K && (hs[j] < ls || (hs[j] == ls && ho[j] < lo))) slot = j, ls = hs[j], lo = ho[j];
        worst = score;                                   // becomes the lowest of what stays
#pragma unroll
        for (int j = 0; j < GA_MAX_K; ++j)
          if (j < K && j != slot && hs[j] < worst) worst = hs[j];
      }
#pragma unroll
      for (int j = 0; j < GA_MAX_K; ++j)
        if (j == slot) hs[j] = score, ho[j] = next;
      ++next;
      for (int t = lane; t < Lt; t += 64) hyp_rows[(long long)slot * Lt + t] = tin[(long long)beam * Lt + t];
    }

    // ---- 3. finish
    const bool now_done = count == K && worst >= (double)s_val[0] / (double)d.cur_len;
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < GA_MAX_K; ++j)
        if (j < K) {
          d.hyp_score[row0 + j] = hs[j];
          d.hyp_order[row0 + j] = ho[j];
        }
      d.hyp_count[b] = count;
      d.hyp_next[b] = next;
      d.worst[b] = worst;
      d.done[b] = now_done ? 1 : 0;
    }
    __syncthreads();                                     // n_val / n_beam / n_tok of lane 0
    if (now_done) {                                      // frozen from here on: its tokens penalise no later group
      for (int j = 0; j < K; ++j)
        for (int t = lane; t < Lt; t += 64) tout[(long long)j * Lt + t] = tin[(long long)j * Lt + t];
      if (lane < K) {
        d.src_row[row0 + lane] = row0 + lane;
        d.next_tok[row0 + lane] = d.stop_token;
      }
      continue;
    }
    for (int j = 0; j < K; ++j) {
      // a slot left over (fewer than K' next beams among the 2K' walked) keeps its own row and is no emitted beam
      const bool have = j < n_next;
      const int beam = have ? n_beam[j] : j;
      const long long tok = have ? n_tok[j] : d.stop_token;
      for (int t = lane; t < Lt; t += 64) tout[(long long)j * Lt + t] = t == d.pos ? tok : tin[(long long)beam * Lt + t];
      if (lane == 0) {
        d.scores[row0 + j] = have ? n_val[j] : -INFINITY;
        d.src_row[row0 + j] = row0 + beam;
        d.next_tok[row0 + j] = tok;
        if (have) e_tok[n_emit + j] = tok;               // n_emit + j < G * K' <= GA_MAX_SEQ
      }
    }
    n_emit += n_next;
  }
}

}  // namespace

extern "C" int mpv_beam_advance_groups(const mpv_beam_advance_groups_desc* d, hipStream_t stream) {
  MPV_REQUIRE(d, MPV_E_ARG, "mpv_beam_advance_groups: null descriptor");
  MPV_REQUIRE(d->beams >= 1 && d->beams <= GA_MAX_K, MPV_E_SHAPE, "mpv_beam_advance_groups: beams per group (%d) must be in [1, %d]",
              d->beams, GA_MAX_K);
  MPV_REQUIRE(d->groups >= 1 && d->groups <= GA_MAX_G, MPV_E_SHAPE, "mpv_beam_advance_groups: groups (%d) must be in [1, %d]", d->groups,
              GA_MAX_G);
  MPV_REQUIRE(d->groups * d->beams <= GA_MAX_SEQ, MPV_E_SHAPE, "mpv_beam_advance_groups: groups * beams (%d x %d) must be at most %d",
              d->groups, d->beams, GA_MAX_SEQ);
  MPV_REQUIRE(d->diversity_penalty >= 0.f && d->diversity_penalty <= 3.402823466e+38f, MPV_E_ARG,
              "mpv_beam_advance_groups: diversity_penalty (%g) must be finite and not negative", (double)d->diversity_penalty);
  MPV_REQUIRE(d->row_len >= 1 && d->row_len <= GA_MAX_LT, MPV_E_SHAPE, "mpv_beam_advance_groups: row_len (%d) must be in [1, %d]",
              d->row_len, GA_MAX_LT);
  MPV_REQUIRE(d->batch >= 1 && d->vocab >= 1 && d->cur_len >= 1 && d->pos >= 0 && d->pos < d->row_len, MPV_E_SHAPE,
              "mpv_beam_advance_groups: bad shape batch=%d vocab=%d cur_len=%d pos=%d (row_len %d)", d->batch, d->vocab, d->cur_len,
              d->pos, d->row_len);
  MPV_REQUIRE(d->cand_val && d->cand_idx && d->tokens_in && d->tokens_out && d->scores && d->hyp_score && d->hyp_order && d->hyp_tokens &&
                  d->hyp_count && d->hyp_next && d->worst && d->done && d->src_row && d->next_tok,
              MPV_E_ARG, "mpv_beam_advance_groups: null pointer");
  MPV_REQUIRE(d->tokens_in != d->tokens_out, MPV_E_ARG, "mpv_beam_advance_groups: tokens_in and tokens_out must be different tables");
  hipLaunchKernelGGL(beam_advance_groups_kernel, dim3((unsigned)d->batch), dim3(64), 0, stream, *d);
  return mpv_check_launch("mpv_beam_advance_groups");
}
