// Lockstep beam search over a batch of clips (caption evaluation), plain and diverse: one kernel behind two entry points.
// mpv_beam_advance does, for every clip of the batch, what ONE iteration of generation.beam_search_loop does on the host for one
// clip -- models/modeling_distributed_gpt3.py:1793-1840 (candidate order, stop-token handling, next beams) and BeamHypotheses.add /
// is_done (:1908-1960) -- so that a decode step of B clips x K beams needs no host bookkeeping: the step's outputs (source row and
// new token of every sequence) stay on the device and feed the KV re-order and the next decode step.  mpv_beam_advance_groups is
// the same for a search whose beams are split into G groups of K beams (Vijayakumar et al., "Diverse Beam Search"; num_beam_groups
// / diversity_penalty of the usual generation interfaces): a (clip, group) pair is a clip of mpv_beam_advance's state -- its own
// beams, hypothesis store, worst score and done flag -- and runs exactly one iteration of that contract per call.
// mpv_beam_advance is the G = 1 case: it fills a groups descriptor with groups = 1, diversity_penalty = 0 and goes through the same
// check-and-launch.  The kernel body is written once and compiled twice, beam_advance_kernel<192, true> for G > 1 and <128, false>
// for G = 1 ("Merged", has the measurement that asked for the second instantiation).
// mpv_beam_advance_steps is both with a generation step per clip (clips that entered a running search at different times, DESIGN.md
// section 27): the third template flag, STEPS, compiled into two more instantiations; the two above are compiled with STEPS = false.
//
// One workgroup of one wave per clip; nothing is shared between clips, so a clip's result depends neither on the batch size nor
// on its place in the batch.  The clip's groups are walked one after the other inside the wave; per group, on a candidate list of
// m = 2K + (G-1)K per beam (DESIGN.md section 21 says why that many stand for the whole vocabulary; 2K at G = 1):
//   1. rank: the group's candidates (m of beam 0 on the first step, K x m afterwards; <= 192) are parked in LDS and every lane
//      counts, for its (at most three) candidates, how many come before them under the order rule
//          value descending, then (beam in group) * V + token ascending (then position in the input, which only matters for
//          malformed input);
//      that count is the candidate's rank -- a total order, so the ranks are distinct -- and the candidates of rank < 2K write
//      themselves to slot `rank` of the sorted list.  No atomics, no dependence on the order in which lanes run.
//   2. walk: the sorted list is walked in rank order with wave-uniform control flow (every lane holds the same heap state in
//      registers and reads the same LDS words).  The walk is latency work (<= 16 entries); the lanes only differ in the row copies:
//      a stop token of rank < K copies the Lt tokens of its source row into the hypothesis store, lane l taking positions
//      l, l + 64, ...  The heap arithmetic is fp64 on fp32 inputs -- double(value) / Lt, compared with `worst` -- which is what the
//      Python floats of the host loop do, bit for bit (one correctly rounded fp64 division; no pow: length_penalty is 1.0).
//   3. finish: done test, state write-back, and unless the group is (or has just become) done the K row copies into the other
//      token table with the new token written at `pos`, the new beam scores, src_row and next_tok.
// A done group is frozen: its rows go to the other token table unchanged (the tables are swapped by the caller after every call),
// it gets identity src_row and the stop token, and nothing else of its state is written.
// The one addition for G > 1 is the coupling between the groups of a clip, inside a call: the tokens of the next beams that the
// groups before g have emitted in this call sit in LDS (at most G * K <= 16, with multiplicity; a frozen group, and one that
// becomes done in this call, appends nothing), and group g ranks the penalised values v' = v - lambda * c, c the number of those
// tokens equal to the candidate's (the Hamming diversity of the paper): two separately rounded fp32 operations, and v itself when
// c = 0 -- so with one group, where nothing has been emitted, the values pass through untouched whatever lambda is.
#include "mpv_common.h"
#include "../../include/mpv.h"

namespace {

constexpr int BA_MAX_K = 8, BA_MAX_G = 8, BA_MAX_SEQ = 16, BA_MAX_LT = 2048;
constexpr int BA_MAX_CAND_PLAIN = BA_MAX_K * 2 * BA_MAX_K;              // G = 1, K = 8: 8 rows of 2K = 16
constexpr int BA_MAX_CAND = BA_MAX_K * (2 * BA_MAX_K + BA_MAX_K);      // K = 8, G = 2: 8 rows of m = 24 (G * K <= 16 bounds the rest)

// candidate (va, ka, ia) comes before (vb, kb, ib)
__device__ __forceinline__ bool ba_before(float va, long long ka, int ia, float vb, long long kb, int ib) {
  return va > vb || (va == vb && (ka < kb || (ka == kb && ia < ib)));
}

// GROUPS = false is the body at G = 1 with the group loop, the penalty and the emitted-token list compiled away.
// STEPS = true (mpv_beam_advance_steps) is the body with a generation step per clip: the workgroup reads clip_prompt_len[clip] and
// clip_step[clip] once (one address for the whole wave, so the three values below are wave-uniform) in place of d.pos / d.cur_len /
// d.first; a clip with a negative step, or whose column lies behind the table, takes the frozen path with all its groups and reads
// neither a candidate nor its done flag.  With STEPS = false the two arrays are not touched (the callers pass null).
template <int MAX_CAND, bool GROUPS, bool STEPS>
__global__ __launch_bounds__(64) void beam_advance_kernel(mpv_beam_advance_groups_desc d, const int32_t* __restrict__ clip_prompt_len,
                                                          const int32_t* __restrict__ clip_step) {
  __shared__ float c_val[MAX_CAND];
  __shared__ long long c_key[MAX_CAND];
  __shared__ long long c_tok[MAX_CAND];
  __shared__ float s_val[2 * BA_MAX_K];
  __shared__ int s_beam[2 * BA_MAX_K];
  __shared__ long long s_tok[2 * BA_MAX_K];
  __shared__ float n_val[BA_MAX_K];                      // the group's next beams: (value, source beam, token)
  __shared__ int n_beam[BA_MAX_K];
  __shared__ long long n_tok[BA_MAX_K];
  __shared__ long long e_tok[BA_MAX_SEQ];                // the tokens of the next beams emitted so far in this call, by this clip
  const int lane = threadIdx.x, K = d.beams, K2 = 2 * K, G = GROUPS ? d.groups : 1, M = K2 + (G - 1) * K, Lt = d.row_len;
  const float lambda = d.diversity_penalty;
  int n_emit = 0;                                        // wave-uniform
  int pos = d.pos, cur_len = d.cur_len;
  bool first = d.first != 0, idle = false;
  if constexpr (STEPS) {
    const int s = clip_step[blockIdx.x], pl = min(max(clip_prompt_len[blockIdx.x], 0), Lt);
    idle = s < 0 || s >= Lt - pl;                        // pl + s >= Lt without the sum (s may be anything)
    pos = idle ? 0 : pl + s, cur_len = idle ? 1 : s + 1, first = s == 0;
  }

  for (int g = 0; g < G; ++g) {
    __syncthreads();                                     // the LDS of the group before: e_tok written, c_* / s_* / n_* read
    const long long b = (long long)blockIdx.x * G + g, row0 = b * K;
    const int64_t* tin = d.tokens_in + row0 * Lt;
    int64_t* tout = d.tokens_out + row0 * Lt;

    if ((STEPS && idle) || d.done[b]) {                  // frozen: wave-uniform
      for (int j = 0; j < K; ++j)
        for (int t = lane; t < Lt; t += 64) tout[(long long)j * Lt + t] = tin[(long long)j * Lt + t];
      if (lane < K) {
        d.src_row[row0 + lane] = row0 + lane;
        d.next_tok[row0 + lane] = d.stop_token;
      }
      continue;
    }

    // ---- 1. penalise and rank
    const int n_cand = first ? M : K * M;                // the first step reads beam 0 of the group only (:1793-1795)
    for (int i = lane; i < n_cand; i += 64) {
      const long long tok = d.cand_idx[row0 * M + i];
      const float v = d.cand_val[row0 * M + i];
      int c = 0;
      if constexpr (GROUPS)
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
      for (int j = 0; j < n_cand; ++j) rank += ba_before(c_val[j], c_key[j], j, v, key, i) ? 1 : 0;
      if (rank < K2) {
        s_val[rank] = v;
        s_beam[rank] = i / M;
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
      if (r >= K) continue;                              // :1809-1812
      const double score = (double)v / (double)Lt;       // BeamHypotheses.add: sum_logprobs / len(row) ** 1.0 (:1936)
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
        worst = score;                                   // becomes the lowest of what stays (:1942-1944: the second lowest of K + 1)
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
    const bool now_done = count == K && worst >= (double)s_val[0] / (double)cur_len;        // is_done (:1946-1960)
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
      // a slot left over (fewer than K next beams among the 2K walked) keeps its own row and is no emitted beam
      const bool have = j < n_next;
      const int beam = have ? n_beam[j] : j;
      const long long tok = have ? n_tok[j] : d.stop_token;
      for (int t = lane; t < Lt; t += 64) tout[(long long)j * Lt + t] = t == pos ? tok : tin[(long long)beam * Lt + t];
      if (lane == 0) {
        d.scores[row0 + j] = have ? n_val[j] : -INFINITY;
        d.src_row[row0 + j] = row0 + beam;
        d.next_tok[row0 + j] = tok;
        if constexpr (GROUPS)
          if (have) e_tok[n_emit + j] = tok;             // n_emit + j < G * K <= BA_MAX_SEQ
      }
    }
    n_emit += n_next;
  }
}

// the refusals both entry points share, then the launch; `who` names the entry point in the messages
// steps = true (mpv_beam_advance_steps): pos / cur_len / first come per clip from the two device arrays, the descriptor's are not looked at
int beam_advance_launch(const mpv_beam_advance_groups_desc& d, const char* who, hipStream_t stream, bool steps = false,
                        const int32_t* clip_prompt_len = nullptr, const int32_t* clip_step = nullptr) {
  MPV_REQUIRE(d.row_len >= 1 && d.row_len <= BA_MAX_LT, MPV_E_SHAPE, "%s: row_len (%d) must be in [1, %d]", who, d.row_len, BA_MAX_LT);
  if (steps) {
    MPV_REQUIRE(d.batch >= 1 && d.vocab >= 1, MPV_E_SHAPE, "%s: bad shape batch=%d vocab=%d", who, d.batch, d.vocab);
    MPV_REQUIRE(clip_prompt_len, MPV_E_ARG, "%s: null clip_prompt_len", who);
    MPV_REQUIRE(clip_step, MPV_E_ARG, "%s: null clip_step", who);
  } else {
    MPV_REQUIRE(d.batch >= 1 && d.vocab >= 1 && d.cur_len >= 1 && d.pos >= 0 && d.pos < d.row_len, MPV_E_SHAPE,
                "%s: bad shape batch=%d vocab=%d cur_len=%d pos=%d (row_len %d)", who, d.batch, d.vocab, d.cur_len, d.pos, d.row_len);
  }
  MPV_REQUIRE(d.cand_val && d.cand_idx && d.tokens_in && d.tokens_out && d.scores && d.hyp_score && d.hyp_order && d.hyp_tokens &&
                  d.hyp_count && d.hyp_next && d.worst && d.done && d.src_row && d.next_tok,
              MPV_E_ARG, "%s: null pointer", who);
  MPV_REQUIRE(d.tokens_in != d.tokens_out, MPV_E_ARG, "%s: tokens_in and tokens_out must be different tables", who);
  const dim3 grid((unsigned)d.batch), block(64);
  const int32_t* none = nullptr;
  if (steps && d.groups == 1)
    hipLaunchKernelGGL((beam_advance_kernel<BA_MAX_CAND_PLAIN, false, true>), grid, block, 0, stream, d, clip_prompt_len, clip_step);
  else if (steps)
    hipLaunchKernelGGL((beam_advance_kernel<BA_MAX_CAND, true, true>), grid, block, 0, stream, d, clip_prompt_len, clip_step);
  else if (d.groups == 1)
    hipLaunchKernelGGL((beam_advance_kernel<BA_MAX_CAND_PLAIN, false, false>), grid, block, 0, stream, d, none, none);
  else
    hipLaunchKernelGGL((beam_advance_kernel<BA_MAX_CAND, true, false>), grid, block, 0, stream, d, none, none);
  return mpv_check_launch(who);
}

// what mpv_beam_advance_groups and mpv_beam_advance_steps refuse about the groups of a descriptor
int beam_groups_check(const mpv_beam_advance_groups_desc* d, const char* who) {
  MPV_REQUIRE(d, MPV_E_ARG, "%s: null descriptor", who);
  MPV_REQUIRE(d->beams >= 1 && d->beams <= BA_MAX_K, MPV_E_SHAPE, "%s: beams per group (%d) must be in [1, %d]", who, d->beams, BA_MAX_K);
  MPV_REQUIRE(d->groups >= 1 && d->groups <= BA_MAX_G, MPV_E_SHAPE, "%s: groups (%d) must be in [1, %d]", who, d->groups, BA_MAX_G);
  MPV_REQUIRE(d->groups * d->beams <= BA_MAX_SEQ, MPV_E_SHAPE, "%s: groups * beams (%d x %d) must be at most %d", who, d->groups, d->beams,
              BA_MAX_SEQ);
  MPV_REQUIRE(d->diversity_penalty >= 0.f && d->diversity_penalty <= 3.402823466e+38f, MPV_E_ARG,
              "%s: diversity_penalty (%g) must be finite and not negative", who, (double)d->diversity_penalty);
  return MPV_OK;
}

}  // namespace

extern "C" int mpv_beam_advance(const mpv_beam_advance_desc* d, hipStream_t stream) {
  MPV_REQUIRE(d, MPV_E_ARG, "mpv_beam_advance: null descriptor");
  MPV_REQUIRE(d->beams >= 1 && d->beams <= BA_MAX_K, MPV_E_SHAPE, "mpv_beam_advance: beams (%d) must be in [1, %d]", d->beams, BA_MAX_K);
  mpv_beam_advance_groups_desc g = {};
  g.cand_val = d->cand_val, g.cand_idx = d->cand_idx, g.tokens_in = d->tokens_in, g.tokens_out = d->tokens_out;
  g.scores = d->scores, g.hyp_score = d->hyp_score, g.hyp_order = d->hyp_order, g.hyp_tokens = d->hyp_tokens;
  g.hyp_count = d->hyp_count, g.hyp_next = d->hyp_next, g.worst = d->worst, g.done = d->done;
  g.src_row = d->src_row, g.next_tok = d->next_tok;
  g.batch = d->batch, g.beams = d->beams, g.row_len = d->row_len, g.vocab = d->vocab, g.pos = d->pos, g.cur_len = d->cur_len;
  g.first = d->first, g.stop_token = d->stop_token;
  g.groups = 1, g.diversity_penalty = 0.f;
  return beam_advance_launch(g, "mpv_beam_advance", stream);
}

extern "C" int mpv_beam_advance_groups(const mpv_beam_advance_groups_desc* d, hipStream_t stream) {
  const int rc = beam_groups_check(d, "mpv_beam_advance_groups");
  return rc ? rc : beam_advance_launch(*d, "mpv_beam_advance_groups", stream);
}

extern "C" int mpv_beam_advance_steps(const mpv_beam_advance_groups_desc* d, const int32_t* clip_prompt_len, const int32_t* clip_step,
                                      hipStream_t stream) {
  const int rc = beam_groups_check(d, "mpv_beam_advance_steps");
  return rc ? rc : beam_advance_launch(*d, "mpv_beam_advance_steps", stream, true, clip_prompt_len, clip_step);
}
