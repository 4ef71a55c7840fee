// decode_shared_attention.hip -- one decode step's attention for sequences that share a per-group prefix KV cache (lockstep beam
// search / sampling: the K beams or samples of a clip share the visual prefix and the prompt).
//
// n_seq sequences in groups of group_size consecutive ones; every sequence has ONE query row, which attends to the prefix_len
// prefix keys of its group and to its own own_len keys (the last one is the current position's), one softmax over both.
//
// Layout: a workgroup = 4 waves serves the (up to) 32 sequences of one row tile of one (group, head); with group_size <= 32 (5
// beams, 16 samples) that is the whole group, so every prefix K/V chunk is fetched once per (group, head) and step.  All four
// waves hold the SAME 32 query rows; the keys are one stream of 32-key tiles -- the prefix tiles, then the own tiles of row 0,
// of row 1, ... (every row's own keys start on a tile boundary) -- brought into LDS 4 tiles (128 rows) at a time.  With 5 query
// rows a split of the ROWS over the waves would leave three waves idle, so the KEY tiles are split instead:
//   prefix tile T       -> wave T % 4, accumulated in that wave's prefix triple (m, l, acc)
//   own tile j of row r -> wave (prefix tiles + r) % 4, accumulated in that wave's own triple; every other row of the tile masks it
// and the five triples of a row (four prefix parts, its own part) are merged through LDS in a fixed order at the end.  A row's
// result therefore depends on the prefix, on its own keys and on nothing else: not on its place in the group, not on the group's
// place in the launch.  Tile arithmetic: prefix_tile.h (S^T = K Q^T on mfma_f32_32x32x16_bf16, online softmax in fp32,
// probabilities rounded to bf16 for the PV product).  No atomics, no stores outside o.
//
// The ragged entry (mpv_attn_decode_shared_ragged_fwd: prompts of different lengths in one lockstep search) is the same kernel with
// a per-group prefix length: plen, the prefix tile count pt and with it the (pt + r) % 4 wave assignment are per-workgroup values,
// read once (a workgroup serves one group).  A group's arithmetic is that of the uniform entry at its length, bit for bit.
//
// The steps entry (mpv_attn_decode_shared_steps_fwd: clips that entered a running loop at different times) adds a per-group OWN
// length the same way: own and the own tile count nt are per-workgroup values too.  It is its own kernel
// (attn_decode_shared_steps_kernel) around the one body, so the two entries above keep their code object; a group of own length 0
// is idle: its workgroups read no key and store zeros.
#include <string.h>

#include "mpv_common.h"
#include "prefix_tile.h"
#include "../../include/mpv.h"

namespace {

constexpr int DS_WAVES = 4;
constexpr int DS_THREADS = DS_WAVES * 64;
constexpr int DS_CH = DS_WAVES * 32;            // stream rows per LDS chunk: one 32-key tile per wave
constexpr int DS_KV = DS_CH * PROWB;            // bytes of a K (or V) chunk
constexpr int DS_MAX_OWN = 2048;

struct SharedArgs {
  const bf16 *q, *k, *v, *pk, *pv;
  const int* glen;                                // per-group prefix lengths (device), or nullptr: plen for every group
  bf16* o;
  long long q_ss, q_hs, k_ss, k_hs, k_rs, v_ss, v_hs, v_rs;
  long long pk_gs, pk_hs, pk_rs, pv_gs, pv_hs, pv_rs, o_ss, o_hs;
  int n_seq, group_size, plen, own, hd;
  float scale;
  const int* gown;                                // the steps entry: per-group own lengths (device); not read by the other two
};

template <int HD>
struct DsLds {
  static constexpr int NDT = (HD + 31) / 32;
  static constexpr int TRIPLE = NDT * 16 * 64 * 4;                 // one wave's accumulators, [d][reg][lane] fp32
  static constexpr int ML = (DS_WAVES + 1) * 2 * 32 * 4;           // m and l of the five triples, per query row
  static constexpr int MERGE = (DS_WAVES + 1) * TRIPLE + ML;
  static constexpr int BYTES = MERGE > 2 * DS_KV ? MERGE : 2 * DS_KV;
};

// One chunk (4 tiles) of the key stream, K and V: global -> registers -> LDS.  Rows past the end of their segment and the
// columns past hd are zeros: they are never read from memory (the caches' rows at and beyond own_len may hold anything).
template <int HD>
struct SharedStage {
  static constexpr int CPR = (HD + 31) / 32 * 4;                   // 16-byte pieces per (padded) row
  static constexpr int NLOAD = DS_CH * CPR / DS_THREADS;           // 4 (hd 64) or 6 (hd 80) b128 per thread and operand
  static_assert(DS_CH * CPR % DS_THREADS == 0, "a chunk is a whole number of loads per thread");
  i32x4 rk[NLOAD], rv[NLOAD];

  // tile T of the stream: prefix tile (T < pt) or own tile (T - pt) % nt of tile-local row (T - pt) / nt
  __device__ __forceinline__ void issue(const SharedArgs& p, const bf16* pkb, const bf16* pvb, const bf16* kb, const bf16* vb, int tid,
                                        int chunk, int plen, int own, int pt, int nt, int nrows) {
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) {
      const int c = tid + DS_THREADS * i;
      const int row = c / CPR, cc = c - row * CPR;
      const int T = chunk * DS_WAVES + (row >> 5), kr = row & 31;
      i32x4 xk = i32x4{0, 0, 0, 0}, xv = i32x4{0, 0, 0, 0};
      if (cc * 8 < p.hd) {
        if (T < pt) {
          const int key = T * 32 + kr;
          if (key < plen) {
            xk = *(const i32x4*)(pkb + (long long)key * p.pk_rs + cc * 8);
            xv = *(const i32x4*)(pvb + (long long)key * p.pv_rs + cc * 8);
          }
        } else {
          const int tt = T - pt;
          const int r = nt == 1 ? tt : tt / nt;
          const int key = (tt - r * nt) * 32 + kr;
          if (r < nrows && key < own) {
            xk = *(const i32x4*)(kb + (long long)r * p.k_ss + (long long)key * p.k_rs + cc * 8);
            xv = *(const i32x4*)(vb + (long long)r * p.v_ss + (long long)key * p.v_rs + cc * 8);
          }
        }
      }
      rk[i] = xk;
      rv[i] = xv;
    }
  }
  __device__ __forceinline__ void commit(char* lds, int tid) {
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) {
      const int c = tid + DS_THREADS * i;
      const int row = c / CPR, cc = c - row * CPR;
      *(i32x4*)(lds + row * PROWB + cc * 16) = rk[i];
      *(i32x4*)(lds + DS_KV + row * PROWB + cc * 16) = rv[i];
    }
  }
};

// the body of both kernels; STEPS: the own length is the group's (p.gown[g] clamped into [0, p.own]) instead of p.own
template <int HD, bool STEPS>
__device__ __forceinline__ void attn_decode_shared_body(const SharedArgs p) {      // (by value, as a kernel takes it: a reference costs hd 64 two registers)
  constexpr int NS = HD / 16;
  constexpr int NDT = (HD + 31) / 32;
  typedef DsLds<HD> L;
  __shared__ __attribute__((aligned(16))) char smem[L::BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.z, h = blockIdx.y;
  const int s0 = g * p.group_size + blockIdx.x * 32;                       // first sequence of this row tile
  const int nrows = min(32, min(p.group_size, p.n_seq - g * p.group_size) - (int)blockIdx.x * 32);
  if (nrows <= 0) return;                                                  // (a short last group): uniform over the workgroup
  const int rr = lane & 31;                                                // this lane's query row inside the tile
  // the group's prefix length: the ragged entry's is clamped into [1, p.plen], so a bad value cannot leave the group's rows
  const int plen = p.glen ? min(max(p.glen[g], 1), p.plen) : p.plen;
  int own = p.own;
  if (STEPS) {
    own = min(max(p.gown[g], 0), p.own);                                   // a bad value cannot leave the group's rows either
    if (own == 0) {                                                        // an idle group (uniform over the workgroup): zeros, no key read
      if (rr < nrows) {
        bf16* orow = p.o + (long long)(s0 + rr) * p.o_ss + (long long)h * p.o_hs;
#pragma unroll
        for (int d = 0; d < NDT; ++d) {
          const int col = d * 32 + 8 * wave + 4 * (lane >> 5);             // the store pattern of the live case
          if (col < p.hd) *(bf16x4*)(orow + col) = cvt4(f32x4{0.f, 0.f, 0.f, 0.f});
        }
      }
      return;
    }
  }
  const int pt = (plen + 31) >> 5, nt = (own + 31) >> 5;                   // prefix tiles, own tiles per row
  const int ntiles = pt + nrows * nt;
  const int nchunk = (ntiles + DS_WAVES - 1) / DS_WAVES;

  bf16x8 qf[NS];
  {
    const bf16* rp = p.q + (long long)(s0 + min(rr, nrows - 1)) * p.q_ss + (long long)h * p.q_hs + (lane >> 5) * 8;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      union { i32x4 i; bf16x8 b; } u;
      const bool cok = s * 16 + (lane >> 5) * 8 < p.hd;
      u.i = *(const i32x4*)(rp + (cok ? s * 16 : 0));
      if (!(rr < nrows && cok)) u.i = i32x4{0, 0, 0, 0};
      qf[s] = u.b;
    }
  }
  const float sc = p.scale;
  float pm = -INFINITY, pl = 0.f, om = -INFINITY, ol = 0.f;                // prefix part and own part of this lane's row
  f32x16 pacc[NDT], oacc[NDT];
#pragma unroll
  for (int d = 0; d < NDT; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) pacc[d][e] = oacc[d][e] = 0.f;

  const bf16* pkb = p.pk + (long long)g * p.pk_gs + (long long)h * p.pk_hs;
  const bf16* pvb = p.pv + (long long)g * p.pv_gs + (long long)h * p.pv_hs;
  const bf16* kb = p.k + (long long)s0 * p.k_ss + (long long)h * p.k_hs;
  const bf16* vb = p.v + (long long)s0 * p.v_ss + (long long)h * p.v_hs;

  SharedStage<HD> st;
  st.issue(p, pkb, pvb, kb, vb, tid, 0, plen, own, pt, nt, nrows);
  st.commit(smem, tid);
  __syncthreads();
  // head_dim 64 keeps the next chunk's loads in flight (in registers) under the tiles of this one; head_dim 80 has 16 more
  // accumulator registers per triple and 16 more staging registers, and would spill: it loads between the two barriers
  constexpr bool PREFETCH = HD == 64;
  for (int c = 0; c < nchunk; ++c) {
    if (PREFETCH && c + 1 < nchunk) st.issue(p, pkb, pvb, kb, vb, tid, c + 1, plen, own, pt, nt, nrows);
#pragma unroll 1
    for (int s = 0; s < DS_WAVES; ++s) {
      const int T = c * DS_WAVES + s;
      if (T >= ntiles) break;
      if (T < pt) {
        if (s != wave) continue;
        const int key0 = T * 32;
        ptile_update<HD>(smem, smem + DS_KV, s, key0, qf, sc, pm, pl, pacc, lane, [&](int key) { return key < plen; });
      } else {
        const int tt = T - pt;
        const int r = nt == 1 ? tt : tt / nt;
        if (((pt + r) & (DS_WAVES - 1)) != wave) continue;
        const int key0 = (tt - r * nt) * 32;
        ptile_update<HD>(smem, smem + DS_KV, s, key0, qf, sc, om, ol, oacc, lane, [&](int key) { return rr == r && key < own; });
      }
    }
    __syncthreads();                                                       // every wave is done with the chunk
    if (c + 1 < nchunk) {
      if (!PREFETCH) st.issue(p, pkb, pvb, kb, vb, tid, c + 1, plen, own, pt, nt, nrows);
      st.commit(smem, tid);
      __syncthreads();
    }
  }

  // ---------------- merge the five triples of every row through LDS (the staging buffers are free: barrier above)
  float* accs = (float*)smem;                                              // [triple][d][reg][lane]
  float* ms = (float*)(smem + (DS_WAVES + 1) * L::TRIPLE);                 // [triple][32]
  float* ls = ms + (DS_WAVES + 1) * 32;
  const bool owner = ((pt + rr) & (DS_WAVES - 1)) == wave;                 // this wave ran the own tiles of row rr
#pragma unroll
  for (int d = 0; d < NDT; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      accs[((wave * NDT + d) * 16 + e) * 64 + lane] = pacc[d][e];
      if (owner) accs[((DS_WAVES * NDT + d) * 16 + e) * 64 + lane] = oacc[d][e];
    }
  if (lane < 32) {
    ms[wave * 32 + rr] = pm;
    ls[wave * 32 + rr] = pl;
    if (owner) {
      ms[DS_WAVES * 32 + rr] = om;
      ls[DS_WAVES * 32 + rr] = ol;
    }
  }
  __syncthreads();
  if (rr < nrows) {
    float f[DS_WAVES + 1], mall = -INFINITY, lall = 0.f;
#pragma unroll
    for (int i = 0; i <= DS_WAVES; ++i) mall = fmaxf(mall, ms[i * 32 + rr]);   // finite: the row sees its current position
#pragma unroll
    for (int i = 0; i <= DS_WAVES; ++i) {
      f[i] = __expf(ms[i * 32 + rr] - mall);                                   // an empty part (m = -inf, l = 0, acc = 0): 0
      lall += f[i] * ls[i * 32 + rr];
    }
    const float inv_l = 1.0f / lall;
    bf16* orow = p.o + (long long)(s0 + rr) * p.o_ss + (long long)h * p.o_hs;
    // wave w finishes accumulator registers 4w .. 4w+3 of every d tile: 4 consecutive columns, one 8-byte store
#pragma unroll
    for (int d = 0; d < NDT; ++d) {
      const int col = d * 32 + 8 * wave + 4 * (lane >> 5);
      if (col < p.hd) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float a = 0.f;
#pragma unroll
          for (int i = 0; i <= DS_WAVES; ++i) a += f[i] * accs[((i * NDT + d) * 16 + 4 * wave + e) * 64 + lane];
          v[e] = a * inv_l;
        }
        *(bf16x4*)(orow + col) = cvt4(v);
      }
    }
  }
}

template <int HD>
__global__ __launch_bounds__(DS_THREADS, 2) void attn_decode_shared_kernel(const SharedArgs p) {
  attn_decode_shared_body<HD, false>(p);
}
template <int HD>
__global__ __launch_bounds__(DS_THREADS, 2) void attn_decode_shared_steps_kernel(const SharedArgs p) {
  attn_decode_shared_body<HD, true>(p);
}

}  // namespace

// the body of the three entries (glen == nullptr: the uniform one; gown != nullptr: the steps one); `who` names the entry in the messages
static int launch_shared(const mpv_attn_decode_shared_desc* d, const int32_t* glen, bool ragged, const char* who, hipStream_t stream,
                         const int32_t* gown = nullptr, bool steps = false) {
  MPV_REQUIRE(d && d->q && d->k && d->v && d->pk && d->pv && d->o, MPV_E_ARG, "%s: null pointer", who);
  MPV_REQUIRE(!ragged || glen, MPV_E_ARG, "%s: null group_prefix_len", who);
  MPV_REQUIRE(!steps || gown, MPV_E_ARG, "%s: null group_own_len", who);
  MPV_REQUIRE(d->head_dim == 64 || d->head_dim == 80, MPV_E_SHAPE,
              "%s: head_dim %d is not supported (64: the 1.3B decoder, 80: 2.7B)", who, d->head_dim);
  MPV_REQUIRE(d->n_seq > 0 && d->group_size > 0 && d->heads > 0, MPV_E_SHAPE,
              "%s: empty problem (n_seq %d, group_size %d, heads %d)", who, d->n_seq, d->group_size, d->heads);
  MPV_REQUIRE(d->prefix_len >= 1 && d->prefix_len < (1 << 24), MPV_E_SHAPE,
              "%s: prefix_len %d must lie in [1, 2^24)", who, d->prefix_len);
  MPV_REQUIRE(d->own_len >= 1 && d->own_len <= DS_MAX_OWN, MPV_E_SHAPE, "%s: own_len %d must lie in [1, %d]", who,
              d->own_len, DS_MAX_OWN);
  MPV_REQUIRE(d->n_groups == (d->n_seq + d->group_size - 1) / d->group_size, MPV_E_SHAPE,
              "%s: n_groups %d must be ceil(n_seq %d / group_size %d)", who, d->n_groups, d->n_seq, d->group_size);
  MPV_REQUIRE(d->n_groups <= 65535 && d->heads <= 65535, MPV_E_SHAPE, "%s: problem too large", who);
  const int64_t st[] = {d->q_ss, d->q_hs, d->k_ss, d->k_hs, d->k_rs, d->v_ss, d->v_hs, d->v_rs,
                        d->pk_gs, d->pk_hs, d->pk_rs, d->pv_gs, d->pv_hs, d->pv_rs};
  bool al = true;
  for (int64_t s : st) al = al && (s % 8 == 0);
  MPV_REQUIRE(al && d->o_ss % 4 == 0 && d->o_hs % 4 == 0, MPV_E_ALIGN,
              "%s: strides must keep q/k/v/pk/pv rows 16-byte and o rows 8-byte aligned", who);
  MPV_REQUIRE((((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->pk | (uintptr_t)d->pv) & 15) == 0 &&
                  ((uintptr_t)d->o & 7) == 0,
              MPV_E_ALIGN, "%s: q/k/v/pk/pv must be 16-byte aligned, o 8-byte aligned", who);
  MPV_REQUIRE(d->scale > 0.f, MPV_E_ARG, "%s: scale must be positive", who);
  SharedArgs a;
  a.q = (const bf16*)d->q;
  a.k = (const bf16*)d->k;
  a.v = (const bf16*)d->v;
  a.pk = (const bf16*)d->pk;
  a.pv = (const bf16*)d->pv;
  a.glen = glen;
  a.gown = gown;
  a.o = (bf16*)d->o;
  a.q_ss = d->q_ss; a.q_hs = d->q_hs;
  a.k_ss = d->k_ss; a.k_hs = d->k_hs; a.k_rs = d->k_rs;
  a.v_ss = d->v_ss; a.v_hs = d->v_hs; a.v_rs = d->v_rs;
  a.pk_gs = d->pk_gs; a.pk_hs = d->pk_hs; a.pk_rs = d->pk_rs;
  a.pv_gs = d->pv_gs; a.pv_hs = d->pv_hs; a.pv_rs = d->pv_rs;
  a.o_ss = d->o_ss; a.o_hs = d->o_hs;
  a.n_seq = d->n_seq;
  a.group_size = d->group_size;
  a.plen = d->prefix_len;
  a.own = d->own_len;
  a.hd = d->head_dim;
  a.scale = d->scale;
  const dim3 grid((unsigned)((d->group_size + 31) / 32), (unsigned)d->heads, (unsigned)d->n_groups);
  if (steps && d->head_dim == 64)
    hipLaunchKernelGGL(attn_decode_shared_steps_kernel<64>, grid, dim3(DS_THREADS), 0, stream, a);
  else if (steps)
    hipLaunchKernelGGL(attn_decode_shared_steps_kernel<80>, grid, dim3(DS_THREADS), 0, stream, a);
  else if (d->head_dim == 64)
    hipLaunchKernelGGL(attn_decode_shared_kernel<64>, grid, dim3(DS_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL(attn_decode_shared_kernel<80>, grid, dim3(DS_THREADS), 0, stream, a);
  return mpv_check_launch(who);
}

extern "C" int mpv_attn_decode_shared_fwd(const mpv_attn_decode_shared_desc* d, hipStream_t stream) {
  return launch_shared(d, nullptr, false, "mpv_attn_decode_shared_fwd", stream);
}

extern "C" int mpv_attn_decode_shared_ragged_fwd(const mpv_attn_decode_shared_desc* d, const int32_t* group_prefix_len,
                                                 hipStream_t stream) {
  return launch_shared(d, group_prefix_len, true, "mpv_attn_decode_shared_ragged_fwd", stream);
}

extern "C" int mpv_attn_decode_shared_steps_fwd(const mpv_attn_decode_shared_desc* d, const int32_t* group_prefix_len,
                                                const int32_t* group_own_len, hipStream_t stream) {
  return launch_shared(d, group_prefix_len, true, "mpv_attn_decode_shared_steps_fwd", stream, group_own_len, true);
}
