// prefix_attention.hip -- causal attention of many continuations against one shared, already computed prefix (evaluation only).
//
// The scoring heads run every (video, candidate) pair as its own decoder sequence; the first P rows of all candidates of one
// video are identical (query features + the common token prefix), so their K/V are computed once per video (the prefix pass)
// and each candidate runs only its own Lc rows.  Query row i of continuation c (absolute position P + i) attends to the P
// prefix keys of its group g = c / group_size and to its own keys j <= i.
//
// Layout: a workgroup = 4 waves = 128 STACKED query rows of one (group, head): the rows of all continuations of the group laid
// end to end (stacked row r = local continuation r / Lc, row r % Lc), so that every prefix K/V chunk brought into LDS serves all
// of them -- with Lc of a few rows (category names) per-continuation tiles would leave the MFMA tiles mostly empty.  Phase 1
// streams the prefix (dense for every row); phase 2 streams the stacked own keys the block can see (block-diagonal causal: key
// row kr is visible to query row r iff both lie in the same continuation and kr <= r).  Conventions of attention.hip's forward
// kernel: S^T = K Q^T so a lane owns one query row of the 32x32 score tile, the probabilities feed the PV MFMA as its B operand
// from registers, V^T fragments come from the transposing LDS read.  The softmax is online (running max / sum per row, fp32
// scores and statistics, probabilities rounded to bf16 for the PV product, one division at the end).
#include <string.h>

#include "mpv_common.h"
#include "../../include/mpv.h"

namespace {

constexpr int PCH = 64;                 // key rows per LDS chunk
constexpr int PROWB = 208;              // LDS row pitch in bytes (96 bf16 + 16 pad: conflict-free ds_read_b128)
constexpr int PCHUNK = PCH * PROWB;
constexpr int PWAVES = 4;
constexpr int PROWS = PWAVES * 32;      // stacked query rows per workgroup
constexpr int PTHREADS = PWAVES * 64;
typedef __attribute__((address_space(3))) s16x4 plds_s16x4;

struct PrefixArgs {
  const bf16 *q, *k, *v, *pk, *pv;
  bf16* o;
  long long q_cs, q_hs, q_rs, k_cs, k_hs, k_rs, v_cs, v_hs, v_rs;
  long long pk_gs, pk_hs, pk_rs, pv_gs, pv_hs, pv_rs, o_cs, o_hs, o_rs;
  int n_cont, group_size, heads, lc, plen, hd;
  float scale;
};

// A-operand fragment: 8 consecutive d of row (lane&31) of 32-row tile t, d-step s (ds_read_b128)
__device__ __forceinline__ bf16x8 pfrag_rows(const char* lds, int t, int s, int lane) {
  return *(const bf16x8*)(lds + (t * 32 + (lane & 31)) * PROWB + (s * 16 + (lane >> 5) * 8) * 2);
}
// transposed fragment: column d = dt*32 + (lane&31); rows t*32 + ks*16 + {0..3}+4h, +8 -- the k order acc_to_frag produces
__device__ __forceinline__ bf16x8 pfrag_cols(const char* lds, int t, int ks, int dt, int lane) {
  const int h = lane >> 5;
  const int rbase = t * 32 + ks * 16 + 4 * h + ((lane & 15) >> 2);
  const int col = dt * 32 + ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((plds_s16x4*)(lds + rbase * PROWB + col * 2));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((plds_s16x4*)(lds + (rbase + 8) * PROWB + col * 2));
  union { struct { s16x4 a, b; } s; bf16x8 v; } u;
  u.s.a = lo;
  u.s.b = hi;
  return u.v;
}
__device__ __forceinline__ bf16x8 pacc_to_frag(const f32x16& a, int ks) {
  f32x8 f;
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = a[8 * ks + e];
  return cvt8(f);
}
// row inside a 32-row tile held by accumulator register `reg` of this lane (mfma_f32_32x32x16 C/D map)
__device__ __forceinline__ int pacc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// 64 key rows x HD columns -> registers -> LDS.  Row kr of the streamed sequence lives in segment kr / seg (a continuation, or
// the one prefix segment) at base + (kr / seg) * seg_stride + (kr % seg) * rs.  Rows past `last` and columns past hd are zeros
// (the PV product multiplies them by exact-zero probabilities; zeros keep it finite).
template <int HD>
struct SegStage {
  static constexpr int CPR = (HD + 31) / 32 * 4;       // 16-byte chunks per (padded) row
  static constexpr int NLOAD = (PCH * CPR + PTHREADS - 1) / PTHREADS;   // 2 (hd 64) or 3 (hd 80) b128 per thread
  i32x4 r[NLOAD];

  __device__ __forceinline__ void issue(const bf16* base, int tid, int row0, int last, int seg, long long seg_stride, long long rs,
                                        int hd) {
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) {
      const int c = tid + PTHREADS * i;
      const int row = c / CPR, cc = c - row * CPR;
      const int kr = row0 + row;
      const bool ok = (c < PCH * CPR) && (kr <= last) && (cc * 8 < hd);
      i32x4 x = i32x4{0, 0, 0, 0};
      if (ok) {
        const int sg = kr / seg;
        x = *(const i32x4*)(base + sg * seg_stride + (long long)(kr - sg * seg) * rs + cc * 8);
      }
      r[i] = x;
    }
  }
  __device__ __forceinline__ void commit(char* lds, int tid) {
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) {
      const int c = tid + PTHREADS * i;
      const int row = c / CPR, cc = c - row * CPR;
      if (c < PCH * CPR) *(i32x4*)(lds + row * PROWB + cc * 16) = r[i];
    }
  }
};

template <int HD>
__global__ __launch_bounds__(PTHREADS, 2) void attn_prefix_fwd_kernel(const PrefixArgs p) {
  constexpr int NS = HD / 16;
  constexpr int NDT = (HD + 31) / 32;
  __shared__ __attribute__((aligned(16))) char smem[4 * PCHUNK];     // [buf][K|V]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.z, h = blockIdx.y;
  const int c0 = g * p.group_size;
  const int nc = min(p.group_size, p.n_cont - c0);
  const int rows_g = nc * p.lc;                          // stacked rows of this group
  const int blk_r0 = blockIdx.x * PROWS;
  if (blk_r0 >= rows_g) return;                          // (a short last group): uniform over the workgroup
  const int wq0 = blk_r0 + wave * 32;
  const int r = wq0 + (lane & 31);                       // this lane's stacked query row
  const int rc = min(r, rows_g - 1);
  const int ci = rc / p.lc, ii = rc - ci * p.lc;
  const int row_first_key = ci * p.lc;                   // first stacked own key visible to row r

  bf16x8 qf[NS];
  {
    const bf16* rp = p.q + (long long)(c0 + ci) * p.q_cs + (long long)h * p.q_hs + (long long)ii * p.q_rs + (lane >> 5) * 8;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      union { i32x4 i; bf16x8 b; } u;
      const bool cok = s * 16 + (lane >> 5) * 8 < p.hd;
      u.i = *(const i32x4*)(rp + (cok ? s * 16 : 0));
      if (!(r < rows_g && cok)) u.i = i32x4{0, 0, 0, 0};
      qf[s] = u.b;
    }
  }
  const float sc = p.scale;
  float m = -INFINITY, l = 0.f;
  f32x16 oacc[NDT];
#pragma unroll
  for (int d = 0; d < NDT; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;

  // one 32-key tile: scores, masked online-softmax update, PV.  visible(key) is this lane's mask for tile key index `key`.
  auto tile = [&](const char* kl, const char* vl, int kt, int key0, auto visible) {
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
    for (int st = 0; st < NS; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pfrag_rows(kl, kt, st, lane), qf[st], s, 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s[e] = visible(key0 + pacc_row(e, lane)) ? s[e] * sc : -INFINITY;
      mx = fmaxf(mx, s[e]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);
    const float mb = mn > -INFINITY ? mn : 0.f;          // a row with nothing visible yet keeps exact zeros
    const float alpha = __expf(m - mb);                  // m = -inf: 0 (nothing accumulated to rescale)
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s[e] = __expf(s[e] - mb);
      sum += s[e];
    }
    sum += __shfl_xor(sum, 32, 64);
    l = l * alpha + sum;
    m = mn;
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[d][e] *= alpha;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 pf = pacc_to_frag(s, ks);
#pragma unroll
      for (int d = 0; d < NDT; ++d)
        oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pfrag_cols(vl, kt, ks, d, lane), pf, oacc[d], 0, 0, 0);
    }
  };

  SegStage<HD> sk_, sv_;
  // ---------------- phase 1: the group's prefix, dense for every row
  if (p.plen > 0) {
    const bf16* kb = p.pk + (long long)g * p.pk_gs + (long long)h * p.pk_hs;
    const bf16* vb = p.pv + (long long)g * p.pv_gs + (long long)h * p.pv_hs;
    const int last = p.plen - 1;
    const int nchunk = (p.plen + PCH - 1) / PCH;
    sk_.issue(kb, tid, 0, last, p.plen, 0, p.pk_rs, p.hd);
    sv_.issue(vb, tid, 0, last, p.plen, 0, p.pv_rs, p.hd);
    sk_.commit(smem, tid);
    sv_.commit(smem + PCHUNK, tid);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
      const int cur = c & 1;
      if (c + 1 < nchunk) {
        sk_.issue(kb, tid, (c + 1) * PCH, last, p.plen, 0, p.pk_rs, p.hd);
        sv_.issue(vb, tid, (c + 1) * PCH, last, p.plen, 0, p.pv_rs, p.hd);
      }
      const char* kl = smem + cur * 2 * PCHUNK;
      {
#pragma unroll 1
        for (int kt = 0; kt < 2; ++kt) {
          const int key0 = c * PCH + kt * 32;
          if (key0 > last) continue;
          tile(kl, kl + PCHUNK, kt, key0, [&](int key) { return key <= last; });
        }
      }
      if (c + 1 < nchunk) {
        sk_.commit(smem + (cur ^ 1) * 2 * PCHUNK, tid);
        sv_.commit(smem + (cur ^ 1) * 2 * PCHUNK + PCHUNK, tid);
      }
      __syncthreads();
    }
  }

  // ---------------- phase 2: own keys, block-diagonal causal over the stacked rows
  {
    const bf16* kb = p.k + (long long)c0 * p.k_cs + (long long)h * p.k_hs;
    const bf16* vb = p.v + (long long)c0 * p.v_cs + (long long)h * p.v_hs;
    const int kb0 = blk_r0 / p.lc * p.lc;                          // first own key any row of the block sees
    const int last = min(rows_g, blk_r0 + PROWS) - 1;              // ... and the last
    const int nchunk = (last - kb0) / PCH + 1;
    const int wk0 = min(wq0, rows_g - 1) / p.lc * p.lc;            // this wave's key window (wave-uniform tile skips)
    const int wk1 = min(wq0 + 31, rows_g - 1);
    sk_.issue(kb, tid, kb0, last, p.lc, p.k_cs, p.k_rs, p.hd);
    sv_.issue(vb, tid, kb0, last, p.lc, p.v_cs, p.v_rs, p.hd);
    sk_.commit(smem, tid);
    sv_.commit(smem + PCHUNK, tid);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
      const int cur = c & 1;
      if (c + 1 < nchunk) {
        sk_.issue(kb, tid, kb0 + (c + 1) * PCH, last, p.lc, p.k_cs, p.k_rs, p.hd);
        sv_.issue(vb, tid, kb0 + (c + 1) * PCH, last, p.lc, p.v_cs, p.v_rs, p.hd);
      }
      const char* kl = smem + cur * 2 * PCHUNK;
      if (wq0 < rows_g) {
#pragma unroll 1
        for (int kt = 0; kt < 2; ++kt) {
          const int key0 = kb0 + c * PCH + kt * 32;
          if (key0 > wk1 || key0 + 31 < wk0) continue;
          tile(kl, kl + PCHUNK, kt, key0, [&](int key) { return key >= row_first_key && key <= rc; });
        }
      }
      if (c + 1 < nchunk) {
        sk_.commit(smem + (cur ^ 1) * 2 * PCHUNK, tid);
        sv_.commit(smem + (cur ^ 1) * 2 * PCHUNK + PCHUNK, tid);
      }
      __syncthreads();
    }
  }

  if (r < rows_g) {
    const float inv_l = 1.0f / l;                        // l >= 1: the row sees at least its own key
    bf16* orow = p.o + (long long)(c0 + ci) * p.o_cs + (long long)h * p.o_hs + (long long)ii * p.o_rs;
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int col = d * 32 + 8 * q4 + 4 * (lane >> 5);
        if (col < p.hd) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = oacc[d][4 * q4 + e] * inv_l;
          *(bf16x4*)(orow + col) = cvt4(v);
        }
      }
  }
}

}  // namespace

extern "C" int mpv_attn_prefix_fwd(const mpv_attn_prefix_desc* d, hipStream_t stream) {
  MPV_REQUIRE(d && d->q && d->k && d->v && d->o && (d->prefix_len == 0 || (d->pk && d->pv)), MPV_E_ARG,
              "mpv_attn_prefix_fwd: null pointer");
  MPV_REQUIRE(d->head_dim == 64 || d->head_dim == 80, MPV_E_SHAPE,
              "mpv_attn_prefix_fwd: head_dim %d is not supported (64: the 1.3B decoder, 80: 2.7B)", d->head_dim);
  MPV_REQUIRE(d->n_cont > 0 && d->group_size > 0 && d->heads > 0 && d->cont_len > 0 && d->prefix_len >= 0, MPV_E_SHAPE,
              "mpv_attn_prefix_fwd: empty problem (n_cont %d, group_size %d, heads %d, cont_len %d, prefix_len %d)", d->n_cont,
              d->group_size, d->heads, d->cont_len, d->prefix_len);
  MPV_REQUIRE(d->n_groups == (d->n_cont + d->group_size - 1) / d->group_size, MPV_E_SHAPE,
              "mpv_attn_prefix_fwd: n_groups %d must be ceil(n_cont %d / group_size %d)", d->n_groups, d->n_cont, d->group_size);
  MPV_REQUIRE((long long)d->group_size * d->cont_len < (1ll << 30) && d->n_groups <= 65535 && d->heads <= 65535, MPV_E_SHAPE,
              "mpv_attn_prefix_fwd: problem too large");
  const int64_t st[] = {d->q_cs, d->q_hs, d->q_rs, d->k_cs, d->k_hs, d->k_rs, d->v_cs, d->v_hs, d->v_rs,
                        d->pk_gs, d->pk_hs, d->pk_rs, d->pv_gs, d->pv_hs, d->pv_rs};
  bool al = true;
  for (int64_t s : st) al = al && (s % 8 == 0);
  MPV_REQUIRE(al && d->o_cs % 4 == 0 && d->o_hs % 4 == 0 && d->o_rs % 4 == 0, MPV_E_ALIGN,
              "mpv_attn_prefix_fwd: strides must keep q/k/v/pk/pv rows 16-byte and o rows 8-byte aligned");
  MPV_REQUIRE((((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->pk | (uintptr_t)d->pv) & 15) == 0 &&
                  ((uintptr_t)d->o & 7) == 0,
              MPV_E_ALIGN, "mpv_attn_prefix_fwd: q/k/v/pk/pv must be 16-byte aligned, o 8-byte aligned");
  MPV_REQUIRE(d->scale > 0.f, MPV_E_ARG, "mpv_attn_prefix_fwd: scale must be positive");
  PrefixArgs a;
  a.q = (const bf16*)d->q;
  a.k = (const bf16*)d->k;
  a.v = (const bf16*)d->v;
  a.pk = (const bf16*)d->pk;
  a.pv = (const bf16*)d->pv;
  a.o = (bf16*)d->o;
  a.q_cs = d->q_cs; a.q_hs = d->q_hs; a.q_rs = d->q_rs;
  a.k_cs = d->k_cs; a.k_hs = d->k_hs; a.k_rs = d->k_rs;
  a.v_cs = d->v_cs; a.v_hs = d->v_hs; a.v_rs = d->v_rs;
  a.pk_gs = d->pk_gs; a.pk_hs = d->pk_hs; a.pk_rs = d->pk_rs;
  a.pv_gs = d->pv_gs; a.pv_hs = d->pv_hs; a.pv_rs = d->pv_rs;
  a.o_cs = d->o_cs; a.o_hs = d->o_hs; a.o_rs = d->o_rs;
  a.n_cont = d->n_cont;
  a.group_size = d->group_size;
  a.heads = d->heads;
  a.lc = d->cont_len;
  a.plen = d->prefix_len;
  a.hd = d->head_dim;
  a.scale = d->scale;
  const int rows = d->group_size * d->cont_len;
  const dim3 grid((unsigned)((rows + PROWS - 1) / PROWS), (unsigned)d->heads, (unsigned)d->n_groups);
  if (d->head_dim == 64)
    hipLaunchKernelGGL(attn_prefix_fwd_kernel<64>, grid, dim3(PTHREADS), 0, stream, a);
  else
    hipLaunchKernelGGL(attn_prefix_fwd_kernel<80>, grid, dim3(PTHREADS), 0, stream, a);
  return mpv_check_launch("mpv_attn_prefix_fwd");
}
