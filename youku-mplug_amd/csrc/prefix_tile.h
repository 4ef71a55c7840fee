// prefix_tile.h -- the 32-key score / online-softmax / PV tile of the shared-prefix attention kernels (prefix_attention.hip's
// attn_prefix_fwd_kernel, decode_shared_attention.hip's attn_decode_shared_kernel): K/V streamed through LDS against 32 query rows
// held in registers.  The tile is a function of the softmax state because the decode kernel keeps two states per wave.  Conventions
// of attention.hip's forward kernel: S^T = K Q^T so a lane owns one query row of the 32x32 score tile, the probabilities feed the PV
// MFMA as its B operand from registers, V^T fragments come from the transposing LDS read.
#pragma once

#include "mpv_common.h"

namespace {

constexpr int PROWB = 208;              // LDS row pitch in bytes (96 bf16 + 16 pad: conflict-free ds_read_b128)
typedef __attribute__((address_space(3))) s16x4 plds_s16x4;

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

// One 32-key tile (tile kt of the chunk at kl / vl) against this wave's 32 query rows qf: scores, masked online-softmax update of
// this lane's row statistics (m, l) and PV into oacc.  visible(key0 + r) is this lane's mask for the tile's key row r.
template <int HD, class Visible>
__device__ __forceinline__ void ptile_update(const char* kl, const char* vl, int kt, int key0, const bf16x8 (&qf)[HD / 16], float sc,
                                             float& m, float& l, f32x16 (&oacc)[(HD + 31) / 32], int lane, Visible visible) {
  constexpr int NS = HD / 16;
  constexpr int NDT = (HD + 31) / 32;
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
}

}  // namespace
