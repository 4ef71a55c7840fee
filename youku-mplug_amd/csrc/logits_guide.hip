// Guided (classifier-free / contrastive) decoding on the device: mpv_logits_guide rewrites one step's conditional logits in place from
// the unconditional ones -- guided = c + scale_m1 * (c - u) on the max-centred rows, with an optional plausibility ban -- before any
// other editor or reader sees them.  The semantics are stated in include/mpv.h.
//
// One workgroup of 1024 threads per row; nothing is shared between rows.  A row of at most 65536 columns is at most 8192 chunks of
// 16 bytes, eight per thread and matrix: the row PAIR is loaded once into registers (64 VGPRs), so the launch moves the byte floor --
// cond and uncond read once, cond written once.  Two steps, one barrier between them:
//   1. load the chunks and take the two maxima: per thread, per wave (xor shuffles), then over the 16 waves through LDS, where every
//      thread folds the same 16 values.  A maximum is order-free; a zero maximum is taken as +0 so that its sign cannot depend on
//      which of two zeros a lane saw first.
//   2. every thread rewrites its own chunks from its registers and stores them once.  One writer per column, 16-byte accesses only,
//      columns >= vocab never touched.
// The arithmetic of an element is five separate fp32 operations (contraction is switched off in lg_one: the multiply and the add
// must not become one fused operation, or the result would differ from the stated one in the last bit).  No scratch, no atomics: the
// result does not depend on thread timing.
#include "mpv_common.h"
#include "../../include/mpv.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int LG_THREADS = 1024, LG_WAVES = LG_THREADS / 64, LG_MAX_VOCAB = 65536, LG_CHUNKS = LG_MAX_VOCAB / 8 / LG_THREADS;   // 8 per thread

__device__ __forceinline__ float lg_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float lg_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

__device__ __forceinline__ float lg_max8(const uint4 x, float m) {
  m = fmaxf(m, fmaxf(lg_lo(x.x), lg_hi(x.x)));
  m = fmaxf(m, fmaxf(lg_lo(x.y), lg_hi(x.y)));
  m = fmaxf(m, fmaxf(lg_lo(x.z), lg_hi(x.z)));
  return fmaxf(m, fmaxf(lg_lo(x.w), lg_hi(x.w)));
}

// one element: the bf16 bits of c + scale_m1 * (c - u), or the ban value where c < plaus_log
__device__ __forceinline__ unsigned lg_one(float x, float y, float m_c, float m_u, float scale_m1, float plaus_log, unsigned ban_bits) {
#pragma clang fp contract(off)
  const float c = x - m_c;
  const float u = y - m_u;
  const float diff = c - u;
  const float prod = scale_m1 * diff;
  const float g = c + prod;
  const unsigned bits = (unsigned)__builtin_bit_cast(unsigned short, f2bf(g));
  return c < plaus_log ? ban_bits : bits;
}

__device__ __forceinline__ unsigned lg_pair(unsigned wc, unsigned wu, float m_c, float m_u, float s, float pl, unsigned ban_bits) {
  return lg_one(lg_lo(wc), lg_lo(wu), m_c, m_u, s, pl, ban_bits) | (lg_one(lg_hi(wc), lg_hi(wu), m_c, m_u, s, pl, ban_bits) << 16);
}

__global__ __launch_bounds__(LG_THREADS) void logits_guide_kernel(mpv_logits_guide_desc d, unsigned ban_bits) {
  __shared__ float red[2][LG_WAVES];
  const int tid = threadIdx.x;
  const long long row = blockIdx.x;
  const int nchunks = d.vocab >> 3;                            // <= 8192 = LG_CHUNKS * LG_THREADS
  uint4* crow = (uint4*)((unsigned short*)d.cond + row * d.ld_c);
  const uint4* urow = (const uint4*)((const unsigned short*)d.uncond + row * d.ld_u);

  // ---- 1. the row pair into registers, and the two maxima
  uint4 rc[LG_CHUNKS], ru[LG_CHUNKS];
  float m_c = -INFINITY, m_u = -INFINITY;
#pragma unroll
  for (int j = 0; j < LG_CHUNKS; ++j) {
    const int k = tid + j * LG_THREADS;
    if (k < nchunks) {
      rc[j] = crow[k];
      ru[j] = urow[k];
      m_c = lg_max8(rc[j], m_c);
      m_u = lg_max8(ru[j], m_u);
    }
  }
  m_c = wave_max(m_c);
  m_u = wave_max(m_u);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = m_c;
    red[1][tid >> 6] = m_u;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < LG_WAVES; ++w) {
    m_c = fmaxf(m_c, red[0][w]);
    m_u = fmaxf(m_u, red[1][w]);
  }
  if (m_c == 0.f) m_c = 0.f;                                   // -0 and +0 are one maximum: +0
  if (m_u == 0.f) m_u = 0.f;

  // ---- 2. one writer per chunk
#pragma unroll
  for (int j = 0; j < LG_CHUNKS; ++j) {
    const int k = tid + j * LG_THREADS;
    if (k < nchunks) {
      uint4 o;
      o.x = lg_pair(rc[j].x, ru[j].x, m_c, m_u, d.scale_m1, d.plaus_log, ban_bits);
      o.y = lg_pair(rc[j].y, ru[j].y, m_c, m_u, d.scale_m1, d.plaus_log, ban_bits);
      o.z = lg_pair(rc[j].z, ru[j].z, m_c, m_u, d.scale_m1, d.plaus_log, ban_bits);
      o.w = lg_pair(rc[j].w, ru[j].w, m_c, m_u, d.scale_m1, d.plaus_log, ban_bits);
      crow[k] = o;
    }
  }
}

// round-to-nearest-even bf16 bits of a float that is -inf or finite
unsigned lg_bf16_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, sizeof u);
  if ((u & 0x7f800000u) == 0x7f800000u) return u >> 16;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

}  // namespace

extern "C" int mpv_logits_guide(const mpv_logits_guide_desc* d, hipStream_t stream) {
  const char* who = "mpv_logits_guide";
  MPV_REQUIRE(d, MPV_E_ARG, "%s: null descriptor", who);
  MPV_REQUIRE(d->cond && d->uncond, MPV_E_ARG, "%s: null cond or uncond", who);
  MPV_REQUIRE(d->rows >= 1, MPV_E_SHAPE, "%s: rows (%d) must be positive", who, d->rows);
  MPV_REQUIRE(d->vocab >= 8 && d->vocab <= LG_MAX_VOCAB && d->vocab % 8 == 0, MPV_E_SHAPE, "%s: vocab (%d) must be a multiple of 8 in [8, %d]", who,
              d->vocab, LG_MAX_VOCAB);
  MPV_REQUIRE(d->ld_c >= d->vocab && d->ld_c % 8 == 0, MPV_E_SHAPE, "%s: ld_c (%lld) must be a multiple of 8 and at least vocab (%d)", who,
              (long long)d->ld_c, d->vocab);
  MPV_REQUIRE(d->ld_u >= d->vocab && d->ld_u % 8 == 0, MPV_E_SHAPE, "%s: ld_u (%lld) must be a multiple of 8 and at least vocab (%d)", who,
              (long long)d->ld_u, d->vocab);
  MPV_REQUIRE(((uintptr_t)d->cond & 15) == 0 && ((uintptr_t)d->uncond & 15) == 0, MPV_E_ALIGN, "%s: cond and uncond must be 16-byte aligned", who);
  MPV_REQUIRE(isfinite(d->scale_m1) && d->scale_m1 >= -1.f, MPV_E_ARG, "%s: scale_m1 (%g) must be finite and at least -1", who,
              (double)d->scale_m1);
  MPV_REQUIRE(!isnan(d->plaus_log) && d->plaus_log <= 0.f, MPV_E_ARG, "%s: plaus_log (%g) must be -inf or at most 0", who, (double)d->plaus_log);
  MPV_REQUIRE(!isnan(d->ban_value) && d->ban_value < 0.f, MPV_E_ARG, "%s: ban_value (%g) must be -inf or a finite negative number", who,
              (double)d->ban_value);
  hipLaunchKernelGGL(logits_guide_kernel, dim3((unsigned)d->rows), dim3(LG_THREADS), 0, stream, *d, lg_bf16_bits(d->ban_value));
  return mpv_check_launch(who);
}
