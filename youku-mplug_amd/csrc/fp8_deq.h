// fp8_deq.h -- the exact e4m3fn -> bf16 conversion, shared by the FP8 weight products (gemm_w8.hip) and the searches over an FP8
// gallery (search_common.h).
#pragma once
#include "mpv_common.h"

namespace {

// exact for all 254 finite codes, subnormals included: v_cvt_pk_f32_fp8 is the OCP e4m3fn conversion on gfx950 and every e4m3 value
// has 4 significant bits, so the upper half of its fp32 pattern IS its bf16 pattern.  Two codes -> one dword of two bf16.
template <bool HI>
__device__ __forceinline__ int deq_pair(int codes) {
  const f32x2 f = __builtin_amdgcn_cvt_pk_f32_fp8(codes, HI);
  return (int)__builtin_amdgcn_perm(__float_as_uint(f[1]), __float_as_uint(f[0]), 0x07060302u);
}
union Frag {
  i32x4 i;
  bf16x8 b;
};
// 16 codes (one 16-byte chunk, k ascending) -> the two bf16x8 MFMA operands of k 0..7 and 8..15
__device__ __forceinline__ void deq_chunk(const i32x4 c, Frag& lo, Frag& hi) {
  lo.i = i32x4{deq_pair<false>(c[0]), deq_pair<true>(c[0]), deq_pair<false>(c[1]), deq_pair<true>(c[1])};
  hi.i = i32x4{deq_pair<false>(c[2]), deq_pair<true>(c[2]), deq_pair<false>(c[3]), deq_pair<true>(c[3])};
}

}  // namespace
