// gemm_w8.hip -- weight-only FP8 (OCP e4m3fn, one power-of-two fp32 scale per output row) for the decode steps of the frozen
// decoder (include/mpv.h, "FP8 decoder weights" states the numeric contract):
//   mpv_quantize_rows_e4m3  row amax -> exponent -> codes, one workgroup per weight row
//   mpv_gemm_w8             C[M,N] = epi(scale[n] * sum_k A[m,k] deq(code[n,k])) for 1 <= M <= 512 rows: the weight-streaming kernel
//                           of gemm.hip (gemm_small_m_kernel) with an 8-bit weight and up to 32 row blocks of 16 rows per workgroup
//   mpv_gpt_embed_w8_fwd    mpv_gpt_embed_fwd with the token rows taken from the codes (the quantised decoder IS a bf16 model whose
//                           tied embedding holds deq(code) * scale: the rows are looked up in that bf16 table without storing it)
#include "../../include/mpv.h"
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

struct W8Args {
  const bf16* A;
  const uint8_t* W;
  const float* scale;
  bf16* C;
  int M, N, K;
  int m0;                                                     // first row of this launch in C's row numbering (A is already offset)
  long long lda, ldw, ldc, ldr;
  RowMap cmap;
  const bf16* bias;
  const bf16* residual;
  int act;
};

// A workgroup owns CG groups of COLS output columns; its NW waves split K in 64-wide blocks (block kb belongs to wave
// kb / ceil(kblocks / NW), as in gemm_small_m_kernel); per K-block and column group a lane loads ONE 16-byte chunk of 16 codes of
// weight row n = lane & 15, turns it into two bf16 operands in registers and multiplies them into every one of the MB 16-row blocks
// of A (32 bytes of an activation row per lane and block, from L2; with CG = 2 they serve 32 columns).  The weight is read once per
// product.  The summation order of an output element is: inside a wave the K-blocks in ascending order (one MFMA accumulator
// chain), then the NW per-wave partials in the fixed order below -- a function of (N, K) only (the host picks NW from N and K), never
// of M, MB, COLS or CG: row m of a 160-row call is bit-identical to the same row computed alone.
// FULL: N % (COLS * CG) == 0 and K % 64 == 0 (no column or chunk guards in the loop).
template <bool FULL, int NW, int COLS, int MB, int CG = 1>
__global__ __launch_bounds__(64 * NW) void gemm_w8_kernel(const W8Args p) {
  __shared__ float part[NW][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * (COLS * CG);
  const int r = lane & 15, g = lane >> 4;                       // operand row (n for W, m for A), 16-wide k group
  const int kblocks = (p.K + 63) >> 6;
  const int per = (kblocks + NW - 1) / NW;
  const int kb0 = wave * per, kb1 = min(kblocks, kb0 + per);
  bool wok[CG];
  const uint8_t* wrow[CG];
#pragma unroll
  for (int cg = 0; cg < CG; ++cg) {
    wok[cg] = r < COLS && (n0 + cg * COLS + r) < p.N;
    wrow[cg] = p.W + (long long)(wok[cg] ? n0 + cg * COLS + r : 0) * p.ldw + g * 16;
  }
  const int nmb = (p.M + 15) >> 4;                              // row blocks in use (<= MB)
  f32x4 acc[MB][CG];
#pragma unroll
  for (int b = 0; b < MB; ++b)
#pragma unroll
    for (int cg = 0; cg < CG; ++cg) acc[b][cg] = f32x4{0.f, 0.f, 0.f, 0.f};
  const i32x4 zero = {0, 0, 0, 0};
  constexpr int UN = MB == 1 ? (NW > 4 ? 4 : 8) : (NW == 4 && CG == 1 ? 4 : 2);      // K-blocks in flight per lane
  int kb = kb0;
  for (; kb + UN <= kb1; kb += UN) {
    i32x4 c[UN][CG];
#pragma unroll
    for (int u = 0; u < UN; ++u)
#pragma unroll
      for (int cg = 0; cg < CG; ++cg) {
        const bool ok = wok[cg] && (FULL || (kb + u) * 64 + g * 16 < p.K);      // K % 16 == 0: a chunk is all-in or all-out
        c[u][cg] = ok ? *(const i32x4*)(wrow[cg] + (long long)(kb + u) * 64) : zero;
      }
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      if (b < nmb) {                                                     // wave-uniform
        const int m = b * 16 + r;
        const bool aok = m < p.M;
        const bf16* arow = p.A + (long long)(aok ? m : 0) * p.lda + g * 16;
        Frag a0[UN], a1[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
          const bool ok = aok && (FULL || (kb + u) * 64 + g * 16 < p.K);
          a0[u].i = ok ? *(const i32x4*)(arow + (long long)(kb + u) * 64) : zero;
          a1[u].i = ok ? *(const i32x4*)(arow + (long long)(kb + u) * 64 + 8) : zero;
        }
#pragma unroll
        for (int u = 0; u < UN; ++u)
#pragma unroll
          for (int cg = 0; cg < CG; ++cg) {
            Frag w0, w1;
            deq_chunk(c[u][cg], w0, w1);
            acc[b][cg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[u].b, w0.b, acc[b][cg], 0, 0, 0);
            acc[b][cg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[u].b, w1.b, acc[b][cg], 0, 0, 0);
          }
      }
    }
  }
  for (; kb < kb1; ++kb) {
    Frag w0[CG], w1[CG];
#pragma unroll
    for (int cg = 0; cg < CG; ++cg) {
      const bool wk = wok[cg] && (FULL || kb * 64 + g * 16 < p.K);
      const i32x4 c = wk ? *(const i32x4*)(wrow[cg] + (long long)kb * 64) : zero;
      deq_chunk(c, w0[cg], w1[cg]);
    }
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      if (b < nmb) {
        const int m = b * 16 + r;
        const bool ok = m < p.M && (FULL || kb * 64 + g * 16 < p.K);
        const bf16* arow = p.A + (long long)(ok ? m : 0) * p.lda + g * 16;
        Frag a0, a1;
        a0.i = ok ? *(const i32x4*)(arow + (long long)kb * 64) : zero;
        a1.i = ok ? *(const i32x4*)(arow + (long long)kb * 64 + 8) : zero;
#pragma unroll
        for (int cg = 0; cg < CG; ++cg) {
          acc[b][cg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0.b, w0[cg].b, acc[b][cg], 0, 0, 0);
          acc[b][cg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1.b, w1[cg].b, acc[b][cg], 0, 0, 0);
        }
      }
    }
  }
  // D layout: lane -> column n = lane & 15, rows m = 4 * (lane >> 4) + i.  One 16 x 16 tile at a time through LDS.
  const int em = tid >> 4, ec = tid & 15;
#pragma unroll
  for (int cg = 0; cg < CG; ++cg) {
    const int n = n0 + cg * COLS + ec;
    const bool eok = tid < 256 && ec < COLS && n < p.N;
    const float sc = eok ? p.scale[n] : 0.f;
    const float bias = (eok && p.bias) ? bf2f(p.bias[n]) : 0.f;
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      if (b < nmb) {
        if (b || cg) __syncthreads();                                    // the previous tile's partials have been read
#pragma unroll
        for (int i = 0; i < 4; ++i) part[wave][4 * g + i][r] = acc[b][cg][i];
        __syncthreads();
        const int m = b * 16 + em;
        if (eok && m < p.M) {
          float v = (part[0][em][ec] + part[1][em][ec]) + (part[2][em][ec] + part[3][em][ec]);
#pragma unroll
          for (int w = 4; w < NW; w += 4) v += (part[w][em][ec] + part[w + 1][em][ec]) + (part[w + 2][em][ec] + part[w + 3][em][ec]);
          v = v * sc + bias;
          if (p.act) v = gelu_tanh_f(bf2f(f2bf(v)));
          const long long crow = map_row(p.cmap, p.m0 + m);
          if (p.residual) v += bf2f(p.residual[crow * p.ldr + n]);
          p.C[crow * p.ldc + n] = f2bf(v);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// one workgroup per weight row: amax, the exponent of the contract, then the codes (v_cvt_pk_fp8_f32: round to nearest even, OCP
// e4m3fn on gfx950; |w * 2^-e| <= 448, so its saturation never acts)
__global__ __launch_bounds__(256) void quantize_rows_e4m3_kernel(const bf16* __restrict__ w, int K, long long ldw, uint8_t* __restrict__ codes,
                                                                 float* __restrict__ scale) {
  __shared__ float red[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const bf16* row = w + (long long)n * ldw;
  float amax = 0.f;
  for (int k = tid * 8; k < K; k += 256 * 8) {
    const f32x8 v = cvt8(*(const bf16x8*)(row + k));
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
  }
  amax = wave_max(amax);
  if ((tid & 63) == 0) red[tid >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  int e = 0;
  if (amax > 0.f) {
    int x;
    const float f = frexpf(amax, &x);
    e = max(f <= 0.875f ? x - 9 : x - 8, -126);                // (a scale below 2^-126 would not be a normal fp32)
  }
  if (tid == 0) scale[n] = ldexpf(1.0f, e);
  const float inv = ldexpf(1.0f, -e);                          // e in [-126, 120]: exact
  uint8_t* crow = codes + (long long)n * K;
  for (int k = tid * 8; k < K; k += 256 * 8) {
    const f32x8 v = cvt8(*(const bf16x8*)(row + k)) * inv;
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], hi, true);
    *(i32x2*)(crow + k) = i32x2{lo, hi};
  }
}

// gpt_embed_fwd_kernel (elementwise.hip) without dropout, the token rows being deq(code) * scale
__global__ void gpt_embed_w8_fwd_kernel(const bf16* __restrict__ query, const int64_t* __restrict__ ids, const uint8_t* __restrict__ codes,
                                        const float* __restrict__ scale, const bf16* __restrict__ wpe, bf16* __restrict__ h, int B, int Q,
                                        int L, int H) {
  const int H8 = H / 8, S = Q + L;
  const long long total = (long long)B * S * H8;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int c8 = (int)(idx % H8);
    const long long row = idx / H8;
    const int s = (int)(row % S);
    const long long b = row / S;
    f32x8 v;
    if (s < Q) {
      v = cvt8(*(const bf16x8*)(query + (b * Q + s) * (long long)H + c8 * 8));
    } else {
      const int64_t id = ids[b * L + (s - Q)];
      const i32x2 c = *(const i32x2*)(codes + id * (long long)H + c8 * 8);
      const float sc = scale[id];
      const f32x2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8(c[0], false), f1 = __builtin_amdgcn_cvt_pk_f32_fp8(c[0], true);
      const f32x2 f2 = __builtin_amdgcn_cvt_pk_f32_fp8(c[1], false), f3 = __builtin_amdgcn_cvt_pk_f32_fp8(c[1], true);
      v = f32x8{f0[0], f0[1], f1[0], f1[1], f2[0], f2[1], f3[0], f3[1]} * sc;        // exact: a bf16 value
    }
    v += cvt8(*(const bf16x8*)(wpe + (long long)s * H + c8 * 8));
    *(bf16x8*)(h + row * H + c8 * 8) = cvt8(v);
  }
}

template <bool FULL, int NW, int COLS>
void launch_w8(const W8Args& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + COLS - 1) / COLS)), block(64 * NW);
  const int nmb = (a.M + 15) / 16;
  if (nmb == 1) hipLaunchKernelGGL((gemm_w8_kernel<FULL, NW, COLS, 1>), grid, block, 0, stream, a);
  else if (nmb <= 4) hipLaunchKernelGGL((gemm_w8_kernel<FULL, NW, COLS, 4>), grid, block, 0, stream, a);
  else if constexpr (NW == 16) hipLaunchKernelGGL((gemm_w8_kernel<FULL, NW, COLS, 8>), grid, block, 0, stream, a);      // (the host sends <= 128 rows)
  else if (nmb <= 16) {
    // many rows: the activations are what a workgroup reads most of -- two column groups per workgroup halve that traffic where
    // enough workgroups remain
    if constexpr (FULL && COLS == 16) {
      if (a.N % 32 == 0 && a.N / 32 >= 192) {
        hipLaunchKernelGGL((gemm_w8_kernel<FULL, NW, COLS, 16, 2>), dim3((unsigned)(a.N / 32)), block, 0, stream, a);
        return;
      }
    }
    hipLaunchKernelGGL((gemm_w8_kernel<FULL, NW, COLS, 16>), grid, block, 0, stream, a);
  } else hipLaunchKernelGGL((gemm_w8_kernel<FULL, NW, COLS, 32>), grid, block, 0, stream, a);
}

}  // namespace

extern "C" int mpv_quantize_rows_e4m3(const void* w, int64_t N, int64_t K, int64_t ldw, void* codes, float* scale, hipStream_t stream) {
  MPV_REQUIRE(w && codes && scale, MPV_E_ARG, "mpv_quantize_rows_e4m3: null pointer");
  MPV_REQUIRE(N > 0 && N < (1ll << 31) && K > 0 && K < (1ll << 31) && K % 16 == 0 && ldw >= K, MPV_E_SHAPE,
              "mpv_quantize_rows_e4m3: N (%lld) must be positive, K (%lld) a positive multiple of 16, ldw (%lld) at least K", (long long)N,
              (long long)K, (long long)ldw);
  MPV_REQUIRE(ldw % 8 == 0 && (((uintptr_t)w | (uintptr_t)codes) & 15) == 0 && ((uintptr_t)scale & 3) == 0, MPV_E_ALIGN,
              "mpv_quantize_rows_e4m3: ldw must be a multiple of 8, w and codes 16-byte aligned");
  hipLaunchKernelGGL(quantize_rows_e4m3_kernel, dim3((unsigned)N), dim3(256), 0, stream, (const bf16*)w, (int)K, (long long)ldw,
                     (uint8_t*)codes, scale);
  return mpv_check_launch("mpv_quantize_rows_e4m3");
}

extern "C" int mpv_gemm_w8(const void* A, const void* codes, const float* scale, void* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                           int64_t ldw, int64_t ldc, const mpv_gemm_epilogue* ep, hipStream_t stream) {
  MPV_REQUIRE(A && codes && scale && C, MPV_E_ARG, "mpv_gemm_w8: null pointer");
  MPV_REQUIRE(M >= 1 && M <= 512, MPV_E_SHAPE, "mpv_gemm_w8: M (%lld) must be in [1, 512]", (long long)M);
  MPV_REQUIRE(N > 0 && N % 8 == 0 && K > 0 && K % 16 == 0 && N < (1ll << 31) && K < (1ll << 31), MPV_E_SHAPE,
              "mpv_gemm_w8: N (%lld) must be a positive multiple of 8 and K (%lld) of 16", (long long)N, (long long)K);
  MPV_REQUIRE(lda >= K && ldw >= K && ldc >= N, MPV_E_SHAPE, "mpv_gemm_w8: leading dimension shorter than its row (lda=%lld ldw=%lld ldc=%lld)",
              (long long)lda, (long long)ldw, (long long)ldc);
  MPV_REQUIRE(lda % 8 == 0 && ldw % 16 == 0 && (((uintptr_t)A | (uintptr_t)codes) & 15) == 0 && ((uintptr_t)C & 1) == 0 &&
                  ((uintptr_t)scale & 3) == 0,
              MPV_E_ALIGN, "mpv_gemm_w8: lda must be a multiple of 8, ldw of 16, A and codes 16-byte aligned");
  W8Args a = {};
  a.A = (const bf16*)A; a.W = (const uint8_t*)codes; a.scale = scale; a.C = (bf16*)C;
  a.N = (int)N; a.K = (int)K;
  a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.ldr = ldc;
  a.cmap = RowMap{0, 0, 0};
  if (ep) {
    MPV_REQUIRE(!ep->a_group && !ep->a_stride && !ep->a_offset && !ep->k_group && !ep->k_stride && !ep->k_offset && !ep->preact_out &&
                    !ep->act_bwd_z && !ep->ldz && !ep->act_bwd && !(ep->dropout_p != 0.f) && !ep->seed && !ep->offset && !ep->alpha_dev &&
                    !(ep->alpha != 0.f) && !ep->out_f32 && !ep->accumulate && !ep->colsum_out && !ep->tile_hint && !ep->row_tap_out &&
                    !ep->row_tap_group && !ep->split_hint && !ep->gm_hint && !ep->preact_deriv && !ep->keep_output && !(ep->colscale != 0.f) &&
                    !ep->colscale_cols,
                MPV_E_ARG, "mpv_gemm_w8: the epilogue takes bias, act = MPV_ACT_GELU_TANH, residual / ldr and the C row map only");
    MPV_REQUIRE(ep->act == MPV_ACT_NONE || ep->act == MPV_ACT_GELU_TANH, MPV_E_ARG, "mpv_gemm_w8: act (%d) must be none or GELU-tanh", ep->act);
    MPV_REQUIRE(ep->c_group >= 0 && ep->ldr >= 0 && (ep->ldr == 0 || ep->ldr >= N) && (ep->residual || ep->ldr == 0), MPV_E_ARG,
                "mpv_gemm_w8: bad c_group (%d) or ldr (%lld)", ep->c_group, (long long)ep->ldr);
    a.cmap = RowMap{ep->c_group, ep->c_stride, ep->c_offset};
    a.bias = (const bf16*)ep->bias;
    a.residual = (const bf16*)ep->residual;
    if (ep->ldr) a.ldr = ep->ldr;
    a.act = ep->act;
  }
  const bool full = N % 16 == 0 && K % 64 == 0;
  // the K split is a function of (N, K) only (row invariance): 16 waves for a long reduction with few workgroups, as gemm.hip does
  const bool long_k = full && K >= 4096 && N / 16 <= 256;
  // 16 waves of 128 registers hold 8 row blocks of accumulators: a longer call of such a shape goes out in launches of 128 rows (the
  // later ones read the codes again, from L2 / MALL where they still are: 16 MiB for the 1.3B decoder's 4h -> h product)
  const int64_t rows_per_launch = long_k ? 128 : 512;
  for (int64_t m0 = 0; m0 < M; m0 += rows_per_launch) {
    W8Args s = a;
    s.M = (int)(M - m0 < rows_per_launch ? M - m0 : rows_per_launch);
    s.A = a.A + m0 * lda;
    s.m0 = (int)m0;
    if (long_k) launch_w8<true, 16, 8>(s, stream);
    else if (full && (s.M <= 16 ? N / 16 <= 384 : N / 16 < 256)) launch_w8<true, 4, 8>(s, stream);     // few workgroups: 8 columns each
    else if (full) launch_w8<true, 4, 16>(s, stream);
    else launch_w8<false, 4, 16>(s, stream);
  }
  return mpv_check_launch("mpv_gemm_w8");
}

extern "C" int mpv_gpt_embed_w8_fwd(const void* query, const int64_t* ids, const void* wte_codes, const float* wte_scale, const void* wpe,
                                    void* h, int B, int Q, int L, int H, hipStream_t stream) {
  MPV_REQUIRE(ids && wte_codes && wte_scale && wpe && h && (query || Q == 0), MPV_E_ARG, "mpv_gpt_embed_w8_fwd: null pointer");
  MPV_REQUIRE(H % 8 == 0 && B > 0 && Q >= 0 && L >= 0 && Q + L > 0, MPV_E_SHAPE, "mpv_gpt_embed_w8_fwd: bad shape");
  const long long total = (long long)B * (Q + L) * (H / 8);
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(gpt_embed_w8_fwd_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, (const bf16*)query, ids,
                     (const uint8_t*)wte_codes, wte_scale, (const bf16*)wpe, (bf16*)h, B, Q, L, H);
  return mpv_check_launch("mpv_gpt_embed_w8_fwd");
}
