// gemm_w8.hip -- weight-only FP8 (OCP e4m3fn, one power-of-two fp32 scale per output row) for the decode steps of the frozen
// decoder (include/mpv.h, "FP8 decoder weights" states the numeric contract):
//   mpv_quantize_rows_e4m3  row amax -> exponent -> codes, one workgroup per weight row
//   mpv_gemm_w8             C[M,N] = epi(scale[n] * sum_k A[m,k] deq(code[n,k])) for 1 <= M <= 512 rows: the weight-streaming kernel
//                           of gemm.hip (gemm_small_m_kernel) with an 8-bit weight and up to 32 row blocks of 16 rows per workgroup
//   mpv_gemm_w8_tiled       the same product for 97-512 rows: tiles of up to 128 rows x 64 columns, A staged through LDS
//   mpv_gpt_embed_w8_fwd    mpv_gpt_embed_fwd with the token rows taken from the codes (the quantised decoder IS a bf16 model whose
//                           tied embedding holds deq(code) * scale: the rows are looked up in that bf16 table without storing it)
#include "../../include/mpv.h"
#include "mpv_common.h"
#include "fp8_deq.h"

namespace {

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
// The many-row product (mpv_gemm_w8_tiled).  A workgroup of four waves owns a tile of RB 16-row blocks (1..8, chosen on the host) x
// 64 columns and walks all of K in stages of 128: wave w owns the 16 columns n0 + 16 w .. and every row block of the tile, so an
// output element is ONE MFMA accumulator chain over ascending k -- no cross-wave reduce, no K split, and the order is the same for
// every M, RB and tile position.  Per stage the workgroup brings its A tile (rows x 256 bytes) into LDS with coalesced 16-byte loads
// (a row's 16 chunks by 16 consecutive lanes) and every wave reads its fragments from there; a lane's codes (16 per 64-wide
// K-block, the layout of gemm_w8_kernel) stay in registers.  The loads of stage s + PD are issued right after the MFMAs of stage s
// and wait in registers: PD = 4 stages are in flight per workgroup (the product is bound by load latency, not by MFMA or LDS time:
// two stages behind a wait for every load took 1.4-2.4 times as long at 160 rows), and the steady-state loop has no branch around a load, so that the
// compiler's vmcnt waits leave the younger stages in flight.  Registers: at most 248, two workgroups per CU.
// LDS image of a stage: 16-byte chunk c (k = 8 c ..) of tile row m at unit 16 m + (c ^ (m & 15)): the ds_write_b128 of 16
// consecutive chunks of a row and the ds_read_b128 of chunks {2g, 2g + 1} + 8 q by lane (r, g) are both free of bank conflicts.
// Tile rows past M repeat row M - 1 (computed, never stored); chunks past K are zero on both operands.
constexpr int TILED_RB = 8;                                     // the most 16-row blocks a workgroup holds (32 KiB of LDS per stage)
constexpr int TILED_RB2 = 4;                                    // ... with two column groups
template <int RB, int CG>
struct TiledStage {
  i32x4 a[RB];                                                  // this thread's chunk of tile rows i * 16 + (tid >> 4)
  i32x4 c[CG][2];                                               // this lane's codes of the stage's two 64-wide K-blocks, per column group
  bool aok, cok[2];                                             // whether they lie inside K
};

// CG = 2: a workgroup owns two groups of 64 columns (wave w: columns 16 w .. of each), which halves the A bytes per output.  Built for
// RB <= 4 only: taller tiles of 128 columns need more than 256 registers, and with one workgroup per CU they were SLOWER than 64
// columns (measured at 512 rows: qkv 35.6 against 32.3 us, the LM head 259 against 227).
template <int RB, int CG>
__global__ __launch_bounds__(256, 2) void gemm_w8_tiled_kernel(const W8Args p) {
  static_assert(CG == 1 || RB <= TILED_RB2, "two column groups: at most TILED_RB2 row blocks");
  constexpr int PD = 4;                                         // stages in flight (even: the LDS buffer of a stage is static)
  __shared__ i32x4 lds[2][RB * 16 * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int row0 = blockIdx.y * RB * 16;                        // first row of the tile
  const int n0 = blockIdx.x * (64 * CG) + wave * 16 + r;        // this lane's column of group cg: n0 + 64 cg
  const uint8_t* wrow[CG];
#pragma unroll
  for (int cg = 0; cg < CG; ++cg) wrow[cg] = p.W + (long long)min(n0 + 64 * cg, p.N - 1) * p.ldw + g * 16;
  // staging role: chunk ac of tile rows am, am + 16, ...
  const int ac = tid & 15, am = tid >> 4;
  const bf16* arow[RB];
#pragma unroll
  for (int i = 0; i < RB; ++i) arow[i] = p.A + (long long)min(row0 + i * 16 + am, p.M - 1) * p.lda + ac * 8;
  const int wunit = am * 16 + (ac ^ am);
  const int nst = (p.K + 127) >> 7;
  f32x4 acc[RB][CG];
#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int cg = 0; cg < CG; ++cg) acc[b][cg] = f32x4{0.f, 0.f, 0.f, 0.f};
  TiledStage<RB, CG> st[PD];
  const i32x4 zero = {0, 0, 0, 0};
  // no branch around a load, and nothing reads a loaded register before the stage's turn (either would make the wait for one stage
  // a wait for all): a chunk past K is read at k = 0 and zeroed when the stage is used
  auto load = [&](int s, TiledStage<RB, CG>& t) {
    const int k0 = s * 128;
    t.aok = k0 + ac * 8 < p.K;                                  // K % 16 == 0: a chunk is all-in or all-out
#pragma unroll
    for (int i = 0; i < RB; ++i) t.a[i] = *(const i32x4*)(arow[i] + (t.aok ? k0 : 0));
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      t.cok[q] = k0 + q * 64 + g * 16 < p.K;
#pragma unroll
      for (int cg = 0; cg < CG; ++cg) t.c[cg][q] = *(const i32x4*)(wrow[cg] + (t.cok[q] ? k0 + q * 64 : 0));
    }
  };
  auto step = [&](i32x4* buf, const TiledStage<RB, CG>& t) {
    __builtin_amdgcn_sched_barrier(0);                          // (a later stage's conversions hoisted to here would wait for its loads)
#pragma unroll
    for (int i = 0; i < RB; ++i) buf[i * 256 + wunit] = t.aok ? t.a[i] : zero;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      Frag w0[CG], w1[CG];
#pragma unroll
      for (int cg = 0; cg < CG; ++cg) deq_chunk(t.cok[q] ? t.c[cg][q] : zero, w0[cg], w1[cg]);
#pragma unroll
      for (int b = 0; b < RB; ++b) {
        Frag a0, a1;
        const i32x4* row = buf + (b * 16 + r) * 16;
        a0.i = row[(8 * q + 2 * g) ^ r];
        a1.i = row[(8 * q + 2 * g + 1) ^ r];
#pragma unroll
        for (int cg = 0; cg < CG; ++cg) {
          acc[b][cg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0.b, w0[cg].b, acc[b][cg], 0, 0, 0);
          acc[b][cg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1.b, w1[cg].b, acc[b][cg], 0, 0, 0);
        }
      }
    }
  };
  // One barrier per stage is enough with two LDS buffers: stage s writes the buffer stage s - 2 read, and every wave passed the
  // barrier of stage s - 1 after those reads.
#pragma unroll
  for (int j = 0; j < PD; ++j) load(min(j, nst - 1), st[j]);    // (a stage past the end repeats the last one: loaded, never used)
  int s = 0;
  for (; s + 2 * PD <= nst; s += PD) {                          // steady state: stage s + j + PD exists for every j
#pragma unroll
    for (int j = 0; j < PD; ++j) {
      step(lds[j & 1], st[j]);
      load(s + j + PD, st[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 2 * PD - 1; ++j) {                        // the last nst - s < 2 PD stages
    if (s + j < nst) {
      step(lds[j & 1], st[j % PD]);
      if (s + j + PD < nst) load(s + j + PD, st[j % PD]);
    }
  }
  // D layout: lane -> column n = lane & 15, rows 4 * (lane >> 4) + i of the block
#pragma unroll
  for (int cg = 0; cg < CG; ++cg) {
    const int n = n0 + 64 * cg;
    if (n < p.N) {
      const float sc = p.scale[n];
      const float bias = p.bias ? bf2f(p.bias[n]) : 0.f;
#pragma unroll
      for (int b = 0; b < RB; ++b) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = row0 + b * 16 + 4 * g + i;
          if (m < p.M) {
            float v = acc[b][cg][i] * sc + bias;
            if (p.act) v = gelu_tanh_f(bf2f(f2bf(v)));
            const long long crow = map_row(p.cmap, p.m0 + m);
            if (p.residual) v += bf2f(p.residual[crow * p.ldr + n]);
            p.C[crow * p.ldc + n] = f2bf(v);
          }
        }
      }
    }
  }
}

template <int RB, int CG>
void launch_w8_tiled(const W8Args& a, int rb, hipStream_t stream) {
  if constexpr (RB > 1) {
    if (rb < RB) return launch_w8_tiled<RB - 1, CG>(a, rb, stream);
  }
  const dim3 grid((unsigned)((a.N + 64 * CG - 1) / (64 * CG)), (unsigned)(((a.M + 15) / 16 + RB - 1) / RB));
  hipLaunchKernelGGL((gemm_w8_tiled_kernel<RB, CG>), grid, dim3(256), 0, stream, a);
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

// eight columns of the tied embedding's row `id` as deq(code) * scale: the one conversion of both embedding kernels below
__device__ __forceinline__ f32x8 deq_row8(const uint8_t* __restrict__ codes, const float* __restrict__ scale, int64_t id, int H, int c8) {
  const i32x2 c = *(const i32x2*)(codes + id * (long long)H + c8 * 8);
  const float sc = scale[id];
  const f32x2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8(c[0], false), f1 = __builtin_amdgcn_cvt_pk_f32_fp8(c[0], true);
  const f32x2 f2 = __builtin_amdgcn_cvt_pk_f32_fp8(c[1], false), f3 = __builtin_amdgcn_cvt_pk_f32_fp8(c[1], true);
  return f32x8{f0[0], f0[1], f1[0], f1[1], f2[0], f2[1], f3[0], f3[1]} * sc;        // exact: a bf16 value
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
      v = deq_row8(codes, scale, id, H, c8);
    }
    v += cvt8(*(const bf16x8*)(wpe + (long long)s * H + c8 * 8));
    *(bf16x8*)(h + row * H + c8 * 8) = cvt8(v);
  }
}

// gpt_embed_rows_fwd_kernel (elementwise.hip: per-row positions, no query rows), the token rows being deq(code) * scale
__global__ void gpt_embed_rows_w8_fwd_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ pos, const uint8_t* __restrict__ codes,
                                             const float* __restrict__ scale, const bf16* __restrict__ wpe, bf16* __restrict__ out, int rows,
                                             int H, int max_positions) {
  const int H8 = H / 8;
  const long long total = (long long)rows * H8;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int c8 = (int)(idx % H8);
    const long long row = idx / H8;
    f32x8 v = deq_row8(codes, scale, ids[row], H, c8);
    v += cvt8(*(const bf16x8*)(wpe + (long long)min(max(pos[row], 0), max_positions - 1) * H + c8 * 8));   // never outside wpe
    *(bf16x8*)(out + row * H + c8 * 8) = cvt8(v);
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

// the host-side checks of both product entries and the kernel arguments they share (a.M, a.m0 and the row range are the caller's)
static int w8_args(const char* who, const void* A, const void* codes, const float* scale, void* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                   int64_t ldw, int64_t ldc, const mpv_gemm_epilogue* ep, W8Args& a) {
  MPV_REQUIRE(A && codes && scale && C, MPV_E_ARG, "%s: null pointer", who);
  MPV_REQUIRE(M >= 1 && M <= 512, MPV_E_SHAPE, "%s: M (%lld) must be in [1, 512]", who, (long long)M);
  MPV_REQUIRE(N > 0 && N % 8 == 0 && K > 0 && K % 16 == 0 && N < (1ll << 31) && K < (1ll << 31), MPV_E_SHAPE,
              "%s: N (%lld) must be a positive multiple of 8 and K (%lld) of 16", who, (long long)N, (long long)K);
  MPV_REQUIRE(lda >= K && ldw >= K && ldc >= N, MPV_E_SHAPE, "%s: leading dimension shorter than its row (lda=%lld ldw=%lld ldc=%lld)", who,
              (long long)lda, (long long)ldw, (long long)ldc);
  MPV_REQUIRE(lda % 8 == 0 && ldw % 16 == 0 && (((uintptr_t)A | (uintptr_t)codes) & 15) == 0 && ((uintptr_t)C & 1) == 0 &&
                  ((uintptr_t)scale & 3) == 0,
              MPV_E_ALIGN, "%s: lda must be a multiple of 8, ldw of 16, A and codes 16-byte aligned", who);
  a = W8Args{};
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
                MPV_E_ARG, "%s: the epilogue takes bias, act = MPV_ACT_GELU_TANH, residual / ldr and the C row map only", who);
    MPV_REQUIRE(ep->act == MPV_ACT_NONE || ep->act == MPV_ACT_GELU_TANH, MPV_E_ARG, "%s: act (%d) must be none or GELU-tanh", who, ep->act);
    MPV_REQUIRE(ep->c_group >= 0 && ep->ldr >= 0 && (ep->ldr == 0 || ep->ldr >= N) && (ep->residual || ep->ldr == 0), MPV_E_ARG,
                "%s: bad c_group (%d) or ldr (%lld)", who, ep->c_group, (long long)ep->ldr);
    a.cmap = RowMap{ep->c_group, ep->c_stride, ep->c_offset};
    a.bias = (const bf16*)ep->bias;
    a.residual = (const bf16*)ep->residual;
    if (ep->ldr) a.ldr = ep->ldr;
    a.act = ep->act;
  }
  return MPV_OK;
}

extern "C" int mpv_gemm_w8(const void* A, const void* codes, const float* scale, void* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                           int64_t ldw, int64_t ldc, const mpv_gemm_epilogue* ep, hipStream_t stream) {
  W8Args a;
  const int rc = w8_args("mpv_gemm_w8", A, codes, scale, C, M, N, K, lda, ldw, ldc, ep, a);
  if (rc) return rc;
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

// The tile of the tiled product: a workgroup reads rb * 16 rows of A (2 bytes an element) and cg * 64 rows of codes over all of K, and
// the 256 CUs take the workgroups in rounds -- the (rb, cg) with the least bytes on the busiest CU; on a tie the larger rb, then one
// column group.  It shapes the launch only: the summation order of an element does not depend on it.
static void tiled_tile(int64_t M, int64_t N, int& rb_out, int& cg_out) {
  const int64_t nrb = (M + 15) / 16;
  int64_t best_cost = 0;
  rb_out = 0;
  for (int cg = 2; cg >= 1; --cg) {
    const int64_t ct = (N + 64 * cg - 1) / (64 * cg);
    for (int rb = 1; rb <= (cg == 2 ? TILED_RB2 : TILED_RB); ++rb) {
      const int64_t wgs = ct * ((nrb + rb - 1) / rb);
      const int64_t cost = ((wgs + 255) / 256) * (rb * 32 + cg * 64);
      if (!rb_out || cost <= best_cost) rb_out = rb, cg_out = cg, best_cost = cost;
    }
  }
}

extern "C" int mpv_gemm_w8_tiled(const void* A, const void* codes, const float* scale, void* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                                 int64_t ldw, int64_t ldc, const mpv_gemm_epilogue* ep, void* workspace, size_t workspace_bytes,
                                 hipStream_t stream) {
  W8Args a;
  const int rc = w8_args("mpv_gemm_w8_tiled", A, codes, scale, C, M, N, K, lda, ldw, ldc, ep, a);
  if (rc) return rc;
  // no variant of this kernel splits K over workgroups: the workspace is not used, so the result cannot depend on it
  (void)workspace;
  (void)workspace_bytes;
  a.M = (int)M;
  int rb, cg;
  tiled_tile(M, N, rb, cg);
  if (cg == 2) launch_w8_tiled<TILED_RB2, 2>(a, rb, stream);
  else launch_w8_tiled<TILED_RB, 1>(a, rb, stream);
  return mpv_check_launch("mpv_gemm_w8_tiled");
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

extern "C" int mpv_gpt_embed_rows_w8_fwd(const int64_t* ids, const int32_t* pos, const void* wte_codes, const float* wte_scale, const void* wpe,
                                         void* out, int rows, int H, int max_positions, hipStream_t stream) {
  MPV_REQUIRE(ids && pos && wte_codes && wte_scale && wpe && out, MPV_E_ARG, "mpv_gpt_embed_rows_w8_fwd: null pointer");
  MPV_REQUIRE(rows > 0 && H > 0 && H % 8 == 0 && max_positions > 0, MPV_E_SHAPE,
              "mpv_gpt_embed_rows_w8_fwd: bad shape (rows %d, H %d, max_positions %d)", rows, H, max_positions);
  const long long total = (long long)rows * (H / 8);
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(gpt_embed_rows_w8_fwd_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, ids, pos,
                     (const uint8_t*)wte_codes, wte_scale, (const bf16*)wpe, (bf16*)out, rows, H, max_positions);
  return mpv_check_launch("mpv_gpt_embed_rows_w8_fwd");
}
