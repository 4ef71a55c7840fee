// Low-rank adapter (LoRA) products of the decoder's fused q/k/v projection (include/mpv.h, "LoRA").
// Three shapes the GEMM family was not built for, all bound by bytes, all on v_mfma_f32_32x32x16_bf16 with fp32 accumulation:
//
//   mpv_lora_down    t[R, r]  = bf16(scale * x[R, C] w(C, r))        8..64 output columns: the long operand x is streamed once.
//                    One workgroup = 32 rows; its 4 waves take every 4th 64-wide chunk of C and are summed through LDS in wave
//                    order, so a row's bits depend on C alone, never on R.
//   mpv_lora_up_add  y[R, N] += scale * t[R, r] w(N, r)^T            a reduction of 8..64 terms onto an existing tensor: one read
//                    and one write of y.  One wave = 32 rows x 64 columns (a lane owns the column PAIR n, n + 1, so y moves as
//                    4-byte words, 128 contiguous bytes per row and half wave).
//   mpv_lora_wgrad   g(C, r)  = bf16(scale * t[R, r]^T x[R, C])      a row reduction onto an [r, C] result.  Rows are cut into
//                    slices (a function of R, C alone); a workgroup reduces one slice of 64 columns, its 4 waves summed through
//                    LDS in wave order, into fp32 partials; a second launch adds the slices in ascending order.  No atomics.
//
// w(c, j) is w[j * ldw + c] when rank-major ([r, in]: lora_A) and w[c * ldw + j] otherwise ([out, r]: lora_B).  r = 8 (and the upper
// half of r = 16 tiles) is padded with zeros in registers; memory is never read or written past r, R, C or N.
// Operand maps (mfma_f32_32x32x16_bf16): lane l feeds A[row l & 31][k = 8 (l >> 5) + e] and B[k][col l & 31], e = 0..7; accumulator
// register i of lane l is D[row 8 (i / 4) + 4 (l >> 5) + i % 4][col l & 31].
#include "mpv_common.h"
#include "../../include/mpv.h"

namespace {

constexpr int LORA_WAVES = 4;

#define LORA_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

// ---------------------------------------------------------------------------------------------------------------- down
template <int NJ>
__global__ __launch_bounds__(64 * LORA_WAVES) void lora_down_kernel(const bf16* __restrict__ x, long long ldx,
                                                                    const bf16* __restrict__ w, long long ldw, int w_rank_major,
                                                                    bf16* __restrict__ t, long long ldt, int R, int C, int r,
                                                                    float scale) {
  __shared__ float red[LORA_WAVES - 1][NJ][16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = lane & 31, h = lane >> 5;
  const int i = blockIdx.x * 32 + p;                                   // the x row this lane feeds (and stores)
  const bf16* xrow = x + (long long)(i < R ? i : 0) * ldx;
  f32x16 acc[NJ];
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) acc[jt] = f32x16{};
  for (int k0 = wave * 64; k0 < C; k0 += 64 * LORA_WAVES) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int c = k0 + 16 * s + 8 * h;                               // C % 8 == 0: a lane's 8 c are all in or all out
      bf16x8 fx = {};
      if (i < R && c < C) fx = *(const bf16x8*)(xrow + c);
#pragma unroll
      for (int jt = 0; jt < NJ; ++jt) {
        const int j = jt * 32 + p;
        bf16x8 fw = {};
        if (j < r && c < C) {
          if (w_rank_major) {
            fw = *(const bf16x8*)(w + (long long)j * ldw + c);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) fw[e] = w[(long long)(c + e) * ldw + j];
          }
        }
        acc[jt] = LORA_MFMA(fw, fx, acc[jt]);                          // D[row j][col i]
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
      for (int q = 0; q < 16; ++q) red[wave - 1][jt][q][lane] = acc[jt][q];
  }
  __syncthreads();
  if (wave != 0 || i >= R) return;
  bf16* trow = t + (long long)i * ldt;
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = jt * 32 + 8 * g + 4 * h;                           // registers 4g .. 4g+3 are columns j .. j+3 of row i
      if (j >= r) continue;                                            // r % 8 == 0: the four are all in or all out
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int q = 4 * g + e;
        const float v = ((acc[jt][q] + red[0][jt][q][lane]) + red[1][jt][q][lane]) + red[2][jt][q][lane];
        o[e] = f2bf(scale * v);
      }
      *(bf16x4*)(trow + j) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- up_add
__global__ __launch_bounds__(64 * LORA_WAVES) void lora_up_add_kernel(const bf16* __restrict__ t, long long ldt,
                                                                      const bf16* __restrict__ w, long long ldw, int w_rank_major,
                                                                      bf16* __restrict__ y, long long ldy, int R, int N, int r,
                                                                      float scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = lane & 31, h = lane >> 5;
  const int i0 = (blockIdx.x * LORA_WAVES + wave) * 32;
  if (i0 >= R) return;
  const int n = blockIdx.y * 64 + 2 * p;                               // this lane's column pair n, n + 1 (N % 8 == 0: both in or both out)
  const int ia = i0 + p;                                               // the t row this lane feeds
  f32x16 acc0 = {}, acc1 = {};
  for (int j0 = 0; j0 < r; j0 += 16) {
    const int jj = j0 + 8 * h;                                         // r % 8 == 0: a lane's 8 j are all in or all out
    bf16x8 ft = {}, f0 = {}, f1 = {};
    if (jj < r) {
      if (ia < R) ft = *(const bf16x8*)(t + (long long)ia * ldt + jj);
      if (n < N) {
        if (w_rank_major) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const bf16x2 v = *(const bf16x2*)(w + (long long)(jj + e) * ldw + n);
            f0[e] = v[0];
            f1[e] = v[1];
          }
        } else {
          f0 = *(const bf16x8*)(w + (long long)n * ldw + jj);
          f1 = *(const bf16x8*)(w + (long long)(n + 1) * ldw + jj);
        }
      }
    }
    acc0 = LORA_MFMA(ft, f0, acc0);                                    // D[row i][col n]
    acc1 = LORA_MFMA(ft, f1, acc1);
  }
  if (n >= N) return;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = i0 + 8 * (q >> 2) + 4 * h + (q & 3);
    if (i >= R) continue;
    bf16x2* py = (bf16x2*)(y + (long long)i * ldy + n);
    bf16x2 v = *py;
    v[0] = f2bf(bf2f(v[0]) + scale * acc0[q]);
    v[1] = f2bf(bf2f(v[1]) + scale * acc1[q]);
    *py = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- wgrad
struct WgradPlan {
  int col_groups, rank_pad, rows_per_slice, slices;
  long long cpad;
};
WgradPlan wgrad_plan(int64_t R, int64_t C, int r) {
  WgradPlan pl;
  pl.col_groups = (int)((C + 63) / 64);
  pl.cpad = (long long)pl.col_groups * 64;
  pl.rank_pad = r <= 32 ? 32 : 64;
  const int64_t target = (1024 + pl.col_groups - 1) / pl.col_groups;   // about four workgroups per CU over the launch
  int64_t rps = ((R + target - 1) / target + 63) / 64 * 64;
  if (rps < 256) rps = 256;
  pl.rows_per_slice = (int)rps;
  pl.slices = (int)((R + rps - 1) / rps);
  return pl;
}

template <int NJ>
__global__ __launch_bounds__(64 * LORA_WAVES) void lora_wgrad_partial_kernel(const bf16* __restrict__ t, long long ldt,
                                                                             const bf16* __restrict__ x, long long ldx,
                                                                             float* __restrict__ ws, int R, int C, int r,
                                                                             int rows_per_slice, long long cpad) {
  __shared__ float red[LORA_WAVES - 1][NJ][2][16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = lane & 31, h = lane >> 5;
  const int c = blockIdx.x * 64 + 2 * p;                               // this lane's column pair c, c + 1 (C % 8 == 0)
  const int r0 = blockIdx.y * rows_per_slice;
  const int r1 = r0 + rows_per_slice < R ? r0 + rows_per_slice : R;
  f32x16 acc[NJ][2];
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) acc[jt][0] = acc[jt][1] = f32x16{};
  for (int i0 = r0 + wave * 16; i0 < r1; i0 += 16 * LORA_WAVES) {
    const int ib = i0 + 8 * h;                                         // this lane's 8 reduction rows
    bf16x8 fx0 = {}, fx1 = {};
    if (c < C) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (ib + e < r1) {
          const bf16x2 v = *(const bf16x2*)(x + (long long)(ib + e) * ldx + c);
          fx0[e] = v[0];
          fx1[e] = v[1];
        }
    }
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
      const int j = jt * 32 + p;
      bf16x8 ft = {};
      if (j < r) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (ib + e < r1) ft[e] = t[(long long)(ib + e) * ldt + j];
      }
      acc[jt][0] = LORA_MFMA(ft, fx0, acc[jt][0]);                     // D[row j][col c]
      acc[jt][1] = LORA_MFMA(ft, fx1, acc[jt][1]);
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int q = 0; q < 16; ++q) red[wave - 1][jt][u][q][lane] = acc[jt][u][q];
  }
  __syncthreads();
  if (wave != 0) return;
  float* out = ws + (long long)blockIdx.y * (NJ * 32) * cpad;          // [rank_pad][cpad] of this slice; c < cpad always
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int j = jt * 32 + 8 * (q >> 2) + 4 * h + (q & 3);
      if (j >= r) continue;
      f32x2 v;
#pragma unroll
      for (int u = 0; u < 2; ++u)
        v[u] = ((acc[jt][u][q] + red[0][jt][u][q][lane]) + red[1][jt][u][q][lane]) + red[2][jt][u][q][lane];
      *(f32x2*)(out + (long long)j * cpad + c) = v;
    }
  }
}

__global__ __launch_bounds__(256) void lora_wgrad_finish_kernel(const float* __restrict__ ws, bf16* __restrict__ g, long long ldg,
                                                                int g_rank_major, int C, int r, int rank_pad, int slices,
                                                                long long cpad, float scale) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= (long long)r * C) return;
  const int j = (int)(idx / C), c = (int)(idx - (long long)j * C);
  float v = 0.f;
  for (int s = 0; s < slices; ++s) v += ws[((long long)s * rank_pad + j) * cpad + c];     // ascending slices: a fixed order
  g[g_rank_major ? (long long)j * ldg + c : (long long)c * ldg + j] = f2bf(scale * v);
}

bool rank_ok(int r) { return r == 8 || r == 16 || r == 32 || r == 64; }
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mpv_lora_down(const void* x, int64_t ldx, const void* w, int64_t ldw, int w_rank_major, void* t, int64_t ldt,
                             int64_t R, int64_t C, int r, float scale, hipStream_t stream) {
  MPV_REQUIRE(x && w && t, MPV_E_ARG, "mpv_lora_down: null pointer");
  MPV_REQUIRE(rank_ok(r), MPV_E_SHAPE, "mpv_lora_down: rank %d is not one of 8, 16, 32, 64", r);
  MPV_REQUIRE(R >= 1 && R < (1ll << 31) - 64 && C >= 8 && C % 8 == 0 && C < (1ll << 31) - 256, MPV_E_SHAPE,
              "mpv_lora_down: bad shape R=%lld C=%lld", (long long)R, (long long)C);
  MPV_REQUIRE(ldx >= C && ldt >= r && ldw >= (w_rank_major ? C : (int64_t)r), MPV_E_SHAPE, "mpv_lora_down: leading dimension too small");
  MPV_REQUIRE(ldx % 8 == 0 && ldt % 8 == 0 && ldw % 8 == 0 && al16(x) && al16(w) && al16(t), MPV_E_ALIGN,
              "mpv_lora_down: pointers must be 16-byte aligned and leading dimensions multiples of 8");
  const dim3 grid((unsigned)((R + 31) / 32));
  if (r <= 32)
    hipLaunchKernelGGL(lora_down_kernel<1>, grid, dim3(64 * LORA_WAVES), 0, stream, (const bf16*)x, (long long)ldx, (const bf16*)w,
                       (long long)ldw, w_rank_major, (bf16*)t, (long long)ldt, (int)R, (int)C, r, scale);
  else
    hipLaunchKernelGGL(lora_down_kernel<2>, grid, dim3(64 * LORA_WAVES), 0, stream, (const bf16*)x, (long long)ldx, (const bf16*)w,
                       (long long)ldw, w_rank_major, (bf16*)t, (long long)ldt, (int)R, (int)C, r, scale);
  return mpv_check_launch("mpv_lora_down");
}

extern "C" int mpv_lora_up_add(const void* t, int64_t ldt, const void* w, int64_t ldw, int w_rank_major, void* y, int64_t ldy,
                               int64_t R, int64_t N, int r, float scale, hipStream_t stream) {
  MPV_REQUIRE(t && w && y, MPV_E_ARG, "mpv_lora_up_add: null pointer");
  MPV_REQUIRE(rank_ok(r), MPV_E_SHAPE, "mpv_lora_up_add: rank %d is not one of 8, 16, 32, 64", r);
  MPV_REQUIRE(R >= 1 && R < (1ll << 31) - 128 && N >= 8 && N % 8 == 0 && N < (1ll << 31) - 64, MPV_E_SHAPE,
              "mpv_lora_up_add: bad shape R=%lld N=%lld", (long long)R, (long long)N);
  MPV_REQUIRE(ldy >= N && ldt >= r && ldw >= (w_rank_major ? N : (int64_t)r), MPV_E_SHAPE, "mpv_lora_up_add: leading dimension too small");
  MPV_REQUIRE(ldy % 8 == 0 && ldt % 8 == 0 && ldw % 8 == 0 && al16(t) && al16(w) && al16(y), MPV_E_ALIGN,
              "mpv_lora_up_add: pointers must be 16-byte aligned and leading dimensions multiples of 8");
  MPV_REQUIRE((N + 63) / 64 <= 65535, MPV_E_SHAPE, "mpv_lora_up_add: too many columns");
  const dim3 grid((unsigned)((R + 32 * LORA_WAVES - 1) / (32 * LORA_WAVES)), (unsigned)((N + 63) / 64));
  hipLaunchKernelGGL(lora_up_add_kernel, grid, dim3(64 * LORA_WAVES), 0, stream, (const bf16*)t, (long long)ldt, (const bf16*)w,
                     (long long)ldw, w_rank_major, (bf16*)y, (long long)ldy, (int)R, (int)N, r, scale);
  return mpv_check_launch("mpv_lora_up_add");
}

extern "C" size_t mpv_lora_wgrad_workspace_size(int64_t R, int64_t C, int r) {
  if (R < 1 || C < 8 || !rank_ok(r)) return 0;
  const WgradPlan pl = wgrad_plan(R, C, r);
  return (size_t)pl.slices * pl.rank_pad * pl.cpad * sizeof(float);
}

extern "C" int mpv_lora_wgrad(const void* t, int64_t ldt, const void* x, int64_t ldx, void* g, int64_t ldg, int g_rank_major,
                              int64_t R, int64_t C, int r, float scale, void* ws, size_t ws_bytes, hipStream_t stream) {
  MPV_REQUIRE(t && x && g && ws, MPV_E_ARG, "mpv_lora_wgrad: null pointer");
  MPV_REQUIRE(rank_ok(r), MPV_E_SHAPE, "mpv_lora_wgrad: rank %d is not one of 8, 16, 32, 64", r);
  MPV_REQUIRE(R >= 1 && R < (1ll << 30) && C >= 8 && C % 8 == 0 && C < (1ll << 31) - 64, MPV_E_SHAPE,
              "mpv_lora_wgrad: bad shape R=%lld C=%lld", (long long)R, (long long)C);
  MPV_REQUIRE(ldx >= C && ldt >= r && ldg >= (g_rank_major ? C : (int64_t)r), MPV_E_SHAPE, "mpv_lora_wgrad: leading dimension too small");
  MPV_REQUIRE(ldx % 8 == 0 && ldt % 8 == 0 && al16(t) && al16(x) && al16(ws), MPV_E_ALIGN,
              "mpv_lora_wgrad: pointers must be 16-byte aligned and leading dimensions multiples of 8");
  const WgradPlan pl = wgrad_plan(R, C, r);
  MPV_REQUIRE(ws_bytes >= (size_t)pl.slices * pl.rank_pad * pl.cpad * sizeof(float), MPV_E_ARG, "mpv_lora_wgrad: workspace too small");
  MPV_REQUIRE(pl.slices <= 65535, MPV_E_SHAPE, "mpv_lora_wgrad: too many row slices");
  const dim3 grid((unsigned)pl.col_groups, (unsigned)pl.slices);
  if (r <= 32)
    hipLaunchKernelGGL(lora_wgrad_partial_kernel<1>, grid, dim3(64 * LORA_WAVES), 0, stream, (const bf16*)t, (long long)ldt,
                       (const bf16*)x, (long long)ldx, (float*)ws, (int)R, (int)C, r, pl.rows_per_slice, pl.cpad);
  else
    hipLaunchKernelGGL(lora_wgrad_partial_kernel<2>, grid, dim3(64 * LORA_WAVES), 0, stream, (const bf16*)t, (long long)ldt,
                       (const bf16*)x, (long long)ldx, (float*)ws, (int)R, (int)C, r, pl.rows_per_slice, pl.cpad);
  const long long total = (long long)r * C;
  hipLaunchKernelGGL(lora_wgrad_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const float*)ws, (bf16*)g,
                     (long long)ldg, g_rank_major, (int)C, r, pl.rank_pad, pl.slices, pl.cpad, scale);
  return mpv_check_launch("mpv_lora_wgrad");
}
