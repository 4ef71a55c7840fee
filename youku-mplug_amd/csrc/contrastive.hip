// Image-text contrastive head of the pre-train model (use_contrastive, models/distributed_gpt3.py:168-212):
//
//   mpv_maxsim_fwd    sim[r][c] = alpha * max_q <A[r][q], T[c]>  (+ the argmax q), bf16 MFMA, fp32 accumulate.
//                     One workgroup = one r and 32 columns c; each of its 4 waves walks every 4th 32-row q chunk of A[r]
//                     with v_mfma_f32_32x32x16_bf16 (operands straight from global memory: A[r] and the 32 rows of T are a
//                     few tens of KiB and stay in L2), keeps (max, argmax) per column in registers and the 4 waves merge
//                     through LDS.  Every merge takes the larger value and, on equal values, the LOWER q: the result does
//                     not depend on the order of the reduction.
//   mpv_maxsim_route  G[r*Q + q][c] = dsim[r][c] * [arg[r][c] == q]: the max's backward as a dense bf16 operand of the
//                     existing GEMMs (dA = alpha G T, dT = alpha G^T A).  Each element is written once, no atomics.
//   mpv_smoothed_ce   F.cross_entropy(sim, target, label_smoothing=eps) per row, its gradient and the temperature term.
#include "mpv_common.h"
#include "../../include/mpv.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int MS_COLS = 32;    // columns c per workgroup
constexpr int MS_WAVES = 4;

// (v, q) beats (bv, bq): larger value, or the same value at a lower q
__device__ __forceinline__ bool ms_better(float v, int q, float bv, int bq) { return v > bv || (v == bv && q < bq); }

__global__ __launch_bounds__(256) void maxsim_fwd_kernel(const bf16* __restrict__ A, const bf16* __restrict__ T,
                                                         const float* __restrict__ alpha_dev, float* __restrict__ sim,
                                                         int* __restrict__ arg, int R, int Q, int C, int E, int trans) {
  __shared__ float s_v[MS_WAVES][MS_COLS];
  __shared__ int s_q[MS_WAVES][MS_COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.y, c0 = blockIdx.x * MS_COLS;
  const int col = c0 + (lane & 31);
  const int kl = 8 * (lane >> 5);                                    // this lane's 8 k of every 16-wide MFMA step
  const bf16* arow = A + (long long)r * Q * E;
  const bf16* trow = T + (long long)(col < C ? col : 0) * E;
  float bv = -INFINITY;
  int bq = 0x7fffffff;
  for (int qc = wave * 32; qc < Q; qc += MS_WAVES * 32) {
    const int qa = qc + (lane & 31);                                 // the A row this lane feeds
    const bf16* ap = arow + (long long)(qa < Q ? qa : 0) * E;
    f32x16 acc = {};
    for (int k = 0; k < E; k += 16) {
      bf16x8 fa = {}, ft = {};
      if (k + kl < E) {                                              // E % 8 == 0: a lane's 8 k are all in or all out
        if (qa < Q) fa = *(const bf16x8*)(ap + k + kl);
        if (col < C) ft = *(const bf16x8*)(trow + k + kl);
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, ft, acc, 0, 0, 0);
    }
    // acc[i] = <A[r][qc + 8(i/4) + 4(lane/32) + i%4], T[col]>: ascending q in i, so a strict > keeps the lowest q
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int q = qc + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
      if (q < Q && ms_better(acc[i], q, bv, bq)) { bv = acc[i]; bq = q; }
    }
  }
  // lanes l and l ^ 32 hold the two halves of the same column's q set
  const float ov = __shfl_xor(bv, 32, 64);
  const int oq = __shfl_xor(bq, 32, 64);
  if (ms_better(ov, oq, bv, bq)) { bv = ov; bq = oq; }
  if (lane < 32) { s_v[wave][lane] = bv; s_q[wave][lane] = bq; }
  __syncthreads();
  if (wave == 0 && lane < 32 && col < C) {
#pragma unroll
    for (int w = 1; w < MS_WAVES; ++w)
      if (ms_better(s_v[w][lane], s_q[w][lane], bv, bq)) { bv = s_v[w][lane]; bq = s_q[w][lane]; }
    const float alpha = alpha_dev ? *alpha_dev : 1.0f;
    const long long o = trans ? (long long)col * R + r : (long long)r * C + col;
    sim[o] = alpha * bv;
    arg[o] = bq;
  }
}

// one thread per 8 consecutive columns of one G row
__global__ __launch_bounds__(256) void maxsim_route_kernel(const bf16* __restrict__ dsim, const int* __restrict__ arg,
                                                           bf16* __restrict__ G, int R, int Q, int C, int trans) {
  const int cc = C / 8;
  const long long total = (long long)R * Q * cc;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long row = i / cc;
    const int c = (int)(i - row * cc) * 8;
    const int r = (int)(row / Q), q = (int)(row - (long long)r * Q);
    bf16x8 out;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const long long o = trans ? (long long)(c + e) * R + r : (long long)r * C + c + e;
      out[e] = arg[o] == q ? dsim[o] : f2bf(0.f);
    }
    *(bf16x8*)(G + row * C + c) = out;
  }
}

// one wave per row (the layout of elementwise.hip's soft_ce_kernel)
__global__ __launch_bounds__(256) void smoothed_ce_kernel(const float* __restrict__ sim, const int64_t* __restrict__ target,
                                                          float eps, float scale, float* __restrict__ losses,
                                                          bf16* __restrict__ dsim, float* __restrict__ dts, int rows, int cols) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* row = sim + (long long)r * cols;
  const long long tgt = target[r];
  float mx = -INFINITY;
  for (int c = lane; c < cols; c += 64) mx = fmaxf(mx, row[c]);
  mx = wave_max(mx);
  float se = 0.f;
  for (int c = lane; c < cols; c += 64) se += __expf(row[c] - mx);
  se = wave_sum(se);
  const float lse = mx + __logf(se), off = eps / (float)cols, on = 1.0f - eps + off;
  float loss = 0.f, dt = 0.f;
  for (int c = lane; c < cols; c += 64) {
    const float t = c == tgt ? on : off;
    const float g = (__expf(row[c] - lse) - t) * scale;
    loss -= (row[c] - lse) * t;
    dt += g * row[c];
    if (dsim) dsim[(long long)r * cols + c] = f2bf(g);
  }
  loss = wave_sum(loss);
  dt = wave_sum(dt);
  if (lane == 0) {
    losses[r] = loss;
    if (dts) dts[r] = dt;
  }
}

}  // namespace

extern "C" int mpv_maxsim_fwd(const void* A, const void* T, const float* alpha_dev, float* sim, int* arg, int64_t R, int64_t Q,
                              int64_t C, int64_t E, int trans, hipStream_t stream) {
  MPV_REQUIRE(A && T && sim && arg, MPV_E_ARG, "mpv_maxsim_fwd: null pointer");
  MPV_REQUIRE(R > 0 && Q > 0 && C > 0 && E > 0 && R <= 65535 && (long long)R * Q * E < (1ll << 31) && (long long)C * E < (1ll << 31),
              MPV_E_SHAPE, "mpv_maxsim_fwd: bad shape R=%lld Q=%lld C=%lld E=%lld", (long long)R, (long long)Q, (long long)C, (long long)E);
  MPV_REQUIRE(E % 8 == 0, MPV_E_ALIGN, "mpv_maxsim_fwd: E (%lld) must be a multiple of 8", (long long)E);
  MPV_REQUIRE((((uintptr_t)A | (uintptr_t)T) & 15) == 0, MPV_E_ALIGN, "mpv_maxsim_fwd: A and T must be 16-byte aligned");
  hipLaunchKernelGGL(maxsim_fwd_kernel, dim3((unsigned)((C + MS_COLS - 1) / MS_COLS), (unsigned)R), dim3(64 * MS_WAVES), 0, stream,
                     (const bf16*)A, (const bf16*)T, alpha_dev, sim, arg, (int)R, (int)Q, (int)C, (int)E, trans ? 1 : 0);
  return mpv_check_launch("mpv_maxsim_fwd");
}

extern "C" int mpv_maxsim_route(const void* dsim, const int* arg, void* G, int64_t R, int64_t Q, int64_t C, int trans,
                                hipStream_t stream) {
  MPV_REQUIRE(dsim && arg && G, MPV_E_ARG, "mpv_maxsim_route: null pointer");
  MPV_REQUIRE(R > 0 && Q > 0 && C > 0 && (long long)R * C < (1ll << 31) && (long long)R * Q < (1ll << 31), MPV_E_SHAPE,
              "mpv_maxsim_route: bad shape");
  MPV_REQUIRE(C % 8 == 0, MPV_E_ALIGN, "mpv_maxsim_route: C (%lld) must be a multiple of 8", (long long)C);
  MPV_REQUIRE(((uintptr_t)G & 15) == 0, MPV_E_ALIGN, "mpv_maxsim_route: G must be 16-byte aligned");
  const long long work = (long long)R * Q * (C / 8);
  long long blocks = (work + 255) / 256;
  blocks = blocks > 16384 ? 16384 : blocks;
  hipLaunchKernelGGL(maxsim_route_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16*)dsim, arg, (bf16*)G, (int)R,
                     (int)Q, (int)C, trans ? 1 : 0);
  return mpv_check_launch("mpv_maxsim_route");
}

extern "C" int mpv_smoothed_ce(const float* sim, const int64_t* target, float eps, float scale, float* losses, void* dsim, float* dts,
                               int64_t rows, int64_t cols, hipStream_t stream) {
  MPV_REQUIRE(sim && target && losses, MPV_E_ARG, "mpv_smoothed_ce: null pointer");
  MPV_REQUIRE(rows > 0 && cols > 0 && rows < (1ll << 31) && cols < (1ll << 31), MPV_E_SHAPE, "mpv_smoothed_ce: empty problem");
  MPV_REQUIRE(eps >= 0.f && eps <= 1.f, MPV_E_ARG, "mpv_smoothed_ce: eps must be in [0, 1]");
  hipLaunchKernelGGL(smoothed_ce_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, sim, target, eps, scale, losses,
                     (bf16*)dsim, dts, (int)rows, (int)cols);
  return mpv_check_launch("mpv_smoothed_ce");
}
