// The bank pass of the inverted-softmax (QB-Norm / dual-softmax) correction: lse[g] = log sum_{b < nb} exp(beta * <bank_b, g>) for
// every gallery row g, the one number per row that mpv_sim_*_prior then takes (negated) as the row's term with scale = beta.
//
// It is the stream of retrieval_search.hip with the roles of the two sides swapped.  A workgroup (4 waves) owns 32 GALLERY rows as
// the LDS-resident tile and streams the whole BANK through the register stage, the LDS stage and sc_tile_mma of search_common.h in
// super-tiles of 128 rows, wave w taking rows 32 w .. 32 w + 31 of each.  A lane ends up with 16 scores of ONE gallery row
// (lane & 31) per tile and folds them into its running (max, sum): m' = max(m, tile max), sum = sum * e^(m - m') + sum_i e^(x_i - m'),
// so that no exponent is ever positive and beta = 1000 cannot overflow.  The 8 partials of a row (4 waves x 2 lane halves) meet in
// LDS and are merged by one lane in ascending order.
//
// lse[g] is a function of (bank, beta, gallery row g) alone, bit for bit: the bank is never cut into slices, which lane sees which
// bank row depends on the bank row's index only, an MFMA output element is a function of its A row, its B column and the
// accumulator, and there is no atomic anywhere.  So a row scored alone, at another position, in a gallery of another size or a
// second time gives the same bits, and an index can compute the value for new rows only (RetrievalIndex.add).
// NaN: a NaN product poisons the sum of the lane that meets it and reaches that row's lse.
//
// mpv_sim_bank_lse_q8 loads the resident tile from e4m3 codes (sc_load_resident over ScCodes): the tile holds bf16(deq * scale), so
// the result is bit for bit that of the bf16 entry on those rows.
#include "search_common.h"
#include "../../include/mpv.h"
#include <cmath>

namespace {

constexpr int BK_SUPER = SC_WAVES * SC_TILE;      // bank rows per workgroup and step

struct BkArgs {
  const bf16* B;
  const void* G;
  long long b_rs, g_rs;
  int nb, ng, D;
  float beta;
  float* lse;
  const float* g_scale;      // *_q8: G points to e4m3 codes, g_rs counts codes
};

template <class Res>
__device__ __forceinline__ void bank_lse_body(const BkArgs& a, const Res G) {
  extern __shared__ __attribute__((aligned(16))) char bk_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
  const int D = a.D, rpitch = D + 8;
  bf16* rbuf = (bf16*)bk_smem;
  bf16* sbuf = rbuf + SC_TILE * rpitch + wave * (SC_TILE * SC_PITCH);
  float* pm = (float*)(bk_smem + (size_t)(SC_TILE * rpitch + SC_WAVES * SC_TILE * SC_PITCH) * sizeof(bf16));      // [8][32]
  float* ps = pm + 2 * SC_WAVES * SC_TILE;
  const long long g0 = (long long)blockIdx.x * SC_TILE;
  sc_load_resident(rbuf, G, a.g_rs, D, [&](int j) -> long long { return g0 + j < a.ng ? g0 + j : -1; }, tid, 64 * SC_WAVES);

  const unsigned nb = (unsigned)a.nb;
  const int n_super = (a.nb + BK_SUPER - 1) / BK_SUPER;
  const int nk = (D + SC_KC - 1) / SC_KC;
  const int nsteps = n_super * nk;
  const bf16* rrow = rbuf + l32 * rpitch;
  ScStage st;
  long long row0 = wave * SC_TILE;
  const long long b_end = a.nb;
  auto rows = [&](long long r0) { return [=](int j) -> long long { return r0 + j < b_end ? r0 + j : -1; }; };
  sc_stage_load(st, a.B, a.b_rs, 0, D, rows(row0), lane);
  f32x16 acc = {};
  float m = -INFINITY, sum = 0.f;
  int kc = 0;
  for (int s = 0; s < nsteps; ++s) {
    sc_stage_store(st, sbuf, lane);
    __syncthreads();                                 // stage (and, first time round, the resident rows) visible
    if (s + 1 < nsteps) {
      const bool wrap = kc + 1 == nk;
      sc_stage_load(st, a.B, a.b_rs, wrap ? 0 : (kc + 1) * SC_KC, D, rows(wrap ? row0 + BK_SUPER : row0), lane);
    }
    if (kc == 0) acc = f32x16{};
    const int kleft = D - kc * SC_KC;
    sc_tile_mma(acc, sbuf, rrow + kc * SC_KC, (kleft < SC_KC ? kleft : SC_KC) >> 4, lane);
    if (kc + 1 == nk) {
      // acc[i] is bank row base + 8 (i / 4) + i % 4 against gallery row g0 + l32
      const unsigned base = (unsigned)row0 + 4 * half;
      float tm = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        acc[i] *= a.beta;
        if (base + 8 * (i >> 2) + (i & 3) < nb) tm = fmaxf(tm, acc[i]);      // a NaN never becomes the max
      }
      if (tm > m) {
        sum *= mpv_exp(m - tm);                      // m = -inf: 0 * 0
        m = tm;
      }
      // a row of the bank whose x is NaN (or -inf before any finite one) turns the sum into NaN, for good
#pragma unroll
      for (int i = 0; i < 16; ++i) sum += base + 8 * (i >> 2) + (i & 3) < nb ? mpv_exp(acc[i] - m) : 0.f;
      kc = 0;
      row0 += BK_SUPER;
    } else {
      ++kc;
    }
    __syncthreads();                                 // every wave is done with its stage before the next store
  }
  pm[(2 * wave + half) * SC_TILE + l32] = m;
  ps[(2 * wave + half) * SC_TILE + l32] = sum;
  __syncthreads();
  if (tid < SC_TILE && g0 + tid < a.ng) {
    float mm = -INFINITY;
    for (int p = 0; p < 2 * SC_WAVES; ++p) mm = fmaxf(mm, pm[p * SC_TILE + tid]);
    float ss = 0.f;
    for (int p = 0; p < 2 * SC_WAVES; ++p) ss += ps[p * SC_TILE + tid] * mpv_exp(pm[p * SC_TILE + tid] - mm);      // ascending, always
    a.lse[g0 + tid] = mm + logf(ss);
  }
}

__global__ __launch_bounds__(64 * SC_WAVES) void bank_lse_kernel(BkArgs a) { bank_lse_body(a, (const bf16*)a.G); }
__global__ __launch_bounds__(64 * SC_WAVES) void bank8_lse_kernel(BkArgs a) {
  bank_lse_body(a, ScCodes{(const uint8_t*)a.G, a.g_scale});
}

constexpr size_t BK_WS = 256;                      // nothing is kept between launches; non-zero so that 0 can mean "refused"

int bk_check(const char* what, const mpv_sim_bank_desc* d, bool codes, const float* g_scale) {
  MPV_REQUIRE(d && d->bank && d->gallery, MPV_E_ARG, "%s: null pointer", what);
  MPV_REQUIRE(d->nb > 0 && d->ng > 0 && d->nb <= 0x7fffffffll && d->ng <= 0x7fffffffll, MPV_E_SHAPE, "%s: bad shape nb=%lld ng=%lld", what,
              (long long)d->nb, (long long)d->ng);
  int rc = sc_check_desc(what, d->bank, d->gallery, d->dim, d->b_rs, d->g_rs, 0);
  if (rc == MPV_OK && codes) rc = sc_check_codes(what, d->gallery, d->g_rs, g_scale);
  if (rc != MPV_OK) return rc;
  MPV_REQUIRE(std::isfinite(d->beta), MPV_E_ARG, "%s: beta must be finite", what);
  return MPV_OK;
}

int bk_run(const char* what, const mpv_sim_bank_desc* d, bool codes, const float* g_scale, float* lse, hipStream_t stream) {
  int rc = bk_check(what, d, codes, g_scale);
  if (rc != MPV_OK) return rc;
  MPV_REQUIRE(lse, MPV_E_ARG, "%s: null pointer", what);
  BkArgs a = {};
  a.B = (const bf16*)d->bank;
  a.G = d->gallery;
  a.b_rs = d->b_rs;
  a.g_rs = d->g_rs;
  a.nb = (int)d->nb;
  a.ng = (int)d->ng;
  a.D = d->dim;
  a.beta = d->beta;
  a.lse = lse;
  a.g_scale = g_scale;
  const size_t lds = sc_stream_lds(d->dim, SC_WAVES, (size_t)4 * SC_WAVES * SC_TILE * sizeof(float));
  auto kern = codes ? bank8_lse_kernel : bank_lse_kernel;
  sc_allow_lds((const void*)kern, lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)((d->ng + SC_TILE - 1) / SC_TILE)), dim3(64 * SC_WAVES), lds, stream, a);
  return mpv_check_launch(what);
}

}  // namespace

extern "C" size_t mpv_sim_bank_lse_workspace_size(const mpv_sim_bank_desc* d) {
  return bk_check("mpv_sim_bank_lse_workspace_size", d, false, nullptr) == MPV_OK ? BK_WS : 0;
}
extern "C" int mpv_sim_bank_lse(const mpv_sim_bank_desc* d, float* lse, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  (void)workspace;
  (void)workspace_bytes;
  return bk_run("mpv_sim_bank_lse", d, false, nullptr, lse, stream);
}
extern "C" size_t mpv_sim_bank_lse_q8_workspace_size(const mpv_sim_bank_desc* d, const float* g_scale) {
  return bk_check("mpv_sim_bank_lse_q8_workspace_size", d, true, g_scale) == MPV_OK ? BK_WS : 0;
}
extern "C" int mpv_sim_bank_lse_q8(const mpv_sim_bank_desc* d, const float* g_scale, float* lse, void* workspace,
                                   size_t workspace_bytes, hipStream_t stream) {
  (void)workspace;
  (void)workspace_bytes;
  return bk_run("mpv_sim_bank_lse_q8", d, true, g_scale, lse, stream);
}
