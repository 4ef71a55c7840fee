// Host side of what the fused searches share (retrieval_search.hip, maxsim_search.hip): the descriptor checks, the workspace
// layout and the LDS sizes that every entry point of both files needs.  The two shared kernels, the slice merge and the rank finish,
// sit in retrieval_search.hip beside the stream kernels they serve; sc_merge_slices / sc_rank_finish launch them for both files.
#include "search_common.h"

namespace {

size_t sc_align(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

int sc_check_desc(const char* what, const void* queries, const void* gallery, int dim, long long q_rs, long long g_rs, int slices) {
  MPV_REQUIRE(dim >= 32 && dim <= 1024 && dim % 32 == 0, MPV_E_SHAPE, "%s: dim (%d) must be a multiple of 32 in [32, 1024]", what, dim);
  MPV_REQUIRE(q_rs >= dim && g_rs >= dim && q_rs % 8 == 0 && g_rs % 8 == 0, MPV_E_ALIGN,
              "%s: row strides (%lld, %lld) must be multiples of 8 and at least dim", what, q_rs, g_rs);
  MPV_REQUIRE((((uintptr_t)queries | (uintptr_t)gallery) & 15) == 0, MPV_E_ALIGN, "%s: queries and gallery must be 16-byte aligned", what);
  MPV_REQUIRE(slices >= 0 && slices <= SC_MAX_SLICES, MPV_E_ARG, "%s: slices (%d) must be in [0, %d]", what, slices, SC_MAX_SLICES);
  return MPV_OK;
}

int sc_check_codes(const char* what, const void* gallery, long long g_rs, const float* g_scale) {
  MPV_REQUIRE(g_scale, MPV_E_ARG, "%s: null g_scale", what);
  MPV_REQUIRE(g_rs % 16 == 0 && ((uintptr_t)gallery & 15) == 0, MPV_E_ALIGN,
              "%s: a gallery of codes must be 16-byte aligned with a row stride (%lld) that is a multiple of 16", what, g_rs);
  return MPV_OK;
}

size_t sc_ws_bytes(size_t n) { return 2 * sc_align(n * 4); }

int sc_ws_check(const char* what, const void* ws, size_t ws_bytes, size_t n) {
  MPV_REQUIRE(ws_bytes >= sc_ws_bytes(n), MPV_E_ARG, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, sc_ws_bytes(n));
  MPV_REQUIRE(((uintptr_t)ws & 3) == 0, MPV_E_ALIGN, "%s: workspace must be 4-byte aligned", what);
  return MPV_OK;
}

void* sc_ws_upper(void* ws, size_t n) { return (char*)ws + sc_align(n * 4); }

size_t sc_stream_lds(int D, int waves, size_t tail) {
  return (size_t)(SC_TILE * (D + 8) + waves * SC_TILE * SC_PITCH) * sizeof(bf16) + tail;
}

void sc_allow_lds(const void* kernel, size_t lds) {
  if (lds > 48 * 1024) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}
