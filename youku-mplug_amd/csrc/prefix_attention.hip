// prefix_attention.hip -- causal attention of many continuations against per-group shared, already computed prefixes (evaluation
// only): one kernel body behind two entries that differ in how a query row is numbered and addressed.
//
// The scoring heads run every (video, candidate) pair as its own decoder sequence; the first P rows of all candidates of one
// video are identical (query features + the common token prefix), so their K/V are computed once per video (the prefix pass)
// and each candidate runs only its own rows.  A query row attends to the P prefix keys of its group and to the keys of its own
// continuation that are not behind it: one softmax over both sets.
//
//   mpv_attn_prefix_fwd          UNIFORM: every continuation has Lc rows and every group (but a short last one) group_size
//                                continuations, each at its own address (x_cs).  The rows of a group are numbered as if stacked end
//                                to end from the group's first continuation: row r = local continuation r / Lc, row r % Lc.
//   mpv_attn_prefix_packed_fwd   PACKED: continuations have their own lengths and groups their own numbers of them; all rows lie end
//                                to end in one [rows] array and are numbered by their place in it.  Two index arrays describe the
//                                packing: seg_start[r], the first row of the continuation row r belongs to (seg_start[r] <= r), and
//                                group_row[g], the first row of group g (group_row[n_groups] == rows).
//
// Those two -- where row r's own keys begin, and how a row number becomes an address -- are the whole difference (the `PACKED`
// branches below); in both numberings a group is one contiguous range of rows and a continuation one contiguous range inside it.
//
// Layout: a workgroup = 4 waves = 128 consecutive rows of one (group, head), so that every prefix K/V chunk brought into LDS serves
// all of them -- with continuations of a few rows (category names) per-continuation tiles would leave the MFMA tiles mostly empty.
// Phase 1 streams the prefix (dense for every row); phase 2 streams the own keys the workgroup can see, from the first key of its
// first row's continuation (a continuation may straddle a workgroup edge: the second workgroup's stream starts inside the first's
// rows) to its last row: key kr is visible to row r iff first_key(r) <= kr <= r.  Both phases are stream_phase(); the prefix is
// the stream whose window covers everything.  The staging, the chunk loop, the kernel body and the entries' tests live in
// prefix_stream.h, which the training kernels of prefix_attention_train.hip share.  Tile arithmetic: prefix_tile.h (S^T = K Q^T on mfma_f32_32x32x16_bf16, online softmax
// in fp32, probabilities rounded to bf16 for the PV product, one division at the end).  A masked key is a true no-op: its score is
// -inf before the running max and its probability exp(-inf) = 0 exactly, so a row's result depends on its group's prefix, on its
// own continuation and on nothing else -- and the two entries, which cut a group into the same tiles, agree bit for bit on a
// uniform problem.
#include "prefix_stream.h"

namespace {

template <int HD, bool PACKED>
__global__ __launch_bounds__(PTHREADS, 2) void attn_prefix_fwd_kernel(const PrefixArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * PCHUNK];     // [buf][K|V]
  prefix_fwd_body<HD, PACKED, false>(p, smem);
}

// The tests and the grid (prefix_stream.h: prefix_fwd_args), then the launch.
template <bool PACKED, class Desc>
int prefix_fwd(const char* name, const char* index_arrays, const Desc* d, hipStream_t stream) {
  PrefixArgs a;
  dim3 grid;
  if (const int rc = prefix_fwd_args(name, index_arrays, d, false, nullptr, a, grid)) return rc;
  if (d->head_dim == 64)
    hipLaunchKernelGGL((attn_prefix_fwd_kernel<64, PACKED>), grid, dim3(PTHREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((attn_prefix_fwd_kernel<80, PACKED>), grid, dim3(PTHREADS), 0, stream, a);
  return mpv_check_launch(name);
}

}  // namespace

extern "C" int mpv_attn_prefix_fwd(const mpv_attn_prefix_desc* d, hipStream_t stream) {
  return prefix_fwd<false>("mpv_attn_prefix_fwd", " aligned", d, stream);
}

extern "C" int mpv_attn_prefix_packed_fwd(const mpv_attn_prefix_packed_desc* d, hipStream_t stream) {
  return prefix_fwd<true>("mpv_attn_prefix_packed_fwd", ", the index arrays 4-byte", d, stream);
}

extern "C" int mpv_attn_prefix_packed_layout(const int32_t* cont_len, int n_cont, const int32_t* conts_per_group, int n_groups,
                                             int32_t* seg_start_out, int32_t* group_row_out, int* rows_out,
                                             int* max_group_rows_out) {
  MPV_REQUIRE(cont_len && conts_per_group && seg_start_out && group_row_out && rows_out && max_group_rows_out, MPV_E_ARG,
              "mpv_attn_prefix_packed_layout: null pointer");
  MPV_REQUIRE(n_cont >= 1 && n_groups >= 1, MPV_E_SHAPE, "mpv_attn_prefix_packed_layout: empty problem (n_cont %d, n_groups %d)",
              n_cont, n_groups);
  long long conts = 0, total = 0;
  for (int g = 0; g < n_groups; ++g) {
    MPV_REQUIRE(conts_per_group[g] >= 1, MPV_E_SHAPE, "mpv_attn_prefix_packed_layout: group %d has no continuation (%d)", g,
                (int)conts_per_group[g]);
    conts += conts_per_group[g];
  }
  MPV_REQUIRE(conts == n_cont, MPV_E_SHAPE, "mpv_attn_prefix_packed_layout: the groups hold %lld continuations, n_cont is %d", conts,
              n_cont);
  for (int c = 0; c < n_cont; ++c) {
    MPV_REQUIRE(cont_len[c] >= 1, MPV_E_SHAPE, "mpv_attn_prefix_packed_layout: continuation %d has length %d (must be >= 1)", c,
                (int)cont_len[c]);
    total += cont_len[c];
    MPV_REQUIRE(total < (1ll << 30), MPV_E_SHAPE, "mpv_attn_prefix_packed_layout: more than 2^30 rows");
  }
  int row = 0, c = 0, max_rows = 0;
  for (int g = 0; g < n_groups; ++g) {
    group_row_out[g] = row;
    for (int i = 0; i < conts_per_group[g]; ++i, ++c) {
      const int first = row;
      for (int j = 0; j < cont_len[c]; ++j) seg_start_out[row++] = first;
    }
    if (row - group_row_out[g] > max_rows) max_rows = row - group_row_out[g];
  }
  group_row_out[n_groups] = row;
  *rows_out = row;
  *max_group_rows_out = max_rows;
  return MPV_OK;
}
