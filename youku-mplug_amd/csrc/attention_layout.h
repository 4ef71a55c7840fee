// attention_layout.h -- the dynamic-LDS layout of every attention kernel family, written once: the kernels place their
// regions with these functions, the host plan (attention.hip: attn_plan / temporal_plan) sizes the launch with the same
// ones, and the variant table derives each instance's LDS opt-in limit from them.  All arithmetic is `int` and constexpr, so
// in a kernel a call folds to exactly the expression it replaces.
#pragma once

namespace attn_layout {

constexpr int ROWB = 208;             // row pitch of the chunked / resident images: 96 bf16 + 16 pad (conflict-free ds_read_b128)
constexpr int ZP = 128;               // paired-block "Z image" row pitch (attention_pair.inc)
constexpr int DUO_KP = 208, DUO_VP = 192;      // duo images (attention_duo.inc): K rows / rotated V, Q, dO rows
constexpr int CU_LDS = 160 * 1024;    // LDS of one CU: no launch may ask for more

__host__ __device__ constexpr int round_1k(int bytes) { return (bytes + 1023) / 1024 * 1024; }      // whole 1 KiB LDS-DMA pieces
__host__ __device__ constexpr int tile_rows(int rows) { return (rows + 31) / 32 * 32; }

// image of whole zero-filled 32-row tiles (resident kernels) / of exactly `rows` rows (persistent, duo), in whole DMA pieces
__host__ __device__ constexpr int tile_region(int rows, int pitch) { return round_1k(tile_rows(rows) * pitch); }
__host__ __device__ constexpr int packed_region(int rows, int pitch) { return round_1k(rows * pitch); }
// Z image: whole 32-row tiles of 128-byte rows (4 KiB per tile: already whole pieces)
__host__ __device__ constexpr int z_region(int rows) { return ((rows + 31) >> 5) * 32 * ZP; }
// fp32 [lse * log2e | delta] rows of the dK/dV roles, in front of their images
__host__ __device__ constexpr int stat_bytes(int padded_rows) { return ((2 * padded_rows * 4 + 1023) / 1024) * 1024; }
__host__ __device__ constexpr int stat_region(int rows) { return stat_bytes(tile_rows(rows)); }

// ---- resident (one-shot) kernels: forward and dQ hold [V | K]; dK/dV holds [stats | V (head_dim > 64) | dO | Q]
__host__ __device__ constexpr int res_fwd_lds(int sk) { return 2 * tile_region(sk, ROWB); }
__host__ __device__ constexpr int res_dq_lds(int sk) { return 2 * tile_region(sk, ROWB); }
__host__ __device__ constexpr int res_dkv_v_region(int sk, int hdc) { return hdc > 64 ? tile_region(sk, ROWB) : 0; }
__host__ __device__ constexpr int res_dkv_lds(int sq, int sk, int hdc) {
  return stat_region(sq) + res_dkv_v_region(sk, hdc) + 2 * tile_region(sq, ROWB);
}

// ---- persistent forward: two operand sets of [V | K]; row-fragment images are conflict-free at 144 / 176 / 208 B, images that
// only serve transposing column reads take 192 B at head_dim 96
__host__ __device__ constexpr int pres_pitch_r(int hdc) { return hdc * 2 + 16; }
__host__ __device__ constexpr int pres_pitch_c(int hdc) { return hdc > 80 ? hdc * 2 : hdc * 2 + 16; }
__host__ __device__ constexpr int pres_set(int sk, int hdc) { return packed_region(sk, pres_pitch_c(hdc)) + packed_region(sk, pres_pitch_r(hdc)); }
__host__ __device__ constexpr int pres_fwd_lds(int sk, int hdc) { return 2 * pres_set(sk, hdc); }

// ---- paired-block causal kernels (head_dim 64): [V | K] / [stats | dO | Q]
__host__ __device__ constexpr int pair_fwd_lds(int s) { return 2 * z_region(s); }
__host__ __device__ constexpr int pair_dq_lds(int s) { return 2 * z_region(s); }
__host__ __device__ constexpr int pair_dkv_lds(int s) { return stat_region(s) + 2 * z_region(s); }

// ---- duo kernels (head_dim 96, 7 tiles): [K | V] / [stats | dO | Q]
__host__ __device__ constexpr int duo_dq_lds(int s) { return packed_region(s, DUO_KP) + packed_region(s, DUO_VP); }
__host__ __device__ constexpr int duo_dkv_lds(int s) { return stat_region(s) + 2 * packed_region(s, DUO_VP); }

// ---- temporal attention: one problem per wave.  fp32 rows at a pitch of hd + 4 floats, bf16 rows at hd + 8 elements; both
// followed by the [T][T+1] fp32 probabilities (and dS in the backward)
__host__ __device__ constexpr int temporal_f32_wave_floats(bool bwd, int T, int hd) {
  return ((bwd ? 4 : 3) * T * (hd + 4) + (bwd ? 2 : 1) * T * (T + 1) + 3) & ~3;
}
__host__ __device__ constexpr int temporal_f32_wave_lds(bool bwd, int T, int hd) { return 4 * temporal_f32_wave_floats(bwd, T, hd); }
__host__ __device__ constexpr int temporal_b16_wave_lds(bool bwd, int T, int hd) {
  return ((bwd ? 4 : 3) * T * (hd + 8) * 2 + (bwd ? 2 : 1) * T * (T + 1) * 4 + 15) & ~15;
}
// Waves (one problem each) per workgroup of the fp32-row kernel: 4 unless fewer waves per workgroup put more waves on a CU (LDS is
// what limits the occupancy of this kernel: a wave's rows are 10 KiB at 8 frames -- 4 x 4 waves either way -- but 20 / 28 KiB at
// 16 frames, where 4-wave workgroups would leave one workgroup = 4 waves per CU and 1- / 2-wave ones fit 7 / 5).
__host__ __device__ constexpr int temporal_f32_waves(int wave_lds) {
  int best = 4, best_waves = CU_LDS / (4 * wave_lds) * 4;
  for (int n = 3; n >= 1; --n) {
    const int waves = CU_LDS / (n * wave_lds) * n;
    if (waves > best_waves) best = n, best_waves = waves;
  }
  return best;
}
constexpr int TEMPORAL_B16_WAVES = 2;      // measured best (or tied) at 8 and at 16 frames in both directions
__host__ __device__ constexpr int temporal_f32_lds(bool bwd, int T, int hd) {
  return temporal_f32_waves(temporal_f32_wave_lds(bwd, T, hd)) * temporal_f32_wave_lds(bwd, T, hd);
}
__host__ __device__ constexpr int temporal_b16_lds(bool bwd, int T, int hd) { return TEMPORAL_B16_WAVES * temporal_b16_wave_lds(bwd, T, hd); }

// ---- temporal attention on the matrix cores (attention_temporal_long.inc; TT = 32 / 64 padded tokens): one problem per wave, one
// per-wave image of 32-row tiles at the ROWB pitch.  Forward: V, TT rows.  Backward: K (TT rows), then a [Q | dO] tile pair --
// 64 rows either way --, followed by the per-query fp32 (lse, delta) pairs.
constexpr int TEMPORAL_MFMA_PITCH = ROWB;
constexpr int TEMPORAL_MFMA_WAVES = 4;
__host__ __device__ constexpr int temporal_mfma_wave_lds(bool bwd, int tt) { return bwd ? 64 * TEMPORAL_MFMA_PITCH + tt * 8 : tt * TEMPORAL_MFMA_PITCH; }
__host__ __device__ constexpr int temporal_mfma_lds(bool bwd, int tt) { return TEMPORAL_MFMA_WAVES * temporal_mfma_wave_lds(bwd, tt); }

}  // namespace attn_layout
