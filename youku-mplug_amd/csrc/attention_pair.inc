// attention_pair.inc -- paired-block causal attention for the GPT decoder (head_dim 64), included by attention.hip inside
// its anonymous namespace (shares AttnArgs, the fragment helpers and the dropout hash).
//
// Replaces, for head_dim 64 / causal / sq == sk <= 224, the one-shot resident forward and dQ kernels on the reference call sites
// models/modeling_distributed_gpt3.py:734-817 (GPT3SelfAttention.forward: QK^T, masked softmax, dropout, PV) and its autograd
// backward (at S <= 160 the dK/dV role stays with attn_bwd_dkv_res_kernel, see the end of this comment).
//
// Why another structure.  A causal problem of NB 32-row blocks gives block i (i + 1) key tiles of work: with one wave per
// block the workgroup lives as long as its LAST block while the first waves idle -- 15 of 25 wave-tile slots used at
// S = 160 -- and those idle waves still hold registers, so only two (batch, head) items fit a CU and the launch runs as two
// rounds of latency-bound workgroups (measured: MFMA pipe ~5 % busy, 2.1x the HBM floor).  Here a wave owns TWO blocks,
// the long one and its complement (NB - 1 - w, then w - 1 or w): every wave does NB + 1 (or NB) tiles, the item needs
// ceil(NB / 2) waves instead of NB, and with the operand images packed to 128-byte rows (below) an item is 3 waves and
// 40 KiB of LDS: FOUR items per CU, the whole decoder launch (1024 items at config B) resident at once, so that the
// loads of late items stream while early items compute.  Measured at the config-B shape (32 x 32 heads x 160 x 64, dropout
// 0.1; tools/attn_pair_ab.py, profiles/r03_c7_attn_pair_ab.log): forward 27.5 -> 21.9 us, backward (dQ + dK/dV) 83.8 -> 75.8 us;
// at S = 208: forward 47.4 -> 34.2 us, backward 150.0 -> 119.6 us.
//
// "Z image": [rows][128 B] = 64 bf16 per row, no padding; the 16-byte chunk c of row r is stored at chunk position
// c ^ zkey(r), zkey(r) = bit-reverse3((r >> 1) & 7).  The LDS-DMA writes lane-linearly, so the permutation is applied to
// the per-lane GLOBAL source address.  ds_read_b128 row fragments: the 16 rows of a hardware lane group ({0-3,12-15,20-27},
// ...) of one chunk column land in 16 distinct 16-byte bank groups; ds_read_b64_tr_b16 column fragments: the 4 rows x 64 B of
// a 32-lane pass land in 16 distinct groups (the bit reversal is what separates rows r and r + 2) --
// tools/probe/sim_zimage_layout.py, run by tests/test_tools_cpu.py.
//
// The dK/dV role as its own launch is at the end of this file (statistics in LDS: three items per CU at S = 160 -- a tie with the
// one-shot kernel there, a clear win at S = 208).  It was first written fused behind the dQ role in one launch (Q, dO re-staged over the K / V
// images, per-row statistics spread with ds_bpermute because LDS has no room for them; in the history: commit 53153c9).
// It does not fit: K and V fragments (32) + two accumulator sets (64) + the S and dP tiles (32) leave 40 of the 168 registers
// of a 3-waves-per-SIMD kernel for everything else, the allocator spilled 400-650 bytes inside the tile loop, and the launch
// ran 152-210 us against 84 for the two one-shot kernels.  (An agent-scope __threadfence() between the phases costs a write-back
// of the XCD's whole L2 per workgroup on this part: `buffer_wbl2 sc1`.)  The loop is VALU-bound either way: ~550 VALU
// instructions per tile, half of them the dropout hash, which in this orientation cannot be shared by the two keys of a pair.

// (ZP, the Z-image row pitch, and z_region / pair_*_lds: attention_layout.h)
__device__ __host__ __forceinline__ int zkey(int r) {
  const int x = (r >> 1) & 7;
  return ((x & 1) << 2) | (x & 2) | (x >> 2);
}
// An image holds whole 32-row tiles, the rows past the sequence end zero-filled by the DMA (out-of-range source): a tile read
// never leaves defined data (the slack between a workgroup's LDS request and its allocation granule holds stale bytes of
// earlier workgroups -- a NaN there times an exactly-zero probability would still be a NaN in the accumulator).
__device__ __forceinline__ void z_dma_rows(const __amdgpu_buffer_rsrc_t src, char* lds, int nrows, long long rs, int wave, int nwaves, int lane) {
  const int ninstr = ((nrows + 31) >> 5) * 4;      // 1 KiB = 8 rows per instruction, 4 instructions per tile
  for (int i = wave; i < ninstr; i += nwaves) {
    const int g = i * 64 + lane;
    const int row = g >> 3, c = (g & 7) ^ zkey(row);
    const uint32_t off = row < nrows ? (uint32_t)(((long long)row * rs + c * 8) * 2) : 0x80000000u;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(src, (lds_void_t*)(lds + i * 1024), 16, off, 0, 0, 0);
  }
}
// per-lane base of row fragments: row (lane & 31) of a tile, chunk 2s + (lane >> 5); `off` = image + tile * 32 * ZP + base
__device__ __forceinline__ int z_rows_base(int lane) {
  const int r = lane & 31, k = zkey(r);
  return r * ZP + (((lane >> 5) ^ (k & 1)) << 4) + ((k >> 1) << 5);
}
__device__ __forceinline__ bf16x8 z_rows(const lds_char* sm, int off, int s) { return *(const lds_bf16x8*)(sm + (off ^ (s << 5))); }
// per-lane base of transposed (column) fragments: rows 4h + m (+ 8), columns dt * 32 + j * 16 + i * 4 .. + 3
__device__ __forceinline__ int z_cols_base(int lane) {
  const int r = 4 * (lane >> 5) + ((lane & 15) >> 2), i = lane & 3;
  return r * ZP + (((((lane >> 4) & 1) * 2 + (i >> 1)) ^ zkey(r)) << 4) + ((i & 1) << 3);
}
__device__ __forceinline__ bf16x8 z_cols(const lds_char* sm, int off, int ks, int dt) {
  const int a = (off + ks * 16 * ZP) ^ (dt << 6);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(sm + a));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(sm + ((a ^ 16) + 8 * ZP)));      // zkey(r + 8) = zkey(r) ^ 1 for r < 8
  union { struct { s16x4 a, b; } s; bf16x8 v; } u;
  u.s.a = lo;
  u.s.b = hi;
  return u.v;
}
// the two blocks of wave w in an NB-block causal problem: `first` is the long one of the role, `second` (< 0: none) its complement
__device__ __forceinline__ void pair_blocks_q(int NB, int w, int& first, int& second) {      // work of block i: i + 1 tiles
  first = NB - 1 - w;
  second = (NB & 1) ? w - 1 : w;
}

// ------------------------------------------------------------------------------------------------------------- forward
template <int NTMAX, int THREADS, int WPE>
__global__ __launch_bounds__(THREADS, WPE) void attn_fwd_pair64_kernel(const AttnArgs p) {
  const MpvSeedKeys seed_k = mpv_seed_keys(p.drop_thr ? mpv_resolve_seed(p.seed) : 0);      // (bit 63 set: the seed lives in device memory, mpv_common.h)
  constexpr int HD = 64, NS = 4, NDT = 2;
  extern __shared__ __attribute__((aligned(1024))) char rsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = blockDim.x >> 6;
  int b, h;
  if (!decode_bh(p, b, h)) return;
  const int bh = b * p.heads + h;
  const int S = p.sk, NB = (S + 31) >> 5;
  const int reg = z_region(S);
  char* vl = rsm;                 // V (column fragments)
  char* kl = rsm + reg;           // K (row fragments)
  const bf16* qb = p.q + b * p.q_bs + h * p.q_hs;
  const __amdgpu_buffer_rsrc_t ksrc = make_rsrc(p.k + b * p.k_bs + h * p.k_hs, (uint32_t)(((long long)(S - 1) * p.k_rs + HD) * 2));
  const __amdgpu_buffer_rsrc_t vsrc = make_rsrc(p.v + b * p.v_bs + h * p.v_hs, (uint32_t)(((long long)(S - 1) * p.v_rs + HD) * 2));
  z_dma_rows(ksrc, kl, S, p.k_rs, wave, nwaves, lane);
  z_dma_rows(vsrc, vl, S, p.v_rs, wave, nwaves, lane);
  int blk0, blk1;
  pair_blocks_q(NB, wave, blk0, blk1);
  float sc = p.scale;
  if (p.scale_q_bf16) sc = 1.0f;
  const float c2 = sc * 1.4426950408889634f;
  const lds_char* sm = (const lds_char*)rsm;
  const int kbase = reg + z_rows_base(lane), vbase = z_cols_base(lane);
  bf16x8 qf[NS];
  auto load_q = [&](int blk) {
    load_row_frags<HD>(qf, qb, p.q_rs, blk * 32 + (lane & 31), p.sq, lane, HD);
    if (p.scale_q_bf16 == 1) scale_frags_bf16(qf, p.scale);
  };
  auto run = [&](int blk) {
    const int q0 = blk * 32, qrow = q0 + (lane & 31);
    const int my_last = min(S - 1, qrow);
    const int nt = blk + 1;
    f32x16 st[NTMAX];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NTMAX; ++kt) {
      if (kt < nt) {
        f32x16 s, s_odd;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = s_odd[e] = 0.f;
#pragma unroll
        for (int sx = 0; sx < NS; ++sx) {
          if (sx & 1) s_odd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z_rows(sm, kbase + kt * 32 * ZP, sx), qf[sx], s_odd, 0, 0, 0);
          else s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z_rows(sm, kbase + kt * 32 * ZP, sx), qf[sx], s, 0, 0, 0);
        }
        s += s_odd;
        if (kt == blk) {      // the diagonal tile (also the only one that can hold keys >= S)
#pragma unroll
          for (int e = 0; e < 16; ++e) s[e] = kt * 32 + acc_row(e, lane) <= my_last ? s[e] : -INFINITY;
        }
#pragma unroll
        for (int e = 0; e < 16; e += 2) mx = fmaxf(fmaxf(mx, s[e]), s[e + 1]);
        st[kt] = s;
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m = mx > -INFINITY ? mx * c2 : 0.f;
    float l = 0.f;
    f32x16 oacc[NDT];
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;
    const uint64_t rb = p.offset + ((uint64_t)bh * p.sq + (uint64_t)qrow) * (uint64_t)p.sk;
#pragma unroll
    for (int kt = 0; kt < NTMAX; ++kt) {
      if (kt < nt) {
        f32x16 pr;
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const f32x2 t = __builtin_elementwise_fma(f32x2{st[kt][e], st[kt][e + 1]}, f32x2{c2, c2}, f32x2{-m, -m});
          pr[e] = fexp2(t[0]);
          pr[e + 1] = fexp2(t[1]);
        }
        {
          f32x2 a2 = {0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 16; e += 2) a2 += f32x2{pr[e], pr[e + 1]};
          l += a2[0] + a2[1];
        }
        if (p.drop_thr) {
#pragma unroll
          for (int e = 0; e < 16; e += 2) {      // registers e, e+1 hold keys k, k+1 with k even: one hash per pair
            const uint32_t r = mpv_rand_pair_k(seed_k, rb + (uint64_t)(kt * 32 + acc_row(e, lane)));
            pr[e] = (r & 0xffffu) >= p.drop_thr ? pr[e] * p.drop_scale : 0.f;
            pr[e + 1] = (r >> 16) >= p.drop_thr ? pr[e + 1] * p.drop_scale : 0.f;
          }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 pf = acc_to_frag(pr, ks);
#pragma unroll
          for (int d = 0; d < NDT; ++d)
            oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z_cols(sm, vbase + kt * 32 * ZP, ks, d), pf, oacc[d], 0, 0, 0);
        }
      }
    }
    l += __shfl_xor(l, 32, 64);
    const float inv_l = l > 0.f ? 1.0f / l : 0.f;
    if (qrow < p.sq && lane < 32 && p.lse) p.lse[(long long)bh * p.sq + qrow] = (m + log2f(l)) * 0.6931471805599453f;
    if (qrow < p.sq) {
      bf16* orow = p.o + b * p.o_bs + h * p.o_hs + (long long)qrow * p.o_rs;
#pragma unroll
      for (int d = 0; d < NDT; ++d)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int col = d * 32 + 8 * q4 + 4 * (lane >> 5);
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = oacc[d][4 * q4 + e] * inv_l;
          *(bf16x4*)(orow + col) = cvt4(v);
        }
    }
  };
  load_q(blk0);      // (two inlined copies of the block code: as a loop over the two passes the score tiles went to scratch)
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
  run(blk0);
  if (blk1 >= 0) {
    load_q(blk1);
    run(blk1);
  }
}

// ------------------------------------------------------------------------------------------------------------ backward
// dQ role (also writes delta = rowsum(dO * O) for the dK/dV kernel launched after it): K, V resident; the wave's own Q / dO rows in
// registers; S^T = K Q^T so that the C layout of dS^T is the B operand of dQ^T += K^T dS^T.
template <int THREADS, int WPE>
__global__ __launch_bounds__(THREADS, WPE) void attn_bwd_dq_pair64_kernel(const AttnArgs p) {
  const MpvSeedKeys seed_k = mpv_seed_keys(p.drop_thr ? mpv_resolve_seed(p.seed) : 0);      // (bit 63 set: the seed lives in device memory, mpv_common.h)
  constexpr int HD = 64, NS = 4, NDT = 2;
  extern __shared__ __attribute__((aligned(1024))) char rsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = blockDim.x >> 6;
  int b, h;
  if (!decode_bh(p, b, h)) return;
  const int bh = b * p.heads + h;
  const int S = p.sk, NB = (S + 31) >> 5;
  const int reg = z_region(S);
  char* im0 = rsm;                // V
  char* im1 = rsm + reg;          // K
  const lds_char* sm = (const lds_char*)rsm;
  const float sc = p.scale_q_bf16 ? 1.0f : p.scale;
  const float c2 = sc * 1.4426950408889634f;
  const int rbase = z_rows_base(lane), cbase = z_cols_base(lane);
  int blk0, blk1;
  pair_blocks_q(NB, wave, blk0, blk1);
  const uint64_t rb0 = p.offset + (uint64_t)bh * (uint64_t)p.sq * (uint64_t)p.sk;      // dropout counter of element (q, k): rb0 + q * sk + k

  {
    const __amdgpu_buffer_rsrc_t ksrc = make_rsrc(p.k + b * p.k_bs + h * p.k_hs, (uint32_t)(((long long)(S - 1) * p.k_rs + HD) * 2));
    const __amdgpu_buffer_rsrc_t vsrc = make_rsrc(p.v + b * p.v_bs + h * p.v_hs, (uint32_t)(((long long)(S - 1) * p.v_rs + HD) * 2));
    z_dma_rows(ksrc, im1, S, p.k_rs, wave, nwaves, lane);
    z_dma_rows(vsrc, im0, S, p.v_rs, wave, nwaves, lane);
    bf16x8 qf[NS], dof[NS];
    float lse2, dl;
    auto load_q = [&](int blk) {
      const int qrow = blk * 32 + (lane & 31);
      bf16x8 of[NS];
      load_row_frags<HD>(qf, p.q + b * p.q_bs + h * p.q_hs, p.q_rs, qrow, p.sq, lane, HD);
      load_row_frags<HD>(dof, p.dO + b * p.o_bs + h * p.o_hs, p.o_rs, qrow, p.sq, lane, HD);
      load_row_frags<HD>(of, p.o + b * p.o_bs + h * p.o_hs, p.o_rs, qrow, p.sq, lane, HD);
      const float lse_any = p.lse[(long long)bh * p.sq + min(qrow, p.sq - 1)];      // (all requests of the block before the first use of any)
      if (p.scale_q_bf16 == 1) scale_frags_bf16(qf, p.scale);
      const bool qok = qrow < p.sq;
      lse2 = qok ? lse_any * 1.4426950408889634f : INFINITY;
      dl = row_delta_from(dof, of);
    };
    auto run_q = [&](int blk) {
      const int q0 = blk * 32, qrow = q0 + (lane & 31);
      const int my_last = min(S - 1, qrow);
      f32x16 dqacc[NDT];
#pragma unroll
      for (int d = 0; d < NDT; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) dqacc[d][e] = 0.f;
      const uint64_t rb = rb0 + (uint64_t)qrow * (uint64_t)p.sk;
      for (int kt = 0; kt <= blk; ++kt) {
        f32x16 s, dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
        const int ko = reg + rbase + kt * 32 * ZP, vo = rbase + kt * 32 * ZP;
#pragma unroll
        for (int st = 0; st < NS; ++st) {
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z_rows(sm, ko, st), qf[st], s, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z_rows(sm, vo, st), dof[st], dp, 0, 0, 0);
        }
        // element code in compile-time variants (DROP: probability dropout drawn; MASK: the diagonal tile -- the only one with
        // invisible or out-of-range keys).  As run-time tests inside one body they became a branch per element.
        auto elems = [&](auto dropc, auto maskc) {
          constexpr bool DROP = decltype(dropc)::value, MASK = decltype(maskc)::value;
#pragma unroll
          for (int e = 0; e < 16; e += 2) {      // registers e, e+1 hold keys k, k+1 with k even: one hash per pair
            const int key = kt * 32 + acc_row(e, lane);
            const f32x2 t = __builtin_elementwise_fma(f32x2{s[e], s[e + 1]}, f32x2{c2, c2}, f32x2{-lse2, -lse2});
            f32x2 pr = {fexp2(t[0]), fexp2(t[1])};
            if constexpr (MASK) {
              pr[0] = key <= my_last ? pr[0] : 0.f;
              pr[1] = key + 1 <= my_last ? pr[1] : 0.f;
            }
            f32x2 dd = {dp[e], dp[e + 1]};
            if constexpr (DROP) {
              const uint32_t r = mpv_rand_pair_k(seed_k, rb + (uint64_t)key);
              dd[0] = (r & 0xffffu) >= p.drop_thr ? dd[0] * p.drop_scale : 0.f;
              dd[1] = (r >> 16) >= p.drop_thr ? dd[1] * p.drop_scale : 0.f;
            }
            const f32x2 ds = pr * (dd - f32x2{dl, dl});
            s[e] = ds[0];
            s[e + 1] = ds[1];
          }
        };
        using T_ = std::true_type;
        using F_ = std::false_type;
        if (p.drop_thr) {
          if (kt < blk) elems(T_{}, F_{});
          else elems(T_{}, T_{});
        } else {
          if (kt < blk) elems(F_{}, F_{});
          else elems(F_{}, T_{});
        }
        const int kc = reg + cbase + kt * 32 * ZP;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 dsf = acc_to_frag(s, ks);
#pragma unroll
          for (int d = 0; d < NDT; ++d) dqacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z_cols(sm, kc, ks, d), dsf, dqacc[d], 0, 0, 0);
        }
      }
      if (qrow < p.sq) {
        // delta goes out with the block's dQ rows, not where it is computed: there its write acknowledgement sat in front of the
        // vmcnt(0) + barrier that waits for the K / V images
        if (lane < 32) p.delta[(long long)bh * p.sq + qrow] = dl;
        bf16* row = p.dq + b * p.q_bs + h * p.q_hs + (long long)qrow * p.q_rs;
#pragma unroll
        for (int d = 0; d < NDT; ++d)
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            const int col = d * 32 + 8 * q4 + 4 * (lane >> 5);
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = dqacc[d][4 * q4 + e] * p.scale;
            *(bf16x4*)(row + col) = cvt4(v);
          }
      }
    };
    for (int pass = 0; pass < 2; ++pass) {
      const int blk = pass ? blk1 : blk0;
      if (blk < 0) break;
      load_q(blk);
      if (pass == 0) {
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
      }
      run_q(blk);
    }
  }
}

// dK/dV role in the same item shape: a wave owns two KEY blocks (the pairing of the dQ role mirrored: block j has NB - j q-tiles of
// work), K and V rows of the current block in registers, Q and dO of the item as Z images, the per-row statistics
// [lse * log2e | delta] in 2 KiB of LDS in front of them -- 42 KiB per item at S = 160: THREE items per CU (the statistics are what
// keeps it from four; the form without them in LDS -- ds_bpermute from a one-row-per-lane copy -- spilled, see the file header).
template <int THREADS, int WPE>
__global__ __launch_bounds__(THREADS, WPE) void attn_bwd_dkv_pair64_kernel(const AttnArgs p) {
  const MpvSeedKeys seed_k = mpv_seed_keys(p.drop_thr ? mpv_resolve_seed(p.seed) : 0);
  constexpr int HD = 64, NS = 4, NDT = 2;
  extern __shared__ __attribute__((aligned(1024))) char rsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = blockDim.x >> 6;
  int b, h;
  if (!decode_bh(p, b, h)) return;
  const int bh = b * p.heads + h;
  const int S = p.sk, NB = (S + 31) >> 5, qrows = NB * 32;
  const int reg = z_region(S), sreg = stat_bytes(qrows);
  float* sl = (float*)rsm;                     // fp32 statistics in front: no bf16 fragment read can ever land on them
  const int dimg = sreg, qimg = sreg + reg;
  const lds_char* sm = (const lds_char*)rsm;
  // (the thread's statistics -- at most two pairs: 192 threads, <= 224 rows -- are requested before the LDS-DMA of the images, not
  // behind the wait the compiler puts between a pending buffer_load..lds and the LDS stores below)
  float lse_pre[2], delta_pre[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rc = min(tid + i * (int)blockDim.x, S - 1);
    lse_pre[i] = p.lse[(long long)bh * S + rc];
    delta_pre[i] = p.delta[(long long)bh * S + rc];
  }
  {
    const __amdgpu_buffer_rsrc_t qsrc = make_rsrc(p.q + b * p.q_bs + h * p.q_hs, (uint32_t)(((long long)(S - 1) * p.q_rs + HD) * 2));
    const __amdgpu_buffer_rsrc_t dosrc = make_rsrc(p.dO + b * p.o_bs + h * p.o_hs, (uint32_t)(((long long)(S - 1) * p.o_rs + HD) * 2));
    z_dma_rows(qsrc, rsm + qimg, S, p.q_rs, wave, nwaves, lane);
    z_dma_rows(dosrc, rsm + dimg, S, p.o_rs, wave, nwaves, lane);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = tid + i * (int)blockDim.x;
    if (r < qrows) {
      sl[r] = r < S ? lse_pre[i] * 1.4426950408889634f : 1e30f;
      sl[qrows + r] = r < S ? delta_pre[i] : 0.f;
    }
  }
  for (int r = tid + 2 * blockDim.x; r < qrows; r += blockDim.x) {
    sl[r] = r < S ? p.lse[(long long)bh * S + r] * 1.4426950408889634f : 1e30f;
    sl[qrows + r] = r < S ? p.delta[(long long)bh * S + r] : 0.f;
  }
  const float sc = p.scale_q_bf16 ? 1.0f : p.scale;
  const float c2 = sc * 1.4426950408889634f;
  const int rbase = z_rows_base(lane), cbase = z_cols_base(lane);
  int blk0, blk1;
  pair_blocks_q(NB, wave, blk0, blk1);
  const int kb0 = NB - 1 - blk0, kb1 = blk1 >= 0 ? NB - 1 - blk1 : -1;
  const uint64_t rb0 = p.offset + (uint64_t)bh * (uint64_t)p.sq * (uint64_t)p.sk;
  bf16x8 kf[NS], vf[NS];
  auto run_k = [&](int jb) {
    const int k0 = jb * 32, krow = k0 + (lane & 31);
    const bool kok = krow < S;
    f32x16 dkacc[NDT], dvacc[NDT];
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) dkacc[d][e] = dvacc[d][e] = 0.f;
    for (int qt = jb; qt < NB; ++qt) {
      f32x16 s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
      const int qo = qimg + rbase + qt * 32 * ZP, dro = dimg + rbase + qt * 32 * ZP;
#pragma unroll
      for (int st = 0; st < NS; ++st) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z_rows(sm, qo, st), kf[st], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z_rows(sm, dro, st), vf[st], dp, 0, 0, 0);
      }
      const bool interior = !p.drop_thr && qt > jb && (qt * 32 + 31 < S);      // qt > jb: every (q, key) pair visible, keys in range
      const int qc = qimg + cbase + qt * 32 * ZP, dc = dimg + cbase + qt * 32 * ZP;
      int lane_t = lane;
      asm volatile("" : "+v"(lane_t));      // per iteration opaque: the row indices / dropout counters derived from it are not hoisted into registers
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        f32x8 pr8, ds8;
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) {
          const int q4 = 2 * ks + qh;
          const int qb4 = qt * 32 + 8 * q4 + 4 * (lane_t >> 5);
          const f32x4 l4 = *(const f32x4*)(sl + qb4), d4 = *(const f32x4*)(sl + qrows + qb4);
          if (interior) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int e = 4 * q4 + j;
              const float pr = fexp2(s[e] * c2 - l4[j]);
              pr8[4 * qh + j] = pr;
              ds8[4 * qh + j] = pr * (dp[e] - d4[j]);
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int e = 4 * q4 + j;
              const int qr = qb4 + j;
              const bool vis = kok && krow <= qr && qr < S;
              const float pr = vis ? fexp2(s[e] * c2 - l4[j]) : 0.f;
              float keep = 1.0f;
              if (p.drop_thr) {
                const uint32_t rw = mpv_rand_pair_k(seed_k, rb0 + (uint64_t)qr * (uint64_t)p.sk + (uint64_t)(krow & ~1));      // (= attn_keep)
                keep = ((krow & 1) ? rw >> 16 : rw & 0xffffu) >= p.drop_thr ? p.drop_scale : 0.f;
              }
              pr8[4 * qh + j] = vis ? pr * keep : 0.f;
              ds8[4 * qh + j] = vis ? pr * (dp[e] * keep - d4[j]) : 0.f;
            }
          }
        }
        const bf16x8 pf = cvt8(pr8), dsf = cvt8(ds8);
#pragma unroll
        for (int d = 0; d < NDT; ++d) {
          dvacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z_cols(sm, dc, ks, d), pf, dvacc[d], 0, 0, 0);
          dkacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z_cols(sm, qc, ks, d), dsf, dkacc[d], 0, 0, 0);
        }
      }
    }
    if (kok) {
      bf16* rv = p.dv + b * p.v_bs + h * p.v_hs + (long long)krow * p.v_rs;
      bf16* rk = p.dk + b * p.k_bs + h * p.k_hs + (long long)krow * p.k_rs;
#pragma unroll
      for (int d = 0; d < NDT; ++d)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int col = d * 32 + 8 * q4 + 4 * (lane >> 5);
          f32x4 a, c;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a[e] = dvacc[d][4 * q4 + e];
            c[e] = dkacc[d][4 * q4 + e] * sc;
          }
          *(bf16x4*)(rv + col) = cvt4(a);
          *(bf16x4*)(rk + col) = cvt4(c);
        }
    }
  };
  for (int pass = 0; pass < 2; ++pass) {
    const int jb = pass ? kb1 : kb0;
    if (jb < 0) break;
    {
      const int krow = jb * 32 + (lane & 31);
      load_row_frags<HD>(kf, p.k + b * p.k_bs + h * p.k_hs, p.k_rs, krow, S, lane, HD);
      load_row_frags<HD>(vf, p.v + b * p.v_bs + h * p.v_hs, p.v_rs, krow, S, lane, HD);
    }
    if (pass == 0) {
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
      if (p.scale_q_bf16 == 1) {      // q' = bf16(q * scale) in place, once (element-wise: the chunk permutation does not matter; 2: q arrives scaled)
        for (int g = tid; g < S * 8; g += blockDim.x) {
          bf16x8* ptr = (bf16x8*)(rsm + qimg + g * 16);
          f32x8 f = cvt8(*ptr);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] *= p.scale;
          *ptr = cvt8(f);
        }
        __syncthreads();
      }
    }
    run_k(jb);
  }
}
