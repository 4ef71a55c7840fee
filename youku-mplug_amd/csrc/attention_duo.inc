// attention_duo.inc -- the backward of the ViT spatial attention (head_dim 96, 7 key tiles: 193..224 keys, no mask, no dropout)
// with TWO (batch, head) items per CU; included by attention.hip inside its anonymous namespace.
//
// Replaces attn_bwd_dq_res_kernel<96, 7> and attn_bwd_dkv_res_kernel<96> on models/vision_transformer.py:179-204 (Attention.forward:
// softmax(q k^T) v) in the backward of the 12 spatial attentions of the TimeSformer blocks.
//
// The one-shot kernels run one 7-wave workgroup per CU: every CU loads its operands, then computes, then stores, and nothing
// overlaps the load (a launch is 8 such rounds).  What this round's decoder kernels showed is that a second ITEM on the CU
// hides more than a pipelined load inside one item (attention_pair.inc) -- but a second 7-wave workgroup fits neither the
// register file (256 registers per wave: 8 waves per CU) nor LDS (two or three 46 KiB whole-tile images per item).
// Here an item is FOUR waves that each own two row blocks (w and w + 4, the last wave one), run one after the other, and
// its images are packed.  dQ role: K as unpadded rows at the 208-byte pitch (row and column fragments both read it), V -- only
// ever read as row fragments -- at 192 bytes with the 16-byte chunk c of row r stored at position (c + ((r >> 2) & 3)) mod 12,
// which is conflict-free for ds_read_b128's hardware lane groups AND for the transposing reads (simulated:
// tools/probe/sim_zimage_layout.py, check_rot192): 41 + 37 KiB per item, two items per CU, 8 waves.  dK/dV role: see below.
// dQ: tile reads past the last key: K's land in V (finite data; their dS is an exact zero), V's run past the workgroup's
// allocation (stale bytes) and feed only dP, which the last tile masks with a select, never with a multiplication.
// Measured (tools/attn_pair_ab.py AB_VIT=1; profiles/r03_c15_vit_dq_duo_ab.log, r03_c17_duo_dkv_ab.log): ViT backward per layer
// 345.7 us (one-shot) -> 324.5 (dQ as two items) -> 290.9 us (dQ and dK/dV); step 78.35 -> 78.05 -> 77.1 ms.  The FORWARD in this
// form (commit a7157d4+1: attn_fwd_duo96_kernel) ran 88 us against 82.7 us for the persistent double-buffered kernel
// (profiles/r03_c16_duo_fwd_ab.log) and is not kept: with the whole score block in registers the forward already has one wave
// per SIMD working at a time, and there the pipelined load wins.  Also measured and not kept: dQ and dK/dV of an item FUSED in
// one 8-wave workgroup (waves 0-3 in the dQ role, 4-7 in the dK/dV role at the same time, all four images resident: 154 KiB, one
// item per CU; q, k, v, dO leave HBM once instead of twice: 930 -> 620 MB per layer): 321 us against 292 us for the two
// two-item launches (profiles/r03_c18_fused_ab.log) -- two co-resident items hide more than a third less traffic saves.

// (DUO_KP / DUO_VP, the image pitches, and packed_region / duo_*_lds: attention_layout.h)
// DMA of the two dQ-role images: K [S][208 B] at kl (13 chunks per row: 12 + the zero-filled pad chunk), V [S][192 B] at vl with the
// chunk at LDS position pos of row r = source chunk (pos - ((r >> 2) & 3)) mod 12
__device__ __forceinline__ void duo_dma_kv(const AttnArgs& p, int b, int h, char* kl, char* vl, int S, int wave, int nwaves, int lane) {
  constexpr int HD = 96;
  const __amdgpu_buffer_rsrc_t ksrc = make_rsrc(p.k + b * p.k_bs + h * p.k_hs, (uint32_t)(((long long)(S - 1) * p.k_rs + HD) * 2));
  const __amdgpu_buffer_rsrc_t vsrc = make_rsrc(p.v + b * p.v_bs + h * p.v_hs, (uint32_t)(((long long)(S - 1) * p.v_rs + HD) * 2));
  {
    const int ninstr = (S * 13 + 63) >> 6;
    for (int i = wave; i < ninstr; i += nwaves) {
      const int g = i * 64 + lane;
      const int row = g / 13, cc = g - row * 13;
      const uint32_t off = (row < S && cc < 12) ? (uint32_t)(((long long)row * p.k_rs + cc * 8) * 2) : 0x80000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ksrc, (lds_void_t*)(kl + i * 1024), 16, off, 0, 0, 0);
    }
  }
  {
    const int ninstr = (S * 12 + 63) >> 6;
    for (int i = wave; i < ninstr; i += nwaves) {
      const int g = i * 64 + lane;
      const int row = g / 12, pos = g - row * 12;
      int cc = pos - ((row >> 2) & 3);
      cc = cc < 0 ? cc + 12 : cc;
      const uint32_t off = row < S ? (uint32_t)(((long long)row * p.v_rs + cc * 8) * 2) : 0x80000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(vsrc, (lds_void_t*)(vl + i * 1024), 16, off, 0, 0, 0);
    }
  }
}

// The dQ role of one wave: query blocks rw and rw + 4 of item (b, h), K image at LDS byte offset kimg, V image at vimg.
// SYNC: the role owns the workgroup's first barrier (the images it reads are complete behind it); in the fused kernel the
// caller has synchronised already.
template <bool SYNC>
__device__ __forceinline__ void duo_dq_role(const AttnArgs& p, const lds_char* sm, int kimg, int vimg, int b, int h, int bh, int S, int lane, int rw) {
  constexpr int HD = 96, NS = 6, NDT = 3, NTC = 7;
  float sc = p.scale;
  if (p.scale_q_bf16) sc = 1.0f;
  const float c2 = sc * 1.4426950408889634f;
  const int kroff = kimg + rows_lane_base<DUO_KP>(lane), kcoff = kimg + cols_lane_base<DUO_KP>(lane);
  // V row fragments: chunk 2 * st + (lane >> 5) of row (lane & 31) sits at position (that + rot) mod 12; only steps 4 and 5 can wrap
  const int vc0 = (lane >> 5) + (((lane & 31) >> 2) & 3);
  const int vbase = vimg + (lane & 31) * DUO_VP + vc0 * 16;
  const int vb4 = vbase + 128 - (vc0 == 4 ? 192 : 0), vb5 = vbase + 160 - (vc0 >= 2 ? 192 : 0);
  auto vfrag = [&](int toff, int st) -> bf16x8 {
    const int a = st < 4 ? vbase + st * 32 : st == 4 ? vb4 : vb5;
    return *(const lds_bf16x8*)(sm + a + toff);
  };
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
    const int qrow = blk * 32 + (lane & 31);
    f32x16 dqacc[NDT];
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) dqacc[d][e] = 0.f;
    // MPV_AB_DQ_PIPE (round 6, a build-time arm, NOT the shipped form): the score / dP products of key tile kt + 1 issued BEFORE the softmax
    // arithmetic of tile kt, into a second pair of accumulators (198 instead of 154 registers, still two waves per SIMD) -- 45 % of this kernel's
    // wave cycles are dependency stalls.  Measured (profiles/r06_c18_dq_pipe_ab.log): kernel 124.6 -> 122.1 us, step 72.40 -> 72.52 ms in three
    // alternations: the SIMD's second wave already fills most of what the pipelining frees.  Buried; the arm stays for the next measurement.
    f32x16 sb[2], dpb[2];
    auto sdp = [&](int kt, f32x16& s, f32x16& dp) __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
      for (int st = 0; st < NS; ++st) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_f(sm, kroff + kt * 32 * DUO_KP, st), qf[st], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfrag(kt * 32 * DUO_VP, st), dof[st], dp, 0, 0, 0);
      }
    };
#ifdef MPV_AB_DQ_PIPE
    sdp(0, sb[0], dpb[0]);
#endif
#pragma unroll
    for (int kt = 0; kt < NTC; ++kt) {
#ifdef MPV_AB_DQ_PIPE
      if (kt + 1 < NTC) sdp(kt + 1, sb[(kt + 1) & 1], dpb[(kt + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);        // keep the next tile's products ahead of this tile's arithmetic
      f32x16& s = sb[kt & 1];
      f32x16& dp = dpb[kt & 1];
#else
      f32x16 s, dp;
      sdp(kt, s, dp);
#endif
      if (kt < NTC - 1) {
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const f32x2 t = __builtin_elementwise_fma(f32x2{s[e], s[e + 1]}, f32x2{c2, c2}, f32x2{-lse2, -lse2});
          const f32x2 pr = {fexp2(t[0]), fexp2(t[1])};
          const f32x2 ds = pr * (f32x2{dp[e], dp[e + 1]} - f32x2{dl, dl});
          s[e] = ds[0];
          s[e + 1] = ds[1];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) {      // keys past the end: a select, not a product with a zero probability (stale V bytes may be NaN)
          const int key = kt * 32 + acc_row(e, lane);
          const float pr = fexp2(s[e] * c2 - lse2);
          s[e] = key < S ? pr * (dp[e] - dl) : 0.f;
        }
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 dsf = acc_to_frag(s, ks);
#pragma unroll
        for (int d = 0; d < NDT; ++d)
          dqacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_f<DUO_KP>(sm, kcoff + kt * 32 * DUO_KP, ks, d), dsf, dqacc[d], 0, 0, 0);
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
    const int blk = rw + 4 * pass;
    if (blk * 32 >= p.sq) break;
    load_q(blk);
    if (SYNC && pass == 0) {      // (uniform over the workgroup: every wave has a first block)
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
    }
    run_q(blk);
  }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS, 2) void attn_bwd_dq_duo96_kernel(const AttnArgs p) {
  extern __shared__ __attribute__((aligned(1024))) char rsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = blockDim.x >> 6;
  int b, h;
  if (!decode_bh(p, b, h)) return;
  const int S = p.sk;
  const int kreg = packed_region(S, DUO_KP);
  duo_dma_kv(p, b, h, rsm, rsm + kreg, S, wave, nwaves, lane);      // [K | V]
  duo_dq_role<true>(p, (const lds_char*)rsm, 0, kreg, b, h, b * p.heads + h, S, lane, wave);
}

// ------------------------------------------------------------------------------------------------------------- dK / dV
// The dK/dV role in the same item shape: 4 waves, each owning two KEY blocks (w and w + 4) with their K and V rows in
// registers; Q and dO of the whole item in LDS, both read as row fragments (S = Q K^T, dP = dO V^T) AND as column fragments
// (dK += dS^T Q, dV += P^T dO), both at the rotated 192-byte pitch -- 37 + 37 KiB + 2 KiB of per-row statistics.
// Rotation and the transposing read: a column fragment's rows are 4h + m (+ 8) + 16 ks + 32 qt, whose (row >> 2) & 3 is h
// (h + 2 for the + 8 half) whatever m, ks and qt are: two per-lane constants per d-tile.
// Reads past the last query row: dO's land in Q (finite); Q's run past the allocation, and Q's column fragments meet exactly-zero
// dS values there, so in the last q-tile those fragments are read with the row index clamped to the last row (finite data).
__device__ __forceinline__ int rot192_addr(int row, int chunk, int sub) {
  int pos = chunk + ((row >> 2) & 3);
  pos = pos >= 12 ? pos - 12 : pos;
  return row * DUO_VP + pos * 16 + sub;
}

// DMA of the two dK/dV-role images (Q at ql, dO at dl: [S][192 B], chunks rotated as V above)
__device__ __forceinline__ void duo_dma_qdo(const AttnArgs& p, int b, int h, char* ql, char* dl, int S, int wave, int nwaves, int lane) {
  constexpr int HD = 96;
  const __amdgpu_buffer_rsrc_t qsrc = make_rsrc(p.q + b * p.q_bs + h * p.q_hs, (uint32_t)(((long long)(S - 1) * p.q_rs + HD) * 2));
  const __amdgpu_buffer_rsrc_t dosrc = make_rsrc(p.dO + b * p.o_bs + h * p.o_hs, (uint32_t)(((long long)(S - 1) * p.o_rs + HD) * 2));
  const int ninstr = (S * 12 + 63) >> 6;
  for (int i = wave; i < ninstr; i += nwaves) {
    const int g = i * 64 + lane;
    const int row = g / 12, pos = g - row * 12;
    int cc = pos - ((row >> 2) & 3);
    cc = cc < 0 ? cc + 12 : cc;
    const bool ok = row < S;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(qsrc, (lds_void_t*)(ql + i * 1024), 16, ok ? (uint32_t)(((long long)row * p.q_rs + cc * 8) * 2) : 0x80000000u, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(dosrc, (lds_void_t*)(dl + i * 1024), 16, ok ? (uint32_t)(((long long)row * p.o_rs + cc * 8) * 2) : 0x80000000u, 0, 0, 0);
  }
}
// q' = bf16(q * scale) in place over the Q image, once per item, by ALL threads of the workgroup (element-wise: the chunk
// rotation does not matter); between two barriers of the caller
__device__ __forceinline__ void duo_scale_q_image(const AttnArgs& p, char* ql, int S, int tid, int nthreads) {
  for (int g = tid; g < S * 12; g += nthreads) {
    bf16x8* ptr = (bf16x8*)(ql + g * 16);
    f32x8 f = cvt8(*ptr);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] *= p.scale;
    *ptr = cvt8(f);
  }
}

// The dK/dV role of one wave: key blocks rw and rw + 4 of item (b, h); statistics [lse * log2e | delta] x qrows (fp32) at sl, dO
// image at LDS byte offset dimg, Q image at qimg (already scaled when scale_q_bf16).  The caller has synchronised.
__device__ __forceinline__ void duo_dkv_role(const AttnArgs& p, const lds_char* sm, const float* sl, int dimg, int qimg, int b, int h, int S, int lane, int rw) {
  constexpr int HD = 96, NS = 6, NDT = 3;
  const int qtiles = (S + 31) >> 5, qrows = qtiles * 32;
  const float sc = p.scale_q_bf16 ? 1.0f : p.scale;
  const float c2 = sc * 1.4426950408889634f;
  // row fragments (both images): chunk 2 st + (lane >> 5) of row (lane & 31), rotated; only steps 4 and 5 can wrap
  const int rc0 = (lane >> 5) + (((lane & 31) >> 2) & 3);
  const int rb = (lane & 31) * DUO_VP + rc0 * 16;
  const int rb4 = rb + 128 - (rc0 == 4 ? 192 : 0), rb5 = rb + 160 - (rc0 >= 2 ? 192 : 0);
  auto rfrag = [&](int img, int toff, int st) -> bf16x8 {
    const int a = st < 4 ? rb + st * 32 : st == 4 ? rb4 : rb5;
    return *(const lds_bf16x8*)(sm + img + a + toff);
  };
  // column fragments (both images): rows 4h + m and 4h + m + 8, chunk dt * 4 + j * 2 + (i >> 1), rotation h / h + 2
  const int ch = lane >> 5, cm = (lane & 15) >> 2, cl = ((lane >> 4) & 1) * 2 + ((lane & 3) >> 1), csub = (lane & 3 & 1) * 8;
  int clo[NDT], chi[NDT];
#pragma unroll
  for (int d = 0; d < NDT; ++d) {
    int plo = d * 4 + cl + ch, phi = d * 4 + cl + ch + 2;
    plo = plo >= 12 ? plo - 12 : plo;
    phi = phi >= 12 ? phi - 12 : phi;
    clo[d] = (4 * ch + cm) * DUO_VP + plo * 16 + csub;
    chi[d] = (4 * ch + cm + 8) * DUO_VP + phi * 16 + csub;
  }
  auto cfrag = [&](int img, int toff, int ks, int d) -> bf16x8 {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(sm + img + toff + ks * 16 * DUO_VP + clo[d]));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(sm + img + toff + ks * 16 * DUO_VP + chi[d]));
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = lo;
    u.s.b = hi;
    return u.v;
  };
  auto cfrag_clamped = [&](int img, int qt, int ks, int d) -> bf16x8 {      // last q-tile of the Q image: rows past the end re-read the last row
    const int r0 = min(qt * 32 + ks * 16 + 4 * ch + cm, S - 1), r1 = min(qt * 32 + ks * 16 + 4 * ch + cm + 8, S - 1);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(sm + img + rot192_addr(r0, d * 4 + cl, csub)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(sm + img + rot192_addr(r1, d * 4 + cl, csub)));
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = lo;
    u.s.b = hi;
    return u.v;
  };
  bf16x8 kf[NS], vf[NS];
  auto load_k = [&](int jb) {
    const int krow = jb * 32 + (lane & 31);
    load_row_frags<HD>(kf, p.k + b * p.k_bs + h * p.k_hs, p.k_rs, krow, S, lane, HD);
    load_row_frags<HD>(vf, p.v + b * p.v_bs + h * p.v_hs, p.v_rs, krow, S, lane, HD);
  };
  auto run_k = [&](int jb) {
    const int k0 = jb * 32, krow = k0 + (lane & 31);
    const bool kok = krow < S;
    f32x16 dkacc[NDT], dvacc[NDT];
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) dkacc[d][e] = dvacc[d][e] = 0.f;
    for (int qt = 0; qt < qtiles; ++qt) {
      f32x16 s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
      const int toff = qt * 32 * DUO_VP;
#pragma unroll
      for (int st = 0; st < NS; ++st) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rfrag(qimg, toff, st), kf[st], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rfrag(dimg, toff, st), vf[st], dp, 0, 0, 0);
      }
      const bool interior = (k0 + 31 < S) && (qt * 32 + 31 < S);
      const bool clamp_q = qt * 32 + 31 >= S;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        f32x8 pr8, ds8;
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) {
          const int q4 = 2 * ks + qh;
          const int qb4 = qt * 32 + 8 * q4 + 4 * (lane >> 5);
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
              const bool vis = kok && (qb4 + j) < S;
              const float pr = fexp2(s[e] * c2 - l4[j]);
              pr8[4 * qh + j] = vis ? pr : 0.f;
              ds8[4 * qh + j] = vis ? pr * (dp[e] - d4[j]) : 0.f;
            }
          }
        }
        const bf16x8 pf = cvt8(pr8), dsf = cvt8(ds8);
#pragma unroll
        for (int d = 0; d < NDT; ++d) {
          dvacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cfrag(dimg, toff, ks, d), pf, dvacc[d], 0, 0, 0);
          const bf16x8 qc = clamp_q ? cfrag_clamped(qimg, qt, ks, d) : cfrag(qimg, toff, ks, d);
          dkacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qc, dsf, dkacc[d], 0, 0, 0);
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
    const int jb = rw + 4 * pass;
    if (jb * 32 >= S) break;
    load_k(jb);
    run_k(jb);
  }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS, 2) void attn_bwd_dkv_duo96_kernel(const AttnArgs p) {
  extern __shared__ __attribute__((aligned(1024))) char rsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = blockDim.x >> 6;
  int b, h;
  if (!decode_bh(p, b, h)) return;
  const int bh = b * p.heads + h;
  const int S = p.sq;                                   // == p.sk (host-checked)
  const int qrows = ((S + 31) >> 5) * 32;
  const int sreg = stat_bytes(qrows), ireg = packed_region(S, DUO_VP);
  float* sl = (float*)rsm;                              // [lse * log2e | delta] x qrows (fp32: in front, never read as bf16)
  char* dl = rsm + sreg;                                // dO [S][192 B] rotated: reads past the end land in Q (finite)
  char* ql = dl + ireg;                                 // Q  [S][192 B] rotated
  // (the thread's first pair of statistics is requested before the LDS-DMA of the images, not behind the wait the compiler puts
  // between a pending buffer_load..lds and the LDS stores below)
  const float lse_first = p.lse[(long long)bh * S + min(tid, S - 1)], delta_first = p.delta[(long long)bh * S + min(tid, S - 1)];
  duo_dma_qdo(p, b, h, ql, dl, S, wave, nwaves, lane);
  if (tid < qrows) {
    sl[tid] = tid < S ? lse_first * 1.4426950408889634f : 1e30f;
    sl[qrows + tid] = tid < S ? delta_first : 0.f;
  }
  for (int r = tid + blockDim.x; r < qrows; r += blockDim.x) {
    sl[r] = r < S ? p.lse[(long long)bh * S + r] * 1.4426950408889634f : 1e30f;
    sl[qrows + r] = r < S ? p.delta[(long long)bh * S + r] : 0.f;
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
  if (p.scale_q_bf16 == 1) {      // (2: q arrives scaled)
    duo_scale_q_image(p, ql, S, tid, blockDim.x);
    __syncthreads();
  }
  duo_dkv_role(p, (const lds_char*)rsm, sl, sreg, sreg + ireg, b, h, S, lane, wave);
}
