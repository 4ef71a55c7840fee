// attention_temporal_long.inc -- temporal attention for 17..64 frames on the matrix cores (included by attention.hip, inside its
// anonymous namespace; DESIGN.md section 15).
//
// One wave owns one (sequence, head) problem of T <= TT tokens, TT = 32 or 64: the score matrix is one or four 32 x 32 tiles.
// Every product is v_mfma_f32_32x32x16_bf16.  The head dimension is walked in 6 steps of 16 (head_dim <= 96; columns past the
// true head_dim are zero-filled on load and never stored), so one instance serves every accepted head_dim.
//
// Lane maps (as in the kernels above): an A / B operand fragment of step s is the 16-byte piece [s * 16 + 8 * (lane >> 5), +8) of
// row (lane & 31) of a 32-row tile -- a plain global load of a token row.  An accumulator holds column (lane & 31) and the 16 rows
// acc_row(e, lane).  Two orientations are used:
//   "query on the lane":  S^T = K (Q scale)^T and dP^T = V dO^T.  A lane owns one query, its keys are its registers: the row
//                         softmax and rowsum(P o dP) are register reductions plus one exchange across the lane halves, and
//                         P^T / dS^T are the B operand of the next product as they stand (acc_to_frag): O^T = V^T P^T,
//                         dQ^T = K^T dS^T.
//   "key on the lane":    S = (Q scale) K^T and dP = dO V^T from the same row fragments with A and B exchanged; P and dS (from the
//                         per-query statistics the first orientation left in LDS) feed dV^T = dO^T P and dK^T = (Q scale)^T dS.
// Only the operands read against their row direction (V^T, K^T, dO^T, Q^T) go through LDS: one per-wave image of 32-row tiles at
// the 208-byte pitch, written from the row fragments the wave holds anyway and read with ds_read_b64_tr_b16 (frag_cols).  The
// backward reuses that image: all of K for the dQ pass, then one [Q scale | dO] tile pair per (key tile, query tile) step.
//
// Padding: token rows t >= T are never dereferenced (the load re-reads row T - 1 and a select zeroes the fragment) and never
// stored.  Keys t >= T score -inf in the query-on-lane orientation (probability exactly 0); in the key-on-lane orientation a
// padded key is a lane whose column is not stored, and a padded query has statistics (+inf, 0): P = dS = 0.
constexpr int TL_NS = 6;       // reduction steps of 16 over the head dimension
constexpr int TL_NDT = 3;      // 32-column output tiles
constexpr float TL_LOG2E = 1.4426950408889634f;

// this lane's fragments of one token row (rowp: its first element of the head; `ok`: the row exists)
__device__ __forceinline__ void tl_load_row(bf16x8 (&f)[TL_NS], const bf16* rowp, bool ok, int lane, int hd) {
  const bf16* rp = rowp + (lane >> 5) * 8;
#pragma unroll
  for (int s = 0; s < TL_NS; ++s) {
    union { i32x4 i; bf16x8 b; } u;
    const bool cok = s * 16 + (lane >> 5) * 8 < hd;
    u.i = *(const i32x4*)(rp + (cok ? s * 16 : 0));
    if (!(ok && cok)) u.i = i32x4{0, 0, 0, 0};
    f[s] = u.b;
  }
}
// the inverse of frag_rows: row fragments of 32-row tile `tile` into the image
__device__ __forceinline__ void tl_put_rows(char* img, int tile, const bf16x8 (&f)[TL_NS], int lane) {
  char* dst = img + (tile * 32 + (lane & 31)) * TEMPORAL_MFMA_PITCH + (lane >> 5) * 16;
#pragma unroll
  for (int s = 0; s < TL_NS; ++s) *(bf16x8*)(dst + s * 32) = f[s];
}
__device__ __forceinline__ void tl_zero(f32x16 (&a)[TL_NDT]) {
#pragma unroll
  for (int d = 0; d < TL_NDT; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) a[d][e] = 0.f;
}
// a transposed 32 x head_dim accumulator set (column = token on the lane) to token row `row` of a [rows][ld] matrix
__device__ __forceinline__ void tl_store_row(bf16* row, const f32x16 (&a)[TL_NDT], float mul, int lane, int hd) {
#pragma unroll
  for (int d = 0; d < TL_NDT; ++d)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int col = d * 32 + 8 * q4 + 4 * (lane >> 5);
      if (col < hd) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = a[d][4 * q4 + e] * mul;
        *(bf16x4*)(row + col) = cvt4(v);
      }
    }
}

template <bool BWD, int TT>
__global__ __launch_bounds__(64 * TEMPORAL_MFMA_WAVES, 2) void temporal_attn_mfma_kernel(const TempArgs p) {
  static_assert(TT == 32 || TT == 64, "one or four score tiles");
  constexpr int NT = TT / 32;
  constexpr int PITCH = TEMPORAL_MFMA_PITCH;
  extern __shared__ __attribute__((aligned(16))) char tlsm[];
  const int lane = threadIdx.x & 63, nwv = (int)(blockDim.x >> 6);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // the problem index and every row base are scalars
  const int T = p.T, hd = p.hd, D = p.heads * hd;
  const int r = lane & 31;
  char* img = tlsm + wave * temporal_mfma_wave_lds(BWD, TT);
  const long long nprob = (long long)p.n_outer * p.n_inner * p.heads;
  const long long pstride = (long long)gridDim.x * nwv;
  for (long long pr = (long long)blockIdx.x * nwv + wave; pr < nprob; pr += pstride) {
    const int h = (int)(pr % p.heads);
    const long long seq = pr / p.heads;
    const long long row0 = (seq / p.n_inner) * p.outer_stride + p.inner_offset + seq % p.n_inner;
    // token t of this problem: its global row (rows past T - 1 re-read row T - 1; the caller zeroes what it loads from them)
    const auto grow = [&](int t) { return row0 + (long long)min(t, T - 1) * p.t_stride; };
    const auto qkv_row = [&](int t) { return p.qkv + grow(t) * (3LL * D) + h * hd; };
    if constexpr (!BWD) {
      // ---- V image
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        bf16x8 vf[TL_NS];
        tl_load_row(vf, qkv_row(kt * 32 + r) + 2 * D, kt * 32 + r < T, lane, hd);
        tl_put_rows(img, kt, vf, lane);
      }
      WAVE_SYNC();
#pragma unroll
      for (int qt = 0; qt < NT; ++qt) {
        const int tq = qt * 32 + r;
        bf16x8 qf[TL_NS];
        tl_load_row(qf, qkv_row(tq), tq < T, lane, hd);
        scale_frags_bf16(qf, p.scale);                           // q * scale rounds to bf16 (reference :179)
        f32x16 st[NT];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          bf16x8 kf[TL_NS];
          tl_load_row(kf, qkv_row(kt * 32 + r) + D, kt * 32 + r < T, lane, hd);
          f32x16 s;
#pragma unroll
          for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
          for (int sx = 0; sx < TL_NS; ++sx) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[sx], qf[sx], s, 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            s[e] = kt * 32 + acc_row(e, lane) < T ? s[e] : -INFINITY;
            mx = fmaxf(mx, s[e]);
          }
          st[kt] = s;
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                  // (key 0 always exists: finite)
        const float m2 = mx * TL_LOG2E;
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            st[kt][e] = fexp2(st[kt][e] * TL_LOG2E - m2);        // masked keys: 2^-inf = 0
            l += st[kt][e];
          }
        l += __shfl_xor(l, 32, 64);
        const float inv_l = 1.0f / l;
        f32x16 oacc[TL_NDT];
        tl_zero(oacc);
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
          for (int e = 0; e < 16; ++e) st[kt][e] *= inv_l;       // normalised, then cast to bf16 (reference :201)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 pf = acc_to_frag(st[kt], ks);
#pragma unroll
            for (int d = 0; d < TL_NDT; ++d)
              oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<PITCH>(img, kt, ks, d, lane), pf, oacc[d], 0, 0, 0);
          }
        }
        if (tq < T) tl_store_row(p.out + grow(tq) * (long long)D + h * hd, oacc, 1.0f, lane, hd);
      }
      WAVE_SYNC();                                               // the next problem overwrites the image
    } else {
      const auto do_row = [&](int t) { return p.dout + grow(t) * (long long)D + h * hd; };
      f32x2* stats = (f32x2*)(img + 64 * PITCH);                 // [TT] per query: (log2-domain lse, rowsum(P o dP))
      // ---- pass 1, query on the lane: statistics and dQ.  The image holds K.
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        bf16x8 kf[TL_NS];
        tl_load_row(kf, qkv_row(kt * 32 + r) + D, kt * 32 + r < T, lane, hd);
        tl_put_rows(img, kt, kf, lane);
      }
      WAVE_SYNC();
#pragma unroll 1      // (the tiles share no registers: rolled, the second tile's loads are not hoisted over the first tile's accumulators)
      for (int qt = 0; qt < NT; ++qt) {
        const int tq = qt * 32 + r;
        bf16x8 qf[TL_NS], dof[TL_NS];
        tl_load_row(qf, qkv_row(tq), tq < T, lane, hd);
        tl_load_row(dof, do_row(tq), tq < T, lane, hd);
        scale_frags_bf16(qf, p.scale);
        f32x16 st[NT], dpt[NT];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          bf16x8 vf[TL_NS];
          tl_load_row(vf, qkv_row(kt * 32 + r) + 2 * D, kt * 32 + r < T, lane, hd);
          f32x16 s, dp;
#pragma unroll
          for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
          for (int sx = 0; sx < TL_NS; ++sx) {
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<PITCH>(img, kt, sx, lane), qf[sx], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[sx], dof[sx], dp, 0, 0, 0);        // dP^T = V dO^T
          }
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            s[e] = kt * 32 + acc_row(e, lane) < T ? s[e] : -INFINITY;
            mx = fmaxf(mx, s[e]);
          }
          st[kt] = s;
          dpt[kt] = dp;
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m2 = mx * TL_LOG2E;
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            st[kt][e] = fexp2(st[kt][e] * TL_LOG2E - m2);
            l += st[kt][e];
          }
        l += __shfl_xor(l, 32, 64);
        const float inv_l = 1.0f / l;
        float dl = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            st[kt][e] *= inv_l;
            dl += st[kt][e] * dpt[kt][e];                        // (a padded key: 0 * 0)
          }
        dl += __shfl_xor(dl, 32, 64);
        if (lane < 32) stats[tq] = tq < T ? f32x2{m2 + log2f(l), dl} : f32x2{INFINITY, 0.f};
        f32x16 dqacc[TL_NDT];
        tl_zero(dqacc);
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
          for (int e = 0; e < 16; ++e) st[kt][e] *= dpt[kt][e] - dl;      // dS = P o (dP - rowsum(P o dP))
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 dsf = acc_to_frag(st[kt], ks);
#pragma unroll
            for (int d = 0; d < TL_NDT; ++d)
              dqacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<PITCH>(img, kt, ks, d, lane), dsf, dqacc[d], 0, 0, 0);
          }
        }
        if (tq < T) tl_store_row(p.dqkv + grow(tq) * (3LL * D) + h * hd, dqacc, p.scale, lane, hd);
      }
      // ---- pass 2, key on the lane: dK and dV.  The image holds tile 0 = a query tile of Q scale, tile 1 = the same of dO.
#pragma unroll 1
      for (int kt = 0; kt < NT; ++kt) {
        const int tk = kt * 32 + r;
        bf16x8 kf[TL_NS], vf[TL_NS];
        tl_load_row(kf, qkv_row(tk) + D, tk < T, lane, hd);
        tl_load_row(vf, qkv_row(tk) + 2 * D, tk < T, lane, hd);
        f32x16 dkacc[TL_NDT], dvacc[TL_NDT];
        tl_zero(dkacc);
        tl_zero(dvacc);
#pragma unroll 1
        for (int qt = 0; qt < NT; ++qt) {
          {
            bf16x8 qf[TL_NS], dof[TL_NS];
            tl_load_row(qf, qkv_row(qt * 32 + r), qt * 32 + r < T, lane, hd);
            tl_load_row(dof, do_row(qt * 32 + r), qt * 32 + r < T, lane, hd);
            scale_frags_bf16(qf, p.scale);
            WAVE_SYNC();                                         // the image's readers (and pass 1's statistics) are done
            tl_put_rows(img, 0, qf, lane);
            tl_put_rows(img, 1, dof, lane);
            WAVE_SYNC();
          }
          // the row fragments come back from the image (the registers they arrived in are free for the accumulators)
          f32x16 s, dp;
#pragma unroll
          for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
          for (int sx = 0; sx < TL_NS; ++sx) {
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<PITCH>(img, 0, sx, lane), kf[sx], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<PITCH>(img, 1, sx, lane), vf[sx], dp, 0, 0, 0);
          }
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const f32x2 sd = stats[qt * 32 + acc_row(e, lane)];
            s[e] = fexp2(s[e] * TL_LOG2E - sd[0]);               // P (a padded query: 2^-inf = 0)
            dp[e] = s[e] * (dp[e] - sd[1]);                      // dS
          }
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 pf = acc_to_frag(s, ks), dsf = acc_to_frag(dp, ks);
#pragma unroll
            for (int d = 0; d < TL_NDT; ++d) {
              dvacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<PITCH>(img, 1, ks, d, lane), pf, dvacc[d], 0, 0, 0);
              dkacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<PITCH>(img, 0, ks, d, lane), dsf, dkacc[d], 0, 0, 0);
            }
          }
        }
        if (tk < T) {
          bf16* dst = p.dqkv + grow(tk) * (3LL * D) + h * hd;
          tl_store_row(dst + D, dkacc, 1.0f, lane, hd);
          tl_store_row(dst + 2 * D, dvacc, 1.0f, lane, hd);
        }
      }
      WAVE_SYNC();
    }
  }
}
