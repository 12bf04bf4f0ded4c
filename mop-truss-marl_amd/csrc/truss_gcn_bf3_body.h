// truss_gcn_bf3_body.h -- the split-weight GCN layer (truss_gcn.h has the description): the statements of one layer, included as
// the body of truss_gcn_layer_bf3_kernel and, once per step, of truss_gcn_group_bf3_kernel.  No include guard: this is a block of
// statements, not declarations.  In scope where it is included: the template arguments NW, KT, EPI, T; P (the layer, TgArgs<EPI>::type),
// ws (the split-weight image), KP (its row length) and tid (the thread index; the group kernel: opaque per step).  Every barrier is
// at the top level of the block, and control leaves it only at its end.
  constexpr int MT = 32 * NW, NT = 64 * NW, CB = 7, WROWS = 32 * CB;
  static_assert(WROWS == TG_CP, "split-weight image rows");
  static_assert(T >= 1 && T <= 3, "bf16 terms per operand");
  extern __shared__ __attribute__((aligned(16))) char tg_smem[];
  float *sXraw = (float *)tg_smem;                                   // [MT][TG_LD] float32 raw input rows of a slab
  char *sXs = tg_smem + MT * TG_LD * 4;                              // [2][T][MT][32 B]    split aggregated rows (MFMA A operand)
  char *sWs = sXs + 2 * T * MT * 32;                                 // [2][T][WROWS][32 B] split W slab, [col][k]
  const int lane = tid & 63, wave = tid >> 6;
  const int N = P.N, Kn = P.Kn, K = P.K, C = P.C;
  const int g0 = blockIdx.x * P.GB;
  const int ng = (P.B - g0 < P.GB) ? P.B - g0 : P.GB;
  const int rows = ng * N;
  const long row0 = (long)g0 * N;

  const int ar = tid >> 1, ah = tid & 1, ak = ah * 8;
  const int ag = ar / N, an = ar - ag * N;
  const bool alive = ar < rows;
  float cf[KT];
  uint32_t cj[(KT + 3) / 4] = {};
  const int abase = ((alive ? ag * N : 0)) * TG_LD + ak;
  {
    int jj[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const bool use = alive && t < Kn;
      jj[t] = P.nbr ? (int)P.nbr[use ? an * Kn + t : 0] : t;
      jj[t] = use ? jj[t] : -1;
    }
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const int j = jj[t];
      const float c = P.adj[j < 0 ? 0 : (long)(g0 + ag) * P.a_stride + (long)an * P.a_row + (P.a_compact ? t : j)];   // compact rows: term t itself
      cf[t] = j < 0 ? 0.0f : c;
      cj[t >> 2] |= (uint32_t)(j < 0 ? 0 : j) << (8 * (t & 3));
    }
  }

  // staging.  X slab: two 16-byte chunks per thread through registers, as in the float32 kernel.  W slab (T terms x 224 cols x two
  // 16-byte halves = 7 T wave-instructions of 1 KB, 21 for T = 3): LDS-DMA (global_load_lds_dwordx4) -- lane i of instruction j fetches the chunk
  // that belongs at LDS position 64 j + i of the (swizzled) image, no registers, no ds_write.  Every wave issues exactly WD of
  // them (instruction numbers past the last repeat it), so that "at most WD vector-memory operations outstanding" means "everything
  // older than the last W slab has landed".
  constexpr int XC = MT * 4 / NT;                                    // = 2
  constexpr int WI = T * WROWS * 2 / 64;                             // = 7 T wave-instructions per slab: 21, 14, 7
  constexpr int WD = (WI + NW - 1) / NW;                             // per wave, NW = 4 / 8: 6 / 3 (T = 3), 4 / 2 (T = 2), 2 / 1 (T = 1)
  static_assert(WI == 7 * T && WI % T == 0 && WD * NW >= WI && (WD - 1) * NW < WI, "LDS-DMA instructions of a W slab");
  const int uwave = __builtin_amdgcn_readfirstlane(wave);
  tg_f4 rx[XC];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int c = 0; c < XC; ++c) {
      const int q = tid + c * NT, r = q >> 2, kk = k0 + (q & 3) * 4;
      const bool ok = r < rows && kk < K;
      const tg_f4 ld = *(const tg_f4 *)(ok ? P.x + (row0 + r) * P.x_stride + kk : P.x);
      const tg_f4 z = {0.0f, 0.0f, 0.0f, 0.0f};
      rx[c] = ok ? ld : z;
    }
  };
  auto stash_x = [&]() {
#pragma unroll
    for (int c = 0; c < XC; ++c) {
      const int q = tid + c * NT;
      *(tg_f4 *)(sXraw + (q >> 2) * TG_LD + (q & 3) * 4) = rx[c];
    }
  };
  auto dma_w = [&](int k0, int buf) {                                // slabs past the end of K read the zero padding of the last one
    const int kc = k0 < KP ? k0 : KP - TG_KS;                        // (a slab past the end is never multiplied: any valid address)
#pragma unroll
    for (int c = 0; c < WD; ++c) {
      int j = uwave + c * NW;
      j = j < WI ? j : WI - 1;
      const int t = j / (WI / T), rem = (j % (WI / T)) * 64 + lane;  // term; position inside the term's [224][2] image
      const int col = rem >> 1, h = (rem & 1) ^ ((col >> 3) & 1);
      const uint16_t *src = ws + ((long)t * TG_CP + col) * KP + kc + h * 8;
      __builtin_amdgcn_global_load_lds((tg_glob_void *)src, (tg_lds_void *)(sWs + (buf * T * WROWS * 2 + j * 64) * 16), 16, 0, 0);
    }
  };
  auto gather = [&](int t_lo, int t_hi, tg_f4 &a0, tg_f4 &a1) {
#pragma unroll
    for (int tt = t_lo; tt < t_hi; ++tt) {
      const float *src = sXraw + abase + (int)((cj[tt >> 2] >> (8 * (tt & 3))) & 255u) * TG_LD;
      a0 += cf[tt] * *(const tg_f4 *)src;
      a1 += cf[tt] * *(const tg_f4 *)(src + 4);
    }
  };
  auto put_split = [&](int buf, const tg_f4 a0, const tg_f4 a1) {    // this thread's eight k of row ar, the first T terms
    float r[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
    for (int t = 0; t < T; ++t)
      *(tg_u4 *)(sXs + (((buf * T + t) * MT + ar) * 2 + (ah ^ ((ar >> 3) & 1))) * 16) = tg_split_term(r, t == T - 1);
  };

  tg_f16 acc[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[cb][i] = 0.0f;
  const int mrow = wave * 32 + (lane & 31), mh = lane >> 5, mcol = lane & 31;

  // Order of the vector-memory operations of a wave (they complete in order): [W 0] [X 0] [W 1] [X 1] | loop s: [X s+2] [W s+2].
  // Waiting for the registers of X s+2 (stash_x, end of iteration s) therefore implies that W s+1 has landed; the explicit
  // "vmcnt(WD)" in front of the top barrier says the same thing for the reader of this code.  Every wave issues exactly WD LDS-DMA
  // instructions per W slab, whatever T is, and the immediate IS the constant WD: at most the youngest W slab is outstanding.
  const int nslab = (K + TG_KS - 1) / TG_KS;
  dma_w(0, 0);
  fetch(0);
  stash_x();
  dma_w(TG_KS, 1);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WD) : "memory");
  tg_lds_barrier();
  fetch(TG_KS);
  {
    tg_f4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0;
    gather(0, KT, a0, a1);
    put_split(0, a0, a1);
  }
  tg_lds_barrier();
  stash_x();
#ifdef TRUSS_GCN_STAMPS
  unsigned long long acc_t[4] = {0, 0, 0, 0};
  const unsigned long long t_loop0 = clock64();
#endif
  for (int s = 0; s < nslab; ++s) {
    TG_T(ta);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WD) : "memory");
    tg_lds_barrier();                                                // X'[s], raw slab s + 1 and W slab s are in LDS
    TG_T(tb);
    const int buf = s & 1;
    fetch((s + 2) * TG_KS);
    tg_bf8 xa[T];
#pragma unroll
    for (int t = 0; t < T; ++t) xa[t] = *(const tg_bf8 *)(sXs + (((buf * T + t) * MT + mrow) * 2 + (mh ^ ((mrow >> 3) & 1))) * 16);
    tg_f4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0;
    if constexpr (T == 3) {
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int col = cb * 32 + mcol;
        tg_bf8 wb[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) wb[t] = *(const tg_bf8 *)(sWs + (((buf * 3 + t) * WROWS + col) * 2 + (mh ^ ((col >> 3) & 1))) * 16);
        if (cb * 2 < KT) gather(cb * 2, cb * 2 + 2 < KT ? cb * 2 + 2 : KT, a0, a1);   // two terms between the MFMAs of each of the first column blocks
        // small partial products first
        acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[2], wb[0], acc[cb], 0, 0, 0);
        acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[1], wb[1], acc[cb], 0, 0, 0);
        acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[0], wb[2], acc[cb], 0, 0, 0);
        acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[1], wb[0], acc[cb], 0, 0, 0);
        acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[0], wb[1], acc[cb], 0, 0, 0);
        acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[0], wb[0], acc[cb], 0, 0, 0);
      }
    } else {
      // T < 3.  With fewer MFMAs to place between them the scheduler would issue the operand reads of all seven column blocks and
      // every gather read at the top of the slab -- more live registers than the 256 of two waves per SIMD, i.e. spills.  So the
      // column blocks go in four regions {0, 1} {2, 3} {4, 5} {6} with a scheduling barrier behind each: the B operands of the next
      // region are requested before the MFMAs of the present one (in flight over them), nothing moves across a region's end.
      tg_bf8 wb[CB][T];
      auto load_wb = [&](int lo, int hi) {
#pragma unroll
        for (int cb = lo; cb < hi; ++cb) {
          const int col = cb * 32 + mcol;
#pragma unroll
          for (int t = 0; t < T; ++t) wb[cb][t] = *(const tg_bf8 *)(sWs + (((buf * T + t) * WROWS + col) * 2 + (mh ^ ((col >> 3) & 1))) * 16);
        }
      };
      load_wb(0, 2);
#pragma unroll
      for (int r = 0; r < (CB + 1) / 2; ++r) {
        const int lo = 2 * r, hi = lo + 2 < CB ? lo + 2 : CB;
        load_wb(hi, hi + 2 < CB ? hi + 2 : CB);
#pragma unroll
        for (int cb = lo; cb < hi; ++cb) {
          if (cb * 2 < KT) gather(cb * 2, cb * 2 + 2 < KT ? cb * 2 + 2 : KT, a0, a1);
          // the products x_i w_j with i + j <= T - 1, small partial products first
          if constexpr (T == 2) {
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[1], wb[cb][0], acc[cb], 0, 0, 0);
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[0], wb[cb][1], acc[cb], 0, 0, 0);
          }
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[0], wb[cb][0], acc[cb], 0, 0, 0);
          // (nine terms, two products: the four gather terms of a region in flight together are three registers too many for the
          // head epilogue's instantiation -- the two column blocks of a region keep their gathers apart)
          if constexpr (T == 2 && KT > 6) __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    put_split(buf ^ 1, a0, a1);                                      // behind the last operand read of this slab
    TG_T(tc);
    tg_lds_barrier();                                                // everybody is done with sXraw (slab s + 1) and with sWs / sXs [buf]
    TG_T(td);
    dma_w((s + 2) * TG_KS, buf);                                     // W slab s + 2 -> sWs[buf]
    stash_x();                                                       // raw slab s + 2 -> sXraw
#ifdef TRUSS_GCN_STAMPS
    const unsigned long long te = clock64();
    acc_t[0] += tb - ta; acc_t[1] += tc - tb; acc_t[2] += td - tc; acc_t[3] += te - td;
#endif
  }
#ifdef TRUSS_GCN_STAMPS
  if (blockIdx.x == 0 && tid == 0) {
    for (int i = 0; i < 4; ++i) g_gcn_stamps[i] = acc_t[i];
    g_gcn_stamps[4] = clock64() - t_loop0;
    g_gcn_stamps[5] = nslab;
  }
#endif
  // no LDS-DMA may still be in flight when the workgroup ends (or a fused epilogue / the group kernel's next step reuses the LDS)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (EPI != TG_EPI_NONE) {
    tg_fused_epilogue<NW, CB, EPI>(P, acc, tg_smem, rows, row0, g0, ng);
  } else {
    const int act = P.act;
    const bool accum = P.accumulate != 0;
    const int rbase = wave * 32 + 4 * (lane >> 5);
    const long ostride = P.out_stride;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int col = cb * 32 + (lane & 31);
      const bool colok = col < C;
      const float bc = (P.bias && colok) ? P.bias[col] : 0.0f;
      float *po = P.out + (row0 + rbase) * ostride + (colok ? col : 0);
#pragma unroll
      for (int i0 = 0; i0 < 16; i0 += 8) {
        float old[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) old[i] = 0.0f;
        if (accum) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int dr = 8 * ((i0 + i) >> 2) + ((i0 + i) & 3);
            old[i] = po[(rbase + dr < rows ? dr : 0 - rbase) * ostride];
          }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int dr = 8 * ((i0 + i) >> 2) + ((i0 + i) & 3);
          const float v = tg_act(acc[cb][i0 + i] + bc, act) + old[i];
          if (colok && rbase + dr < rows) po[dr * ostride] = v;
        }
      }
    }
  }
