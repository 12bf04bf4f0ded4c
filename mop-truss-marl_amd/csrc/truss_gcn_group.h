// truss_gcn_group.h -- truss_gcn_layer_group: several split-weight GCN layers (truss_gcn.h, truss_gcn_layer_bf3_kernel) in ONE launch.
//
// The layers form n_chains chains of steps_per_chain steps.  Grid = (row tiles, chains): a workgroup owns one row tile of one chain
// and runs the chain's steps one after the other, each step a whole layer in the arithmetic of truss_gcn_layer_bf3_kernel<NW, KT, EPI,
// T> -- coefficient / neighbour registers of that step's adjacency, the slab loop, the epilogue with bias, activation and
// `accumulate`.  Chains do not depend on each other (the layers of one depth of the actors: truss2D_RL.py:86-120, for all three
// agents); the steps of a chain write the same `out` (the five second-level layers of an actor, which only add into one tensor).  A
// later step that accumulates reads what THE SAME THREAD stored in the step before: the epilogue's load and its store of `out` use
// one thread-to-element mapping, so this is program order within a thread.  Nothing new is kept on chip between steps.
//
// The kernel is a COPY of truss_gcn_layer_bf3_kernel inside a loop over the steps, not a shared body: the layer kernel's T = 2,
// KT = 9 instantiations sit at the 256 VGPRs of two waves per SIMD, and its resource report is an invariant of this file (DESIGN.md
// 4.2b has the precedent, 4.2j this kernel).  What differs from the layer kernel:
//   * the layer's descriptor is an element of an array in the kernel arguments, picked by (blockIdx.y, step): uniform over the
//     workgroup, read through scalar loads;
//   * everything derived from the thread index is worked out again at the top of every step, behind an opaque copy of it, so
//     that no step's row / graph / node numbers stay live across another step's slab loop;
//   * between two steps every wave waits for ALL its memory operations and passes a workgroup barrier (below).
#pragma once
#ifdef __HIPCC__

// One step: the layer as the layer kernel takes it, its split-weight image and that image's row length.
// (HEAD and POOL share one argument type, as TgArgs has it)
template <bool FUSED> struct TgGroupStepT {
  typename TgArgs<FUSED ? TG_EPI_HEAD : TG_EPI_NONE>::type L;
  const uint16_t *ws;
  int KP, pad;
};
template <bool FUSED> struct TgGroupArgsT {
  int steps;                                                           // per chain (1 with an epilogue)
  TgGroupStepT<FUSED> step[FUSED ? TRUSS_GCN_GROUP_MAX_EPI : TRUSS_GCN_GROUP_MAX_STEPS];   // [chain][step]
};
template <int EPI> using TgGroupStep = TgGroupStepT<EPI != TG_EPI_NONE>;
template <int EPI> using TgGroupArgs = TgGroupArgsT<EPI != TG_EPI_NONE>;
static_assert(sizeof(TgGroupArgs<TG_EPI_NONE>) <= 4096 && sizeof(TgGroupArgs<TG_EPI_HEAD>) <= 4096, "kernel-argument segment");

template <int NW, int KT, int EPI = TG_EPI_NONE, int T = 3>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2))) void truss_gcn_group_bf3_kernel(const TgGroupArgs<EPI> G) {
  constexpr int MT = 32 * NW, NT = 64 * NW, CB = 7, WROWS = 32 * CB;
  static_assert(WROWS == TG_CP, "split-weight image rows");
  static_assert(T >= 1 && T <= 3, "bf16 terms per operand");
  extern __shared__ __attribute__((aligned(16))) char tg_smem[];
  float *sXraw = (float *)tg_smem;                                   // [MT][TG_LD] float32 raw input rows of a slab
  char *sXs = tg_smem + MT * TG_LD * 4;                              // [2][T][MT][32 B]    split aggregated rows (MFMA A operand)
  char *sWs = sXs + 2 * T * MT * 32;                                 // [2][T][WROWS][32 B] split W slab, [col][k]
  constexpr int XC = MT * 4 / NT;                                    // = 2
  constexpr int WI = T * WROWS * 2 / 64;                             // LDS-DMA wave-instructions per W slab (see the layer kernel)
  constexpr int WD = (WI + NW - 1) / NW;                             // per wave
  static_assert(WI == 7 * T && WI % T == 0 && WD * NW >= WI && (WD - 1) * NW < WI, "LDS-DMA instructions of a W slab");

  // The step count is the same for every chain: the loop and every barrier in it are uniform over the workgroup.  All barriers of
  // the body are at its top level (those of tg_fused_epilogue included); there is no way out of the loop but its end.
  const int nsteps = EPI == TG_EPI_NONE ? G.steps : 1;
  int tid = threadIdx.x;
  for (int step = 0; step < nsteps; ++step) {
    const TgGroupStep<EPI> &D = G.step[blockIdx.y * nsteps + step];
    const typename TgArgs<EPI>::type &P = D.L;
    const uint16_t *__restrict__ ws = D.ws;
    const int KP = D.KP;
    asm volatile("" : "+v"(tid));                                    // opaque (in place, no copy): nothing derived from it is shared between steps
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
        const float c = P.adj[j < 0 ? 0 : (long)(g0 + ag) * P.a_stride + (long)an * N + j];
        cf[t] = j < 0 ? 0.0f : c;
        cj[t >> 2] |= (uint32_t)(j < 0 ? 0 : j) << (8 * (t & 3));
      }
    }

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
      const int kc = k0 < KP ? k0 : KP - TG_KS;
#pragma unroll
      for (int c = 0; c < WD; ++c) {
        int j = uwave + c * NW;
        j = j < WI ? j : WI - 1;
        const int t = j / (WI / T), rem = (j % (WI / T)) * 64 + lane;
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
    auto put_split = [&](int buf, const tg_f4 a0, const tg_f4 a1) {
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

    // the slab loop of the layer kernel, instruction for instruction (its comments say why each wait is where it is)
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
    for (int s = 0; s < nslab; ++s) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WD) : "memory");
      tg_lds_barrier();                                                // X'[s], raw slab s + 1 and W slab s are in LDS
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
          if (cb * 2 < KT) gather(cb * 2, cb * 2 + 2 < KT ? cb * 2 + 2 : KT, a0, a1);
          // small partial products first
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[2], wb[0], acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[1], wb[1], acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[0], wb[2], acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[1], wb[0], acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[0], wb[1], acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[0], wb[0], acc[cb], 0, 0, 0);
        }
      } else {
        // T < 3: the column blocks in four regions with a scheduling barrier behind each, as in the layer kernel
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
            if constexpr (T == 2) {
              acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[1], wb[cb][0], acc[cb], 0, 0, 0);
              acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[0], wb[cb][1], acc[cb], 0, 0, 0);
            }
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[0], wb[cb][0], acc[cb], 0, 0, 0);
            if constexpr (T == 2 && KT > 6) __builtin_amdgcn_sched_barrier(0);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      put_split(buf ^ 1, a0, a1);                                      // behind the last operand read of this slab
      tg_lds_barrier();                                                // everybody is done with sXraw (slab s + 1) and with sWs / sXs [buf]
      dma_w((s + 2) * TG_KS, buf);                                     // W slab s + 2 -> sWs[buf]
      stash_x();                                                       // raw slab s + 2 -> sXraw
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // no LDS-DMA may still be in flight when the epilogue reuses the LDS

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
              old[i] = po[(rbase + dr < rows ? dr : 0 - rbase) * ostride];    // a dead row re-reads the tile's first row
            }
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int dr = 8 * ((i0 + i) >> 2) + ((i0 + i) & 3);
            float v = acc[cb][i0 + i] + bc;
            if (act == 1) v = fmaxf(v, 0.0f);
            else if (act == 2) v = __builtin_amdgcn_rcpf(1.0f + __expf(-v));
            v += old[i];
            if (colok && rbase + dr < rows) po[dr * ostride] = v;
          }
        }
      }
    }
    // Between two steps.  The last iterations of the slab loop still posted slabs past the end of K (LDS-DMA of W, register -> LDS
    // copies of X: DESIGN.md 4.2h) into the LDS the next step's first LDS-DMA / LDS write goes to.  Every wave's own have landed
    // here -- vmcnt(0) lgkmcnt(0), which also covers the epilogue's stores to `out`, all issued above -- and the barrier says so to
    // the rest of the workgroup before any wave starts the next step.  (Behind the last step it is one barrier for nothing.)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
}

// [p, p + n floats) of one chain against every range of a layer of another
static bool tgg_hits(const float *p, int64_t n, const truss_gcn_layer_args_t *a, const truss_gcn_epilogue_t *e) {
  const int64_t R = (int64_t)a->n_batch * a->n_nodes;
  const int64_t nx = (R - 1) * (a->x_row_stride ? a->x_row_stride : a->k_in) + a->k_in;
  const int64_t no = (R - 1) * (a->out_row_stride ? a->out_row_stride : a->c_out) + a->c_out;
  if (tb_gcn_overlap(p, n, a->out, no)) return true;
  if (e) {
    const int64_t n2 = (R - 1) * (e->out2_row_stride ? e->out2_row_stride : e->c2) + e->c2;
    const int64_t np = ((int64_t)a->n_batch - 1) * (e->pool_row_stride ? e->pool_row_stride : a->c_out) + a->c_out;
    if (e->kind == TRUSS_GCN_EPI_HEAD ? tb_gcn_overlap(p, n, e->out2, n2) : tb_gcn_overlap(p, n, e->pool, np)) return true;
  }
  const int64_t nadj = a->a_batch_stride ? ((int64_t)a->n_batch - 1) * a->a_batch_stride + (int64_t)a->n_nodes * a->n_nodes
                                         : (int64_t)a->n_nodes * a->n_nodes;
  if (tb_gcn_overlap(p, n, a->x, nx) || tb_gcn_overlap(p, n, a->adj, nadj) || tb_gcn_overlap(p, n, a->w, (int64_t)a->c_out * a->k_in) ||
      tb_gcn_overlap(p, n, a->bias, a->c_out))
    return true;
  const int64_t kp = (a->k_in + 15) & ~15;
  if (tb_gcn_overlap(p, n, (const float *)a->w_bf16x3, 3 * TG_CP * kp / 2)) return true;          // (bf16: two per float)
  if (a->nbr && tb_gcn_overlap(p, n, (const float *)a->nbr, ((int64_t)a->n_nodes * a->k_nbr + 1) / 2)) return true;
  if (e && e->kind == TRUSS_GCN_EPI_HEAD) {
    const int64_t nadj2 = e->a2_batch_stride ? ((int64_t)a->n_batch - 1) * e->a2_batch_stride + (int64_t)a->n_nodes * a->n_nodes
                                             : (int64_t)a->n_nodes * a->n_nodes;
    if (tb_gcn_overlap(p, n, e->w2, (int64_t)e->c2 * a->c_out) || tb_gcn_overlap(p, n, e->bias2, e->c2) || tb_gcn_overlap(p, n, e->adj2, nadj2))
      return true;
    if (e->nbr2 && tb_gcn_overlap(p, n, (const float *)e->nbr2, ((int64_t)a->n_nodes * e->k_nbr2 + 1) / 2)) return true;
  }
  return false;
}

template <int EPI, int T>
static int tgg_launch(const TgGroupArgs<EPI> &G, int NW, int Kn, unsigned tiles, unsigned chains, hipStream_t st) {
  const size_t MT = 32 * (size_t)NW;
  size_t lds = MT * TG_LD * 4 + 2 * T * MT * 32 + 2 * T * 224 * 32;
  if (EPI != TG_EPI_NONE && lds < tg_epi_lds_bytes(NW)) lds = tg_epi_lds_bytes(NW);
#define TGG_LAUNCH(nw, kt)                                                                                                          \
  do {                                                                                                                              \
    static TbLdsOptIn optin;                                                                                                        \
    if (int rc = optin.ensure((const void *)truss_gcn_group_bf3_kernel<nw, kt, EPI, T>)) return rc;                                 \
    hipLaunchKernelGGL((truss_gcn_group_bf3_kernel<nw, kt, EPI, T>), dim3(tiles, chains), dim3(64 * nw), lds, st, G);               \
  } while (0)
  if (NW == 4) { if (Kn <= 6) TGG_LAUNCH(4, 6); else TGG_LAUNCH(4, 9); }
  else { if (Kn <= 6) TGG_LAUNCH(8, 6); else TGG_LAUNCH(8, 9); }
#undef TGG_LAUNCH
  return TRUSS_OK;
}

// The header has the contract.  Every check is made before anything is launched.
extern "C" int truss_gcn_layer_group(const truss_gcn_layer_args_t *layers, const truss_gcn_epilogue_t *epis, int32_t n_chains,
                                     int32_t steps_per_chain, int32_t bf16_terms, void *stream) {
  const char *what = "truss_gcn_layer_group";
  auto fail = [what](int code, const std::string &msg) { return tb_fail(code, what + msg); };
  if (n_chains < 0 || steps_per_chain < 1) return fail(TRUSS_EINVAL, ": n_chains >= 0, steps_per_chain >= 1");
  if (bf16_terms < 1 || bf16_terms > 3) return fail(TRUSS_EINVAL, ": bf16_terms 1..3");
  if (epis && steps_per_chain != 1) return fail(TRUSS_EINVAL, ": epilogues go with chains of one step");
  if ((int64_t)n_chains * steps_per_chain > TRUSS_GCN_GROUP_MAX_STEPS || (epis && n_chains > TRUSS_GCN_GROUP_MAX_EPI))
    return fail(TRUSS_EINVAL, ": at most " + std::to_string(TRUSS_GCN_GROUP_MAX_STEPS) + " plain layers, " +
                                  std::to_string(TRUSS_GCN_GROUP_MAX_EPI) + " with epilogues");
  if (n_chains == 0) return TRUSS_OK;
  if (!layers) return fail(TRUSS_EINVAL, ": NULL argument");
  const int S = steps_per_chain, L = n_chains * S;
  for (int i = 0; i < L; ++i) {
    const truss_gcn_layer_args_t *a = &layers[i];
    if (int rc = epis ? tb_gcn_fused_check(a, &epis[i]) : tb_gcn_layer_check(a, what, 256, 0, false)) return rc;
    if (!a->w_bf16x3) return fail(TRUSS_EINVAL, ": w_bf16x3 is NULL (the split-weight path only)");
    if (int rc = tb_gcn_bf16x3_check(a)) return rc;
  }
  const truss_gcn_layer_args_t *a0 = &layers[0];
  const int NW = a0->n_nodes > 128 ? 8 : 4;
  const int Kn0 = a0->nbr ? a0->k_nbr : a0->n_nodes;
  for (int i = 1; i < L; ++i) {
    const truss_gcn_layer_args_t *a = &layers[i];
    if (a->n_batch != a0->n_batch || a->n_nodes != a0->n_nodes || (a->nbr == nullptr) != (a0->nbr == nullptr))
      return fail(TRUSS_EINVAL, ": the layers of a group share n_batch, n_nodes and table / dense");
    if (((a->nbr ? a->k_nbr : a->n_nodes) <= 6) != (Kn0 <= 6))
      return fail(TRUSS_EINVAL, ": the layers of a group take one kernel instantiation (<= 6 terms per row, or 7..9)");
    if (epis && epis[i].kind != epis[0].kind) return fail(TRUSS_EINVAL, ": the epilogues of a group are of one kind");
  }
  if (a0->n_batch == 0) return TRUSS_OK;
  const int64_t R = (int64_t)a0->n_batch * a0->n_nodes;
  auto n_x = [R](const truss_gcn_layer_args_t *a) { return (R - 1) * (a->x_row_stride ? a->x_row_stride : a->k_in) + a->k_in; };
  auto n_out = [R](const truss_gcn_layer_args_t *a) { return (R - 1) * (a->out_row_stride ? a->out_row_stride : a->c_out) + a->c_out; };
  for (int c = 0; c < n_chains; ++c) {
    const truss_gcn_layer_args_t *h = &layers[c * S];
    for (int s = 1; s < S; ++s) {
      const truss_gcn_layer_args_t *a = h + s;
      if (a->out != h->out || a->out_row_stride != h->out_row_stride || a->c_out != h->c_out)
        return fail(TRUSS_EINVAL, ": the steps of a chain write one out (out, out_row_stride, c_out)");
      // (every step writes the chain's out: "the out of an earlier step" is that range)
      if (tb_gcn_overlap(a->x, n_x(a), h->out, n_out(h))) return fail(TRUSS_EINVAL, ": a step's x overlaps the out of an earlier step of its chain");
    }
    // the chain's outputs against everything another chain reads or writes
    for (int o = 0; o < n_chains; ++o) {
      if (o == c) continue;
      for (int s = 0; s < S; ++s) {
        const truss_gcn_layer_args_t *b = &layers[o * S + s];
        const truss_gcn_epilogue_t *eb = epis ? &epis[o] : nullptr;
        bool hit = tgg_hits(h->out, h->out ? n_out(h) : 0, b, eb);
        if (epis) {
          const truss_gcn_epilogue_t *e = &epis[c];
          const int64_t n2 = (R - 1) * (e->out2_row_stride ? e->out2_row_stride : e->c2) + e->c2;
          const int64_t np = ((int64_t)h->n_batch - 1) * (e->pool_row_stride ? e->pool_row_stride : h->c_out) + h->c_out;
          hit = hit || (e->kind == TRUSS_GCN_EPI_HEAD ? tgg_hits(e->out2, n2, b, eb) : tgg_hits(e->pool, np, b, eb));
        }
        if (hit) return fail(TRUSS_EINVAL, ": an output of one chain overlaps an input or output of another chain");
      }
    }
  }
  const unsigned tiles = (unsigned)((a0->n_batch + (32 * NW) / a0->n_nodes - 1) / ((32 * NW) / a0->n_nodes));
  hipStream_t st = (hipStream_t)stream;
  int rc;
#define TGG_TERMS(epi, G) (bf16_terms == 3 ? tgg_launch<epi, 3>(G, NW, Kn0, tiles, (unsigned)n_chains, st)       \
                           : bf16_terms == 2 ? tgg_launch<epi, 2>(G, NW, Kn0, tiles, (unsigned)n_chains, st)     \
                                             : tgg_launch<epi, 1>(G, NW, Kn0, tiles, (unsigned)n_chains, st))
  if (!epis) {
    TgGroupArgs<TG_EPI_NONE> G;
    G.steps = S;
    for (int i = 0; i < L; ++i) {
      G.step[i].L = tg_layer_dev(&layers[i], 32 * NW);
      G.step[i].ws = layers[i].w_bf16x3;
      G.step[i].KP = (layers[i].k_in + 15) & ~15;
      G.step[i].pad = 0;
    }
    for (int i = L; i < TRUSS_GCN_GROUP_MAX_STEPS; ++i) G.step[i] = G.step[0];
    rc = TGG_TERMS(TG_EPI_NONE, G);
  } else {
    TgGroupArgs<TG_EPI_HEAD> G;
    G.steps = 1;
    for (int i = 0; i < L; ++i) {
      G.step[i].L = tg_fused_dev(&layers[i], &epis[i], 32 * NW);
      G.step[i].ws = layers[i].w_bf16x3;
      G.step[i].KP = (layers[i].k_in + 15) & ~15;
      G.step[i].pad = 0;
    }
    for (int i = L; i < TRUSS_GCN_GROUP_MAX_EPI; ++i) G.step[i] = G.step[0];
    rc = epis[0].kind == TRUSS_GCN_EPI_HEAD ? TGG_TERMS(TG_EPI_HEAD, G) : TGG_TERMS(TG_EPI_POOL, G);
  }
#undef TGG_TERMS
  if (rc) return rc;
  return tb_launched("gcn layer group kernel launch failed: ");
}
#endif  // __HIPCC__
