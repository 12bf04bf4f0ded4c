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
// The kernel is truss_gcn_bf3_body.h, the body of truss_gcn_layer_bf3_kernel, inside a loop over the steps: one text for the
// layer's arithmetic, so group == layers bit for bit by construction (tests/test_gcn_group.py still pins it).  The layer kernel's
// T = 2, KT = 9 instantiations sit at the 256 VGPRs of two waves per SIMD; with the shared text all 72 instantiations keep their
// VGPR count, occupancy and LDS (profiles/r16/README.md).  What this kernel adds to the body:
//   * the layer's descriptor is an element of an array in the kernel arguments, picked by (blockIdx.y, step): uniform over the
//     workgroup, read through scalar loads;
//   * the thread index the body reads is made opaque (in place) at the top of every step, so that everything derived from it is
//     worked out again and no step's row / graph / node numbers stay live across another step's slab loop;
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
    {
#include "truss_gcn_bf3_body.h"
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
  const int64_t arow = a->adj_layout == TRUSS_GCN_ADJ_COMPACT ? a->k_nbr : a->n_nodes;     // floats per row of adj
  const int64_t nadj = a->a_batch_stride ? ((int64_t)a->n_batch - 1) * a->a_batch_stride + (int64_t)a->n_nodes * arow
                                         : (int64_t)a->n_nodes * arow;
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
  const size_t lds = tg_bf3_lds_bytes(NW, T, EPI != TG_EPI_NONE);
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
#define TGG_TERMS(epi, G) TG_BY_TERMS(bf16_terms, tgg_launch, epi, G, NW, Kn0, tiles, (unsigned)n_chains, st)
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
