// truss_gcn.h -- one whole GCN layer on the matrix cores (gfx950): out[b] = act(A[b] (X[b] W^T) + bias), Spektral GCNConv as the
// reference's actors / critics use it (truss2D_RL.py:49-127: 13 layers per actor, 21 per critic, hidden width 200).
//
// Evaluated as ((A X) W^T): the neighbourhood sum is applied to the INPUT rows on their way into LDS (a row of A has <= 9
// non-zeros on a truss -- the sparsity pattern of every node-graph adjacency the reference builds -- or N <= 64 dense entries on the
// Pareto graph), the product with W^T runs on v_mfma_f32_32x32x2_f32 with float32 accumulation, bias / activation (/ accumulation into
// `out`) sit in the epilogue.  H = X W never exists in HBM, and the [M, C] result is written exactly once.
//
// Tiling.  A workgroup of NW wavefronts owns MT = 32 NW rows = whole graphs (GB = MT / N graphs of N nodes; the 256-node class takes
// NW = 8, everything else NW = 4) and ALL c_out <= 32 CB columns (CB = 7 column blocks for the hidden width 200, 1 for the action
// heads): wave w accumulates the 32 x (32 CB) block of its 32 rows in 16 CB accumulator registers.  K is streamed in slabs of 16:
//   global -> registers (next slab: X rows as 64-byte pieces, W rows as 64-byte pieces of nn.Linear's [c_out][k_in] layout)
//   registers -> LDS (raw X slab, W slab [col][16 k])          | barrier
//   aggregate: X'[r][k] = sum_t coef[r][t] * Xraw[row(r, t)][k]  (VALU, from LDS to LDS)      | barrier
//   MFMA: lane (row | col = l % 32, half h = l / 32) holds k = 8 h .. 8 h + 7 of its row / column (two ds_read_b128); step s of the
//         eight multiplies k = s (lanes of half 0) and k = 8 + s (half 1): the order of a sum over k is free.
// W (160 KB at 200 x 200) is re-read by every workgroup from L2; X is read once, `out` written once.
//
// On top the argument checks of truss_gcn_layer and truss_gcn_level (truss_gcn_level.h), shared with the plain loops of the CPU
// test backend in tests/emu/truss_emu.cpp; below them, for the device compiler only, the kernels, their dispatch and the C entries.
#pragma once
#include <cstdint>
#include <string>

static int tb_fail(int code, const std::string &msg);

#define TG_LEVEL_MAX_K_IN 256    // truss_gcn_level: the kernel's TGL_SLABS slabs of TGL_KS k's (truss_gcn_level.h asserts it)
#define TG_KREG 9                // neighbourhood terms per row held in registers (a truss node joins <= 8 elements: <= 9 terms with the diagonal)

// One layer's argument block as entry `what` takes it: truss_gcn_layer (n_nodes <= 256, any k_in: max_k_in 0), or -- `level` -- a layer of
// truss_gcn_level (128, TG_LEVEL_MAX_K_IN), where an empty layer passes unread and there is neither accumulation into out nor a
// split-weight product.  The two `level` rules sit where truss_gcn_level has always applied them: the order of the checks decides
// which text a doubly invalid block gets, and that text is part of the library's behaviour.
static inline int tb_gcn_layer_check(const truss_gcn_layer_args_t *a, const char *what, int max_nodes, int max_k_in, bool level) {
  auto fail = [what](int code, const std::string &msg) { return tb_fail(code, what + msg); };
  if (a->struct_size != sizeof(truss_gcn_layer_args_t)) return tb_fail(TRUSS_EINVAL, "truss_gcn_layer_args_t size mismatch (ABI)");
  if (level && a->n_batch == 0) return TRUSS_OK;           // nothing to read, nothing to write
  if (!a->x || !a->adj || !a->w || !a->out) return fail(TRUSS_EINVAL, ": a required pointer is NULL");
  if (a->n_batch < 0 || a->n_nodes < 1 || a->k_in < 1 || a->c_out < 1 || a->act < 0 || a->act > 2) return fail(TRUSS_EINVAL, ": bad sizes / act");
  if (level && (a->accumulate || a->w_bf16x3)) return fail(TRUSS_EUNSUPPORTED, ": float32 product, no accumulation into out");
  if (a->c_out > 224) return fail(TRUSS_EUNSUPPORTED, level ? ": c_out <= 224" : ": c_out <= 224 (the reference's hidden width is 200)");
  if (a->n_nodes > max_nodes) return fail(TRUSS_EUNSUPPORTED, ": n_nodes <= " + std::to_string(max_nodes));
  if (max_k_in && a->k_in > max_k_in) return fail(TRUSS_EUNSUPPORTED, ": k_in <= " + std::to_string(max_k_in));
  if (a->nbr ? (a->k_nbr < 1 || a->k_nbr > 16) : a->n_nodes > 64)
    return fail(TRUSS_EUNSUPPORTED, ": a sparsity pattern of 1..16 terms per row, or a dense adjacency of at most 64 nodes");
  if (a->x == a->out) return fail(TRUSS_EINVAL, ": out must not alias x");
  // adj_layout: 0 dense rows of n_nodes, 1 compact rows of k_nbr (term t of row i at adj[i * k_nbr + t]); the layer kernels only
  if (a->adj_layout != TRUSS_GCN_ADJ_DENSE && a->adj_layout != TRUSS_GCN_ADJ_COMPACT) return fail(TRUSS_EINVAL, ": adj_layout is 0 (dense) or 1 (compact)");
  if (a->adj_layout == TRUSS_GCN_ADJ_COMPACT) {
    if (!a->nbr) return fail(TRUSS_EINVAL, ": a compact adjacency needs its neighbour table (nbr)");
    if (a->a_batch_stride != 0 && a->a_batch_stride != (int64_t)a->n_nodes * a->k_nbr)
      return fail(TRUSS_EINVAL, ": a compact adjacency has a_batch_stride n_nodes * k_nbr, or 0");
    if (level) return fail(TRUSS_EUNSUPPORTED, ": dense adjacencies only");
#ifndef __HIPCC__
    return fail(TRUSS_EUNSUPPORTED, ": this backend reads dense adjacencies only");   // the plain loops of the CPU test backend
#endif
  }
  return TRUSS_OK;
}

// x may be read in 16-byte pieces: alignment, and every 4-float chunk of a row whole or past the end
static inline bool tb_gcn_x_vec(const truss_gcn_layer_args_t *a) {
  return (size_t)a->x % 16 == 0 && (a->x_row_stride ? a->x_row_stride : a->k_in) % 4 == 0 && a->k_in % 4 == 0;
}

// The envelope of the bf16x3 product (truss_gcn_layer with split weights).  A shape outside it is an error, not a silent change of
// arithmetic: the caller asked for this path by passing split weights.
static inline int tb_gcn_bf16x3_check(const truss_gcn_layer_args_t *a) {
  if (a->c_out <= 32 || !tb_gcn_x_vec(a) || (a->nbr ? a->k_nbr : a->n_nodes) > TG_KREG || ((size_t)a->w_bf16x3 & 15) != 0)
    return tb_fail(TRUSS_EUNSUPPORTED, "truss_gcn_layer: the bf16x3 path takes c_out 33..224, k_in % 4 == 0, 16-byte aligned x / split weights, <= 9 terms per row");
  return TRUSS_OK;
}

// [p, p + n floats) and [q, q + m floats) share a byte
static inline bool tb_gcn_overlap(const float *p, int64_t n, const float *q, int64_t m) {
  return p && q && n > 0 && m > 0 && (uintptr_t)p < (uintptr_t)(q + m) && (uintptr_t)q < (uintptr_t)(p + n);
}

// The argument blocks of truss_gcn_layer_fused: the epilogue's own fields, then the layer through tb_gcn_layer_check as truss_gcn_layer
// takes it -- except that `out` may be NULL (the check then sees the epilogue's result in its place) and nothing accumulates.
static inline int tb_gcn_fused_check(const truss_gcn_layer_args_t *a, const truss_gcn_epilogue_t *e) {
  const char *what = "truss_gcn_layer_fused";
  auto fail = [what](int code, const std::string &msg) { return tb_fail(code, what + msg); };
  if (a->struct_size != sizeof(truss_gcn_layer_args_t)) return tb_fail(TRUSS_EINVAL, "truss_gcn_layer_args_t size mismatch (ABI)");
  if (e->struct_size != sizeof(truss_gcn_epilogue_t)) return tb_fail(TRUSS_EINVAL, "truss_gcn_epilogue_t size mismatch (ABI)");
  const bool head = e->kind == TRUSS_GCN_EPI_HEAD;
  if (!head && e->kind != TRUSS_GCN_EPI_POOL) return fail(TRUSS_EINVAL, ": unknown epilogue kind");
  if (head) {
    if (!e->w2 || !e->adj2 || !e->out2) return fail(TRUSS_EINVAL, ": a required pointer of the head is NULL");
    if (e->c2 < 1 || e->c2 > 8 || e->act2 < 0 || e->act2 > 2) return fail(TRUSS_EINVAL, ": c2 1..8, act2 0..2");
  } else if (!e->pool) {
    return fail(TRUSS_EINVAL, ": pool is NULL");
  }
  if (a->accumulate) return fail(TRUSS_EINVAL, ": no accumulation into out");
  float *res = head ? e->out2 : e->pool;
  truss_gcn_layer_args_t c = *a;
  if (!c.out) c.out = res;
  if (int rc = tb_gcn_layer_check(&c, what, 256, 0, false)) return rc;
  if (head && (e->nbr2 ? (e->k_nbr2 < 1 || e->k_nbr2 > 16) : a->n_nodes > 64))
    return fail(TRUSS_EUNSUPPORTED, ": head: a sparsity pattern of 1..16 terms per row, or a dense adjacency of at most 64 nodes");
  if (a->n_batch == 0) return TRUSS_OK;
  const int64_t R = (int64_t)a->n_batch * a->n_nodes;
  const int64_t nx = (R - 1) * (a->x_row_stride ? a->x_row_stride : a->k_in) + a->k_in;
  const int64_t no = (R - 1) * (a->out_row_stride ? a->out_row_stride : a->c_out) + a->c_out;
  const int64_t n2 = (R - 1) * (e->out2_row_stride ? e->out2_row_stride : e->c2) + e->c2;
  const int64_t np = ((int64_t)a->n_batch - 1) * (e->pool_row_stride ? e->pool_row_stride : a->c_out) + a->c_out;
  const int64_t nr = head ? n2 : np;
  if (tb_gcn_overlap(res, nr, a->x, nx) || tb_gcn_overlap(res, nr, a->out, no) || tb_gcn_overlap(e->out2, n2, e->pool, np))
    return fail(TRUSS_EINVAL, ": out2 / pool must not overlap x, out or each other");
  return TRUSS_OK;
}

#ifdef __HIPCC__
typedef float tg_f4 __attribute__((ext_vector_type(4)));
typedef float tg_f16 __attribute__((ext_vector_type(16)));

struct GcnLayerDev {
  const float *x;
  const float *adj;
  const int16_t *nbr;
  const float *w;
  const float *bias;
  float *out;
  long x_stride, out_stride, a_stride;     // floats between rows of x / out; between graphs of adj (0: one adjacency for all)
  int B, N, K, C, act, accumulate;
  int Kn;                                  // terms per row: k_nbr (pattern) or N (dense)
  int GB;                                  // graphs per tile
  int x_vec, w_vec;                        // 16-byte loads allowed (alignment + k_in % 4 == 0)
  int a_compact, a_row;                    // adj rows hold the Kn terms themselves (adj_layout 1), not N columns; floats per row of adj: Kn / N
};

#define TG_KS 16                 // K slab
#define TG_LD 20                 // floats per LDS row of a slab (16 + 4 padding: rows 80 bytes apart)

// Workgroup barrier for data handed over THROUGH LDS: waits for this wave's LDS operations only.  __syncthreads() also waits for
// vmcnt(0), i.e. for the global loads of the slab after next that are meant to stay in flight across the barrier.
__device__ __forceinline__ void tg_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// the activation of the C ABI: 0 none, 1 relu, 2 sigmoid (`act` is uniform)
__device__ __forceinline__ float tg_act(float v, int act) {
  if (act == 1) v = fmaxf(v, 0.0f);
  else if (act == 2) v = __builtin_amdgcn_rcpf(1.0f + __expf(-v));
  return v;
}

// The first KT terms of row `an` of an adjacency in registers: coefficients cf[], source nodes cj[] (one byte each, n_nodes <= 256;
// the caller zeroes cj).  adj_row_offset: float offset of the row in adj.  Branch-free, so that the KT table reads and then the KT
// coefficient reads are in flight together (a dead row / a term past Kn reads entry 0 and is masked afterwards).
// compact (uniform): the row holds its Kn terms in table order -- term t lies at adj_row_offset + t, its source node is still nbr's.
template <int KT>
__device__ __forceinline__ void tg_load_terms(const int16_t *nbr, const float *adj, long adj_row_offset, int an, int Kn, bool alive,
                                              float (&cf)[KT], uint32_t (&cj)[(KT + 3) / 4], bool compact = false) {
  int jj[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const bool use = alive && t < Kn;
    jj[t] = nbr ? (int)nbr[use ? an * Kn + t : 0] : t;
    jj[t] = use ? jj[t] : -1;
  }
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const int j = jj[t];
    const float c = adj[j < 0 ? 0 : adj_row_offset + (compact ? t : j)];
    cf[t] = j < 0 ? 0.0f : c;
    cj[t >> 2] |= (uint32_t)(j < 0 ? 0 : j) << (8 * (t & 3));            // a missing term re-reads a live row with coefficient 0
  }
}

// ---- a consumer of the layer's output in the epilogue of the same launch (truss_gcn_layer_fused) ----
// The epilogue mode is a template parameter of both kernels; TG_EPI_NONE is the layer as truss_gcn_layer launches it, with the
// argument block it has always had.  The other two hand the output V = act(acc + bias) over through LDS, one 32-column block
// at a time (MT x 32 floats in the LDS the slab loop has finished with), to threads that own whole output elements:
//   HEAD  thread (row, 16-column half) extends its partial sums of h2 = V W2^T, c2 <= 8 of them, block after block; the two
//         halves are added, h2 [MT][8] goes to LDS, and thread (row, four of the c2 columns) forms act2(sum_t A2[r][t] h2[row(r, t)]
//         + b2) -- through LDS for every shape, since a graph's rows lie in several waves;
//   POOL  thread (graph, column) adds the N rows of its graph in row order and writes pool[b][c].
// One owner per element, a fixed order of every sum, no atomics.  V itself is written to `out` only when out != NULL.
#define TG_EPI_NONE 0
#define TG_EPI_HEAD 1            // = TRUSS_GCN_EPI_HEAD
#define TG_EPI_POOL 2            // = TRUSS_GCN_EPI_POOL
static_assert(TG_EPI_HEAD == TRUSS_GCN_EPI_HEAD && TG_EPI_POOL == TRUSS_GCN_EPI_POOL, "epilogue kinds of the C ABI");
#define TG_VLD 36                // floats per LDS row of a 32-column block of V (32 + 4 padding: rows 144 bytes apart)
#define TG_W2LD 224              // floats per LDS row of W2 (c_out padded to the 7 column blocks, zeros)

struct GcnFusedDev : GcnLayerDev {
  const float *w2, *bias2, *adj2;
  const int16_t *nbr2;
  float *out2, *pool;
  long a2_stride, out2_stride, pool_stride;
  int c2, act2, Kn2;
};
template <int EPI> struct TgArgs { typedef GcnFusedDev type; };
template <> struct TgArgs<TG_EPI_NONE> { typedef GcnLayerDev type; };

static size_t tg_epi_lds_bytes(int NW) { return sizeof(float) * ((size_t)32 * NW * (TG_VLD + 8) + 8 * TG_W2LD); }

// All barriers of the epilogue are at the top level of this function (the loop over the column blocks is unrolled), and the kernels
// call it outside every branch: every wave of the workgroup passes every one of them.
template <int NW, int CB, int EPI>
__device__ __forceinline__ void tg_fused_epilogue(const GcnFusedDev &P, const tg_f16 (&acc)[CB], char *smem, int rows, long row0, int g0, int ng) {
  constexpr int MT = 32 * NW, NT = 64 * NW;
  float *sV = (float *)smem;                               // [MT][TG_VLD]  one 32-column block of V
  float *sW2 = sV + MT * TG_VLD;                           // [8][TG_W2LD]  W2, zero rows / columns past c2 / c_out
  float *sH = sW2 + 8 * TG_W2LD;                           // [MT][8]       h2 = V W2^T
  // (opaque to the optimiser: the row / graph / node numbers below are worked out again here.  Shared with the copies from before
  // the slab loop, they would stay live across it, and the float32 loop has no register to spare.)
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, wave = tid >> 6;
  const int N = P.N, C = P.C, c2 = P.c2, Kn2 = P.Kn2;
  // The last iterations of the slab loops still post slabs past the end of K (register -> LDS copies, LDS-DMA): they must have
  // landed in EVERY wave before the first write of the epilogue reuses that LDS.
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");

  // item of this thread: row ar, half ah (HEAD: columns 16 ah .. of every block, then the head's columns 4 ah ..)
  const int ar = tid >> 1, ah = tid & 1;
  const int ag = ar / N, an = ar - ag * N;
  const bool alive = ar < rows;
  const bool kreg2 = Kn2 <= TG_KREG;                       // uniform
  float cf2[TG_KREG], hs[8];
  uint32_t cj2[(TG_KREG + 3) / 4] = {};
#pragma unroll
  for (int t = 0; t < TG_KREG; ++t) cf2[t] = 0.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j) hs[j] = 0.0f;
  if constexpr (EPI == TG_EPI_HEAD) {
    for (int i = tid; i < 8 * TG_W2LD; i += NT) {
      const int j = i / TG_W2LD, c = i - j * TG_W2LD;
      const bool ok = j < c2 && c < C;
      const float w = P.w2[ok ? j * C + c : 0];
      sW2[i] = ok ? w : 0.0f;
    }
    if (kreg2)                                             // A2's terms of this row: in flight over the rounds below
      tg_load_terms<TG_KREG>(P.nbr2, P.adj2, (long)(g0 + ag) * P.a2_stride + (long)an * N, an, Kn2, alive, cf2, cj2);
  }

  const int act = P.act;
  const int rbase = wave * 32 + 4 * (lane >> 5);            // row of accumulator register 0; register i: + 8 (i / 4) + i % 4
  const long ostride = P.out_stride;
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int col = cb * 32 + (lane & 31);
    const bool colok = col < C;
    const float bc = (P.bias && colok) ? P.bias[col] : 0.0f;
    float *po = P.out + (row0 + rbase) * ostride + (colok ? col : 0);
    const bool store = P.out != nullptr && colok;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int dr = 8 * (i >> 2) + (i & 3);
      const float v = tg_act(acc[cb][i] + bc, act);
      sV[(rbase + dr) * TG_VLD + (lane & 31)] = colok ? v : 0.0f;
      if (store && rbase + dr < rows) po[dr * ostride] = v;
    }
    tg_lds_barrier();                                       // the block (and, first round, W2) is in LDS
    if constexpr (EPI == TG_EPI_HEAD) {
      if (alive) {
        const float *pv = sV + ar * TG_VLD + ah * 16;
        const float *pw = sW2 + cb * 32 + ah * 16;
        tg_f4 v4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v4[q] = *(const tg_f4 *)(pv + 4 * q);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (j < c2) {                                     // uniform
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const tg_f4 w4 = *(const tg_f4 *)(pw + j * TG_W2LD + 4 * q);
#pragma unroll
              for (int e = 0; e < 4; ++e) hs[j] += v4[q][e] * w4[e];
            }
          }
        }
      }
    } else {
      for (int it = tid; it < ng * 32; it += NT) {          // (graph, column) of the block
        const int g = it >> 5, c = it & 31;
        if (cb * 32 + c < C) {
          const float *pv = sV + (g * N) * TG_VLD + c;
          float s = 0.0f;
          for (int n = 0; n < N; ++n) s += pv[n * TG_VLD];
          P.pool[(long)(g0 + g) * P.pool_stride + cb * 32 + c] = s;
        }
      }
    }
    tg_lds_barrier();                                       // everybody is done with the block
  }

  if constexpr (EPI == TG_EPI_HEAD) {
#pragma unroll
    for (int j = 0; j < 8; ++j) hs[j] += __shfl_xor(hs[j], 1);          // the other half's 16 columns of every block
    if (alive) {
      const tg_f4 lo = {hs[0], hs[1], hs[2], hs[3]}, hi = {hs[4], hs[5], hs[6], hs[7]};
      *(tg_f4 *)(sH + ar * 8 + ah * 4) = ah ? hi : lo;
    }
    tg_lds_barrier();                                       // h2 of every live row is in LDS
    if (alive && ah * 4 < c2) {
      const float *hb = sH + (ag * N) * 8 + ah * 4;
      tg_f4 s = {0.0f, 0.0f, 0.0f, 0.0f};
      if (kreg2) {
#pragma unroll
        for (int t = 0; t < TG_KREG; ++t)
          s += cf2[t] * *(const tg_f4 *)(hb + (int)((cj2[t >> 2] >> (8 * (t & 3))) & 255u) * 8);
      } else {
        for (int t = 0; t < Kn2; ++t) {
          const int j = P.nbr2 ? (int)P.nbr2[an * Kn2 + t] : t;
          if (j < 0) continue;
          s += P.adj2[(long)(g0 + ag) * P.a2_stride + (long)an * N + j] * *(const tg_f4 *)(hb + j * 8);
        }
      }
      const int act2 = P.act2;
      float *po2 = P.out2 + (row0 + ar) * P.out2_stride;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = ah * 4 + q;
        if (j < c2) po2[j] = tg_act(s[q] + (P.bias2 ? P.bias2[j] : 0.0f), act2);
      }
    }
  }
}

// The plain epilogue of the float32 layer kernel (truss_gcn_bf3_body.h has the same statements written out): accumulator
// register i of a lane = row 8 (i / 4) + 4 (l / 32) + i % 4, column l % 32 of the 32 x 32 block.
// Per column block: (accumulate: the 16 old values, from clamped addresses, in flight together) -> bias, activation
// -> 16 predicated stores; 32 lanes write 128 contiguous bytes of a row.  `act` / `accumulate` are uniform.
template <int CB>
__device__ __forceinline__ void tg_store_epilogue(const GcnLayerDev &P, const tg_f16 (&acc)[CB], int rows, long row0, int lane, int wave) {
  const int C = P.C, act = P.act;
  const bool accum = P.accumulate != 0;
  const int rbase = wave * 32 + 4 * (lane >> 5);            // row of accumulator register 0; register i: + 8 (i / 4) + i % 4
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
          old[i] = po[(rbase + dr < rows ? dr : 0 - rbase) * ostride];      // a dead row re-reads the tile's first row
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

#ifdef TRUSS_GCN_STAMPS   // diagnostic build: cycles of the slab loop's sections, block 0 / wave 0 (tools/gcn_stamps.py)
__device__ unsigned long long g_gcn_stamps[8];
#define TG_T(v) unsigned long long v = clock64()
#else
#define TG_T(v)
#endif

// VEC: x and w are 16-byte aligned with k_in % 4 == 0 -- every 4-float chunk of a slab is either whole or past the end, so the loads
// are branch-free 16-byte loads from clamped addresses; otherwise (the 13-feature input layers) element-wise guarded loads.
template <int NW, int CB, bool VEC, int EPI = TG_EPI_NONE>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2))) void truss_gcn_layer_kernel(const typename TgArgs<EPI>::type P) {
  constexpr int MT = 32 * NW, NT = 64 * NW, WROWS = 32 * CB;
  extern __shared__ __attribute__((aligned(16))) char tg_smem[];
  float *sXraw = (float *)tg_smem;                         // [MT][TG_LD]       raw input rows of a slab
  float *sXa = sXraw + MT * TG_LD;                         // [2][MT][TG_LD]    aggregated rows (MFMA A operand)
  float *sW = sXa + 2 * MT * TG_LD;                        // [2][WROWS][TG_LD] W slab, [col][k]
  float *sCoef = sW + 2 * WROWS * TG_LD;                   // [MT][Kn]          (only read from LDS when Kn > TG_KREG)
  int16_t *sIdx = (int16_t *)(sCoef + MT * P.Kn);          // [N][Kn]           source node of term t (-1: none)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = P.N, Kn = P.Kn, K = P.K, C = P.C;
  const int g0 = blockIdx.x * P.GB;
  const int ng = (P.B - g0 < P.GB) ? P.B - g0 : P.GB;
  const int rows = ng * N;                                 // live rows of this tile (<= MT)
  const long row0 = (long)g0 * N;

  // ---- aggregation item of this thread: row ar, eight k's from ak (MT * 2 items, NT = 2 MT threads) ----
  const int ar = tid >> 1, ak = (tid & 1) * 8;
  const int ag = ar / N, an = ar - ag * N;                 // graph in the tile, node
  const bool alive = ar < rows;
  const bool kreg = Kn <= TG_KREG;                         // uniform
  float cf[TG_KREG];
  uint32_t cj[(TG_KREG + 3) / 4] = {};                     // source nodes of the terms, one byte each (n_nodes <= 256)
  const int abase = ((alive ? ag * N : 0)) * TG_LD + ak;   // float offset of the graph's first row (this thread's eight k's) in sXraw
  if (kreg) {
    tg_load_terms<TG_KREG>(P.nbr, P.adj, (long)(g0 + ag) * P.a_stride + (long)an * P.a_row, an, Kn, alive, cf, cj, P.a_compact != 0);
  } else {
    for (int i = tid; i < N * Kn; i += NT) sIdx[i] = P.nbr ? P.nbr[i] : (int16_t)(i % Kn);
    for (int i = tid; i < rows * Kn; i += NT) {
      const int r = i / Kn, t = i - r * Kn, g = r / N, n = r - g * N;
      const int j = P.nbr ? (int)P.nbr[n * Kn + t] : t;
      sCoef[i] = j < 0 ? 0.0f : P.adj[(long)(g0 + g) * P.a_stride + (long)n * P.a_row + (P.a_compact ? t : j)];
    }
  }

  // ---- staging: X slab = MT * 4 chunks of 4 floats (chunk q -> row q / 4, k (q % 4) * 4), two per thread; W slab = WROWS * 4 chunks ----
  constexpr int XC = MT * 4 / NT;                          // = 2
  constexpr int WC = (WROWS * 4 + NT - 1) / NT;
  tg_f4 rx[XC], rw[WC];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int c = 0; c < XC; ++c) {
      const int q = tid + c * NT, r = q >> 2, kk = k0 + (q & 3) * 4;
      tg_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (VEC) {
        const bool ok = r < rows && kk < K;
        const tg_f4 ld = *(const tg_f4 *)(ok ? P.x + (row0 + r) * P.x_stride + kk : P.x);    // always a valid address, no branch
        v = ok ? ld : v;
      } else if (r < rows) {
        const float *src = P.x + (row0 + r) * P.x_stride + kk;
        if (kk + 0 < K) v[0] = src[0];
        if (kk + 1 < K) v[1] = src[1];
        if (kk + 2 < K) v[2] = src[2];
        if (kk + 3 < K) v[3] = src[3];
      }
      rx[c] = v;
    }
#pragma unroll
    for (int c = 0; c < WC; ++c) {
      const int q = tid + c * NT, col = q >> 2, kk = k0 + (q & 3) * 4;
      tg_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (VEC) {
        const bool ok = col < C && kk < K;                 // (q >= WROWS * 4 implies col >= 32 CB >= C)
        const tg_f4 ld = *(const tg_f4 *)(ok ? P.w + (long)col * K + kk : P.w);
        v = ok ? ld : v;
      } else if (col < C) {
        const float *src = P.w + (long)col * K + kk;
        if (kk + 0 < K) v[0] = src[0];
        if (kk + 1 < K) v[1] = src[1];
        if (kk + 2 < K) v[2] = src[2];
        if (kk + 3 < K) v[3] = src[3];
      }
      rw[c] = v;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int c = 0; c < XC; ++c) {
      const int q = tid + c * NT;
      *(tg_f4 *)(sXraw + (q >> 2) * TG_LD + (q & 3) * 4) = rx[c];
    }
#pragma unroll
    for (int c = 0; c < WC; ++c) {
      const int q = tid + c * NT;
      if (q < WROWS * 4) *(tg_f4 *)(sW + (buf * WROWS + (q >> 2)) * TG_LD + (q & 3) * 4) = rw[c];
    }
  };
  // X'[ar][ak .. ak + 7] of the slab in sXraw -> sXa[buf]
  auto aggregate = [&](int buf) {
    tg_f4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0;
    if (kreg) {
      // all TG_KREG terms, no branch (terms past Kn have coefficient 0 and re-read a live row): the loop body below must stay ONE
      // basic block so that the scheduler can spread these reads and multiply-adds between the MFMAs of the previous slab
#pragma unroll
      for (int t0 = 0; t0 < TG_KREG; t0 += 3) {
        tg_f4 v0[3], v1[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const int tt = t0 + t;
          const float *src = sXraw + abase + (int)((cj[tt >> 2] >> (8 * (tt & 3))) & 255u) * TG_LD;
          v0[t] = *(const tg_f4 *)src;
          v1[t] = *(const tg_f4 *)(src + 4);
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          a0 += cf[t0 + t] * v0[t];
          a1 += cf[t0 + t] * v1[t];
        }
      }
    } else if (alive) {
      const float *cfl = sCoef + ar * Kn;
      const int16_t *ix = sIdx + an * Kn;
      const float *base = sXraw + (ag * N) * TG_LD + ak;
      for (int t = 0; t < Kn; ++t) {
        const int j = ix[t];
        if (j < 0) continue;
        const float c = cfl[t];
        a0 += c * *(const tg_f4 *)(base + j * TG_LD);
        a1 += c * *(const tg_f4 *)(base + j * TG_LD + 4);
      }
    }
    float *dst = sXa + (buf * MT + ar) * TG_LD + ak;
    *(tg_f4 *)dst = a0;
    *(tg_f4 *)(dst + 4) = a1;
  };

  tg_f16 acc[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[cb][i] = 0.0f;
  const int mrow = wave * 32 + (lane & 31), mh = lane >> 5;
  // the 8 MFMA steps of a slab in two halves of 4 (B operands of a half: CB x 4 registers); accumulators round-robin over the column
  // blocks, so that consecutive MFMAs are independent
  auto mfma_slab = [&](int buf) {
    const float *pa = sXa + (buf * MT + mrow) * TG_LD + mh * 8;
    const float *pb = sW + (buf * WROWS + (lane & 31)) * TG_LD + mh * 8;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const tg_f4 xa = *(const tg_f4 *)(pa + 4 * h);
      tg_f4 wb[CB];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) wb[cb] = *(const tg_f4 *)(pb + cb * 32 * TG_LD + 4 * h);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[q], wb[cb][q], acc[cb], 0, 0, 0);
    }
  };

  // ---- pipeline: slab s is multiplied while slab s + 1 is aggregated (same wave: the MFMAs run in the matrix pipe, the gathers on
  // VALU / LDS) and slab s + 2 is in flight from HBM / L2.  Two barriers per slab, both next to the (short) register -> LDS copy.
  const int nslab = (K + TG_KS - 1) / TG_KS;
  fetch(0);
  stash(0);
  tg_lds_barrier();
  if (nslab > 1) fetch(TG_KS);
  aggregate(0);
  tg_lds_barrier();
  if (nslab > 1) stash(1);
  if (VEC && kreg) {       // (the element-wise loader of the 13-feature input layers keeps the plain loop: one slab, nothing to overlap)
    // Straight-line body: work on slabs past the end is harmless (fetch returns zeros, the extra aggregate / stash fill buffers
    // nobody reads), so nothing in it is conditional and the whole body is one scheduling region.  Source order = the order the
    // memory model allows: the MFMA operand reads of a half, then the gathers of the NEXT slab (reads of sXraw only) between that
    // half's MFMAs, and the one LDS write of the gathered row behind the last operand read (the compiler cannot tell sXa[0] from
    // sXa[1]).  The sched_group_barrier sequence asks for one MFMA, then a few VALU / LDS / VMEM instructions, 56 times (a wave
    // issues in order: what is not placed BETWEEN the MFMAs waits behind them).
    auto gather = [&](int t_lo, int t_hi, tg_f4 &a0, tg_f4 &a1) {
#pragma unroll
      for (int tt = t_lo; tt < t_hi; ++tt) {
        const float *src = sXraw + abase + (int)((cj[tt >> 2] >> (8 * (tt & 3))) & 255u) * TG_LD;
        a0 += cf[tt] * *(const tg_f4 *)src;
        a1 += cf[tt] * *(const tg_f4 *)(src + 4);
      }
    };
#ifdef TRUSS_GCN_STAMPS
    unsigned long long acc_t[4] = {0, 0, 0, 0};
    const unsigned long long t_loop0 = clock64();
#endif
    for (int s = 0; s < nslab; ++s) {
      TG_T(ta);
      tg_lds_barrier();                                     // X'[s] (and, s > 0: raw slab s + 1, W slab s + 1) are in LDS
      TG_T(tb);
      const int buf = s & 1;
      fetch((s + 2) * TG_KS);
      const float *pa = sXa + (buf * MT + mrow) * TG_LD + mh * 8;
      const float *pb = sW + (buf * WROWS + (lane & 31)) * TG_LD + mh * 8;
      tg_f4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const tg_f4 xa = *(const tg_f4 *)(pa + 4 * h);
        tg_f4 wb[CB];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) wb[cb] = *(const tg_f4 *)(pb + cb * 32 * TG_LD + 4 * h);
        gather(h == 0 ? 0 : (TG_KREG + 1) / 2, h == 0 ? (TG_KREG + 1) / 2 : TG_KREG, a0, a1);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[q], wb[cb][q], acc[cb], 0, 0, 0);
      }
      {
        float *dst = sXa + ((buf ^ 1) * MT + ar) * TG_LD + ak;
        *(tg_f4 *)dst = a0;
        *(tg_f4 *)(dst + 4) = a1;
      }
#pragma unroll
      for (int i = 0; i < 8 * CB; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                     // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                     // VALU
        if (i % 2 == 0) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // LDS read
        if (i % 8 == 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);     // VMEM read
      }
      TG_T(tc);
      tg_lds_barrier();                                     // everybody is done with sXraw (slab s + 1) and with sW / sXa [s & 1]
      TG_T(td);
      stash(s & 1);                                        // raw slab s + 2 -> sXraw, W slab s + 2 -> sW[s & 1]
#ifdef TRUSS_GCN_STAMPS
      __builtin_amdgcn_s_waitcnt(0);
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
  } else {
    for (int s = 0; s < nslab; ++s) {
      tg_lds_barrier();
      if (s + 2 < nslab) fetch((s + 2) * TG_KS);
      if (s + 1 < nslab) aggregate((s + 1) & 1);
      mfma_slab(s & 1);
      tg_lds_barrier();
      if (s + 2 < nslab) stash(s & 1);
    }
  }

  if constexpr (EPI != TG_EPI_NONE) {                      // a consumer of the output in the same launch; its barriers are inside
    tg_fused_epilogue<NW, CB, EPI>(P, acc, tg_smem, rows, row0, g0, ng);
  } else {
    tg_store_epilogue<CB>(P, acc, rows, row0, lane, wave);
  }
}

// ============================================================================================================================
// The same layer with the product on the BF16 matrix cores at float32 accuracy ("bf16x3"): every float32 operand is split EXACTLY
// into three bfloat16 terms (x = x0 + x1 + x2, truncation: 8 + 8 + 8 significant bits), and a . b is evaluated as the six partial
// products  a0 b0 + (a0 b1 + a1 b0) + (a0 b2 + a1 b1 + a2 b0)  by v_mfma_f32_32x32x16_bf16 with float32 accumulation; the three
// dropped products are below 2^-24 |a| |b|, the size of a float32 rounding.  Six bf16 MFMAs of K = 16 replace eight fp32 MFMAs of
// K = 2 per 16 k: 42 x 32 cycles instead of 56 x 64 per slab and wave (the fp32 matrix pipe is the bound of the kernel above: it
// runs at 95 % busy while two workgroups share a CU, at a power-limited ~1.45 GHz).  W arrives already split ([3][c_out][kp] bf16,
// truss_gcn_split_w, once per weight version); X' is split by the thread that gathers it.  LDS images are [term][row][16 k] bf16 =
// 32-byte rows, the two 16-byte halves of a row swapped in every other group of 8 rows (conflict-free ds_read_b128 without padding).
// Envelope: the hidden layers (c_out 33..224, k_in % 4 == 0, x 16-byte aligned, <= 9 terms per row); everything else takes the
// float32 kernel.
//
// Fewer terms (truss_gcn_layer_terms; template parameter T, the number of bf16 terms per operand: 3, 2 or 1).  The kept partial
// products are those x_i w_j with i + j <= T - 1 -- T = 3: the six above; T = 2 ("bf16x2"): x1 w0 + x0 w1 + x0 w0; T = 1 ("bf16"):
// x0 w0 -- small ones first.  Both operands stay TRUNCATED to their first T terms: X' by tg_split_term, W by reading planes t < T
// of the same [3][224][kp] image, so one weight image serves all three precisions and gcn_reference.split3 is the host model of
// all of them.  What is left out of a product a w is below tau_T |a| |w|: tau_2 = 2^-13 (a1 w1 < 2^-14, two remainders < 2^-15
// each), tau_1 = 2^-6.  Truncation rounds every operand towards zero, so "bf16" biases every PRODUCT towards zero (a product of
// two truncated operands is never larger in magnitude than the exact one); with T = 2 the same bias is 2^-13 of a product.  Per
// wave and 16-k slab: 42 / 21 / 7 MFMAs and 41 / 32 / 23 sixteen-byte LDS operations.  Everything that is sized by the number
// of terms -- the LDS images, the LDS-DMA count WI, the per-wave count WD and the vmcnt(WD) that goes with it -- is sized by T.
typedef __bf16 tg_bf8 __attribute__((ext_vector_type(8)));
typedef uint32_t tg_u4 __attribute__((ext_vector_type(4)));

// the next bf16 term of eight floats: packs their upper halves (two per dword, element 2 i in the low half) and leaves the
// (exact) remainders in place -- term after term, so that only the eight remainders stay live
__device__ __forceinline__ tg_u4 tg_split_term(float (&r)[8], bool last) {
  tg_u4 out;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t a = __float_as_uint(r[2 * i]), b = __float_as_uint(r[2 * i + 1]);
    out[i] = __builtin_amdgcn_perm(b, a, 0x07060302u);
    if (!last) {
      r[2 * i] = r[2 * i] - __uint_as_float(a & 0xffff0000u);           // exact
      r[2 * i + 1] = r[2 * i + 1] - __uint_as_float(b & 0xffff0000u);
    }
  }
  return out;
}

#define TG_CP 224                // rows of the split-weight image: c_out padded to the kernel's 7 column blocks (zero rows)

// w [c_out][k_in] float32 -> ws [3][TG_CP][kp] bf16 (kp = k_in rounded up to 16; rows >= c_out and columns >= k_in are zero)
__global__ __launch_bounds__(256) void truss_gcn_split_w_kernel(const float *__restrict__ w, uint16_t *__restrict__ ws, int C, int K, int KP) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= TG_CP * KP) return;
  const int c = i / KP, k = i - c * KP;
  const float x = (c < C && k < K) ? w[(long)c * K + k] : 0.0f;
  const uint32_t u0 = __float_as_uint(x) & 0xffff0000u;
  const float r1 = x - __uint_as_float(u0);
  const uint32_t u1 = __float_as_uint(r1) & 0xffff0000u;
  const float r2 = r1 - __uint_as_float(u1);
  ws[i] = (uint16_t)(u0 >> 16);
  ws[(long)TG_CP * KP + i] = (uint16_t)(u1 >> 16);
  ws[2L * TG_CP * KP + i] = (uint16_t)(__float_as_uint(r2) >> 16);
}

typedef __attribute__((address_space(3))) void tg_lds_void;
typedef __attribute__((address_space(1))) const void tg_glob_void;

// KT: neighbourhood terms per row that are gathered (6: the grid trusses -- a node joins at most five others; 9: any pattern the
// register path takes).  Terms past k_nbr have coefficient 0, but every one of them is two 16-byte LDS reads per slab and thread.
//
// The layer's text is truss_gcn_bf3_body.h, included as the body of two kernels: truss_gcn_layer_bf3_kernel runs it once,
// truss_gcn_group_bf3_kernel (truss_gcn_group.h) once per step of a chain.  Keep it an include: as a __device__ function the text is
// simplified on its own before it is inlined, the T = 2 slab loop changes and ran 0.9 % slower.  Its term load and store epilogue
// are written out and are not calls of tg_load_terms / tg_store_epilogue: with the two calls the slab loop stayed the parent's, the
// code round it did not, and T = 2 ran 0.8 % slower; written out (and with tg_act, which changes nothing) the plain and POOL
// kernels are instruction for instruction what they were before the text was shared (profiles/r16/README.md sections 1 and 3).
template <int NW, int KT, int EPI = TG_EPI_NONE, int T = 3>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2))) void truss_gcn_layer_bf3_kernel(const typename TgArgs<EPI>::type P, const uint16_t *__restrict__ ws, int KP) {
  const int tid = threadIdx.x;
#include "truss_gcn_bf3_body.h"
}

static size_t tg_lds_bytes(int NW, int CB, int N, int Kn) {
  const size_t MT = 32 * NW;
  size_t b = sizeof(float) * (MT * TG_LD + 2 * MT * TG_LD + 2 * (size_t)(32 * CB) * TG_LD + MT * (size_t)Kn);
  b += sizeof(int16_t) * (size_t)N * Kn;
  return (b + 15) & ~(size_t)15;
}

// the layer as the kernels take it; tile_rows: rows of a workgroup's tile (whole graphs)
static GcnLayerDev tg_layer_dev(const truss_gcn_layer_args_t *a, int tile_rows) {
  GcnLayerDev P;
  P.x = a->x; P.adj = a->adj; P.nbr = a->nbr; P.w = a->w; P.bias = a->bias; P.out = a->out;
  P.x_stride = a->x_row_stride ? a->x_row_stride : a->k_in;
  P.out_stride = a->out_row_stride ? a->out_row_stride : a->c_out;
  P.a_stride = a->a_batch_stride;
  P.B = a->n_batch; P.N = a->n_nodes; P.K = a->k_in; P.C = a->c_out; P.act = a->act; P.accumulate = a->accumulate ? 1 : 0;
  P.Kn = a->nbr ? a->k_nbr : a->n_nodes;
  P.GB = tile_rows / a->n_nodes;
  P.x_vec = tb_gcn_x_vec(a) ? 1 : 0;
  P.w_vec = ((size_t)a->w % 16 == 0 && a->k_in % 4 == 0) ? 1 : 0;
  P.a_compact = a->adj_layout == TRUSS_GCN_ADJ_COMPACT ? 1 : 0;
  P.a_row = P.a_compact ? a->k_nbr : a->n_nodes;
  return P;
}

// the layer and its epilogue as the HEAD / POOL instantiations take them
static GcnFusedDev tg_fused_dev(const truss_gcn_layer_args_t *a, const truss_gcn_epilogue_t *e, int tile_rows) {
  const bool head = e->kind == TRUSS_GCN_EPI_HEAD;
  GcnFusedDev P;
  (GcnLayerDev &)P = tg_layer_dev(a, tile_rows);
  P.w2 = e->w2; P.bias2 = e->bias2; P.adj2 = e->adj2; P.nbr2 = e->nbr2; P.out2 = e->out2; P.pool = e->pool;
  P.a2_stride = e->a2_batch_stride;
  P.out2_stride = e->out2_row_stride ? e->out2_row_stride : e->c2;
  P.pool_stride = e->pool_row_stride ? e->pool_row_stride : a->c_out;
  P.c2 = head ? e->c2 : 0; P.act2 = e->act2;
  P.Kn2 = head ? (e->nbr2 ? e->k_nbr2 : a->n_nodes) : 0;
  return P;
}

// LDS of truss_gcn_bf3_body.h in a kernel <NW, KT, EPI, T>: the slab loop's footprint shrinks with T (77 824 / 55 296 / 32 768
// bytes at NW = 4); a fused epilogue reuses it and needs tg_epi_lds_bytes(NW), which is the larger one only for T = 1 at NW = 8.
static size_t tg_bf3_lds_bytes(int NW, int T, bool fused) {
  const size_t MT = 32 * (size_t)NW;
  const size_t lds = MT * TG_LD * 4 + 2 * T * MT * 32 + 2 * T * TG_CP * 32;
  return fused && lds < tg_epi_lds_bytes(NW) ? tg_epi_lds_bytes(NW) : lds;
}

// the run-time number of bf16 terms as the last template argument of launch<EPI, T>(...): tg_launch_bf3, tgg_launch
#define TG_BY_TERMS(terms, launch, epi, ...) \
  ((terms) == 3 ? launch<epi, 3>(__VA_ARGS__) : (terms) == 2 ? launch<epi, 2>(__VA_ARGS__) : launch<epi, 1>(__VA_ARGS__))

// The launch of truss_gcn_layer_bf3_kernel<NW, KT, EPI, T> for a checked layer (every entry that takes split weights ends here).
template <int EPI, int T>
static int tg_launch_bf3(const typename TgArgs<EPI>::type &P, int NW, const uint16_t *ws, int k_in, hipStream_t st) {
  const int KP = (k_in + 15) & ~15;
  const size_t lds = tg_bf3_lds_bytes(NW, T, EPI != TG_EPI_NONE);
  const unsigned grid = (unsigned)((P.B + P.GB - 1) / P.GB);
#define TG_LAUNCH3(nw, kt)                                                                                                        \
  do {                                                                                                                            \
    static TbLdsOptIn optin;                                                                                                      \
    if (int rc = optin.ensure((const void *)truss_gcn_layer_bf3_kernel<nw, kt, EPI, T>)) return rc;                               \
    hipLaunchKernelGGL((truss_gcn_layer_bf3_kernel<nw, kt, EPI, T>), dim3(grid), dim3(64 * nw), lds, st, P, ws, KP);              \
  } while (0)
  if (NW == 4) { if (P.Kn <= 6) TG_LAUNCH3(4, 6); else TG_LAUNCH3(4, 9); }
  else { if (P.Kn <= 6) TG_LAUNCH3(8, 6); else TG_LAUNCH3(8, 9); }
#undef TG_LAUNCH3
  return TRUSS_OK;
}

// The launch of truss_gcn_layer_kernel<NW, CB, VEC, EPI> for a checked layer, shaped like tg_launch_bf3.
template <int EPI>
static int tg_launch_f32(const typename TgArgs<EPI>::type &P, int NW, hipStream_t st) {
  const bool fused = EPI != TG_EPI_NONE;
  const int CB = P.C <= 32 ? 1 : 7;
  size_t lds = tg_lds_bytes(NW, CB, P.N, P.Kn);
  if (fused && lds < tg_epi_lds_bytes(NW)) lds = tg_epi_lds_bytes(NW);
  if (lds > 160 * 1024)
    return tb_fail(TRUSS_EUNSUPPORTED, fused ? "truss_gcn_layer_fused: tile does not fit the LDS" : "truss_gcn_layer: tile does not fit the LDS");
  const unsigned grid = (unsigned)((P.B + P.GB - 1) / P.GB);
#define TG_LAUNCH(nw, cb, vec)                                                                                   \
  do {                                                                                                           \
    static TbLdsOptIn optin;                                                                                     \
    if (int rc = optin.ensure((const void *)truss_gcn_layer_kernel<nw, cb, vec, EPI>)) return rc;                \
    hipLaunchKernelGGL((truss_gcn_layer_kernel<nw, cb, vec, EPI>), dim3(grid), dim3(64 * nw), lds, st, P);       \
  } while (0)
  const bool vec = P.x_vec && P.w_vec;
  if (NW == 4 && CB == 7) { if (vec) TG_LAUNCH(4, 7, true); else TG_LAUNCH(4, 7, false); }
  else if (NW == 4) { if (vec) TG_LAUNCH(4, 1, true); else TG_LAUNCH(4, 1, false); }
  else if (CB == 7) { if (vec) TG_LAUNCH(8, 7, true); else TG_LAUNCH(8, 7, false); }
  else { if (vec) TG_LAUNCH(8, 1, true); else TG_LAUNCH(8, 1, false); }
#undef TG_LAUNCH
  return TRUSS_OK;
}

extern "C" int truss_gcn_layer(const truss_gcn_layer_args_t *a, void *stream) {
  if (!a) return tb_fail(TRUSS_EINVAL, "truss_gcn_layer: NULL argument");
  if (int rc = tb_gcn_layer_check(a, "truss_gcn_layer", 256, 0, false)) return rc;
  if (a->n_batch == 0) return TRUSS_OK;
  const int NW = a->n_nodes > 128 ? 8 : 4;
  const GcnLayerDev P = tg_layer_dev(a, 32 * NW);
  hipStream_t st = (hipStream_t)stream;
  if (a->w_bf16x3) {
    // product on the bf16 matrix cores at float32 accuracy (see truss_gcn_layer_bf3_kernel)
    if (int rc = tb_gcn_bf16x3_check(a)) return rc;
    if (int rc = tg_launch_bf3<TG_EPI_NONE, 3>(P, NW, a->w_bf16x3, a->k_in, st)) return rc;
    return tb_launched("gcn layer (bf16x3) kernel launch failed: ");
  }
  if (int rc = tg_launch_f32<TG_EPI_NONE>(P, NW, st)) return rc;
  return tb_launched("gcn layer kernel launch failed: ");
}

// The layer with a consumer of its output in the epilogue (the header has the contract): the dispatch of truss_gcn_layer over the
// HEAD / POOL instantiations of the same two kernels.
extern "C" int truss_gcn_layer_fused(const truss_gcn_layer_args_t *a, const truss_gcn_epilogue_t *e, void *stream) {
  if (!a || !e) return tb_fail(TRUSS_EINVAL, "truss_gcn_layer_fused: NULL argument");
  if (int rc = tb_gcn_fused_check(a, e)) return rc;
  if (a->w_bf16x3)
    if (int rc = tb_gcn_bf16x3_check(a)) return rc;
  if (a->n_batch == 0) return TRUSS_OK;
  const bool head = e->kind == TRUSS_GCN_EPI_HEAD;
  const int NW = a->n_nodes > 128 ? 8 : 4;
  const GcnFusedDev P = tg_fused_dev(a, e, 32 * NW);
  hipStream_t st = (hipStream_t)stream;
  if (a->w_bf16x3) {
    if (int rc = head ? tg_launch_bf3<TG_EPI_HEAD, 3>(P, NW, a->w_bf16x3, a->k_in, st) : tg_launch_bf3<TG_EPI_POOL, 3>(P, NW, a->w_bf16x3, a->k_in, st))
      return rc;
    return tb_launched("gcn fused layer (bf16x3) kernel launch failed: ");
  }
  if (int rc = head ? tg_launch_f32<TG_EPI_HEAD>(P, NW, st) : tg_launch_f32<TG_EPI_POOL>(P, NW, st)) return rc;
  return tb_launched("gcn fused layer kernel launch failed: ");
}

// The split-weight layer, plain (e == NULL) or with an epilogue, on the first `terms` bf16 terms of both operands (the header has the
// contract).  terms == 3 launches the instantiations of the two entries above.
extern "C" int truss_gcn_layer_terms(const truss_gcn_layer_args_t *a, const truss_gcn_epilogue_t *e, int32_t terms, void *stream) {
  if (!a) return tb_fail(TRUSS_EINVAL, "truss_gcn_layer_terms: NULL argument");
  if (terms < 1 || terms > 3) return tb_fail(TRUSS_EINVAL, "truss_gcn_layer_terms: bf16_terms 1..3");
  if (int rc = e ? tb_gcn_fused_check(a, e) : tb_gcn_layer_check(a, "truss_gcn_layer_terms", 256, 0, false)) return rc;
  if (!a->w_bf16x3) return tb_fail(TRUSS_EINVAL, "truss_gcn_layer_terms: w_bf16x3 is NULL (the split-weight path only)");
  if (int rc = tb_gcn_bf16x3_check(a)) return rc;
  if (a->n_batch == 0) return TRUSS_OK;
  const int NW = a->n_nodes > 128 ? 8 : 4;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (!e) {
    const GcnLayerDev P = tg_layer_dev(a, 32 * NW);
    rc = TG_BY_TERMS(terms, tg_launch_bf3, TG_EPI_NONE, P, NW, a->w_bf16x3, a->k_in, st);
  } else {
    const GcnFusedDev P = tg_fused_dev(a, e, 32 * NW);
    rc = e->kind == TRUSS_GCN_EPI_HEAD ? TG_BY_TERMS(terms, tg_launch_bf3, TG_EPI_HEAD, P, NW, a->w_bf16x3, a->k_in, st)
                                       : TG_BY_TERMS(terms, tg_launch_bf3, TG_EPI_POOL, P, NW, a->w_bf16x3, a->k_in, st);
  }
  if (rc) return rc;
  return tb_launched("gcn layer (bf16 terms) kernel launch failed: ");
}

#ifdef TRUSS_GCN_STAMPS
extern "C" int truss_debug_gcn_stamps(unsigned long long *out8) {
  return hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_gcn_stamps), 8 * sizeof(unsigned long long)) == hipSuccess ? 0 : -3;
}
#endif

extern "C" int truss_gcn_split_w(const float *w, int32_t c_out, int32_t k_in, uint16_t *w_bf16x3, void *stream) {
  if (!w || !w_bf16x3 || c_out < 1 || k_in < 1) return tb_fail(TRUSS_EINVAL, "truss_gcn_split_w: bad argument");
  if (c_out > TG_CP) return tb_fail(TRUSS_EUNSUPPORTED, "truss_gcn_split_w: c_out <= 224");
  const int KP = (k_in + 15) & ~15;
  const int n = TG_CP * KP;
  hipLaunchKernelGGL(truss_gcn_split_w_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, w_bf16x3, c_out, k_in, KP);
  return tb_launched("gcn split kernel launch failed: ");
}
#endif  // __HIPCC__
