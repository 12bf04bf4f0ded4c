// truss_gcn_level_bwd.h -- the BACKWARD of a whole level of GCN layers in one launch (gfx950), the counterpart of truss_gcn_level.h:
// for up to TGL_MAX layers out_i = act(A_i (X_i W_i^T) + b_i) that do not depend on each other, from dOut_i, out_i and the X'_i = A_i X_i
// the forward stored,
//   dZ = dOut * act'(out)   (relu: out > 0; sigmoid: out (1 - out); formed when the operands are loaded: never in HBM)
//   db = sum_rows dZ,  dW = dZ^T X',  dX = A^T (dZ W)
// in float32 with float32 accumulation (v_mfma_f32_32x32x2_f32).  This is the backward of the MADDPG update (batch 32: 512 .. 1 536
// rows per layer), bound by its launch count when run as library calls (about seven per group of equally shaped layers).  Layers are
// slices of the grid (grid.y), and within a layer grid.x enumerates two kinds of workgroups (4 waves each):
//   dW role  one per 32 c x 64 k tile of dW; contracts over ALL B N rows.  The MFMA operands are what a lane reads from HBM anyway
//            (lane l: c / k = l % 32 of row 2 s + l / 32 -- 128-byte row pieces), so nothing goes through LDS on the way in.  Wave w
//            takes the fixed row range [w Mq, (w + 1) Mq); the four partial tiles meet in LDS and are added in the order of the waves.
//            The workgroups of k-block 0 also produce db (the lanes' running sums of dZ, added in a fixed order as well).
//   dX role  one per 128 rows (whole graphs, as in the forward) x 64 k's of dX: G = dZ W in slabs of 64 c through LDS (dZ [128][64 + 4],
//            W [64][64 + 4]; the next slab is requested as soon as the registers of the previous one are in LDS and is in flight during
//            its arithmetic), the 128 x 64 tile of G back through LDS, then the transposed neighbourhood sum dX[r] = sum_t A[t][r] G[t]
//            from there with the columns of A parked in LDS ([128][N | 1]).
// No atomics: every output element has one owner and every sum a fixed order -- results are bitwise reproducible from call to call.
// Slices whose output pointer is NULL do not exist in the grid (the host gives them no workgroups) or return before any barrier.
#pragma once

#define TGB_KB 64                // k's per tile of dW / dX, c's per slab of dZ W
#define TGB_LD 68                // floats per LDS row (64 + 4 padding: rows 272 bytes apart)
#define TGB_U 8                  // MFMA steps (of 2 rows) per batch of requests of the dW role

struct GcnBwdLayerDev {
  const float *d_out, *out, *xagg, *adj, *w;
  float *d_w, *d_b, *d_x;
  long a_stride;                 // floats between graphs of adj (0: one adjacency for all)
  int B, N, K, C, act;
  int GB;                        // graphs per 128-row tile
  int kbs;                       // 64-wide blocks of k
  int kbw;                       // k-blocks the dW role covers: kbs, or 1 when only db is asked for
  int wt, xt;                    // workgroups of the dW role / of the dX role
  int dz_vec, w_vec, dx_vec;     // 16-byte accesses allowed (alignment and c_out % 4 == 0 / k_in % 4 == 0)
};
struct GcnLevelBwdDev {
  GcnBwdLayerDev l[TGL_MAX];
};

__device__ __forceinline__ float tgb_dz(float d, float o, int act) {
  return act == 1 ? (o > 0.0f ? d : 0.0f) : act == 2 ? d * (1.0f - o) * o : d;
}

struct TgbBatch {
  float d[TGB_U], o[TGB_U], a[TGB_U], b[TGB_U];
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void truss_gcn_level_bwd_kernel(const GcnLevelBwdDev LV) {
  constexpr int MT = 128, NT = 256;
  extern __shared__ __attribute__((aligned(16))) char tg_smem[];
  const GcnBwdLayerDev &P = LV.l[blockIdx.y];
  int slice = blockIdx.x;
  if (slice >= P.wt + P.xt) return;                          // (uniform: before any barrier)
  const int N = P.N, K = P.K, C = P.C, act = P.act;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float *smem = (float *)tg_smem;

  if (slice < P.wt) {
    // ---- dW role: tile [c0, + 32) x [k0, + 64) of dW = dZ^T X' (and db of these c's where k0 == 0) ----
    const int cb = slice / P.kbw, kb = slice - cb * P.kbw;
    const int c0 = cb * 32, k0 = kb * TGB_KB;
    const int M = P.B * N;
    const int Mq = (((M + 3) >> 2) + 1) & ~1;                // rows per wave (even: an MFMA step takes two rows)
    const int rb = wave * Mq, re = rb + Mq < M ? rb + Mq : M;
    const int hr = lane >> 5, c = c0 + (lane & 31), ka = k0 + (lane & 31), kc = ka + 32;
    const bool has_x = P.d_w != nullptr;                     // (the host refuses d_w without x_agg)
    const bool cok = c < C, aok = has_x && ka < K, bok = has_x && kc < K;
    const float *xs = has_x ? P.xagg : P.d_out;              // (never read without has_x: only a valid address)
    // requests of TGB_U steps = 16 rows: every load from a valid (clamped) address and nothing between the loads; the values are
    // masked when they are used.  The next batch is in flight during the arithmetic of the current one.
    auto request = [&](int r0, TgbBatch &q) {
#pragma unroll
      for (int u = 0; u < TGB_U; ++u) {
        const int r = r0 + 2 * u + hr;
        const bool ok = r < re;
        const long oz = (ok && cok) ? (long)r * C + c : 0;
        q.d[u] = P.d_out[oz];
        q.o[u] = P.out[oz];
        q.a[u] = xs[(ok && aok) ? (long)r * K + ka : 0];
        q.b[u] = xs[(ok && bok) ? (long)r * K + kc : 0];
      }
    };
    tg_f16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = 0.0f, acc1[i] = 0.0f;
    float dbs = 0.0f;
    TgbBatch cur, nxt;
    request(rb, cur);
    for (int r0 = rb; r0 < re; r0 += 2 * TGB_U) {
      request(r0 + 2 * TGB_U, nxt);                          // (past the end: clamped addresses, masked values)
      float dz[TGB_U];
#pragma unroll
      for (int u = 0; u < TGB_U; ++u) {
        const bool ok = r0 + 2 * u + hr < re;
        dz[u] = (ok && cok) ? tgb_dz(cur.d[u], cur.o[u], act) : 0.0f;
        const float xa = (ok && aok) ? cur.a[u] : 0.0f, xb = (ok && bok) ? cur.b[u] : 0.0f;
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[u], xa, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[u], xb, acc1, 0, 0, 0);
      }
      dbs += ((dz[0] + dz[1]) + (dz[2] + dz[3])) + ((dz[4] + dz[5]) + (dz[6] + dz[7]));      // (pairwise within a batch: a shorter chain)
      cur = nxt;
    }
    // partial tiles -> LDS (accumulator register i of a lane = c 8 (i / 4) + 4 (l / 32) + i % 4, k l % 32), added in the order of the waves
    float *sP = smem + wave * 32 * TGB_LD;
    float *sB = smem + 4 * 32 * TGB_LD;                      // [4 waves][64 lanes] running sums of dZ
    {
      const int crow = 4 * (lane >> 5), col = lane & 31;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        sP[(crow + 8 * (i >> 2) + (i & 3)) * TGB_LD + col] = acc0[i];
        sP[(crow + 8 * (i >> 2) + (i & 3)) * TGB_LD + 32 + col] = acc1[i];
      }
      sB[wave * 64 + lane] = dbs;
    }
    tg_lds_barrier();
    if (has_x) {
#pragma unroll
      for (int e = 0; e < 32 * TGB_KB / NT; ++e) {
        const int q = tid + e * NT, cr = q >> 6, kk = q & 63;
        const float *p = smem + cr * TGB_LD + kk;
        const float v = ((p[0] + p[32 * TGB_LD]) + p[2 * 32 * TGB_LD]) + p[3 * 32 * TGB_LD];
        if (c0 + cr < C && k0 + kk < K) P.d_w[(long)(c0 + cr) * K + k0 + kk] = v;
      }
    }
    if (kb == 0 && P.d_b && tid < 32 && c0 + tid < C) {
      float s = 0.0f;
#pragma unroll
      for (int w = 0; w < 4; ++w) s += sB[w * 64 + tid] + sB[w * 64 + 32 + tid];
      P.d_b[c0 + tid] = s;
    }
    return;
  }

  // ---- dX role: rows of the graphs [g0, + GB) x k's [k0, + 64) of dX = A^T (dZ W) ----
  slice -= P.wt;
  const int tile = slice / P.kbs, kb = slice - tile * P.kbs;
  const int g0 = tile * P.GB, k0 = kb * TGB_KB;
  const int ng = (P.B - g0 < P.GB) ? P.B - g0 : P.GB;
  const int rows = ng * N;                                   // live rows of this tile (<= MT)
  const long row0 = (long)g0 * N;
  float *sZ = smem;                                          // [MT][TGB_LD] slab of dZ; afterwards the tile of G
  float *sW = smem + MT * TGB_LD;                            // [64][TGB_LD] slab of W (c's x this block's k's)
  float *sAT = smem + (MT + TGB_KB) * TGB_LD;                // [MT][NP] sAT[r][t] = A[graph of r][t][node of r]
  const int NP = N | 1;
  const bool zv = P.dz_vec != 0, wv = P.w_vec != 0;

  tg_f4 rd[8], ro[8], rw[4];
  auto guarded4 = [&](const float *src, int col, int lim, bool ok) {
    tg_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ok) {
      if (col + 0 < lim) v[0] = src[0];
      if (col + 1 < lim) v[1] = src[1];
      if (col + 2 < lim) v[2] = src[2];
      if (col + 3 < lim) v[3] = src[3];
    }
    return v;
  };
  // a slab: dOut / out rows [128][64 c] and W [64 c][64 k] as 16-byte pieces, 16 lanes per 256-byte row piece.  Vector path: one
  // load from a clamped address and nothing else (pieces are whole or past the end; masked when they go to LDS).
  auto request = [&](int sl) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int q = tid + e * NT, r = q >> 4, cc = sl * TGB_KB + (q & 15) * 4;
      const bool ok = r < rows && cc < C;
      const long off = (row0 + (r < rows ? r : 0)) * (long)C + cc;
      if (zv) {
        rd[e] = *(const tg_f4 *)(ok ? P.d_out + off : P.d_out);
        ro[e] = *(const tg_f4 *)(ok ? P.out + off : P.out);
      } else {
        rd[e] = guarded4(P.d_out + off, cc, C, ok);
        ro[e] = guarded4(P.out + off, cc, C, ok);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = tid + e * NT, wc = sl * TGB_KB + (q >> 4), kk = k0 + (q & 15) * 4;
      const bool ok = wc < C && kk < K;
      const long off = (long)(wc < C ? wc : 0) * K + kk;
      if (wv) rw[e] = *(const tg_f4 *)(ok ? P.w + off : P.w);
      else rw[e] = guarded4(P.w + off, kk, K, ok);
    }
  };
  request(0);

  // the columns of A of this tile's graphs -> LDS, transposed (batches of 8 loads per thread, coalesced along a row of A)
  {
    const int NN = N * N, total = ng * NN;
    for (int i0 = 0; i0 < total; i0 += 8 * NT) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + tid + j * NT;
        const int g = i / NN, rem = i - g * NN;
        v[j] = P.adj[i < total ? (long)(g0 + g) * P.a_stride + rem : 0];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + tid + j * NT;
        if (i < total) {
          const int g = i / NN, rem = i - g * NN, t = rem / N, n = rem - t * N;
          sAT[(g * N + n) * NP + t] = v[j];
        }
      }
    }
  }

  // ---- G = dZ W of this tile, slab by slab: registers -> LDS (dZ formed here) | next request | barrier | per 16 c's: lane (row
  // l % 32 of the wave's 32, half h = l / 32) reads c = 8 h .. 8 h + 7 of its row; MFMA q of half-step hh multiplies c = 4 hh + q
  // (lanes of half 0) and 8 + 4 hh + q (half 1) with W[c][k l % 32] and W[c][k 32 + l % 32] | barrier.
  const int mrow = wave * 32 + (lane & 31), mh = lane >> 5;
  const bool two = k0 + 32 < K;                              // (uniform) the second 32 k's of the block exist
  tg_f16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc0[i] = 0.0f, acc1[i] = 0.0f;
#pragma unroll
  for (int sl = 0; sl < 4; ++sl)
    if (sl * TGB_KB < C) {
      if (sl) tg_lds_barrier();                              // everybody is done with the previous slab
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int q = tid + e * NT, r = q >> 4, cc = sl * TGB_KB + (q & 15) * 4;
        const bool ok = r < rows && cc < C;
        tg_f4 z;
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = (ok && cc + j < C) ? tgb_dz(rd[e][j], ro[e][j], act) : 0.0f;
        *(tg_f4 *)(sZ + r * TGB_LD + (q & 15) * 4) = z;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int q = tid + e * NT, wc = sl * TGB_KB + (q >> 4), kk = k0 + (q & 15) * 4;
        tg_f4 z;
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = (wc < C && kk + j < K) ? rw[e][j] : 0.0f;
        *(tg_f4 *)(sW + (q >> 4) * TGB_LD + (q & 15) * 4) = z;
      }
      if ((sl + 1) * TGB_KB < C) request(sl + 1);            // into the registers just emptied: in flight during the arithmetic
      tg_lds_barrier();
      const float *pa = sZ + mrow * TGB_LD + mh * 8;
      const float *pb = sW + mh * 8 * TGB_LD + (lane & 31);
#pragma unroll
      for (int u = 0; u < TGB_KB / 16; ++u)
        if (sl * TGB_KB + 16 * u < C) {
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            const tg_f4 za = *(const tg_f4 *)(pa + 16 * u + 4 * hh);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float *pw = pb + (16 * u + 4 * hh + q) * TGB_LD;
              acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(za[q], pw[0], acc0, 0, 0, 0);
              if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(za[q], pw[32], acc1, 0, 0, 0);
            }
          }
        }
    }

  tg_lds_barrier();                                          // every wave is done reading the last slab: the tile of G goes over it
  {
    const int rbase = wave * 32 + 4 * (lane >> 5), col = lane & 31;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      sZ[(rbase + 8 * (i >> 2) + (i & 3)) * TGB_LD + col] = acc0[i];
      sZ[(rbase + 8 * (i >> 2) + (i & 3)) * TGB_LD + 32 + col] = acc1[i];
    }
  }
  tg_lds_barrier();
  // dX[row ar][k0 + 32 ah .. + 31] = sum_t A[t][node of ar] G[graph row t][same k's], in two passes of 16 k's
  const int ar = tid >> 1, ah = tid & 1;
  if (ar >= rows) return;                                    // (no barrier below)
  const int gbase = ar / N * N;
  const float *cf = sAT + ar * NP;
  float *xo = P.d_x + (row0 + ar) * (long)K;
#pragma unroll
  for (int hp = 0; hp < 2; ++hp) {
    const int off = ah * 32 + hp * 16, kk = k0 + off;
    if (kk >= K) break;
    tg_f4 a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = tg_f4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int t = 0; t < N; ++t) {
      const float cft = cf[t];
      const float *src = sZ + (gbase + t) * TGB_LD + off;
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] += cft * *(const tg_f4 *)(src + 4 * q);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (P.dx_vec) {
        if (kk + 4 * q < K) *(tg_f4 *)(xo + kk + 4 * q) = a[q];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (kk + 4 * q + j < K) xo[kk + 4 * q + j] = a[q][j];
      }
    }
  }
}

extern "C" int truss_gcn_level_backward(const truss_gcn_layer_args_t *layers, int32_t n_layers, const truss_gcn_level_bwd_t *bwd, void *stream) {
  if (n_layers < 0 || (n_layers > 0 && (!layers || !bwd))) return tb_fail(TRUSS_EINVAL, "truss_gcn_level_backward: bad argument");
  for (int i = 0; i < n_layers; ++i) {
    const truss_gcn_layer_args_t *a = layers + i;
    const truss_gcn_level_bwd_t *g = bwd + i;
    if (a->struct_size != sizeof(truss_gcn_layer_args_t)) return tb_fail(TRUSS_EINVAL, "truss_gcn_layer_args_t size mismatch (ABI)");
    if (a->n_batch == 0 || (!g->d_w && !g->d_b && !g->d_x)) continue;      // nothing to read, nothing to write
    if (!g->d_out || !g->out || (g->d_x && (!a->adj || !a->w)))
      return tb_fail(TRUSS_EINVAL, "truss_gcn_level_backward: a required pointer is NULL");
    if (a->n_batch < 0 || a->n_nodes < 1 || a->k_in < 1 || a->c_out < 1 || a->act < 0 || a->act > 2)
      return tb_fail(TRUSS_EINVAL, "truss_gcn_level_backward: bad sizes / act");
    if (g->d_w && !g->x_agg) return tb_fail(TRUSS_EINVAL, "truss_gcn_level_backward: d_w needs x_agg (X' = A X as truss_gcn_level stored it)");
    if (g->d_x && (g->d_x == g->d_out || g->d_x == g->out)) return tb_fail(TRUSS_EINVAL, "truss_gcn_level_backward: d_x must not alias d_out / out");
    if (a->accumulate || a->w_bf16x3) return tb_fail(TRUSS_EUNSUPPORTED, "truss_gcn_level_backward: float32 product, no accumulation");
    if (a->nbr) return tb_fail(TRUSS_EUNSUPPORTED, "truss_gcn_level_backward: dense adjacencies only (nbr must be NULL)");
    if (a->out_row_stride && a->out_row_stride != a->c_out) return tb_fail(TRUSS_EUNSUPPORTED, "truss_gcn_level_backward: out / d_out rows are contiguous");
    if (a->c_out > 224) return tb_fail(TRUSS_EUNSUPPORTED, "truss_gcn_level_backward: c_out <= 224");
    if (a->n_nodes > 64) return tb_fail(TRUSS_EUNSUPPORTED, "truss_gcn_level_backward: n_nodes <= 64");
    if (a->k_in > 4 * TGB_KB) return tb_fail(TRUSS_EUNSUPPORTED, "truss_gcn_level_backward: k_in <= 256");
    if ((long)a->n_batch * a->n_nodes > (1L << 30) / 256) return tb_fail(TRUSS_EUNSUPPORTED, "truss_gcn_level_backward: n_batch * n_nodes <= 4194304");
  }
  hipStream_t st = (hipStream_t)stream;
  for (int i0 = 0; i0 < n_layers; i0 += TGL_MAX) {
    const int nl = n_layers - i0 < TGL_MAX ? n_layers - i0 : TGL_MAX;
    GcnLevelBwdDev LV;
    memset(&LV, 0, sizeof LV);
    unsigned slices = 0;
    int live = 0, nmax = 1;
    for (int i = 0; i < nl; ++i) {
      const truss_gcn_layer_args_t *a = layers + i0 + i;
      const truss_gcn_level_bwd_t *g = bwd + i0 + i;
      if (a->n_batch == 0 || (!g->d_w && !g->d_b && !g->d_x)) continue;
      GcnBwdLayerDev &P = LV.l[live];
      P.d_out = g->d_out; P.out = g->out; P.xagg = g->x_agg; P.adj = a->adj; P.w = a->w;
      P.d_w = g->d_w; P.d_b = g->d_b; P.d_x = g->d_x;
      P.a_stride = a->a_batch_stride;
      P.B = a->n_batch; P.N = a->n_nodes; P.K = a->k_in; P.C = a->c_out; P.act = a->act;
      P.GB = 128 / a->n_nodes;
      P.kbs = (a->k_in + TGB_KB - 1) / TGB_KB;
      P.kbw = g->d_w ? P.kbs : 1;
      P.wt = (g->d_w || g->d_b) ? (a->c_out + 31) / 32 * P.kbw : 0;
      P.xt = g->d_x ? (a->n_batch + P.GB - 1) / P.GB * P.kbs : 0;
      P.dz_vec = ((size_t)g->d_out % 16 == 0 && (size_t)g->out % 16 == 0 && a->c_out % 4 == 0) ? 1 : 0;
      P.w_vec = ((size_t)a->w % 16 == 0 && a->k_in % 4 == 0) ? 1 : 0;
      P.dx_vec = ((size_t)g->d_x % 16 == 0 && a->k_in % 4 == 0) ? 1 : 0;
      if (g->d_x && a->n_nodes > nmax) nmax = a->n_nodes;
      const unsigned s = (unsigned)(P.wt + P.xt);
      slices = s > slices ? s : slices;
      ++live;
    }
    if (!live) continue;
    // dX role: a slab of dZ (128 x 68 floats) and of W (64 x 68) -- the tile of G goes over the first -- and the columns of A
    // (128 x (N | 1)); the dW role's four partial tiles (4 x 32 x 68) and running sums (256) fit the first two
    size_t lds = sizeof(float) * ((128 + TGB_KB) * TGB_LD + 128 * (size_t)(nmax | 1));
    lds = (lds + 15) & ~(size_t)15;
    static TbLdsOptIn optin;
    if (int rc = optin.ensure((const void *)truss_gcn_level_bwd_kernel)) return rc;
    hipLaunchKernelGGL(truss_gcn_level_bwd_kernel, dim3(slices, (unsigned)live), dim3(256), lds, st, LV);
    if (int rc = tb_launched("gcn level backward kernel launch failed: ")) return rc;
  }
  return TRUSS_OK;
}
