// truss_gcn_level_agg.h -- the neighbour sums of a level of the MADDPG update through the node table (include/truss_mi355.h,
// truss_gcn_level_aggregate): y = A x or y = A^T x per graph for up to TRUSS_GCN_AGG_MAX independent items in one launch, for
// graphs beyond the 64 nodes whose whole adjacency the level kernels (truss_gcn_level.h, truss_gcn_level_bwd.h) keep in a tile.
// No tiles here and no LDS: thread = (row, channel quad) -- or (row, channel) where the item cannot take 16-byte accesses --
// flat over an item, as in truss_gcn_aggregate_sparse_kernel (truss_gcn_aggregate.h); grid = (blocks of the largest item, items).
// On top the argument check (host only: a stand-alone program can drive it); below it, for the device compiler only, the kernel
// and the C entry.  truss_hip.hip includes this file after truss_gcn_aggregate.h.
#pragma once
#include <cstdint>
#include <string>

static int tb_fail(int code, const std::string &msg);

// every item is checked before anything is launched; an item with n_batch == 0 passes unread (its pointers included)
static inline int tb_gcn_level_aggregate_check(const truss_gcn_agg_t *items, int32_t n_items) {
  if (n_items < 0 || (n_items > 0 && !items)) return tb_fail(TRUSS_EINVAL, "truss_gcn_level_aggregate: bad argument");
  for (int32_t i = 0; i < n_items; ++i) {
    const truss_gcn_agg_t &a = items[i];
    if (a.struct_size != sizeof(truss_gcn_agg_t)) return tb_fail(TRUSS_EINVAL, "truss_gcn_level_aggregate: struct_size mismatch");
    if (a.n_batch < 0) return tb_fail(TRUSS_EINVAL, "truss_gcn_level_aggregate: n_batch < 0");
    if (a.n_batch == 0) continue;
    if (!a.x || !a.adj || !a.nbr || !a.y) return tb_fail(TRUSS_EINVAL, "truss_gcn_level_aggregate: NULL argument");
    if (a.n_nodes < 1 || a.n_nodes > 32767 || a.k_nbr < 1 || a.k_nbr > 16 || a.n_ch < 1 || a.a_batch_stride < 0)
      return tb_fail(TRUSS_EINVAL, "truss_gcn_level_aggregate: n_nodes 1..32767, k_nbr 1..16, n_ch >= 1, a_batch_stride >= 0");
    const uint64_t n = (uint64_t)a.n_batch * (uint64_t)a.n_nodes * (uint64_t)a.n_ch;
    if (n > (uint64_t)1 << 38) return tb_fail(TRUSS_EINVAL, "truss_gcn_level_aggregate: more than 2^38 elements in one item");
    const uintptr_t x0 = (uintptr_t)a.x, y0 = (uintptr_t)a.y, bytes = (uintptr_t)(n * sizeof(float));
    if (x0 < y0 + bytes && y0 < x0 + bytes) return tb_fail(TRUSS_EINVAL, "truss_gcn_level_aggregate: y overlaps x");
  }
  return TRUSS_OK;
}

#ifdef __HIPCC__
struct GcnAggItemDev {
  const float *x, *adj;
  const int16_t *nbr;
  float *y;
  long a_stride;
  long total;                    // threads of the item: rows x (channel quads | channels)
  int N, C, K;
  int flags;                     // bit 0: transposed coefficients, bit 1: channel quads (16-byte accesses)
};
struct GcnAggDev {
  GcnAggItemDev it[TRUSS_GCN_AGG_MAX];       // 24 x 64 bytes of kernel arguments
};

// one output piece: V = tb_f4 (a channel quad) or float (one channel); cu = pieces per row.  All KR loads of a round are issued
// from valid addresses (a -1 entry reads the row's own diagonal coefficient and its own x row) with nothing between them; the
// entries are masked where the values are used.
template <typename V, int KR>
__device__ __forceinline__ void tga_piece(const GcnAggItemDev &P, int cu, long g, int i, int c, long t) {
  const int N = P.N, K = P.K;
  const bool tr = P.flags & 1;
  const float *Ag = P.adj + g * P.a_stride;
  const V *Xg = (const V *)P.x + (size_t)g * N * cu + c;
  const int16_t *nb = P.nbr + (long)i * K;
  V acc = {};
  for (int k0 = 0; k0 < K; k0 += KR) {
    int j[KR];
    float a[KR];
    V xv[KR];
#pragma unroll
    for (int q = 0; q < KR; ++q) {
      j[q] = k0 + q < K ? (int)nb[k0 + q] : -1;
      const int jc = (j[q] < 0 || j[q] >= N) ? i : j[q];          // (an entry beyond the graph reads nothing out of bounds)
      a[q] = Ag[tr ? (long)jc * N + i : (long)i * N + jc];
      xv[q] = Xg[(size_t)jc * cu];
    }
#pragma unroll
    for (int q = 0; q < KR; ++q) {
      if (j[q] < 0 || j[q] >= N) continue;
      if constexpr (sizeof(V) == sizeof(float)) acc = fmaf(a[q], xv[q], acc);
      else tb_gcn_fma4(acc, a[q], xv[q]);
    }
  }
  ((V *)P.y)[t] = acc;
}

template <typename V>
__device__ __forceinline__ void tga_item(const GcnAggItemDev &P, int cu, long t) {
  int c, i;
  long g;
  if (P.total <= 0x7fffffffL) {            // (the update's items: 32-bit divisions)
    const unsigned tt = (unsigned)t, r = tt / (unsigned)cu;
    c = (int)(tt - r * (unsigned)cu);
    g = r / (unsigned)P.N;
    i = (int)(r - (unsigned)g * (unsigned)P.N);
  } else {
    const long r = t / cu;
    c = (int)(t - r * cu);
    g = r / P.N;
    i = (int)(r - g * P.N);
  }
  if (P.K <= 4) tga_piece<V, 4>(P, cu, g, i, c, t);
  else if (P.K <= 6) tga_piece<V, 6>(P, cu, g, i, c, t);          // a grid truss: six entries, one round
  else tga_piece<V, 8>(P, cu, g, i, c, t);                        // up to nine: two rounds, the second mostly masked
}

__global__ __launch_bounds__(256) void truss_gcn_level_aggregate_kernel(const GcnAggDev A) {
  const GcnAggItemDev &P = A.it[blockIdx.y];
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if ((long)blockIdx.x * 256 >= P.total) return;                  // a block past this item's end leaves before anything else
  if (t >= P.total) return;
  if (P.flags & 2) tga_item<tb_f4>(P, P.C >> 2, t);
  else tga_item<float>(P, P.C, t);
}

extern "C" int truss_gcn_level_aggregate(const truss_gcn_agg_t *items, int32_t n_items, void *stream) {
  if (int rc = tb_gcn_level_aggregate_check(items, n_items)) return rc;
  for (int i0 = 0; i0 < n_items;) {
    GcnAggDev A;
    memset(&A, 0, sizeof A);
    int live = 0;
    long most = 0;
    for (; i0 < n_items && live < TRUSS_GCN_AGG_MAX; ++i0) {
      const truss_gcn_agg_t &a = items[i0];
      if (a.n_batch == 0) continue;
      GcnAggItemDev &P = A.it[live++];
      const bool quads = (a.n_ch & 3) == 0 && (((size_t)a.x | (size_t)a.y) & 15) == 0;
      P.x = a.x, P.adj = a.adj, P.nbr = a.nbr, P.y = a.y, P.a_stride = (long)a.a_batch_stride;
      P.N = a.n_nodes, P.C = a.n_ch, P.K = a.k_nbr;
      P.flags = (a.transpose ? 1 : 0) | (quads ? 2 : 0);
      P.total = (long)a.n_batch * a.n_nodes * (quads ? a.n_ch / 4 : a.n_ch);
      most = P.total > most ? P.total : most;
    }
    if (!live) continue;
    const long blocks = (most + 255) / 256;                         // (<= 2^30: the check's limit of 2^38 elements per item)
    hipLaunchKernelGGL(truss_gcn_level_aggregate_kernel, dim3((unsigned)blocks, (unsigned)live), dim3(256), 0, (hipStream_t)stream, A);
    if (int rc = tb_launched("gcn level aggregate launch failed: ")) return rc;
  }
  return TRUSS_OK;
}
#endif  // __HIPCC__
