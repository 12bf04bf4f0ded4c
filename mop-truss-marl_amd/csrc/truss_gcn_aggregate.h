// truss_gcn_aggregate.h -- act(A @ H + b) per graph (include/truss_mi355.h, truss_gcn_aggregate / truss_gcn_aggregate_sparse).
// On top the argument checks, shared with the plain loops of the CPU test backend in tests/emu/truss_emu.cpp; below them, for
// the device compiler only, the gfx950 kernels, their dispatch and the C entries.  truss_hip.hip includes this file after
// truss_host.h.
#pragma once
#include <cstdint>
#include <string>

static int tb_fail(int code, const std::string &msg);

static inline int tb_gcn_aggregate_check(const float *adj, const float *h, const float *out, int32_t n_batch, int32_t n_nodes,
                                         int32_t n_channels, int32_t act) {
  if (!adj || !h || !out) return tb_fail(TRUSS_EINVAL, "truss_gcn_aggregate: NULL argument");
  if (n_batch < 0 || n_nodes < 1 || n_nodes > 64 || n_channels < 1 || act < 0 || act > 2)
    return tb_fail(TRUSS_EINVAL, "truss_gcn_aggregate: n_nodes must be 1..64, act 0..2");
  return TRUSS_OK;
}

static inline int tb_gcn_aggregate_sparse_check(const float *adj, const int16_t *nbr, int32_t k_nbr, const float *h, const float *bias,
                                                const float *out, int32_t n_batch, int32_t n_nodes, int32_t n_channels, int32_t act) {
  if (!adj || !nbr || !h || !out) return tb_fail(TRUSS_EINVAL, "truss_gcn_aggregate_sparse: NULL argument");
  if (n_batch < 0 || n_nodes < 1 || n_nodes > 32767 || k_nbr < 1 || k_nbr > 16 || n_channels < 4 || (n_channels & 3) || act < 0 || act > 2)
    return tb_fail(TRUSS_EINVAL, "truss_gcn_aggregate_sparse: n_nodes 1..32767, k_nbr 1..16, n_channels a multiple of 4, act 0..2");
  if ((((size_t)h | (size_t)out | (size_t)bias) & 15) != 0 || h == out)
    return tb_fail(TRUSS_EINVAL, "truss_gcn_aggregate_sparse: h / out / bias must be 16-byte aligned, out must not alias h");
  return TRUSS_OK;
}

#ifdef __HIPCC__
// the fused epilogue: 0 none, 1 relu, 2 sigmoid.  truss_gcn_aggregate_kernel and truss_gcn_aggregate4_kernel spell it out
// instead: through this helper their register allocation came out different (SGPR spills of <64>, VGPRs of the quad kernel)
__device__ __forceinline__ float tb_gcn_act(float v, int act) {
  if (act == 1) v = v > 0.0f ? v : 0.0f;
  else if (act == 2) v = 1.0f / (1.0f + expf(-v));
  return v;
}
// acc += a * h over the four channels of a quad
__device__ __forceinline__ void tb_gcn_fma4(tb_f4 &acc, float a, tb_f4 h) {
  acc[0] = fmaf(a, h[0], acc[0]);
  acc[1] = fmaf(a, h[1], acc[1]);
  acc[2] = fmaf(a, h[2], acc[2]);
  acc[3] = fmaf(a, h[3], acc[3]);
}

// ---- GCN aggregation (inference): one workgroup per env and 256 channels, thread = channel -------------
// Memory-bound (reads H once, writes out once, 16-64 FMAs per element): every global access is a contiguous
// run of channels across the threads of a wave; the adjacency row block sits in LDS and is read as a
// broadcast.  Bias and activation are fused (no extra passes over the [B, N, C] tensor).
template <int NMAX>
__global__ __launch_bounds__(256) void truss_gcn_aggregate_kernel(const float *__restrict__ adj, long a_stride, const float *h,
                                                                  const float *__restrict__ bias, float *out, int N, int C, int act) {
  __shared__ float sA[NMAX * NMAX];
  const int b = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  const float *A = adj + (size_t)b * a_stride;
  for (int i = threadIdx.x; i < N * N; i += 256) sA[i] = A[i];
  __syncthreads();
  if (c >= C) return;
  const float *H = h + (size_t)b * N * C + c;
  float col[NMAX];
#pragma unroll
  for (int j = 0; j < NMAX; ++j) col[j] = j < N ? H[(size_t)j * C] : 0.0f;
  const float bc = bias ? bias[c] : 0.0f;
  float *O = out + (size_t)b * N * C + c;
  for (int i = 0; i < N; ++i) {
    float acc = bc;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) acc = fmaf(j < N ? sA[i * N + j] : 0.0f, col[j], acc);
    if (act == 1) acc = acc > 0.0f ? acc : 0.0f;
    else if (act == 2) acc = 1.0f / (1.0f + expf(-acc));
    O[(size_t)i * C] = acc;
  }
}

// The same for channel counts that are multiples of 4, sized to the channel count: a thread owns FOUR channels of one
// graph (16-byte loads / stores) and the threads of a block are dealt over (graph, channel quad) pairs without gaps, so
// no lane idles whatever C is (thread = channel in 256-wide blocks left 22 % of the lanes idle at C = 200); a block of
// 256 threads then spans up to 256 / (C / 4) + 2 graphs, whose adjacencies it stages in LDS.
template <int NMAX>
__global__ __launch_bounds__(256) void truss_gcn_aggregate4_kernel(const float *__restrict__ adj, long a_stride, const float *h,
                                                                   const float *__restrict__ bias, float *out, int B, int N, int C4, int act,
                                                                   int gmax) {
  extern __shared__ float sA[];                       // [graphs of this block][N][N]
  const long t0 = (long)blockIdx.x * 256, t = t0 + threadIdx.x;
  const int g0 = (int)(t0 / C4);
  int g1 = (int)((t0 + 255) / C4);
  g1 = g1 < B - 1 ? g1 : B - 1;
  const int ng = a_stride ? g1 - g0 + 1 : 1, nn = N * N;
  for (int i = threadIdx.x; i < ng * nn; i += 256) sA[i] = adj[(a_stride ? (size_t)(g0 + i / nn) * a_stride : 0) + i % nn];
  __syncthreads();
  const int gph = (int)(t / C4), c4 = (int)(t % C4);
  if (gph >= B) return;
  const tb_f4 *H = (const tb_f4 *)h + ((size_t)gph * N) * C4 + c4;
  tb_f4 col[NMAX];
#pragma unroll
  for (int j = 0; j < NMAX; ++j) col[j] = j < N ? H[(size_t)j * C4] : (tb_f4){0.0f, 0.0f, 0.0f, 0.0f};
  const tb_f4 bc = bias ? ((const tb_f4 *)bias)[c4] : (tb_f4){0.0f, 0.0f, 0.0f, 0.0f};
  const float *A = sA + (a_stride ? (gph - g0) * nn : 0);
  tb_f4 *O = (tb_f4 *)out + ((size_t)gph * N) * C4 + c4;
  for (int i = 0; i < N; ++i) {
    tb_f4 acc = bc;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
      const float aij = j < N ? A[i * N + j] : 0.0f;
      tb_gcn_fma4(acc, aij, col[j]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (act == 1) acc[q] = acc[q] > 0.0f ? acc[q] : 0.0f;
      else if (act == 2) acc[q] = 1.0f / (1.0f + expf(-acc[q]));
    }
    O[(size_t)i * C4] = acc;
  }
}

// Slab variant (dense or sparse pattern): a block owns a 128-byte channel slab (8 quads) of GB whole graphs.  It stages the slab of
// H in LDS with full-line loads (8 threads = one 128-byte line), then every (graph, row, quad) item sums its terms from LDS and
// stores 16 bytes -- 8 items = one whole line.  HBM sees H once and `out` once; the neighbours' rows come from LDS, not from L2.
// nbr == nullptr: dense, the K = N columns in order.
__global__ __launch_bounds__(256) void truss_gcn_aggregate_slab_kernel(const float *__restrict__ adj, long a_stride,
                                                                       const int16_t *__restrict__ nbr, int K, const float *__restrict__ h,
                                                                       const float *__restrict__ bias, float *__restrict__ out, int B, int N,
                                                                       int C4, int GB, int act) {
  extern __shared__ tb_f4 sH[];                           // [GB][N][8]
  const int slab = blockIdx.y, q0 = slab * 8;
  const int nq = C4 - q0 < 8 ? C4 - q0 : 8;               // quads of this slab (the last one may be short)
  const int b0 = blockIdx.x * GB;
  const int gb = B - b0 < GB ? B - b0 : GB;
  const int items = gb * N * 8;
  for (int it = threadIdx.x; it < items; it += 256) {
    const int q = it & 7, r = it >> 3;                    // r = g * N + row
    if (q < nq) sH[it] = ((const tb_f4 *)h)[((size_t)b0 * N + r) * C4 + q0 + q];
  }
  __syncthreads();
  for (int it = threadIdx.x; it < items; it += 256) {
    const int q = it & 7, r = it >> 3;
    if (q >= nq) continue;
    const int g = r / N, i = r - g * N;
    const float *Arow = adj + (size_t)(b0 + g) * a_stride + (size_t)i * N;
    const tb_f4 *Hg = sH + (size_t)g * N * 8 + q;
    tb_f4 acc = bias ? ((const tb_f4 *)bias)[q0 + q] : (tb_f4){0.0f, 0.0f, 0.0f, 0.0f};
    if (nbr) {
      const int16_t *nb = nbr + (size_t)i * K;
      for (int k = 0; k < K; ++k) {     // (an unrolled round of 12 with all loads in flight was slower: 45 against 34 us at 64 nodes)
        const int j = nb[k];
        if (j < 0) continue;
        tb_gcn_fma4(acc, Arow[j], Hg[j * 8]);
      }
    } else {
      for (int j = 0; j < N; ++j) tb_gcn_fma4(acc, Arow[j], Hg[j * 8]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = tb_gcn_act(acc[c], act);
    ((tb_f4 *)out)[((size_t)b0 * N + r) * C4 + q0 + q] = acc;
  }
}
// launch helper: false when the shape does not suit the slab kernel (the callers' other kernels take over)
static bool tb_launch_gcn_slab(const float *adj, int64_t a_stride, const int16_t *nbr, int K, const float *h, const float *bias, float *out,
                               int B, int N, int C, int act, hipStream_t st) {
  if ((C & 3) || (((size_t)h | (size_t)out | (size_t)bias) & 15) != 0) return false;   // (out may alias h: a block reads its whole tile first)
  const int GB = std::max(1, tb_env_int("TRUSS_GCN_SLAB_ITEMS", 512) / (8 * N));   // graphs per block: >= two rounds of items for small graphs
  const size_t lds = (size_t)GB * N * 8 * 16;
  if (lds > 48 * 1024) return false;
  const int C4 = C / 4;
  dim3 grid((unsigned)((B + GB - 1) / GB), (unsigned)((C4 + 7) / 8));
  hipLaunchKernelGGL(truss_gcn_aggregate_slab_kernel, grid, dim3(256), lds, st, adj, (long)a_stride, nbr, K, h, bias, out, B, N, C4, GB, act);
  return true;
}

// Sparse-pattern variant: thread = (graph, row, channel quad), flat over the launch; a row's <= 16 listed neighbours instead of
// all N columns.  The H rows a thread reads are 16-byte loads that the threads of a row issue contiguously (C floats); a graph's
// rows are re-read by their neighbours' threads from L2 / L1, so HBM sees H once and `out` once.
template <int KR>   // neighbours per round: all loads of a round are in flight together (KR = 12 covers a truss row in one round)
__global__ __launch_bounds__(256) void truss_gcn_aggregate_sparse_kernel(const float *__restrict__ adj, long a_stride,
                                                                         const int16_t *__restrict__ nbr, int K, const float *__restrict__ h,
                                                                         const float *__restrict__ bias, float *__restrict__ out, long total,
                                                                         int N, int C4, int act) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int c4 = (int)(t % C4);
  const long r = t / C4;
  const int i = (int)(r % N);
  const long b = r / N;
  const float *Arow = adj + b * a_stride + (long)i * N;
  const tb_f4 *Hb = (const tb_f4 *)h + (size_t)b * N * C4 + c4;
  const int16_t *nb = nbr + (long)i * K;
  tb_f4 acc = bias ? ((const tb_f4 *)bias)[c4] : (tb_f4){0.0f, 0.0f, 0.0f, 0.0f};
  for (int k0 = 0; k0 < K; k0 += KR) {
    int j[KR];
    float a[KR];
    tb_f4 hv[KR];
#pragma unroll
    for (int q = 0; q < KR; ++q) {
      j[q] = k0 + q < K ? (int)nb[k0 + q] : -1;
      const int jc = j[q] < 0 ? i : j[q];
      a[q] = Arow[jc];
      hv[q] = Hb[(size_t)jc * C4];
    }
#pragma unroll
    for (int q = 0; q < KR; ++q) {
      if (j[q] < 0) continue;
      tb_gcn_fma4(acc, a[q], hv[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = tb_gcn_act(acc[q], act);
  ((tb_f4 *)out)[t] = acc;
}

extern "C" int truss_gcn_aggregate_sparse(const float *adj, int64_t a_batch_stride, const int16_t *nbr, int32_t k_nbr, const float *h,
                                          const float *bias, float *out, int32_t n_batch, int32_t n_nodes, int32_t n_channels,
                                          int32_t act, void *stream) {
  if (int rc = tb_gcn_aggregate_sparse_check(adj, nbr, k_nbr, h, bias, out, n_batch, n_nodes, n_channels, act)) return rc;
  if (n_batch == 0) return TRUSS_OK;
  // up to 128 nodes the slab kernel (rows from LDS: 33-36 us at 64 / 128 nodes against 40-42; at 256 nodes a block walks 8 rounds
  // over its 32 KB tile and loses: 52 against 42 us, tools/agg_probe.py)
  if (n_nodes <= tb_env_int("TRUSS_GCN_SLAB_MAX_N", 128) &&
      tb_launch_gcn_slab(adj, a_batch_stride, nbr, k_nbr, h, bias, out, n_batch, n_nodes, n_channels, act, (hipStream_t)stream)) {
    return tb_launched("gcn slab aggregate launch failed: ");
  }
  const int C4 = n_channels / 4;
  const long total = (long)n_batch * n_nodes * C4;
  const dim3 grid((unsigned)((total + 255) / 256));
  const auto kern = k_nbr <= 4 ? truss_gcn_aggregate_sparse_kernel<4> : k_nbr <= 8 ? truss_gcn_aggregate_sparse_kernel<8> : truss_gcn_aggregate_sparse_kernel<12>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, adj, (long)a_batch_stride, nbr, k_nbr, h, bias, out, total, n_nodes, C4, act);
  return tb_launched("gcn sparse aggregate launch failed: ");
}

extern "C" int truss_gcn_aggregate(const float *adj, int64_t a_batch_stride, const float *h, const float *bias, float *out,
                                   int32_t n_batch, int32_t n_nodes, int32_t n_channels, int32_t act, void *stream) {
  if (int rc = tb_gcn_aggregate_check(adj, h, out, n_batch, n_nodes, n_channels, act)) return rc;
  if (n_batch == 0) return TRUSS_OK;
  // 17..64 nodes: the slab kernel (32 nodes: 58-61 us against 73-84 for the channel-quad kernel below, 64 nodes: 44 against 182 for
  // the thread-per-channel kernel and 75 for rocBLAS + bias + activation); <= 16 nodes: the channel-quad kernel (56 against 74 us)
  if (n_nodes > tb_env_int("TRUSS_GCN_SLAB_DENSE_ABOVE", 16) && tb_launch_gcn_slab(adj, a_batch_stride, nullptr, n_nodes, h, bias, out, n_batch, n_nodes, n_channels, act, (hipStream_t)stream)) {
    return tb_launched("gcn slab aggregate launch failed: ");
  }
  if ((n_channels & 3) == 0 && n_nodes <= 32 && (((size_t)h | (size_t)out | (size_t)bias) & 15) == 0) {
    // channel-quad threads, no idle lanes
    const int C4 = n_channels / 4;
    const int gmax = a_batch_stride ? 256 / C4 + 2 : 1;
    const size_t lds = (size_t)gmax * n_nodes * n_nodes * sizeof(float);
    const long total = (long)n_batch * C4;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (lds <= 64 * 1024) {
      const auto kern4 = n_nodes <= 16 ? truss_gcn_aggregate4_kernel<16> : truss_gcn_aggregate4_kernel<32>;
      hipLaunchKernelGGL(kern4, dim3(blocks), dim3(256), lds, (hipStream_t)stream, adj, (long)a_batch_stride, h, bias, out, n_batch, n_nodes, C4, act, gmax);
      return tb_launched("gcn aggregate launch failed: ");
    }
  }
  dim3 grid((unsigned)n_batch, (unsigned)((n_channels + 255) / 256));
  const auto kern = n_nodes <= 16 ? truss_gcn_aggregate_kernel<16> : n_nodes <= 32 ? truss_gcn_aggregate_kernel<32> : truss_gcn_aggregate_kernel<64>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, adj, (long)a_batch_stride, h, bias, out, n_nodes, n_channels, act);
  return tb_launched("gcn aggregate launch failed: ");
}
#endif  // __HIPCC__
