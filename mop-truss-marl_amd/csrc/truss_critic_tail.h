// truss_critic_tail.h -- the tail of a critic pass of the MADDPG update (include/truss_mi355.h, truss_critic_tail and
// truss_critic_tail_backward): the sum pools of the second GCN level, their concatenation and the three dense layers, forward in one
// launch and backward in two, for up to TRUSS_CRITIC_TAIL_MAX independent items (critic passes) per launch.
// Latency-bound work on small operands, no matrix cores: a workgroup of 512 threads owns TRUSS_CRITIC_TAIL_SAMPLES samples of one
// item end to end, its intermediate vectors live in LDS, rows of the weight matrices are read coalesced along their length and
// every row is read once for all samples of the workgroup.  No atomics, no grid-wide synchronisation: every output element has
// one owner and every sum a fixed order.  Every barrier is a top-level __syncthreads().
// On top the argument checks (host only: a stand-alone program can drive them); below them, for the device compiler only, the
// kernels and the C entries.  truss_hip.hip includes this file last.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

static int tb_fail(int code, const std::string &msg);

struct TbCtSpan {
  uintptr_t a;
  uint64_t bytes;
};
static inline bool tb_ct_overlaps(const std::vector<TbCtSpan> &outs, const std::vector<TbCtSpan> &ins) {
  for (size_t i = 0; i < outs.size(); ++i) {
    const TbCtSpan &x = outs[i];
    for (size_t j = 0; j < ins.size(); ++j)
      if (x.a < ins[j].a + ins[j].bytes && ins[j].a < x.a + x.bytes) return true;
    for (size_t j = i + 1; j < outs.size(); ++j)
      if (x.a < outs[j].a + outs[j].bytes && outs[j].a < x.a + x.bytes) return true;
  }
  return false;
}
static inline void tb_ct_span(std::vector<TbCtSpan> &v, const void *p, uint64_t floats) {
  if (p && floats) v.push_back(TbCtSpan{(uintptr_t)p, floats * sizeof(float)});
}
static inline int tb_ct_sizes(const std::string &me, int64_t B, int64_t N, int64_t L, int64_t H, int64_t Q) {
  if (B < 0 || N < 1 || L < 1 || H < 1 || Q < 1) return tb_fail(TRUSS_EINVAL, me + ": n_batch < 0 or a size < 1");
  if (L > TRUSS_CRITIC_TAIL_MAX_LAYERS || H > 256 || Q > 256 || L * H > 4096)
    return tb_fail(TRUSS_EUNSUPPORTED, me + ": outside the envelope n_layers <= 16, n_hidden <= 256, n_q <= 256, n_layers n_hidden <= 4096");
  if (N > INT32_MAX / 256) return tb_fail(TRUSS_EUNSUPPORTED, me + ": n_nodes beyond 2^23 - 1");
  return TRUSS_OK;
}

// everything is checked before anything is launched; *groups: the workgroups of the whole list
static inline int tb_critic_tail_check(const truss_critic_tail_args_t *items, int32_t n, int64_t *groups) {
  const std::string me = "truss_critic_tail";
  *groups = 0;
  if (n < 0 || (n > 0 && !items)) return tb_fail(TRUSS_EINVAL, me + ": n_items < 0 or NULL items");
  std::vector<TbCtSpan> ins, outs;
  for (int32_t k = 0; k < n; ++k) {
    const truss_critic_tail_args_t &a = items[k];
    if (a.struct_size != sizeof(truss_critic_tail_args_t)) return tb_fail(TRUSS_EINVAL, me + ": struct_size mismatch");
    if (int rc = tb_ct_sizes(me, a.n_batch, a.n_nodes, a.n_layers, a.n_hidden, a.n_q)) return rc;
    if (a.n_batch == 0) continue;
    const uint64_t B = a.n_batch, N = a.n_nodes, L = a.n_layers, H = a.n_hidden, Q = a.n_q;
    for (uint64_t i = 0; i < L; ++i) {
      if (!a.o[i]) return tb_fail(TRUSS_EINVAL, me + ": NULL o[i]");
      tb_ct_span(ins, a.o[i], B * N * H);
    }
    if (!a.w1 || !a.b1 || !a.w2 || !a.b2 || !a.w3 || !a.b3 || !a.q) return tb_fail(TRUSS_EINVAL, me + ": NULL parameter or q");
    if (a.save && (!a.p || !a.z1 || !a.z2)) return tb_fail(TRUSS_EINVAL, me + ": save needs p, z1 and z2");
    tb_ct_span(ins, a.w1, Q * L * H), tb_ct_span(ins, a.b1, Q), tb_ct_span(ins, a.w2, Q * Q), tb_ct_span(ins, a.b2, Q);
    tb_ct_span(ins, a.w3, Q), tb_ct_span(ins, a.b3, 1);
    tb_ct_span(outs, a.q, B);
    if (a.save) tb_ct_span(outs, a.p, B * L * H), tb_ct_span(outs, a.z1, B * Q), tb_ct_span(outs, a.z2, B * Q);
    *groups += (a.n_batch + TRUSS_CRITIC_TAIL_SAMPLES - 1) / TRUSS_CRITIC_TAIL_SAMPLES;
  }
  if (tb_ct_overlaps(outs, ins)) return tb_fail(TRUSS_EINVAL, me + ": an output overlaps an input or another output");
  return TRUSS_OK;
}

static inline bool tb_ct_bwd_wants_params(const truss_critic_tail_bwd_t &a) {
  return a.d_w1 || a.d_b1 || a.d_w2 || a.d_b2 || a.d_w3 || a.d_b3;
}
static inline bool tb_ct_bwd_wants_inputs(const truss_critic_tail_bwd_t &a) {
  for (int i = 0; i < a.n_layers; ++i)
    if (a.d_o[i]) return true;
  return false;
}
static inline int tb_critic_tail_bwd_check(const truss_critic_tail_bwd_t *items, int32_t n) {
  const std::string me = "truss_critic_tail_backward";
  if (n < 0 || (n > 0 && !items)) return tb_fail(TRUSS_EINVAL, me + ": n_items < 0 or NULL items");
  std::vector<TbCtSpan> ins, outs;
  for (int32_t k = 0; k < n; ++k) {
    const truss_critic_tail_bwd_t &a = items[k];
    if (a.struct_size != sizeof(truss_critic_tail_bwd_t)) return tb_fail(TRUSS_EINVAL, me + ": struct_size mismatch");
    if (int rc = tb_ct_sizes(me, a.n_batch, a.n_nodes, a.n_layers, a.n_hidden, a.n_q)) return rc;
    if (a.dq_stride < 0) return tb_fail(TRUSS_EINVAL, me + ": dq_stride < 0");
    const bool params = tb_ct_bwd_wants_params(a);
    if (a.n_batch == 0 || !(params || tb_ct_bwd_wants_inputs(a))) continue;
    const uint64_t B = a.n_batch, N = a.n_nodes, L = a.n_layers, H = a.n_hidden, Q = a.n_q;
    if (!a.dq || !a.z1 || !a.z2 || !a.w1 || !a.w2 || !a.w3) return tb_fail(TRUSS_EINVAL, me + ": NULL dq, z1, z2, w1, w2 or w3");
    if (a.d_w1 && !a.p) return tb_fail(TRUSS_EINVAL, me + ": d_w1 needs p");
    if (params && (!a.dz1 || !a.dz2)) return tb_fail(TRUSS_EINVAL, me + ": parameter gradients need the scratch dz1 and dz2");
    tb_ct_span(ins, a.dq, (B - 1) * (uint64_t)a.dq_stride + 1), tb_ct_span(ins, a.z1, B * Q), tb_ct_span(ins, a.z2, B * Q);
    tb_ct_span(ins, a.w1, Q * L * H), tb_ct_span(ins, a.w2, Q * Q), tb_ct_span(ins, a.w3, Q);
    if (a.d_w1) tb_ct_span(ins, a.p, B * L * H);
    for (uint64_t i = 0; i < L; ++i) tb_ct_span(outs, a.d_o[i], B * N * H), tb_ct_span(ins, a.o[i], B * N * H);
    if (params) tb_ct_span(outs, a.dz1, B * Q), tb_ct_span(outs, a.dz2, B * Q);
    tb_ct_span(outs, a.d_w1, Q * L * H), tb_ct_span(outs, a.d_b1, Q), tb_ct_span(outs, a.d_w2, Q * Q), tb_ct_span(outs, a.d_b2, Q);
    tb_ct_span(outs, a.d_w3, Q), tb_ct_span(outs, a.d_b3, 1);
  }
  if (tb_ct_overlaps(outs, ins)) return tb_fail(TRUSS_EINVAL, me + ": an output overlaps an input or another output");
  return TRUSS_OK;
}

#ifdef __HIPCC__
#define TB_CT_THREADS 512
#define TB_CT_S TRUSS_CRITIC_TAIL_SAMPLES
#define TB_CT_ROWS 4      // rows of a weight matrix a wave of the forward has in flight together
// which row families of an item take 16-byte accesses (decided by the host from the sizes and the pointers)
#define TB_CT_VEC_O 1   // o[i] / d_o[i] rows of H
#define TB_CT_VEC_W1 2  // rows of K1: w1 (and in launch B p, d_w1)
#define TB_CT_VEC_W2 4  // rows of Q: w2, w3 (and in launch B z1, d_w2)

struct CtItemDev {
  const float *o[TRUSS_CRITIC_TAIL_MAX_LAYERS];
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  float *q, *p, *z1, *z2;        // p, z1, z2: NULL without save
  int B, N, L, H, Q;
  int wg0;                       // the item's first workgroup of this launch
  int vec;
};
struct CtDev {
  CtItemDev it[TRUSS_CRITIC_TAIL_MAX];
  int n;
};
struct CtBwdItemDev {
  float *d_o[TRUSS_CRITIC_TAIL_MAX_LAYERS];
  const float *dq, *p, *z1, *z2, *w1, *w2, *w3;
  float *dz1, *dz2;              // NULL without parameter gradients
  float *d_w1, *d_b1, *d_w2, *d_b2, *d_w3, *d_b3;
  int B, N, L, H, Q;
  int wg0;                       // the item's first workgroup of the launch (A: groups of samples; B: rows)
  int vec;
  int inputs;                    // any d_o[i] wanted
  int dqs;                       // floats between the samples of dq
};
struct CtBwdDev {
  CtBwdItemDev it[TRUSS_CRITIC_TAIL_MAX];
  int n;
};
static_assert(sizeof(CtDev) < 2048 && sizeof(CtBwdDev) < 2048, "the descriptors travel in the kernel arguments");

// The item a workgroup belongs to: the last one whose first workgroup is <= g.  g is the workgroup's index, so every index into the
// by-value array is uniform over the workgroup (scalar loads from the argument block).
template <class D>
__device__ __forceinline__ int tb_ct_find(const D &A, int g) {
  int j = 0;
  for (int k = 1; k < TRUSS_CRITIC_TAIL_MAX; ++k)
    if (k < A.n && A.it[k].wg0 <= g) j = k;
  return j;
}

// sum over the 64 lanes, every lane gets it: lanes 2m and 2m + 1, then pairs of those, ... (the first four levels stay inside a row
// of 16 lanes: DPP; the last two cross rows)
__device__ __forceinline__ float tb_ct_wave_sum(float v) {
  auto dpp = [](float x, auto ctrl) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xf, 0xf, false));
  };
  v = v + dpp(v, std::integral_constant<int, 0xB1>{});    // quad_perm [1, 0, 3, 2]
  v = v + dpp(v, std::integral_constant<int, 0x4E>{});    // quad_perm [2, 3, 0, 1]
  v = v + dpp(v, std::integral_constant<int, 0x141>{});   // row_half_mirror: the other quad of the 8
  v = v + dpp(v, std::integral_constant<int, 0x140>{});   // row_mirror: the other 8 of the row
  v = v + __shfl_xor(v, 16);
  v = v + __shfl_xor(v, 32);
  return v;
}

// acc[t][s] += the lane's share of w_t . x_s for TB_CT_ROWS rows w_t and the TB_CT_S vectors x_s = x + s * xs in LDS: the element quads
// lane, lane + 64, ... of the K elements, in ascending order; vec: K is a multiple of 4 and the rows 16-byte aligned (xs is a
// multiple of 4 always).  The rows' loads are independent: TB_CT_ROWS of them are in flight together.
__device__ __forceinline__ void tb_ct_dot(const float *const (&w)[TB_CT_ROWS], const float *x, int xs, int K, bool vec, int lane,
                                          float (&acc)[TB_CT_ROWS][TB_CT_S]) {
  if (vec) {
    const int KQ = K >> 2;
#pragma unroll 2
    for (int c = lane; c < KQ; c += 64) {
      tb_f4 wv[TB_CT_ROWS];
      TRUSS_UNROLL
      for (int t = 0; t < TB_CT_ROWS; ++t) wv[t] = *(const tb_f4 *)(w[t] + 4 * c);
      TRUSS_UNROLL
      for (int s = 0; s < TB_CT_S; ++s) {
        const tb_f4 xv = *(const tb_f4 *)(x + s * xs + 4 * c);
        TRUSS_UNROLL
        for (int t = 0; t < TB_CT_ROWS; ++t) {
          TRUSS_UNROLL
          for (int j = 0; j < 4; ++j) acc[t][s] = acc[t][s] + wv[t][j] * xv[j];
        }
      }
    }
  } else {
    for (int c = lane; 4 * c < K; c += 64) {
      TRUSS_UNROLL
      for (int j = 0; j < 4; ++j) {
        const int k = 4 * c + j;
        if (k < K) {
          TRUSS_UNROLL
          for (int t = 0; t < TB_CT_ROWS; ++t) {
            const float wv = w[t][k];
            TRUSS_UNROLL
            for (int s = 0; s < TB_CT_S; ++s) acc[t][s] = acc[t][s] + wv * x[s * xs + k];
          }
        }
      }
    }
  }
}

// one dense layer for the workgroup's samples: y_s[r] = act(w[r] . x_s + bias[r]); a wave takes the rows wave, wave + 8, ... of
// w [R][K], TB_CT_ROWS of them at a time (beyond R: the last row again, not written); y in LDS (stride ys), and to
// g[(b0 + s) * R + r] for the live samples when g is not NULL
template <bool RELU>
__device__ __forceinline__ void tb_ct_dense(const float *__restrict__ w, const float *__restrict__ bias, int R, int K, bool vec, const float *x,
                                            int xs, float *y, int ys, float *g, long b0, int ns, int tid) {
  constexpr int WAVES = TB_CT_THREADS / 64;
  const int lane = tid & 63;
  for (int r = tid >> 6; r < R; r += WAVES * TB_CT_ROWS) {
    const float *wr[TB_CT_ROWS];
    float acc[TB_CT_ROWS][TB_CT_S];
    TRUSS_UNROLL
    for (int t = 0; t < TB_CT_ROWS; ++t) {
      wr[t] = w + (long)min(r + WAVES * t, R - 1) * K;
      TRUSS_UNROLL
      for (int s = 0; s < TB_CT_S; ++s) acc[t][s] = 0.0f;
    }
    tb_ct_dot(wr, x, xs, K, vec, lane, acc);
    TRUSS_UNROLL
    for (int t = 0; t < TB_CT_ROWS; ++t) {
      TRUSS_UNROLL
      for (int s = 0; s < TB_CT_S; ++s) acc[t][s] = tb_ct_wave_sum(acc[t][s]);
    }
    TRUSS_UNROLL
    for (int t = 0; t < TB_CT_ROWS; ++t) {
      const int rt = r + WAVES * t;            // uniform over the wave
      if (rt < R) {
        const float br = bias[rt];
        TRUSS_UNROLL
        for (int s = 0; s < TB_CT_S; ++s) {
          float v = acc[t][s] + br;
          if (RELU) v = fmaxf(v, 0.0f);
          if (lane == s) {
            if (y) y[s * ys + rt] = v;
            if (g && s < ns) g[(b0 + s) * R + rt] = v;
          }
        }
      }
    }
  }
}

// LDS of the forward and of launch A, in floats: three families of TB_CT_S vectors, then the layers' pointers
__host__ __device__ static inline int tb_ct_lds_floats(int K1, int Q) {
  return TB_CT_S * (((K1 + 3) & ~3) + 2 * ((Q + 3) & ~3)) + 2 * TRUSS_CRITIC_TAIL_MAX_LAYERS;
}

__global__ __launch_bounds__(TB_CT_THREADS) void truss_critic_tail_kernel(const CtDev A) {
  extern __shared__ __attribute__((aligned(16))) float tb_ct_lds[];
  const int tid = threadIdx.x, g = blockIdx.x;
  const CtItemDev &T = A.it[tb_ct_find(A, g)];
  const int N = T.N, L = T.L, H = T.H, Q = T.Q, K1 = L * H, KP = (K1 + 3) & ~3, QP = (Q + 3) & ~3;
  const long b0 = (long)(g - T.wg0) * TB_CT_S;
  const int ns = T.B - b0 < TB_CT_S ? (int)(T.B - b0) : TB_CT_S;
  float *p = tb_ct_lds, *z1 = p + TB_CT_S * KP, *z2 = z1 + TB_CT_S * QP;
  const float **optr = (const float **)(z2 + TB_CT_S * QP);
  // the layers' pointers to LDS: i is uniform here, lane-varying below
  for (int i = 0; i < L; ++i)
    if (tid == i) optr[i] = T.o[i];
  __syncthreads();
  // the pools of the workgroup's samples: one owner per element (quad), nodes in ascending order; dead samples: zeros
  if (T.vec & TB_CT_VEC_O) {
    const int HQ = H >> 2, per = L * HQ;
    for (int e = tid; e < TB_CT_S * per; e += TB_CT_THREADS) {
      const int s = e / per, r = e - s * per, i = r / HQ, cq = r - i * HQ;
      tb_f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      if (s < ns) {
        const tb_f4 *src = (const tb_f4 *)(optr[i] + (b0 + s) * N * H) + cq;
        acc = src[0];
#pragma unroll 8
        for (int n = 1; n < N; ++n) acc = acc + src[(long)n * HQ];
        if (T.p) {
          float *dst = T.p + (b0 + s) * K1 + i * H + 4 * cq;
          dst[0] = acc[0], dst[1] = acc[1], dst[2] = acc[2], dst[3] = acc[3];
        }
      }
      *(tb_f4 *)(p + s * KP + i * H + 4 * cq) = acc;
    }
  } else {
    for (int e = tid; e < TB_CT_S * K1; e += TB_CT_THREADS) {
      const int s = e / K1, r = e - s * K1, i = r / H, c = r - i * H;
      float acc = 0.0f;
      if (s < ns) {
        const float *src = optr[i] + (b0 + s) * N * H + c;
        acc = src[0];
#pragma unroll 8
        for (int n = 1; n < N; ++n) acc = acc + src[(long)n * H];
        if (T.p) T.p[(b0 + s) * K1 + r] = acc;
      }
      p[s * KP + r] = acc;
    }
  }
  __syncthreads();
  tb_ct_dense<true>(T.w1, T.b1, Q, K1, (T.vec & TB_CT_VEC_W1) != 0, p, KP, z1, QP, T.z1, b0, ns, tid);
  __syncthreads();
  tb_ct_dense<true>(T.w2, T.b2, Q, Q, (T.vec & TB_CT_VEC_W2) != 0, z1, QP, z2, QP, T.z2, b0, ns, tid);
  __syncthreads();
  // the output unit: one row, wave 0
  if (tid < 64) tb_ct_dense<false>(T.w3, T.b3, 1, Q, (T.vec & TB_CT_VEC_W2) != 0, z2, QP, nullptr, 0, T.q, b0, ns, tid);
}

// Launch A of the backward: dz2, dz1 and dp of the workgroup's samples in LDS, dz1 / dz2 to the caller's scratch where launch B
// follows, dp broadcast over the nodes into the wanted d_o[i].
__global__ __launch_bounds__(TB_CT_THREADS) void truss_critic_tail_bwd_kernel(const CtBwdDev A) {
  extern __shared__ __attribute__((aligned(16))) float tb_ct_lds[];
  const int tid = threadIdx.x, g = blockIdx.x;
  const CtBwdItemDev &T = A.it[tb_ct_find(A, g)];
  const int N = T.N, L = T.L, H = T.H, Q = T.Q, K1 = L * H, KP = (K1 + 3) & ~3, QP = (Q + 3) & ~3;
  const long b0 = (long)(g - T.wg0) * TB_CT_S;
  const int ns = T.B - b0 < TB_CT_S ? (int)(T.B - b0) : TB_CT_S;
  float *dp = tb_ct_lds, *dz1 = dp + TB_CT_S * KP, *dz2 = dz1 + TB_CT_S * QP;
  // dz2 = (dq w3) [z2 > 0]; dead samples: zeros
  for (int e = tid; e < TB_CT_S * Q; e += TB_CT_THREADS) {
    const int s = e / Q, k = e - s * Q;
    float v = 0.0f;
    if (s < ns) {
      const long at = (b0 + s) * Q + k;
      v = T.z2[at] > 0.0f ? T.dq[(b0 + s) * T.dqs] * T.w3[k] : 0.0f;
      if (T.dz2) T.dz2[at] = v;
    }
    dz2[s * QP + k] = v;
  }
  __syncthreads();
  // dz1_j = (sum_k dz2_k W2[k][j]) [z1_j > 0]: the thread owns (s, j), rows of W2 are read along j
  for (int e = tid; e < TB_CT_S * Q; e += TB_CT_THREADS) {
    const int s = e / Q, j = e - s * Q;
    float v = 0.0f;
    if (s < ns) {
      const float *w = T.w2 + j, *d = dz2 + s * QP;
      float acc = 0.0f;
#pragma unroll 16
      for (int k = 0; k < Q; ++k) acc = acc + d[k] * w[(long)k * Q];
      const long at = (b0 + s) * Q + j;
      v = T.z1[at] > 0.0f ? acc : 0.0f;
      if (T.dz1) T.dz1[at] = v;
    }
    dz1[s * QP + j] = v;
  }
  __syncthreads();
  // dp_m = sum_j dz1_j W1[j][m]: the thread owns column (quad) m of all the workgroup's samples, rows of W1 are read along m
  if (T.inputs) {
    if (T.vec & TB_CT_VEC_W1) {
      for (int c = tid; 4 * c < K1; c += TB_CT_THREADS) {
        tb_f4 acc[TB_CT_S];
        TRUSS_UNROLL
        for (int s = 0; s < TB_CT_S; ++s) acc[s] = tb_f4{0.0f, 0.0f, 0.0f, 0.0f};
        const tb_f4 *w = (const tb_f4 *)T.w1 + c;
        const int KQ = K1 >> 2;
#pragma unroll 8
        for (int j = 0; j < Q; ++j) {
          const tb_f4 wv = w[(long)j * KQ];
          TRUSS_UNROLL
          for (int s = 0; s < TB_CT_S; ++s) acc[s] = acc[s] + dz1[s * QP + j] * wv;
        }
        TRUSS_UNROLL
        for (int s = 0; s < TB_CT_S; ++s) *(tb_f4 *)(dp + s * KP + 4 * c) = acc[s];
      }
    } else {
      for (int m = tid; m < K1; m += TB_CT_THREADS) {
        float acc[TB_CT_S];
        TRUSS_UNROLL
        for (int s = 0; s < TB_CT_S; ++s) acc[s] = 0.0f;
        const float *w = T.w1 + m;
#pragma unroll 8
        for (int j = 0; j < Q; ++j) {
          const float wv = w[(long)j * K1];
          TRUSS_UNROLL
          for (int s = 0; s < TB_CT_S; ++s) acc[s] = acc[s] + dz1[s * QP + j] * wv;
        }
        TRUSS_UNROLL
        for (int s = 0; s < TB_CT_S; ++s) dp[s * KP + m] = acc[s];
      }
    }
  }
  __syncthreads();
  // d_o[i][b][n][:] = dp[b][i H :] for every node: (s, i) uniform, the threads over the nodes' rows
  for (int si = 0; si < ns * L; ++si) {
    const int s = si / L, i = si - s * L;
    float *dst = T.d_o[i];
    if (!dst) continue;
    dst += (b0 + s) * N * H;
    const float *src = dp + s * KP + i * H;
    if (T.vec & TB_CT_VEC_O) {
      const int HQ = H >> 2;
      for (int e = tid; e < N * HQ; e += TB_CT_THREADS) ((tb_f4 *)dst)[e] = *(const tb_f4 *)(src + 4 * (e % HQ));
    } else {
      for (int e = tid; e < N * H; e += TB_CT_THREADS) dst[e] = src[e % H];
    }
  }
}

// acc over the samples in ascending b of a[b * as] * x[b * xs + m] for the columns m of a row of `cols`: 256 threads, one owner each
__device__ __forceinline__ void tb_ct_outer_row(float *__restrict__ out, const float *__restrict__ a, int as, const float *__restrict__ x, int cols,
                                                int B, bool vec, int tid) {
  if (vec) {
    const int CQ = cols >> 2;
    for (int c = tid; c < CQ; c += 256) {
      tb_f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 8
      for (int b = 0; b < B; ++b) acc = acc + a[(long)b * as] * ((const tb_f4 *)x)[(long)b * CQ + c];
      ((tb_f4 *)out)[c] = acc;
    }
  } else {
    for (int m = tid; m < cols; m += 256) {
      float acc = 0.0f;
#pragma unroll 8
      for (int b = 0; b < B; ++b) acc = acc + a[(long)b * as] * x[(long)b * cols + m];
      out[m] = acc;
    }
  }
}

// Launch B of the backward: workgroup r < Q of an item owns row r of d_w1 and of d_w2 and element r of d_b1 and d_b2; workgroup Q
// owns d_w3 and d_b3
__global__ __launch_bounds__(256) void truss_critic_tail_bwd_params_kernel(const CtBwdDev A) {
  const int tid = threadIdx.x, g = blockIdx.x;
  const CtBwdItemDev &T = A.it[tb_ct_find(A, g)];
  const int B = T.B, Q = T.Q, K1 = T.L * T.H, r = g - T.wg0;
  if (r < Q) {
    if (T.d_w1) tb_ct_outer_row(T.d_w1 + (long)r * K1, T.dz1 + r, Q, T.p, K1, B, (T.vec & TB_CT_VEC_W1) != 0, tid);
    if (T.d_w2) tb_ct_outer_row(T.d_w2 + (long)r * Q, T.dz2 + r, Q, T.z1, Q, B, (T.vec & TB_CT_VEC_W2) != 0, tid);
    if ((tid == 0 && T.d_b1) || (tid == 64 && T.d_b2)) {
      const float *d = (tid == 0 ? T.dz1 : T.dz2) + r;
      float acc = 0.0f;
      for (int b = 0; b < B; ++b) acc = acc + d[(long)b * Q];
      (tid == 0 ? T.d_b1 : T.d_b2)[r] = acc;
    }
  } else {
    if (T.d_w3) {
      for (int k = tid; k < Q; k += 256) {
        float acc = 0.0f;
        for (int b = 0; b < B; ++b) acc = acc + T.dq[(long)b * T.dqs] * T.z2[(long)b * Q + k];
        T.d_w3[k] = acc;
      }
    }
    if (tid == 0 && T.d_b3) {
      float acc = 0.0f;
      for (int b = 0; b < B; ++b) acc = acc + T.dq[(long)b * T.dqs];
      T.d_b3[0] = acc;
    }
  }
}

static inline bool tb_ct_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// dynamic LDS beyond 64 KiB is an opt-in per kernel and device (TbLdsOptIn, truss_hip.hip)
static int tb_ct_lds_optin(const void *kern, size_t bytes, TbLdsOptIn &optin) { return bytes > 64 * 1024 ? optin.ensure(kern) : TRUSS_OK; }

extern "C" int truss_critic_tail(const truss_critic_tail_args_t *items, int32_t n_items, void *stream) {
  int64_t groups = 0;
  if (int rc = tb_critic_tail_check(items, n_items, &groups)) return rc;
  if (groups > INT32_MAX) return tb_fail(TRUSS_EUNSUPPORTED, "truss_critic_tail: more than 2^31 - 1 workgroups");
  static TbLdsOptIn optin;
  int32_t k = 0;
  while (k < n_items) {
    CtDev A;
    memset(&A, 0, sizeof A);
    int64_t wgs = 0;
    int lds = 0;
    for (; k < n_items && A.n < TRUSS_CRITIC_TAIL_MAX; ++k) {
      const truss_critic_tail_args_t &a = items[k];
      if (a.n_batch == 0) continue;
      CtItemDev &T = A.it[A.n++];
      const int K1 = a.n_layers * a.n_hidden;
      bool vo = a.n_hidden % 4 == 0;
      for (int i = 0; i < a.n_layers; ++i) T.o[i] = a.o[i], vo = vo && tb_ct_al16(a.o[i]);
      T.w1 = a.w1, T.b1 = a.b1, T.w2 = a.w2, T.b2 = a.b2, T.w3 = a.w3, T.b3 = a.b3, T.q = a.q;
      if (a.save) T.p = a.p, T.z1 = a.z1, T.z2 = a.z2;
      T.B = a.n_batch, T.N = a.n_nodes, T.L = a.n_layers, T.H = a.n_hidden, T.Q = a.n_q, T.wg0 = (int)wgs;
      T.vec = (vo ? TB_CT_VEC_O : 0) | (K1 % 4 == 0 && tb_ct_al16(a.w1) ? TB_CT_VEC_W1 : 0) |
              (a.n_q % 4 == 0 && tb_ct_al16(a.w2) && tb_ct_al16(a.w3) ? TB_CT_VEC_W2 : 0);
      wgs += (a.n_batch + TB_CT_S - 1) / TB_CT_S;
      lds = std::max(lds, tb_ct_lds_floats(K1, a.n_q));
    }
    if (A.n == 0) continue;
    const size_t bytes = (size_t)lds * sizeof(float);
    if (int rc = tb_ct_lds_optin((const void *)truss_critic_tail_kernel, bytes, optin)) return rc;
    hipLaunchKernelGGL(truss_critic_tail_kernel, dim3((unsigned)wgs), dim3(TB_CT_THREADS), bytes, (hipStream_t)stream, A);
    if (int rc = tb_launched("critic tail launch failed: ")) return rc;
  }
  return TRUSS_OK;
}

extern "C" int truss_critic_tail_backward(const truss_critic_tail_bwd_t *items, int32_t n_items, void *stream) {
  if (int rc = tb_critic_tail_bwd_check(items, n_items)) return rc;
  static TbLdsOptIn optin;
  int32_t k = 0;
  while (k < n_items) {
    CtBwdDev A, P;                 // launch A: every live item; launch B: those with parameter gradients
    memset(&A, 0, sizeof A);
    memset(&P, 0, sizeof P);
    int64_t wgs = 0, rows = 0;
    int lds = 0;
    for (; k < n_items && A.n < TRUSS_CRITIC_TAIL_MAX; ++k) {
      const truss_critic_tail_bwd_t &a = items[k];
      const bool params = tb_ct_bwd_wants_params(a), inputs = tb_ct_bwd_wants_inputs(a);
      if (a.n_batch == 0 || !(params || inputs)) continue;
      CtBwdItemDev &T = A.it[A.n++];
      const int K1 = a.n_layers * a.n_hidden;
      bool vo = a.n_hidden % 4 == 0;
      for (int i = 0; i < a.n_layers; ++i) T.d_o[i] = a.d_o[i], vo = vo && tb_ct_al16(a.d_o[i]);
      T.dq = a.dq, T.p = a.p, T.z1 = a.z1, T.z2 = a.z2, T.w1 = a.w1, T.w2 = a.w2, T.w3 = a.w3;
      if (params) T.dz1 = a.dz1, T.dz2 = a.dz2;
      T.d_w1 = a.d_w1, T.d_b1 = a.d_b1, T.d_w2 = a.d_w2, T.d_b2 = a.d_b2, T.d_w3 = a.d_w3, T.d_b3 = a.d_b3;
      T.B = a.n_batch, T.N = a.n_nodes, T.L = a.n_layers, T.H = a.n_hidden, T.Q = a.n_q, T.wg0 = (int)wgs, T.inputs = inputs, T.dqs = a.dq_stride;
      // launch A reads w1 by rows of K1; launch B reads p and writes d_w1 by rows of K1, reads z1 and writes d_w2 by rows of Q
      T.vec = (vo ? TB_CT_VEC_O : 0) | (K1 % 4 == 0 && tb_ct_al16(a.w1) ? TB_CT_VEC_W1 : 0);
      wgs += (a.n_batch + TB_CT_S - 1) / TB_CT_S;
      lds = std::max(lds, tb_ct_lds_floats(K1, a.n_q));
      if (params) {
        CtBwdItemDev &R = P.it[P.n++];
        R = T;
        R.wg0 = (int)rows;
        R.vec = (K1 % 4 == 0 && tb_ct_al16(a.p) && tb_ct_al16(a.d_w1) ? TB_CT_VEC_W1 : 0) |
                (a.n_q % 4 == 0 && tb_ct_al16(a.z1) && tb_ct_al16(a.d_w2) ? TB_CT_VEC_W2 : 0);
        rows += a.n_q + 1;
      }
    }
    if (A.n == 0) continue;
    if (wgs > INT32_MAX) return tb_fail(TRUSS_EUNSUPPORTED, "truss_critic_tail_backward: more than 2^31 - 1 workgroups");
    const size_t bytes = (size_t)lds * sizeof(float);
    if (int rc = tb_ct_lds_optin((const void *)truss_critic_tail_bwd_kernel, bytes, optin)) return rc;
    hipLaunchKernelGGL(truss_critic_tail_bwd_kernel, dim3((unsigned)wgs), dim3(TB_CT_THREADS), bytes, (hipStream_t)stream, A);
    if (int rc = tb_launched("critic tail backward launch failed: ")) return rc;
    if (P.n > 0) {
      hipLaunchKernelGGL(truss_critic_tail_bwd_params_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, P);
      if (int rc = tb_launched("critic tail parameter gradients launch failed: ")) return rc;
    }
  }
  return TRUSS_OK;
}
#endif  // __HIPCC__
