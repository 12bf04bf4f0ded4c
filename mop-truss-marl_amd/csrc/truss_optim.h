// truss_optim.h -- one optimiser step of the MADDPG update over a list of parameter tensors (include/truss_mi355.h,
// truss_optim_step): per-tensor gradient clip to L2 norm <= 1, then Adam with persistent moments or the first step of a fresh Adam.
// Pure streaming, two launches: truss_optim_norm_kernel writes the float64 sum of squares of every chunk of TRUSS_OPTIM_CHUNK
// gradient elements, truss_optim_apply_kernel adds its tensor's partial sums in chunk order, forms the clip factor and updates its
// chunk.  One 256-thread workgroup per chunk in both, thread t of a chunk owns the four element quads t, t + 256, t + 512, t + 768:
// 16-byte accesses where every address of the chunk allows and its length is a multiple of 4, word by word otherwise, the same
// elements either way.  No atomics, no
// grid-wide synchronisation: every output element has one owner and every sum a fixed order.
// On top the argument check (host only: a stand-alone program can drive it); below it, for the device compiler only, the kernels
// and the C entry.  truss_hip.hip includes this file last.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

static int tb_fail(int code, const std::string &msg);

static inline bool tb_optim_overlaps(const void *p, uint64_t bytes, const float *g, uint64_t g_bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)g;
  return p && a < b + g_bytes && b < a + bytes;
}

// everything is checked before anything is launched; *n_chunks: the chunks of the whole list (the doubles of `partials`)
static inline int tb_optim_check(const truss_optim_args_t *a, int64_t *n_chunks) {
  if (!a || a->struct_size != sizeof(truss_optim_args_t)) return tb_fail(TRUSS_EINVAL, "truss_optim_step: struct_size mismatch");
  if (a->mode != TRUSS_OPTIM_ADAM && a->mode != TRUSS_OPTIM_FIRST_STEP) return tb_fail(TRUSS_EINVAL, "truss_optim_step: unknown mode");
  if (a->n_tensors < 0) return tb_fail(TRUSS_EINVAL, "truss_optim_step: n_tensors < 0");
  *n_chunks = 0;
  if (a->n_tensors == 0) return TRUSS_OK;
  if (!a->tensors || !a->grad || !a->partials) return tb_fail(TRUSS_EINVAL, "truss_optim_step: NULL tensors / grad / partials");
  if (a->mode == TRUSS_OPTIM_ADAM && (!a->exp_avg || !a->exp_avg_sq || !a->step))
    return tb_fail(TRUSS_EINVAL, "truss_optim_step: TRUSS_OPTIM_ADAM needs exp_avg, exp_avg_sq and step");
  if (!std::isfinite(a->lr) || !std::isfinite(a->eps) || !(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0))
    return tb_fail(TRUSS_EINVAL, "truss_optim_step: lr and eps must be finite, the betas in [0, 1)");
  int64_t end = INT64_MIN, chunks = 0;
  for (int32_t i = 0; i < a->n_tensors; ++i) {
    const truss_optim_tensor_t &t = a->tensors[i];
    if (!t.p) return tb_fail(TRUSS_EINVAL, "truss_optim_step: NULL parameter pointer");
    if (t.numel < 1 || t.numel > INT32_MAX) return tb_fail(TRUSS_EINVAL, "truss_optim_step: numel outside 1..2^31-1");
    if (t.offset < 0 || t.offset < end || t.offset > INT64_MAX / 8 - t.numel)
      return tb_fail(TRUSS_EINVAL, "truss_optim_step: the tensors' ranges must be ascending and disjoint");
    end = t.offset + t.numel;
    chunks += (t.numel + TRUSS_OPTIM_CHUNK - 1) / TRUSS_OPTIM_CHUNK;
  }
  // what the call writes must not overlap what it reads of grad: the span of the tensors' ranges
  const int64_t first = a->tensors[0].offset;
  const float *g0 = a->grad + first;
  const uint64_t span = (uint64_t)(end - first) * sizeof(float);
  bool over = tb_optim_overlaps(a->partials, (uint64_t)chunks * sizeof(double), g0, span) ||
              tb_optim_overlaps(a->norms, (uint64_t)a->n_tensors * sizeof(float), g0, span) ||
              tb_optim_overlaps(a->clipped ? a->clipped + first : nullptr, span, g0, span);
  if (a->mode == TRUSS_OPTIM_ADAM)
    over = over || tb_optim_overlaps(a->exp_avg + first, span, g0, span) || tb_optim_overlaps(a->exp_avg_sq + first, span, g0, span);
  for (int32_t i = 0; i < a->n_tensors && !over; ++i)
    over = tb_optim_overlaps(a->tensors[i].p, (uint64_t)a->tensors[i].numel * sizeof(float), g0, span);
  if (over) return tb_fail(TRUSS_EINVAL, "truss_optim_step: an output overlaps grad");
  *n_chunks = chunks;
  return TRUSS_OK;
}

#ifdef __HIPCC__
struct OptimTensorDev {
  float *p;
  long offset;                   // of the tensor in the flat vectors
  int numel;
  int chunk0;                    // the tensor's first chunk (= workgroup) of this launch
};
struct OptimDev {
  OptimTensorDev t[TRUSS_OPTIM_MAX_TENSORS];      // 160 x 24 bytes of kernel arguments
  const float *grad;
  float *m, *v;
  const double *step;
  double *partials;              // this launch's: [chunk]
  float *clipped;
  float *norms;                  // this launch's: [tensor]
  double lr, b1, b2, eps;
  int n;                         // tensors of this launch
};
static_assert(sizeof(OptimDev) < 4096, "the descriptors travel in the kernel arguments");

// The tensor a chunk belongs to: the last one whose first chunk is <= c.  c is the workgroup's index, so every index into the
// by-value array is uniform over the workgroup (scalar loads from the argument block; a lane-varying one would move it to scratch).
__device__ __forceinline__ int tb_optim_find(const OptimDev &A, int c) {
  int lo = 0, hi = A.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (A.t[mid].chunk0 <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The 16 elements of thread `tid` of a chunk of n live elements at x; beyond n: 0.  VEC: n is a multiple of 4 and x 16-byte aligned, so
// a quad is inside the chunk or outside it as a whole.  Every load is issued, from an address inside the chunk (the last quad / the
// last element where the thread's own lies beyond n), and masked afterwards: straight-line code, all loads in flight together.
template <bool VEC>
__device__ __forceinline__ void tb_optim_load(const float *x, int n, int tid, float (&r)[16]) {
  TRUSS_UNROLL
  for (int q = 0; q < 4; ++q) {
    const int e = (tid + 256 * q) * 4;
    if constexpr (VEC) {
      const tb_f4 t = *(const tb_f4 *)(x + min(e, n - 4));
      TRUSS_UNROLL
      for (int j = 0; j < 4; ++j) r[4 * q + j] = e < n ? t[j] : 0.0f;
    } else {
      TRUSS_UNROLL
      for (int j = 0; j < 4; ++j) {
        const float t = x[min(e + j, n - 1)];
        r[4 * q + j] = e + j < n ? t : 0.0f;
      }
    }
  }
}
template <bool VEC>
__device__ __forceinline__ void tb_optim_store(float *x, int n, int tid, const float (&r)[16]) {
  TRUSS_UNROLL
  for (int q = 0; q < 4; ++q) {
    const int e = (tid + 256 * q) * 4;
    if constexpr (VEC) {
      tb_f4 t;
      t[0] = r[4 * q], t[1] = r[4 * q + 1], t[2] = r[4 * q + 2], t[3] = r[4 * q + 3];
      if (e < n) *(tb_f4 *)(x + e) = t;
    } else {
      TRUSS_UNROLL
      for (int j = 0; j < 4; ++j)
        if (e + j < n) x[e + j] = r[4 * q + j];
    }
  }
}

__global__ __launch_bounds__(256) void truss_optim_norm_kernel(const OptimDev A) {
  __shared__ double wave_sum[4];
  const int c = blockIdx.x, tid = threadIdx.x;
  const OptimTensorDev &T = A.t[tb_optim_find(A, c)];
  const int e0 = (c - T.chunk0) * TRUSS_OPTIM_CHUNK;
  const int n = min(TRUSS_OPTIM_CHUNK, T.numel - e0);
  const float *g = A.grad + T.offset + e0;
  float x[16];
  if ((((uintptr_t)g & 15) | (n & 3)) == 0) tb_optim_load<true>(g, n, tid, x);
  else tb_optim_load<false>(g, n, tid, x);
  // per thread in element order, a butterfly within the wave, the four waves in wave order
  double s = 0.0;
  TRUSS_UNROLL
  for (int j = 0; j < 16; ++j) s += (double)x[j] * (double)x[j];
  s = tb_group_reduce_sum<64>(s);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) A.partials[c] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// lane j (uniform) of a double
__device__ __forceinline__ double tb_optim_lane(double v, int j) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

template <int MODE, bool VEC>
__device__ __forceinline__ void tb_optim_apply(const OptimDev &A, const OptimTensorDev &T, int it, int c, int e0, int n, int tid) {
  constexpr bool ADAM = MODE == TRUSS_OPTIM_ADAM;
  const long o = T.offset + e0;
  float g[16], w[16], m[16], v[16];
  // every load of the chunk first; the partial sums and the step's scalars are in flight with them
  tb_optim_load<VEC>(A.grad + o, n, tid, g);
  tb_optim_load<VEC>(T.p + e0, n, tid, w);
  if constexpr (ADAM) {
    tb_optim_load<VEC>(A.m + o, n, tid, m);
    tb_optim_load<VEC>(A.v + o, n, tid, v);
  }
  // the tensor's sum of squares: its partials in chunk order -- 64 at a time, one per lane, added lane by lane; every wave of every
  // workgroup of the tensor does the same additions
  const int c1 = T.chunk0 + (T.numel - 1) / TRUSS_OPTIM_CHUNK + 1, lane = tid & 63;
  double s = 0.0;
  for (int b = T.chunk0; b < c1; b += 64) {
    const int cnt = min(64, c1 - b);
    const double part = lane < cnt ? A.partials[b + lane] : 0.0;
    for (int j = 0; j < cnt; ++j) s += tb_optim_lane(part, j);
  }
  const float norm = (float)sqrt(s);
  const float fac = fminf(1.0f, 1.0f / (norm + 1e-12f));
  if (A.norms && c == T.chunk0 && tid == 0) A.norms[it] = norm;
  TRUSS_UNROLL
  for (int j = 0; j < 16; ++j) g[j] = g[j] * fac;
  if (A.clipped) tb_optim_store<VEC>(A.clipped + o, n, tid, g);
  const float eps = (float)A.eps;
  if constexpr (ADAM) {
    const double t = *A.step;
    const float w1 = (float)(1.0 - A.b1), b2 = (float)A.b2, w2 = (float)(1.0 - A.b2);
    const float bc2_sqrt = (float)sqrt(1.0 - pow(A.b2, t)), scale = (float)(-A.lr / (1.0 - pow(A.b1, t)));
    TRUSS_UNROLL
    for (int j = 0; j < 16; ++j) {
      m[j] = m[j] + w1 * (g[j] - m[j]);
      v[j] = v[j] * b2 + (w2 * g[j]) * g[j];
      const float den = sqrtf(v[j]) / bc2_sqrt + eps;
      w[j] = w[j] + ((1.0f / den) * m[j]) * scale;
    }
    tb_optim_store<VEC>(A.m + o, n, tid, m);
    tb_optim_store<VEC>(A.v + o, n, tid, v);
  } else {
    const float scale = (float)(-A.lr);
    TRUSS_UNROLL
    for (int j = 0; j < 16; ++j) w[j] = w[j] + scale * (g[j] / (fabsf(g[j]) + eps));
  }
  tb_optim_store<VEC>(T.p + e0, n, tid, w);
}

template <int MODE>
__global__ __launch_bounds__(256) void truss_optim_apply_kernel(const OptimDev A) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const int it = tb_optim_find(A, c);
  const OptimTensorDev &T = A.t[it];
  const int e0 = (c - T.chunk0) * TRUSS_OPTIM_CHUNK;
  const int n = min(TRUSS_OPTIM_CHUNK, T.numel - e0);
  const long o = T.offset + e0;
  // 16-byte accesses: every address of the chunk aligned (a chunk starts a multiple of 16 KB into its tensor: its alignment is the
  // tensor's) and whole quads only
  uintptr_t al = (uintptr_t)(A.grad + o) | (uintptr_t)T.p | (A.clipped ? (uintptr_t)(A.clipped + o) : 0);
  if (MODE == TRUSS_OPTIM_ADAM) al |= (uintptr_t)(A.m + o) | (uintptr_t)(A.v + o);
  if (((al & 15) | (n & 3)) == 0) tb_optim_apply<MODE, true>(A, T, it, c, e0, n, tid);
  else tb_optim_apply<MODE, false>(A, T, it, c, e0, n, tid);
}

extern "C" int truss_optim_step(const truss_optim_args_t *args, void *stream) {
  int64_t n_chunks = 0;
  if (int rc = tb_optim_check(args, &n_chunks)) return rc;
  const truss_optim_args_t &a = *args;
  const bool adam = a.mode == TRUSS_OPTIM_ADAM;
  int64_t chunk_base = 0;
  for (int32_t i0 = 0; i0 < a.n_tensors; i0 += TRUSS_OPTIM_MAX_TENSORS) {
    OptimDev A;
    memset(&A, 0, sizeof A);
    A.n = a.n_tensors - i0 < TRUSS_OPTIM_MAX_TENSORS ? a.n_tensors - i0 : TRUSS_OPTIM_MAX_TENSORS;
    int64_t chunks = 0;          // (<= 160 x 2^19: an int)
    for (int i = 0; i < A.n; ++i) {
      const truss_optim_tensor_t &t = a.tensors[i0 + i];
      A.t[i].p = t.p, A.t[i].offset = (long)t.offset, A.t[i].numel = (int)t.numel, A.t[i].chunk0 = (int)chunks;
      chunks += (t.numel + TRUSS_OPTIM_CHUNK - 1) / TRUSS_OPTIM_CHUNK;
    }
    A.grad = a.grad, A.m = adam ? a.exp_avg : nullptr, A.v = adam ? a.exp_avg_sq : nullptr, A.step = adam ? a.step : nullptr;
    A.partials = a.partials + chunk_base, A.clipped = a.clipped, A.norms = a.norms ? a.norms + i0 : nullptr;
    A.lr = a.lr, A.b1 = a.beta1, A.b2 = a.beta2, A.eps = a.eps;
    chunk_base += chunks;
    hipLaunchKernelGGL(truss_optim_norm_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, A);
    if (int rc = tb_launched("optim norm launch failed: ")) return rc;
    if (adam) hipLaunchKernelGGL(truss_optim_apply_kernel<TRUSS_OPTIM_ADAM>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(truss_optim_apply_kernel<TRUSS_OPTIM_FIRST_STEP>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, A);
    if (int rc = tb_launched("optim apply launch failed: ")) return rc;
  }
  return TRUSS_OK;
}
#endif  // __HIPCC__
