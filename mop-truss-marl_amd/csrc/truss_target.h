// truss_target.h -- the target networks of the MADDPG update follow their online networks (include/truss_mi355.h,
// truss_target_update): t <- t + tau (p - t) over a list of (target, source) tensor pairs, every `period`-th update, the gate decided
// on the device from the optimiser's step counter.  Pure streaming, one launch per TRUSS_TARGET_MAX_PAIRS pairs: one 256-thread
// workgroup per chunk of TRUSS_TARGET_CHUNK elements of a pair, thread t of a chunk owns the four element quads t, t + 256, t + 512,
// t + 768 (the loads and stores of truss_optim.h): 16-byte accesses where both addresses of the chunk allow and its length is a
// multiple of 4, word by word otherwise, the same elements either way.  No atomics, no LDS, no grid-wide synchronisation: every
// element has one owner.
// On top the argument check (host only: a stand-alone program can drive it); below it, for the device compiler only, the kernel
// and the C entry.  truss_hip.hip includes this file last, behind truss_optim.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

static int tb_fail(int code, const std::string &msg);

// everything is checked before anything is launched
static inline int tb_target_check(const truss_target_args_t *a) {
  if (!a || a->struct_size != sizeof(truss_target_args_t)) return tb_fail(TRUSS_EINVAL, "truss_target_update: struct_size mismatch");
  if (a->n_pairs < 0) return tb_fail(TRUSS_EINVAL, "truss_target_update: n_pairs < 0");
  if (!(a->tau > 0.0 && a->tau <= 1.0)) return tb_fail(TRUSS_EINVAL, "truss_target_update: tau must be in (0, 1]");
  if (a->period < 1) return tb_fail(TRUSS_EINVAL, "truss_target_update: period < 1");
  if (a->n_pairs == 0) return TRUSS_OK;
  if (!a->pairs) return tb_fail(TRUSS_EINVAL, "truss_target_update: NULL pairs");
  struct Range {
    uintptr_t begin, end;
    bool target;
  };
  std::vector<Range> r;
  r.reserve(2 * (size_t)a->n_pairs);
  for (int32_t i = 0; i < a->n_pairs; ++i) {
    const truss_target_pair_t &q = a->pairs[i];
    if (!q.t || !q.p) return tb_fail(TRUSS_EINVAL, "truss_target_update: NULL target or source pointer");
    if (q.numel < 1 || q.numel > INT32_MAX) return tb_fail(TRUSS_EINVAL, "truss_target_update: numel outside 1..2^31-1");
    const uintptr_t bytes = (uintptr_t)q.numel * sizeof(float);
    r.push_back({(uintptr_t)q.t, (uintptr_t)q.t + bytes, true});
    r.push_back({(uintptr_t)q.p, (uintptr_t)q.p + bytes, false});
  }
  // a target range may meet no other range, a source range no target range: in ascending order of their starts, a target must
  // begin at or behind the end of everything before it, a source at or behind the end of every target before it
  std::sort(r.begin(), r.end(), [](const Range &x, const Range &y) { return x.begin < y.begin; });
  uintptr_t end_any = 0, end_target = 0;
  for (const Range &x : r) {
    if (x.begin < (x.target ? end_any : end_target))
      return tb_fail(TRUSS_EINVAL, "truss_target_update: a target range overlaps a source range or another target range");
    end_any = std::max(end_any, x.end);
    if (x.target) end_target = std::max(end_target, x.end);
  }
  return TRUSS_OK;
}

#ifdef __HIPCC__
#define TRUSS_TARGET_LOW 0             // tau < 0.5:       t + w (p - t), w = (float) tau
#define TRUSS_TARGET_HIGH 1            // 0.5 <= tau < 1:  p - (p - t) w, w = (float) (1 - tau)
#define TRUSS_TARGET_COPY 2            // tau == 1:        p
struct TargetPairDev {
  float *t;
  const float *p;
  int numel;
  int chunk0;                    // the pair's first chunk (= workgroup) of this launch
};
struct TargetDev {
  TargetPairDev q[TRUSS_TARGET_MAX_PAIRS];        // 160 x 24 bytes of kernel arguments
  const double *step;            // NULL: always fires
  double period;                 // the ABI's int64 as the double fmod takes: exact up to 2^53, and a step counter beyond that is not one
  float w;
  int n;                         // pairs of this launch
};
static_assert(sizeof(TargetPairDev) == 24 && sizeof(TargetDev) < 4096, "the descriptors travel in the kernel arguments");

// the pair a chunk belongs to: the last one whose first chunk is <= c (uniform over the workgroup, as tb_optim_find)
__device__ __forceinline__ int tb_target_find(const TargetDev &A, int c) {
  int lo = 0, hi = A.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (A.q[mid].chunk0 <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

template <int MODE, bool VEC>
__device__ __forceinline__ void tb_target_apply(float *t, const float *p, int n, int tid, float w) {
  float x[16], y[16];
  // every load of the chunk first, from clamped addresses, masked afterwards (tb_optim_load)
  tb_optim_load<VEC>(p, n, tid, y);
  if constexpr (MODE != TRUSS_TARGET_COPY) {
    tb_optim_load<VEC>(t, n, tid, x);
    TRUSS_UNROLL
    for (int j = 0; j < 16; ++j) y[j] = MODE == TRUSS_TARGET_LOW ? x[j] + w * (y[j] - x[j]) : y[j] - (y[j] - x[j]) * w;
  }
  tb_optim_store<VEC>(t, n, tid, y);
}

template <int MODE>
__global__ __launch_bounds__(256) void truss_target_update_kernel(const TargetDev A) {
  // the gate, on the device: an update that is not due stores nothing
  if (A.step && fmod(*A.step, A.period) != 0.0) return;
  const int c = blockIdx.x, tid = threadIdx.x;
  const TargetPairDev &Q = A.q[tb_target_find(A, c)];
  const int e0 = (c - Q.chunk0) * TRUSS_TARGET_CHUNK;
  const int n = min(TRUSS_TARGET_CHUNK, Q.numel - e0);
  // 16-byte accesses: both addresses of the chunk aligned (a chunk starts a multiple of 16 KB into its tensor) and whole quads only
  if (((((uintptr_t)Q.t | (uintptr_t)Q.p) & 15) | (n & 3)) == 0) tb_target_apply<MODE, true>(Q.t + e0, Q.p + e0, n, tid, A.w);
  else tb_target_apply<MODE, false>(Q.t + e0, Q.p + e0, n, tid, A.w);
}

extern "C" int truss_target_update(const truss_target_args_t *args, void *stream) {
  if (int rc = tb_target_check(args)) return rc;
  const truss_target_args_t &a = *args;
  const int mode = a.tau == 1.0 ? TRUSS_TARGET_COPY : a.tau < 0.5 ? TRUSS_TARGET_LOW : TRUSS_TARGET_HIGH;
  for (int32_t i0 = 0; i0 < a.n_pairs; i0 += TRUSS_TARGET_MAX_PAIRS) {
    TargetDev A;
    memset(&A, 0, sizeof A);
    A.n = a.n_pairs - i0 < TRUSS_TARGET_MAX_PAIRS ? a.n_pairs - i0 : TRUSS_TARGET_MAX_PAIRS;
    int64_t chunks = 0;          // (<= 160 x 2^19: an int)
    for (int i = 0; i < A.n; ++i) {
      const truss_target_pair_t &q = a.pairs[i0 + i];
      A.q[i].t = q.t, A.q[i].p = q.p, A.q[i].numel = (int)q.numel, A.q[i].chunk0 = (int)chunks;
      chunks += (q.numel + TRUSS_TARGET_CHUNK - 1) / TRUSS_TARGET_CHUNK;
    }
    A.step = a.step, A.period = (double)a.period;
    A.w = mode == TRUSS_TARGET_HIGH ? (float)(1.0 - a.tau) : (float)a.tau;
    const dim3 grid((unsigned)chunks), block(256);
    if (mode == TRUSS_TARGET_LOW) hipLaunchKernelGGL(truss_target_update_kernel<TRUSS_TARGET_LOW>, grid, block, 0, (hipStream_t)stream, A);
    else if (mode == TRUSS_TARGET_HIGH) hipLaunchKernelGGL(truss_target_update_kernel<TRUSS_TARGET_HIGH>, grid, block, 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(truss_target_update_kernel<TRUSS_TARGET_COPY>, grid, block, 0, (hipStream_t)stream, A);
    if (int rc = tb_launched("target update launch failed: ")) return rc;
  }
  return TRUSS_OK;
}
#endif  // __HIPCC__
