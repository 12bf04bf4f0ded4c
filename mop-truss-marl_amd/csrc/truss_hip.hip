// truss_hip.hip -- gfx950 (MI355X / CDNA4) backend of include/truss_mi355.h.
//
// One 64-lane wavefront per workgroup; G lanes own one env (64/G envs per wave).  The lane program
// and its phase schedule live in truss_body.h, the host logic in truss_host.h.  Everything an env
// needs between the first load and the last store stays in LDS/registers: the assembled band of K
// (n_pad x W float64), its L*D factor (in place), the load vector and the solution.  HBM sees only
// the algorithmic bytes of the step (DESIGN.md "bytes per env-step").
//
// This file holds the step, rollout and observation kernels and their launch glue only.  Every other kernel family has a
// header of its own, included at the end: truss_gcn.h, truss_gcn_level.h, truss_gcn_level_bwd.h, truss_replay.h, truss_front.h
// (Pareto front + hypervolume), truss_reward.h (the difference reward), truss_archive.h (the archive update),
// truss_pairs.h (the set-up of a chunk of pairs), truss_gcn_aggregate.h and truss_gcn_level_agg.h (a level's neighbour sums
// through the node table), truss_optim.h (clip and Adam of the MADDPG update), truss_critic_tail.h (pools and dense layers of a
// critic pass of the update, forward and backward), truss_target.h (the target networks follow the online ones).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../include/truss_mi355.h"

#pragma clang fp contract(off)  // float32 decode arithmetic must round like numpy: no implicit FMA

#define TRUSS_HD __device__ __forceinline__
#define TRUSS_UNROLL _Pragma("unroll")
#define TB_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
// a value the optimiser cannot trace back to its source: what is computed from it is computed behind this point
__device__ __forceinline__ int tb_opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}
#define TB_OPAQUE(x) tb_opaque(x)
// Kernel arguments that are wanted together: their scalar loads are issued (the arguments are read before the fence, and no
// load sinks below it), then every value is pinned in a scalar register, which is where the one s_waitcnt for all of them lands.
template <class V>
__device__ __forceinline__ void tb_pin_scalar(V v) {
  asm volatile("" : : "s"(v));
}
template <class... Vs>
__device__ __forceinline__ void tb_args_first(Vs... v) {
  TB_SCHED_FENCE();
  (tb_pin_scalar(v), ...);
  TB_SCHED_FENCE();
}
#define TB_ARGS_FIRST(...) tb_args_first(__VA_ARGS__)
// The kernel arguments through a pointer the optimiser cannot see through, in the constant address space (through a generic
// pointer the reads became flat_load's).  What is read through it is read behind this point, and no load or store crosses it:
// the step kernels of the metric configuration fetch everything but the staging's own arguments behind the row loads this way
// (StepLane::stage_issue).
typedef const char __attribute__((address_space(4))) *tb_kernarg_ptr;
__device__ __forceinline__ tb_kernarg_ptr tb_kernargs_here() {
  tb_kernarg_ptr ka = (tb_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ka) : : "memory");
  return ka;
}
// result rows are written once and not read again by this launch: streaming (non-temporal) stores leave
// no dirty lines behind for the end-of-kernel write-back
#define TB_STREAM_STORE(p, v) __builtin_nontemporal_store((v), (p))
// observation tensors of the fused step (~100 MB per 4096-env launch, re-written every step): see DESIGN.md section 4.1b / tools/write_probe.hip
#ifdef TRUSS_OBS_STORE_NT
#define TB_OBS_STORE(p, v) __builtin_nontemporal_store((v), (p))
#else
#define TB_OBS_STORE(p, v) (*(p) = (v))
#endif

// LDS float64 scatter-add (ds_add_f64 on gfx950)
__device__ __forceinline__ void tb_lds_add(double *p, double v) { unsafeAtomicAdd(p, v); }

// Broadcast of a double from lane SRC of every WL-lane team to the lanes of that team, through the DPP
// cross-lane path (no LDS): row_newbcast inside 16-lane rows, one bank-masked move per 8-lane half when
// a row holds two teams; quad_perm for 4-lane teams.
template <int WL, int SRC>
__device__ __forceinline__ double tb_dpp_bcast(double v) {
#ifndef TRUSS_BCAST32   // (-DTRUSS_BCAST32: the two 32-bit halves moved separately, for A/B builds)
  // row_newbcast moves 64 bits at once on gfx950 (v_mov_b64_dpp): one move per team of a row instead of one per half
  if constexpr (WL == 16 || WL == 8) {
    // Every lane is written (all rows; bank masks 0x3 and 0xc together), so the `old` operand never shows: a constant, and
    // the move that sets it up does not wait for v.
    const long long b = __double_as_longlong(v);
    long long r;
    if constexpr (WL == 16) {
      r = __builtin_amdgcn_update_dpp(0ll, b, 0x150 + SRC, 0xf, 0xf, false);
    } else {
      r = __builtin_amdgcn_update_dpp(0ll, b, 0x150 + SRC, 0xf, 0x3, false);
      r = __builtin_amdgcn_update_dpp(r, b, 0x150 + 8 + SRC, 0xf, 0xc, false);
    }
    return __longlong_as_double(r);
  }
#endif
  const int lo = __double2loint(v), hi = __double2hiint(v);
  int rlo, rhi;
  if constexpr (WL == 16) {
    rlo = __builtin_amdgcn_update_dpp(lo, lo, 0x150 + SRC, 0xf, 0xf, false);
    rhi = __builtin_amdgcn_update_dpp(hi, hi, 0x150 + SRC, 0xf, 0xf, false);
  } else if constexpr (WL == 8) {
    rlo = __builtin_amdgcn_update_dpp(lo, lo, 0x150 + SRC, 0xf, 0x3, false);
    rlo = __builtin_amdgcn_update_dpp(rlo, lo, 0x150 + 8 + SRC, 0xf, 0xc, false);
    rhi = __builtin_amdgcn_update_dpp(hi, hi, 0x150 + SRC, 0xf, 0x3, false);
    rhi = __builtin_amdgcn_update_dpp(rhi, hi, 0x150 + 8 + SRC, 0xf, 0xc, false);
  } else {
    static_assert(WL == 4, "team width");
    constexpr int qp = SRC | (SRC << 2) | (SRC << 4) | (SRC << 6);
    rlo = __builtin_amdgcn_update_dpp(lo, lo, qp, 0xf, 0xf, false);
    rhi = __builtin_amdgcn_update_dpp(hi, hi, qp, 0xf, 0xf, false);
  }
  return __hiloint2double(rhi, rlo);
}
// src is a compile-time constant after unrolling; the switch folds to one case
template <class LN>
__device__ __forceinline__ double tb_team_bcast(LN &ln, int src) {
  constexpr int WL = LN::WL_;
  switch (src) {
#define TB_CASE(i) \
  case i:          \
    if constexpr (i < WL) return tb_dpp_bcast<WL, i>(ln.bx); else break;
    TB_CASE(0) TB_CASE(1) TB_CASE(2) TB_CASE(3) TB_CASE(4) TB_CASE(5) TB_CASE(6) TB_CASE(7)
    TB_CASE(8) TB_CASE(9) TB_CASE(10) TB_CASE(11) TB_CASE(12) TB_CASE(13) TB_CASE(14) TB_CASE(15)
#undef TB_CASE
  }
  return ln.bx;
}

// 1/d for the pivot: v_rcp_f64 seed + two Newton steps (full double accuracy for normal d)
__device__ __forceinline__ double tb_rcp(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.0), r, r);
  r = fma(fma(-d, r, 1.0), r, r);
  return r;
}

// 1/d in float32: v_rcp_f32 (1 ulp) + one Newton step
__device__ __forceinline__ float tb_rcpf(float d) {
  float r = __builtin_amdgcn_rcpf(d);
  return fmaf(fmaf(-d, r, 1.0f), r, r);
}

#ifdef TRUSS_STOP_AT
// Diagnostic build only (tools/lds_by_phase.sh): the step kernel returns at phase boundary TRUSS_STOP_AT (a TRUSS_ST index of the
// schedule), so that PMC counters of builds with increasing boundaries give per-phase differences.  Results are wrong by construction.
#define TRUSS_ST(i) do { if ((i) == TRUSS_STOP_AT) return; } while (0)
#endif
#ifdef TRUSS_STAMPS
// Diagnostic build only (make diag): lane 0 of one mid-grid workgroup records s_memtime at the phase
// boundaries into a buffer nothing else reads.  Never enabled in libtruss_mi355.so.
__device__ unsigned long long g_truss_stamps[32];
// g_truss_span: every workgroup's first and last stamp as (shader clock, 100 MHz wall clock): spread of
// the workgroups over the launch, effective shader frequency (tools/span.py).
__device__ unsigned long long g_truss_span[4096][6];   // [4], [5]: the streaming wave's start / end wall clock (EMIT)
#define TRUSS_ST(i)                                                  \
  do {                                                               \
    __builtin_amdgcn_sched_barrier(0);                               \
    if (threadIdx.x == 0 && blockIdx.x == gridDim.x / 2) g_truss_stamps[i] = clock64(); \
    if (threadIdx.x == 0 && ((i) == 0 || (i) == 9) && blockIdx.x < 4096) {              \
      g_truss_span[blockIdx.x][(i) == 0 ? 0 : 2] = clock64();                            \
      g_truss_span[blockIdx.x][(i) == 0 ? 1 : 3] = wall_clock64();                       \
    }                                                                \
    __builtin_amdgcn_sched_barrier(0);                               \
  } while (0)
#endif

// 1/sqrt(x): v_rsq_f64 seed (measured 5.2e-8 relative on gfx950, tools/rcp_accuracy.hip) + two Newton
// steps (one step leaves 4e-15)
__device__ __forceinline__ double tb_rsqrt(double x) {
  double r = __builtin_amdgcn_rsq(x);
  r = r * fma(-0.5 * x, r * r, 1.5);
  r = r * fma(-0.5 * x, r * r, 1.5);
  return r;
}

// min / max over the G lanes of an env (all lanes get the result), DPP only: xor 1, xor 2 inside a quad,
// row_half_mirror (other quad of the 8), row_mirror (other half of the 16-lane row); beyond a row: ds_bpermute
template <int G, bool MAX>
__device__ __forceinline__ float tb_group_reduce(float v) {
  auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); };
  auto dpp = [](float x, auto ctrl) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xf, 0xf, false));
  };
  if constexpr (G >= 2) v = op(v, dpp(v, std::integral_constant<int, 0xB1>{}));   // quad_perm [1,0,3,2]
  if constexpr (G >= 4) v = op(v, dpp(v, std::integral_constant<int, 0x4E>{}));   // quad_perm [2,3,0,1]
  if constexpr (G >= 8) v = op(v, dpp(v, std::integral_constant<int, 0x141>{}));  // row_half_mirror
  if constexpr (G >= 16) v = op(v, dpp(v, std::integral_constant<int, 0x140>{})); // row_mirror
  if constexpr (G >= 32) v = op(v, __shfl_xor(v, 16));
  if constexpr (G >= 64) v = op(v, __shfl_xor(v, 32));
  return v;
}
template <class LN>
__device__ __forceinline__ float tb_group_min(LN &ln, int c) { return tb_group_reduce<LN::G_, false>(ln.pmn[c]); }
template <class LN>
__device__ __forceinline__ float tb_group_max(LN &ln, int c) { return tb_group_reduce<LN::G_, true>(ln.pmx[c]); }

// sum of a double over the G lanes of an env (all lanes get the result): the same butterfly as tb_group_reduce
template <int G>
__device__ __forceinline__ double tb_group_reduce_sum(double v) {
  auto dpp = [](double x, auto ctrl) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), decltype(ctrl)::value, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), decltype(ctrl)::value, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
  };
  if constexpr (G >= 2) v = v + dpp(v, std::integral_constant<int, 0xB1>{});
  if constexpr (G >= 4) v = v + dpp(v, std::integral_constant<int, 0x4E>{});
  if constexpr (G >= 8) v = v + dpp(v, std::integral_constant<int, 0x141>{});
  if constexpr (G >= 16) v = v + dpp(v, std::integral_constant<int, 0x140>{});
  if constexpr (G >= 32) v = v + __shfl_xor(v, 16);
  if constexpr (G >= 64) v = v + __shfl_xor(v, 32);
  return v;
}
// objective partials of the step lane: 0 volume, 1 target distance, 2 strain energy / 0 stress ratio, 1 deflection ratio, 2 bad pivot
template <class LN>
__device__ __forceinline__ double tb_group_sum_d(LN &ln, int which) {
  return tb_group_reduce_sum<LN::G_>(which == 0 ? ln.p_vol : which == 1 ? ln.p_dt : ln.p_en);
}
template <class LN>
__device__ __forceinline__ float tb_group_max_f(LN &ln, int which) {
  return tb_group_reduce<LN::G_, true>(which == 0 ? ln.p_c1 : which == 1 ? ln.p_c2 : (float)ln.bad);
}

// EMIT workgroups: the word behind the progress word is set by a streaming wave that gave up waiting (tb_obs_timeout)
template <class LN, class TD>
__device__ __forceinline__ bool tb_obs_timed_out(LN &ln, const TD &T) {
  if constexpr (LN::EMIT_) return *((const __attribute__((address_space(3))) int *)(ln.TB + T.o_flag) + 1) != 0;
  return false;
}

#include "truss_body.h"

// Progress word of an EMIT workgroup (LDS): the compute wave raises it, the streaming wave sleeps on it.  Everything the two waves
// hand over lives in LDS, so the hand-off is a workgroup-scope release store / acquire load of an LDS word: on gfx950 (waves of a
// workgroup share the CU, LDS operations of a wave retire in issue order) that is `s_waitcnt lgkmcnt(0); ds_write_b32` on one side
// and `ds_read_b32; s_waitcnt lgkmcnt(0)` on the other.  The pointer MUST carry the LDS address space: through a generic
// `volatile int *` (rounds 1-2) the compiler emitted flat_store / flat_load ... sc0 sc1 + s_waitcnt vmcnt(0), i.e. every publish and
// every poll went through the vector-memory path and waited for ALL outstanding global stores of the wave.
typedef __attribute__((address_space(3))) int tb_lds_word;
__device__ __forceinline__ tb_lds_word *tb_flag_ptr(char *lds, int o_flag) { return (tb_lds_word *)(lds + o_flag); }
__device__ __forceinline__ void tb_publish(char *lds, int o_flag, int k) {
  __builtin_amdgcn_wave_barrier();
#ifdef TRUSS_FLAG_RELAXED   // A/B only (tools/experiments/README.md): rounds 1-2's reliance on the in-order LDS pipeline, without the release's lgkmcnt(0)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  if (threadIdx.x == 0) __hip_atomic_store(tb_flag_ptr(lds, o_flag), k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
  if (threadIdx.x == 0) __hip_atomic_store(tb_flag_ptr(lds, o_flag), k, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
}
// Bounded wait of the streaming wave for progress >= k.  false = gave up (the compute wave never got there -- it faulted or the
// launch is being torn down); the caller then flags the env in status[] (TRUSS_STATUS_OBS_TIMEOUT) instead of streaming garbage.
// The bound (~2^22 polls of >= 64 clocks: >= 0.1 s) keeps the grid draining in every case; a compute wave publishes within tens of
// microseconds.  `tb_await_limit` is lowered by the emulator-side test of the timeout path only.
#ifndef TB_AWAIT_SPINS
#define TB_AWAIT_SPINS (1 << 22)
#endif
__device__ __forceinline__ bool tb_await(char *lds, int o_flag, int k) {
  for (int spin = 0; spin < TB_AWAIT_SPINS; ++spin) {
    const int v = __hip_atomic_load(tb_flag_ptr(lds, o_flag), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (__builtin_amdgcn_readfirstlane(v) >= k) return true;
    __builtin_amdgcn_s_sleep(1);
  }
  return false;
}

// the streaming wave gave up (tb_await): leave the timeout word for the compute wave's status store and raise the bit directly too
template <class LN>
__device__ __forceinline__ void tb_obs_timeout(LN &ln, char *lds, int o_flag, int32_t *status) {
  if ((threadIdx.x & 63) == 0) *(tb_flag_ptr(lds, o_flag) + 1) = 1;
  if (ln.g == 0 && ln.active && status) atomicOr(&status[ln.env], TRUSS_STATUS_OBS_TIMEOUT);
}

// Phase boundaries of the step and rollout kernels (TRUSS_STEP_SCHEDULE / TRUSS_STREAM_SEG* of truss_body.h).  A wave has the
// LDS bytes it works on to itself: its LDS instructions execute in issue order, so a later ds_read sees an earlier ds_write of
// any lane without waiting for it.  A wavefront-scope fence plus wave_barrier keeps the compiler from reordering across a phase
// boundary and emits no s_waitcnt / s_barrier (a __syncthreads() here costs a full LDS round trip per pivot of the
// factorisation).  EMIT_POINT differs per kernel and is defined there; truss_obs_kernel redefines PH / PH_NS for itself.
#define TB_WAVE_SYNC()                                    \
  do {                                                    \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                      \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  } while (0)
#define PH(call) \
  ln.call;       \
  TB_WAVE_SYNC()
#define PH_NS(call) ln.call
#define BAR() TB_WAVE_SYNC()

template <int G, int WL, int RPL, int EPL, bool EMIT>
__global__ __launch_bounds__(EMIT ? 128 : 64) void truss_step_kernel(const TopoDev T_, const StepArgsDev A_) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  StepLane<G, WL, RPL, EPL, EMIT> ln;
  if (!EMIT || __builtin_amdgcn_readfirstlane(threadIdx.x) < 64) ln.stage_issue(threadIdx.x & 63, blockIdx.x, T_, A_);   // (EMIT: the compute wave)
  TB_SCHED_FENCE();   // the rows are on their way: every other kernel argument is fetched behind them, under the HBM trip.
  // (Read from T_ / A_ directly, the optimiser hoists argument loads of the whole kernel to the entry, in front of the row loads,
  // with a wait of their own.)  The second argument follows the first at its natural alignment.
  // The launch signature is (TopoDev, StepArgsDev) by value: hip_run passes exactly these two.
  struct Kernargs { TopoDev T; StepArgsDev A; };
  constexpr size_t a_off = (sizeof(TopoDev) + 7) & ~(size_t)7;
  static_assert(alignof(StepArgsDev) == 8 && alignof(TopoDev) == 8 && offsetof(Kernargs, A) == a_off, "kernel-argument layout");
  constexpr bool PRE = StepLane<G, WL, RPL, EPL, EMIT>::PRE;   // variants without the early issue read T_ / A_ as they always did
  tb_kernarg_ptr ka = nullptr;
  if constexpr (PRE) ka = tb_kernargs_here();
  const TopoDev &T = [&]() -> const TopoDev & { if constexpr (PRE) return *(const TopoDev *)ka; else return T_; }();
  const StepArgsDev &A = [&]() -> const StepArgsDev & { if constexpr (PRE) return *(const StepArgsDev *)(ka + a_off); else return A_; }();
  ln.stage_args_second(T, A);
  ln.init(threadIdx.x & 63, blockIdx.x, T, A, smem);
  constexpr int W_ = StepLane<G, WL, RPL, EPL, EMIT>::W;
  constexpr bool EMIT_ = EMIT;
  if constexpr (EMIT) {
    // two wavefronts: 0 computes the step, 1 streams the observation tensors (truss_body.h, "WHO streams")
    if (threadIdx.x == 0) {
      *tb_flag_ptr(smem, T.o_flag) = 0;
      *(tb_flag_ptr(smem, T.o_flag) + 1) = 0;   // timeout word
    }
    __syncthreads();   // the only workgroup barrier of the kernel: the progress word starts at 0
    if (threadIdx.x >= 64) {
#ifdef TRUSS_STAMPS
#define SST(i)                                                                                        \
  do {                                                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    if (threadIdx.x == 64 && blockIdx.x == gridDim.x / 2) g_truss_stamps[i] = clock64();              \
    if (threadIdx.x == 64 && ((i) == 20 || (i) == 26) && blockIdx.x < 4096)                           \
      g_truss_span[blockIdx.x][(i) == 20 ? 4 : 5] = wall_clock64();                                   \
    __builtin_amdgcn_sched_barrier(0);                                                                \
  } while (0)
#else
#define SST(i)
#endif
      ln.emit_tables_load(T);   // ahead of every store of this wave in the vmcnt order ...
      __builtin_amdgcn_s_waitcnt(0);   // ... and waited for HERE, while this wave has nothing else to do: gfx9 counts loads and stores
                                       // in one vmcnt, so a first use of a table register behind stores would wait for all of them
                                       // (the compiler put s_waitcnt vmcnt(0) in front of the row tensors' gathers: segment 3 could
                                       // not start before segment 2's 32 KB per workgroup had retired)
      bool ok = tb_await(smem, T.o_flag, 1);
      if (ok) {
        SST(20);
        TRUSS_STREAM_SEG1(PH, T, A)
        SST(21);
        ok = tb_await(smem, T.o_flag, 2);
      }
      if (ok) {
        SST(22);
        TRUSS_STREAM_SEG2(PH, T, A)
        SST(23);
        ok = tb_await(smem, T.o_flag, 3);
      }
      if (ok) {
        SST(24);
        TRUSS_STREAM_SEG3(PH, T, A)
        SST(25);
      } else {
        tb_obs_timeout(ln, smem, T.o_flag, A.status);   // one exit for the three waits
      }
#ifdef TRUSS_STAMPS
      __builtin_amdgcn_s_waitcnt(0);   // all stores of this wave retired (vmcnt(0))
      SST(26);
#endif
#undef SST
      return;
    }
  }
#ifdef TRUSS_FAULT_DROP_PUBLISH3   // fault-injection build (make faultinj; tests only): progress 3 is never announced
#define EMIT_POINT(k) do { if ((k) != 3) tb_publish(smem, T.o_flag, k); } while (0)
#else
#define EMIT_POINT(k) tb_publish(smem, T.o_flag, k)
#endif
  TRUSS_STEP_SCHEDULE(PH, PH_NS, BAR, T, A)
#undef EMIT_POINT
}

// truss_rollout as ONE launch: every workgroup plays its envs through all n_steps chained steps.  Topology tables,
// per-env constants and the design state (the previous step's result) stay in LDS between steps; the next step's
// actions are fetched while the current step assembles and solves (rollout_prefetch / rollout_stash), so after the
// first step no step waits for HBM.  Per step the same result rows are written as by truss_step (design state into
// the alternating buffers, everything else overwritten), envs are independent: nothing crosses workgroups.
struct RolloutDev {
  TopoDev T;
  StepArgsDev A;                  // the first step's arguments (buffers 0 -> 1, action set 0)
  int32_t n_steps, n_sets;
  size_t gstride, tstride;        // floats between consecutive action sets
};
template <int G, int WL, int RPL, int EPL>
__global__ __launch_bounds__(64) void truss_rollout_kernel(const RolloutDev P_) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int W_ = StepLane<G, WL, RPL, EPL, false>::W;
  constexpr bool EMIT_ = false;
#define EMIT_POINT(k) (void)0
  const int n_steps = P_.n_steps;
  for (int s = 0; s < n_steps; ++s) {
    // The arguments are read through a pointer the optimiser cannot see through, once per step: hoisting the ~150
    // loop-invariant kernel-argument loads (and the addresses derived from them) out of the step loop cost 492 SGPR +
    // 199 VGPR spills and 760 bytes of scratch per lane; a step re-reads what it needs from the scalar cache instead.
    // (the pointer keeps the constant address space: through a generic pointer the reads became 500 flat_load's)
    typedef const char __attribute__((address_space(4))) *tb_kernarg_ptr;
    tb_kernarg_ptr ka = (tb_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const RolloutDev &P = *(const RolloutDev *)ka;
    const TopoDev &T = P.T;
    const StepArgsDev &A = P.A;
    StepLane<G, WL, RPL, EPL, false> ln;   // per step: no lane state is carried from one step to the next except through LDS
    // The lane index goes the same way: the lane-derived indices and LDS addresses of a step (clamped element / node / pair
    // numbers, row offsets, ...) are a VALU instruction or two each, but hoisted out of the step loop they held ~80 VGPRs for
    // the whole launch, and the allocator parked what the solver needs in AGPRs instead (v_accvgpr_read on the pivot chain).
    int lane_id = threadIdx.x;
    asm volatile("" : "+v"(lane_id));
    ln.init(lane_id, blockIdx.x, T, A, smem);
    const int nset = (s + 1) % P.n_sets;
    ln.rs_first_step = s;
    ln.rs_y_out = (s & 1) ? (float *)A.y_in : A.y_out;          // step s reads buffer s & 1, writes the other one
    ln.rs_sec_out = (s & 1) ? (int32_t *)A.sec_in : A.sec_out;
    ln.rs_next_geo = s + 1 < n_steps ? A.a_geo + (size_t)nset * P.gstride : nullptr;
    ln.rs_next_topo = s + 1 < n_steps ? A.a_topo + (size_t)nset * P.tstride : nullptr;
    TRUSS_STEP_SCHEDULE(PH, PH_NS, BAR, T, A)
    TB_WAVE_SYNC();
  }
#undef EMIT_POINT
}

#undef PH   // the observation kernel's phases end in workgroup barriers
#undef PH_NS
#undef BAR
#undef TB_WAVE_SYNC

__global__ __launch_bounds__(64) void truss_obs_kernel(const TopoDev T, const ObsArgsDev A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  ObsLane ln;
  ln.init(threadIdx.x, blockIdx.x, blockIdx.y, T, A, smem);
#define PH(call) \
  ln.call;       \
  __syncthreads()
#define PH_NS(call) ln.call
  const int r0_tile = ln.role == 1 ? ((int)blockIdx.y - 1) * A.tile_rows : 0;   // uniform over the workgroup: the barriers stay convergent
  TRUSS_OBS_SCHEDULE(PH, PH_NS, T, A, r0_tile)
#undef PH
#undef PH_NS
}

// ---- host backend ---------------------------------------------------------------------------
#define TRUSS_BACKEND_NAME "hip"
struct truss_topo;
static void *tb_dev_alloc(size_t n) {
  void *p = nullptr;
  return hipMalloc(&p, n) == hipSuccess ? p : nullptr;
}
static void tb_dev_free(void *p) { (void)hipFree(p); }
static bool tb_dev_upload(void *dst, const void *src, size_t n) {
  return hipMemcpy(dst, src, n, hipMemcpyHostToDevice) == hipSuccess;
}
static int tb_launch_step(const truss_topo *t, const StepArgsDev &A, bool emit, void *stream);
static int tb_launch_obs(const truss_topo *t, const ObsArgsDev &A, void *stream);
static int tb_launch_rollout(const truss_topo *t, const StepArgsDev &A, int n_steps, int n_sets, void *stream);

#include "truss_host.h"

// Dynamic LDS beyond 64 KiB needs an opt-in per kernel AND per device; one flag per (kernel, device), set once
// (the C ABI promises thread safety per stream: relaxed atomics, a repeated hipFuncSetAttribute is harmless).
static constexpr int TB_MAX_DEVICES = 64;
struct TbLdsOptIn {
  std::atomic<bool> done[TB_MAX_DEVICES];
  int ensure(const void *kern) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= TB_MAX_DEVICES) return tb_fail(TRUSS_EHIP, "hipGetDevice failed");
    if (done[dev].load(std::memory_order_acquire)) return TRUSS_OK;
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return tb_fail(TRUSS_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    done[dev].store(true, std::memory_order_release);
    return TRUSS_OK;
  }
};
// behind every kernel launch: TRUSS_OK, or TRUSS_EHIP with `what` (the site's own "... launch failed: ") + HIP's error text
static int tb_launched(const char *what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? TRUSS_OK : tb_fail(TRUSS_EHIP, std::string(what) + hipGetErrorString(e));
}

static int tb_launch_obs(const truss_topo *t, const ObsArgsDev &A, void *stream) {
  static TbLdsOptIn optin;
  if (int rc = optin.ensure((const void *)truss_obs_kernel)) return rc;
  hipLaunchKernelGGL(truss_obs_kernel, dim3((unsigned)A.B, (unsigned)(A.n_split > 1 ? A.n_split + 1 : 1)), dim3(64), tb_obs_lds_bytes(t->N), (hipStream_t)stream, t->dev, A);
  return tb_launched("obs kernel launch failed: ");
}

template <int G, int WL, int RPL, int EPL, bool EMIT>
static int hip_run(const truss_topo *t, const StepArgsDev &A, hipStream_t st) {
  static TbLdsOptIn optin;
  auto kern = truss_step_kernel<G, WL, RPL, EPL, EMIT>;
  if (int rc = optin.ensure((const void *)kern)) return rc;
  constexpr int EPB = 64 / G;
  const unsigned grid = (unsigned)((A.B + EPB - 1) / EPB);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(EMIT ? 128 : 64), EMIT ? t->lds_bytes_emit : t->lds_bytes, st, EMIT ? t->dev_emit : t->dev, A);
  return tb_launched("kernel launch failed: ");
}

template <int G, int WL, int RPL, int EPL>
static int hip_run_rollout(const truss_topo *t, const StepArgsDev &A, int n_steps, int n_sets, hipStream_t st) {
  static TbLdsOptIn optin;
  auto kern = truss_rollout_kernel<G, WL, RPL, EPL>;
  if (int rc = optin.ensure((const void *)kern)) return rc;
  RolloutDev Q;
  Q.T = t->dev;
  Q.A = A;
  Q.n_steps = n_steps;
  Q.n_sets = n_sets;
  Q.gstride = (size_t)A.B * t->N * 2;
  Q.tstride = (size_t)A.B * t->N * 3;
  constexpr int EPB = 64 / G;
  const unsigned grid = (unsigned)((A.B + EPB - 1) / EPB);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64), t->lds_bytes, st, Q);
  return tb_launched("rollout kernel launch failed: ");
}
static int tb_launch_rollout(const truss_topo *t, const StepArgsDev &A, int n_steps, int n_sets, void *stream) {
  const TbVariant &v = kVariants[t->variant];
#define X(g, wl, r, e) \
  if (v.G == g && v.WL == wl && v.RPL == r && v.EPL == e) return hip_run_rollout<g, wl, r, e>(t, A, n_steps, n_sets, (hipStream_t)stream);
  TRUSS_ROLLOUT_VARIANTS(X)
#undef X
  return tb_fail(TRUSS_EUNSUPPORTED, "variant not compiled with the persistent rollout");
}

static int tb_launch_step(const truss_topo *t, const StepArgsDev &A, bool emit, void *stream) {
  const TbVariant &v = kVariants[t->variant];
  hipStream_t st = (hipStream_t)stream;
  if (emit) {
#define X(g, wl, r, e) \
  if (v.G == g && v.WL == wl && v.RPL == r && v.EPL == e) return hip_run<g, wl, r, e, true>(t, A, st);
    TRUSS_EMIT_VARIANTS(X)
#undef X
    return tb_fail(TRUSS_EUNSUPPORTED, "variant not compiled with the observation writer");
  }
#define X(g, wl, r, e) \
  if (v.G == g && v.WL == wl && v.RPL == r && v.EPL == e) return hip_run<g, wl, r, e, false>(t, A, st);
  TRUSS_VARIANTS(X)
#undef X
  return tb_fail(TRUSS_EUNSUPPORTED, "variant not compiled");
}

#ifdef TRUSS_STAMPS
extern "C" int truss_debug_span(unsigned long long *out, int nblocks) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_truss_span), (size_t)nblocks * 6 * sizeof(unsigned long long)) == hipSuccess ? 0 : -3;
}
extern "C" int truss_debug_stamps32(unsigned long long *out32) {
  return hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_truss_stamps), 32 * sizeof(unsigned long long)) == hipSuccess ? 0 : -3;
}
extern "C" int truss_debug_stamps(unsigned long long *out16) {
  return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_truss_stamps), 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : -3;
}
#endif

#include "truss_gcn.h"
#include "truss_gcn_group.h"
#include "truss_gcn_level.h"
#include "truss_gcn_level_bwd.h"
#include "truss_replay.h"

#include "truss_front.h"
#include "truss_reward.h"
#include "truss_archive.h"
#include "truss_pairs.h"
#include "truss_gcn_aggregate.h"
#include "truss_gcn_level_agg.h"
#include "truss_optim.h"
#include "truss_critic_tail.h"
#include "truss_target.h"
