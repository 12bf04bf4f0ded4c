// truss_pairs.h -- the set-up of a chunk of (env, member) pairs of a game step as one launch (include/truss_mi355.h, truss_pair_setup).
// On top the host-side argument check; below it, for the device compiler only, the gfx950 kernel (truss_pair_kernel) and the C
// entry.  truss_hip.hip includes this file after truss_archive.h.
// Nothing is solved here: every output is a copy of a word the step already holds, one conversion, one float32 division or one
// float32 product.  Two workgroups per pair; within them a thread moves PIECES of four 32-bit words as in
// truss_replay.h -- one 16-byte access where the piece is whole and the address allows it, word by word otherwise (row strides such
// as P P 4 bytes at P = 3 or N 4 bytes at odd N are not multiples of 16).  No LDS, no atomics: every output word has one owner.
#pragma once
#include <cstdint>
#include <string>

static int tb_fail(int code, const std::string &msg);

static inline int tb_pair_check(const truss_pair_args_t *a) {
  if (!a || a->struct_size != sizeof(truss_pair_args_t)) return tb_fail(TRUSS_EINVAL, "truss_pair_setup: bad args / struct_size");
  if (a->n_pairs < 0) return tb_fail(TRUSS_EINVAL, "truss_pair_setup: n_pairs < 0");
  if (a->n_envs < 0) return tb_fail(TRUSS_EINVAL, "truss_pair_setup: n_envs < 0");
  if (a->max_points < 1 || a->max_points > TRUSS_PAIR_MAXP) return tb_fail(TRUSS_EINVAL, "truss_pair_setup: max_points outside 1..256");
  if (a->n_y < 1 || a->n_sec < 1 || a->n_param < 1) return tb_fail(TRUSS_EINVAL, "truss_pair_setup: n_y / n_sec / n_param < 1");
  if (a->rep != 1 && a->rep != 3) return tb_fail(TRUSS_EINVAL, "truss_pair_setup: rep must be 1 or 3");
  if (a->flags != 0) return tb_fail(TRUSS_EINVAL, "truss_pair_setup: flags must be 0");
  const int64_t K = a->n_pairs, B = a->n_envs, P = a->max_points, N = a->n_y, E = a->n_sec, NP = a->n_param;
  int64_t widest = P * P;                                    // words of the widest row, inputs and outputs
  widest = N > widest ? N : widest;
  widest = E > widest ? E : widest;
  widest = 2 * NP > widest ? 2 * NP : widest;
  widest = 8 * P > widest ? 8 * P : widest;
  if (3 * K * widest > INT32_MAX || B * P * widest > INT32_MAX)
    return tb_fail(TRUSS_EINVAL, "truss_pair_setup: 3 x n_pairs (or n_envs x max_points) x the widest row >= 2^31 words");
  if (K == 0) return TRUSS_OK;
  if (B < 1) return tb_fail(TRUSS_EINVAL, "truss_pair_setup: n_envs < 1 with pairs to set up");
  struct Range { const void *p; size_t bytes; const char *name; unsigned align; };
  const size_t k = (size_t)K, b = (size_t)B, p = (size_t)P, n = (size_t)N, e = (size_t)E, np = (size_t)NP, r = (size_t)a->rep;
  const Range in[] = {{a->idx, k * 8, "idx", 8}, {a->ms, k * 8, "ms", 8}, {a->pts, b * p * 32, "pts", 8}, {a->n, b * 4, "n", 4},
                      {a->arch_y, b * p * n * 4, "arch_y", 4}, {a->arch_sec, b * p * e * 4, "arch_sec", 4}, {a->c_x, b * n * 4, "c_x", 4},
                      {a->c_target, b * n * 4, "c_target", 4}, {a->c_params, b * np * 8, "c_params", 8}, {a->ref_points, b * 16, "ref_points", 8},
                      {a->env_ids, b * 8, "env_ids", 8}, {a->frac_tab, (p + 1) * 4, "frac_tab", 4}};
  const Range out[] = {{a->par_x, k * n * 4, "par_x", 4}, {a->par_target, k * n * 4, "par_target", 4}, {a->par_params, k * np * 8, "par_params", 8},
                       {a->par_y, k * n * 4, "par_y", 4}, {a->par_sec, k * e * 4, "par_sec", 4}, {a->cand_x, 3 * k * n * 4, "cand_x", 4},
                       {a->cand_target, 3 * k * n * 4, "cand_target", 4}, {a->cand_params, 3 * k * np * 8, "cand_params", 8},
                       {a->cand_y, 3 * k * n * 4, "cand_y", 4}, {a->cand_sec, 3 * k * e * 4, "cand_sec", 4}, {a->p0, k * p * 32, "p0", 8},
                       {a->nn0, k * 4, "nn0", 4}, {a->parent_obj, k * 16, "parent_obj", 8}, {a->ref, k * 16, "ref", 8},
                       {a->x_p, r * k * p * 16, "x_p", 4}, {a->A_p, r * k * p * p * 4, "A_p", 4}, {a->coin, 3 * k, "coin", 1}};
  const int n_in = (int)(sizeof in / sizeof in[0]), n_out = (int)(sizeof out / sizeof out[0]);
  for (int i = 0; i < n_in; ++i) {
    const bool optional = i == n_in - 1 || (i == n_in - 2 && !a->coin);             // frac_tab; env_ids, which the coins alone read
    if (!in[i].p && !optional) return tb_fail(TRUSS_EINVAL, std::string("truss_pair_setup: ") + in[i].name + " is NULL");
    if ((uintptr_t)in[i].p & (in[i].align - 1)) return tb_fail(TRUSS_EINVAL, std::string("truss_pair_setup: ") + in[i].name + " is not aligned to its type");
  }
  for (int o = 0; o < n_out; ++o) {
    const bool optional = o == n_out - 1;                                             // coin: NULL in the train game
    if (!out[o].p && !optional) return tb_fail(TRUSS_EINVAL, std::string("truss_pair_setup: ") + out[o].name + " is NULL");
    if ((uintptr_t)out[o].p & (out[o].align - 1)) return tb_fail(TRUSS_EINVAL, std::string("truss_pair_setup: ") + out[o].name + " is not aligned to its type");
  }
  // outputs must not overlap the inputs or each other: pairs of one env read the rows another pair's workgroup would be writing
  auto overlap = [](const Range &u, const Range &v) {
    if (!u.p || !v.p || !u.bytes || !v.bytes) return false;
    const uintptr_t u0 = (uintptr_t)u.p, v0 = (uintptr_t)v.p;
    return u0 < v0 + v.bytes && v0 < u0 + u.bytes;
  };
  for (int o = 0; o < n_out; ++o) {
    for (int i = 0; i < n_in; ++i)
      if (overlap(out[o], in[i])) return tb_fail(TRUSS_EINVAL, std::string("truss_pair_setup: output ") + out[o].name + " overlaps input " + in[i].name);
    for (int i = 0; i < o; ++i)
      if (overlap(out[o], out[i])) return tb_fail(TRUSS_EINVAL, std::string("truss_pair_setup: output ") + out[o].name + " overlaps output " + out[i].name);
  }
  return TRUSS_OK;
}

#ifdef __HIPCC__
#define TPR_NT 256

// up to four words of a piece: as one 16-byte access where the piece is whole and the address is 16-byte aligned
__device__ __forceinline__ uint4 tpr_load(const uint32_t *s, int cnt) {
  if (cnt == 4 && ((uintptr_t)s & 15) == 0) return *(const uint4 *)s;
  uint4 v = make_uint4(s[0], 0u, 0u, 0u);
  if (cnt > 1) v.y = s[1];
  if (cnt > 2) v.z = s[2];
  if (cnt > 3) v.w = s[3];
  return v;
}
__device__ __forceinline__ void tpr_store(uint32_t *d, uint4 v, int cnt) {
  if (cnt == 4 && ((uintptr_t)d & 15) == 0) {
    *(uint4 *)d = v;
  } else {
    d[0] = v.x;
    if (cnt > 1) d[1] = v.y;
    if (cnt > 2) d[2] = v.z;
    if (cnt > 3) d[3] = v.w;
  }
}
// One row of `width` words, read once, to `first` and -- `fan` more times, `fan_stride` words apart -- behind `fan_base`: the parent's
// design row and the three candidates' (fan = 3), or a plain copy (fan = 0)
__device__ __forceinline__ void tpr_row(const uint32_t *src, uint32_t *first, uint32_t *fan_base, size_t fan_stride, int fan, int width, int tid) {
  const int npc = (width + 3) >> 2;
  for (int t = tid; t < npc; t += TPR_NT) {
    const int w0 = 4 * t, cnt = width - w0 < 4 ? width - w0 : 4;
    const uint4 v = tpr_load(src + w0, cnt);
    tpr_store(first + w0, v, cnt);
    for (int a = 0; a < fan; ++a) tpr_store(fan_base + a * fan_stride + w0, v, cnt);
  }
}
__device__ __forceinline__ unsigned long long tpr_splitmix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Workgroups (k, 0) and (k, 1) <-> pair (env idx[k], member ms[k]): the first moves the design rows, the second everything else (two
// halves with 17 and 14 pointers: the kernel arguments of both together do not fit the scalar registers).  Both indices are clamped
// into their ranges before anything is read with them (a pair outside them is the caller's error: its rows then hold some env's
// data, and nothing outside the pair's rows is written).
__global__ __launch_bounds__(TPR_NT) void truss_pair_kernel(const truss_pair_args_t A) {
  const int k = blockIdx.x, tid = threadIdx.x;
  const int K = A.n_pairs, P = A.max_points, N = A.n_y, E = A.n_sec, NP2 = 2 * A.n_param, rep = A.rep;
  long long eb = A.idx[k], mm = A.ms[k];
  eb = eb < 0 ? 0 : (eb >= A.n_envs ? A.n_envs - 1 : eb);
  mm = mm < 0 ? 0 : (mm >= P ? P - 1 : mm);
  const size_t b = (size_t)eb, m = (size_t)mm, kk = (size_t)k, KK = (size_t)K;
  if (blockIdx.y == 0) {
    // ---- the design rows: the parent's (row k) and, three times, the candidates' (rows a K + k) ----
    tpr_row((const uint32_t *)A.c_x + b * N, (uint32_t *)A.par_x + kk * N, (uint32_t *)A.cand_x + kk * N, KK * N, 3, N, tid);
    tpr_row((const uint32_t *)A.c_target + b * N, (uint32_t *)A.par_target + kk * N, (uint32_t *)A.cand_target + kk * N, KK * N, 3, N, tid);
    tpr_row((const uint32_t *)A.c_params + b * NP2, (uint32_t *)A.par_params + kk * NP2, (uint32_t *)A.cand_params + kk * NP2, KK * NP2, 3, NP2, tid);
    tpr_row((const uint32_t *)A.arch_y + (b * P + m) * N, (uint32_t *)A.par_y + kk * N, (uint32_t *)A.cand_y + kk * N, KK * N, 3, N, tid);
    tpr_row((const uint32_t *)A.arch_sec + (b * P + m) * E, (uint32_t *)A.par_sec + kk * E, (uint32_t *)A.cand_sec + kk * E, KK * E, 3, E, tid);
    return;
  }
  int n = A.n[b];
  n = n < 0 ? 0 : (n > P ? P : n);
  // ---- the step-start archive of the pair's env, as it lies ----
  const double *pts = A.pts + b * P * 4;
  tpr_row((const uint32_t *)pts, (uint32_t *)(A.p0 + kk * P * 4), nullptr, 0, 0, 8 * P, tid);
  // ---- the per-pair scalars, from the last wave (the first ones have the most pieces to move at small widths) ----
  const int u = TPR_NT - 1 - tid;
  if (u == 0) A.nn0[k] = A.n[b];
  if (u == 1 || u == 2) A.parent_obj[kk * 2 + (u - 1)] = pts[m * 4 + (u - 1)];
  if (u == 3 || u == 4) A.ref[kk * 2 + (u - 3)] = A.ref_points[b * 2 + (u - 3)];
  if (A.coin && u >= 5 && u < 8) {
    const unsigned long long ag = (unsigned long long)(u - 5);
    const unsigned long long key = ((unsigned long long)A.env_ids[b] << 26) | ((unsigned long long)A.game_step << 10) |
                                   ((unsigned long long)mm << 2) | ag;
    A.coin[ag * KK + kk] = (uint8_t)(tpr_splitmix64(key ^ tpr_splitmix64((unsigned long long)A.seed)) >> 63);
  }
  // ---- the Pareto graph: node features [P][4] ... ----
  const float frac = A.frac_tab ? A.frac_tab[n] : (float)n / (float)P;     // the caller's value, or one float32 division
  for (int i = tid; i < P; i += TPR_NT) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                            // rows >= n: exact zeros, whatever the archive holds there
    if (i < n) v = make_float4((float)pts[i * 4], (float)pts[i * 4 + 1], i == (int)mm ? 1.f : 0.f, frac);
    const uint4 w = make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w));
    for (int a = 0; a < rep; ++a) tpr_store((uint32_t *)A.x_p + ((a * KK + kk) * P + i) * 4, w, 4);
  }
  // ---- ... and the adjacency [P][P]: the path over the n members with self loops, d_i d_j on the three central diagonals ----
  const float t1 = A.dtab[1], t2 = A.dtab[2], t3 = A.dtab[3];
  const int PP = P * P, npc = (PP + 3) >> 2;
  for (int t = tid; t < npc; t += TPR_NT) {
    const int e0 = 4 * t, cnt = PP - e0 < 4 ? PP - e0 : 4;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    int i = e0 / P, j = e0 - i * P;                                        // (row, column) of the piece's first element; stepped below
#pragma unroll
    for (int q = 0; q < 4; ++q, i += (j + 1 == P), j = (j + 1 == P ? 0 : j + 1)) {
      if (q < cnt && i < n && j < n && j - i <= 1 && i - j <= 1) {
        const int di = 1 + (i > 0) + (i + 1 < n), dj = 1 + (j > 0) + (j + 1 < n);
        const float fi = di == 1 ? t1 : (di == 2 ? t2 : t3), fj = dj == 1 ? t1 : (dj == 2 ? t2 : t3);
        w[q] = __float_as_uint(fi * fj);                                   // one float32 product
      }
    }
    const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
    for (int a = 0; a < rep; ++a) tpr_store((uint32_t *)A.A_p + (a * KK + kk) * PP + e0, v, cnt);
  }
}

extern "C" int truss_pair_setup(const truss_pair_args_t *a, void *stream) {
  if (int rc = tb_pair_check(a)) return rc;
  if (a->n_pairs == 0) return TRUSS_OK;
  hipLaunchKernelGGL(truss_pair_kernel, dim3((unsigned)a->n_pairs, 2), dim3(TPR_NT), 0, (hipStream_t)stream, *a);
  return tb_launched("pair set-up kernel launch failed: ");
}
#endif  // __HIPCC__
