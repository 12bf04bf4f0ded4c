// truss_host.h -- host side of the C ABI (include/truss_mi355.h).  truss_topo_create is a sequence of phases, one function each:
// tb_check_args, tb_dof_numbering, tb_vertical_pairs, tb_node_ordering, tb_pick_variant, TbGeometry (teams, band offsets),
// tb_build_tables (the blob), tb_lds_layout, tb_build_emit; truss_topo owns its device memory.  Header-only; the includer provides
//     TRUSS_BACKEND_NAME                           "hip" | "emu"
//     void *tb_dev_alloc(size_t);  void tb_dev_free(void *);
//     bool tb_dev_upload(void *dst, const void *src, size_t bytes);
//     int  tb_launch_step(const truss_topo *, const StepArgsDev &, bool emit, void *stream);
//          (emit: the instantiation that also writes the observation tensors; only asked for when dev.emit_ok)
//     int  tb_launch_obs(const truss_topo *, const ObsArgsDev &, void *stream);
//     int  tb_launch_rollout(const truss_topo *, const StepArgsDev &, int n_steps, int n_sets, void *stream);
//          (all chained steps in one launch; only asked for when tb_rollout_one_launch() says the topology allows it)
// truss_hip.hip implements them with the HIP runtime; tests/emu/truss_emu.cpp with malloc and the CPU lane emulator.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <queue>
#include <string>
#include <vector>

#include "../../include/truss_mi355.h"

static thread_local std::string g_truss_err;
static int tb_fail(int code, const std::string &msg) {
  g_truss_err = msg;
  return code;
}

// compiled (G, RPL, EPL) instantiations of the step kernel; keep in sync with the dispatch tables
struct TbVariant {
  int G, WL, RPL, EPL;  // lanes per env, window lanes, rows per lane, elements per lane
};
#ifdef TRUSS_ONLY_DEFAULT_VARIANT   // diagnostic builds (tools/ablate.sh, `make diag`): compile one kernel only
#ifndef TRUSS_DIAG_VARIANT           // -D'TRUSS_DIAG_VARIANT(X)=X(64,8,1,10)' -DTRUSS_DIAG_NO_EMIT for another one
#define TRUSS_DIAG_VARIANT(X) X(16, 8, 1, 5)
#endif
#define TRUSS_VARIANTS(X) TRUSS_DIAG_VARIANT(X)
#else
#define TRUSS_VARIANTS(X) \
  X(8, 8, 1, 5) X(8, 8, 1, 10) X(16, 8, 1, 3) X(16, 8, 1, 5) X(32, 8, 1, 3) X(16, 16, 1, 5) X(16, 8, 2, 5) X(4, 4, 2, 20) \
  X(32, 8, 1, 10) X(64, 8, 1, 10) /* large trusses: up to 320 / 640 elements, 128 / 256 nodes (BASELINE config 5) */
#endif
// variants that are also compiled with the fused observation emission (StepLane<..., EMIT = true>)
#if defined(TRUSS_ONLY_DEFAULT_VARIANT) && defined(TRUSS_DIAG_NO_EMIT)
#define TRUSS_EMIT_VARIANTS(X)
#elif defined(TRUSS_ONLY_DEFAULT_VARIANT)
#define TRUSS_EMIT_VARIANTS(X) TRUSS_DIAG_VARIANT(X)
#else
#define TRUSS_EMIT_VARIANTS(X) X(8, 8, 1, 5) X(16, 8, 1, 3) X(16, 8, 1, 5)
#endif
// variants with a persistent rollout kernel (truss_rollout as one launch)
#ifdef TRUSS_ONLY_DEFAULT_VARIANT
#define TRUSS_ROLLOUT_VARIANTS(X) TRUSS_DIAG_VARIANT(X)
#else
#define TRUSS_ROLLOUT_VARIANTS(X) X(8, 8, 1, 5) X(8, 8, 1, 10) X(16, 8, 1, 3) X(16, 8, 1, 5) X(32, 8, 1, 3) X(32, 8, 1, 10) X(64, 8, 1, 10)
#endif
static bool tb_variant_rolls(int G, int WL, int RPL, int EPL) {
#define X(g, wl, r, e) \
  if (G == g && WL == wl && RPL == r && EPL == e) return true;
  TRUSS_ROLLOUT_VARIANTS(X)
#undef X
  return false;
}
static bool tb_variant_emits(int G, int WL, int RPL, int EPL) {
#define X(g, wl, r, e) \
  if (G == g && WL == wl && RPL == r && EPL == e) return true;
  TRUSS_EMIT_VARIANTS(X)
#undef X
  return false;
}
static const TbVariant kVariants[] = {
#define X(g, wl, r, e) {g, wl, r, e},
    TRUSS_VARIANTS(X)
#undef X
};
static const int kNumVariants = (int)(sizeof(kVariants) / sizeof(kVariants[0]));

// observation kernel LDS: raw[N][13] | mn[13] | mx[13] | part[128] | (pad to 16) | three [TR][N] matrix tiles.
// TR = rows per tile: all N rows when the three N x N matrices fit (one pass, 32-node trusses: 12 KB); large
// trusses are written in row tiles (256 nodes: 3 x 256 KB would not fit any CU).
static int tb_env_int(const char *name, int dflt) {
  const char *v = getenv(name);
  return v && *v ? atoi(v) : dflt;
}

// Trusses of 64 nodes and more: a batch has few envs and each writes 70-870 KB -- one workgroup per (env, tile of rows) with small
// tiles (64 nodes: 8 rows = 6 KB, 128 nodes: 8 rows, 256 nodes: 4 rows = 12 KB) plus one workgroup per env for the per-node / per-element
// rows, dispatched first (it is the longest), instead of one workgroup per env walking over 96 KB tiles: 256 envs of 256 nodes were 256
// waves on 1024 SIMDs, 2.1 TB/s; now 5.8 TB/s (128 nodes: 2.1 -> 5.1, 64 nodes: 3.3 -> 4.0; tools/obs_probe.py).
// TRUSS_OBS_SPLIT_MIN_N / TRUSS_OBS_TILE_KB: diagnostic overrides for sweeps.
static inline bool tb_obs_splits(int N) { return N >= tb_env_int("TRUSS_OBS_SPLIT_MIN_N", 64); }
static inline int tb_obs_tile_rows(int N) {
  if (tb_obs_splits(N)) {
    const int tr = (int)(((size_t)tb_env_int("TRUSS_OBS_TILE_KB", N >= 128 ? 12 : 6) * 1024) / ((size_t)3 * N * 4)) & ~1;
    return tr < 2 ? 2 : tr;
  }
  const size_t budget = 96 * 1024;
  size_t tr = budget / ((size_t)3 * N * 4);
  if (tr >= (size_t)N) {
    // everything would fit in one pass -- but two passes of half the rows halve the LDS of a workgroup, and
    // the launch then fits the CUs in one round (4096 envs x 13.8 KB did not: 26.8 -> 24.9 us at 32 nodes)
    tr = N >= 16 ? (size_t)(((N + 1) / 2 + 3) & ~3) : (size_t)N;
  }
  if (tr > (size_t)N) tr = (size_t)N;
  return tr < 1 ? 1 : (int)tr;
}
static inline size_t tb_obs_lds_bytes(int N) {
  return ((((size_t)(N * 13 + 26 + 128) * 4 + 15) & ~(size_t)15) + (size_t)3 * tb_obs_tile_rows(N) * N * 4 + 15) & ~(size_t)15;
}

// appends a table to a blob, 16-byte aligned; returns its byte offset (a TopoDev f_* / et_* field)
template <typename T>
static int32_t tb_push(std::vector<char> &blob, const std::vector<T> &v) {
  size_t off = (blob.size() + 15) & ~size_t(15);
  blob.resize(off + std::max<size_t>(v.size(), 1) * sizeof(T));
  if (!v.empty()) memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
  return (int32_t)off;
}

struct TbFrag {   // a byte range [lo, hi) inside one env's LDS region
  size_t lo, hi;
};
// what truss_topo_lds_info reports of one layout: byte ranges inside an env
struct TbLayoutInfo {
  TbFrag band{}, ev{};
  std::vector<TbFrag> live_with_ev;   // what holds a value somebody still reads while the element values are in their buffer
};

struct truss_topo {
  int N = 0, E = 0, NP = 0, ndof = 0, n_pad = 0, n_rest = 0, bw = 0;
  int G = 0, WL = 0, RPL = 0, EPL = 0, W = 0, variant = -1;
  std::vector<int32_t> nsc, ttnsc, perm;
  TopoDev dev{};        // what a plain step launch gets
  TopoDev dev_emit{};   // ... an EMIT launch: the staged tables include the nN_x_e gather table (larger blob_bytes / o_env0)
  size_t lds_bytes_emit = 0;
  // neighbour table (TrussTopology.neighbor_table()): int16 [N][k_nbr], ascending, the diagonal included, -1 = unused slot
  std::vector<int16_t> nbr;
  int k_nbr = 0;
  // TRUSS_F_OBS_COMPACT on a topology with the fused writer: a twin whose dev_emit is the COMPACT image (matrix table, chunk count
  // and env stride of the [N][k_nbr] rows; everything else equal to dev_emit).  tb_launch_step gets the twin in place of this
  // topology, so a backend launches the same kernel with another image and knows nothing of layouts.  The twin owns no memory.
  std::unique_ptr<truss_topo> compact;
  int32_t et_mat_c = 0, nc_mat_c = 0;   // the compact image's matrix table in etab and its chunks per env (tb_build_emit)
  void *blob = nullptr;   // device memory, owned: the topology tables (TopoDev::blob) ...
  void *etab = nullptr;   // ... and the emission tables of the fused observation writer (TopoDev::etab)
  size_t lds_bytes = 0;
  int n_sections = 0;
  // for truss_topo_lds_info, [0] plain / rollout launches, [1] EMIT launches: the band offsets the tables hold, the layout's ranges
  std::vector<int32_t> band_offsets[2];
  TbLayoutInfo layout[2];
  truss_topo() = default;
  truss_topo(const truss_topo &) = delete;
  truss_topo &operator=(const truss_topo &) = delete;
  ~truss_topo() {
    if (blob) tb_dev_free(blob);
    if (etab) tb_dev_free(etab);
  }
};

// ---- fused observation emission: feature bank placement + gather tables (TopoDev "emit" fields) -------------
// Dead byte ranges of one env's LDS region, by the time from which the streaming wave may overwrite them:
//   early = once the member results are staged (behind phase_post_elements): band behind the staging rows and the
//           objective partials; action rows
//   late  = behind phase_post_nodes: solver scratch (z vectors, solution vector, trash slots -- not the reactions
//           and the objective partials, so that the placement does not depend on where phase_finish runs)
// Builds the register tables (t->etab, uploaded here) and appends the LDS-resident nN_x_e table to `blob`.
// Returns false when the topology is outside what the fused writer covers; truss_step then runs the observation
// kernel as a second launch.
static bool tb_build_emit(truss_topo *t, TopoDev &D, const int32_t *conn, const uint8_t *res, const uint8_t *top,
                          std::vector<TbFrag> early, std::vector<TbFrag> late, std::vector<char> &blob) {
  const int N = t->N, E = t->E, G = t->G;
  D.emit_ok = 0;
  if (!tb_variant_emits(t->G, t->WL, t->RPL, t->EPL) || tb_env_int("TRUSS_NO_FUSED_OBS", 0)) return false;
  const int NPL = (2 * t->EPL + 4) / 5, NF = G * NPL, EF = G * t->EPL;
  if ((N & 3) || N > NF || E > EF || !D.has_pairs) return false;
  // the kernel's compile-time iteration counts (StepLane::IX ...)
  const int IX = (13 * NF / 4 + G - 1) / G, IN_ = (12 * NF / 4 + G - 1) / G, IE = (21 * EF / 4 + G - 1) / G,
            IM = (NF * NF / 4 + G - 1) / G;
  // first-fit placement of the bank arrays (sizes in floats; all multiples of 4 but the constants, placed last)
  struct Arr {
    int32_t *dst;
    int n;
  };
  auto place = [](std::vector<Arr> arrs, std::vector<TbFrag> &frags) {
    for (auto &f : frags) f.lo = (f.lo + 15) & ~size_t(15);
    for (const Arr &a : arrs) {
      bool placed = false;
      for (auto &f : frags)
        if (f.lo + (size_t)a.n * 4 <= f.hi) {
          *a.dst = (int32_t)(f.lo / 4);
          f.lo += ((size_t)a.n * 4 + 15) & ~size_t(15);
          placed = true;
          break;
        }
      if (!placed) return false;
    }
    return true;
  };
  if (!place({{&D.b_tc, 2 * (E + 1)}, {&D.b_erec, 4 * E}, {&D.b_erec2, 2 * E}, {&D.b_const, 3}}, early)) return false;   // written with / right behind the member results
  for (const TbFrag &f : early) late.push_back(f);                                   // what the element records left over
  if (!place({{&D.b_nna, 4 * N}, {&D.b_nnb, 4 * N}, {&D.b_nraw, 4 * N}, {&D.b_nn8, N}}, late)) return false;
  if (D.env_stride / 4 > 65535 || E + 1 > 65535) return false;
  const int ZERO = D.b_const, ONE = D.b_const + 1, C1 = D.b_const + 2;
  const int fX = D.o_x / 4, fY = D.o_y / 4, fMU = (D.o_kb + D.so_mu) / 4, fMD = (D.o_kb + D.so_md) / 4,
            fQ0 = (D.o_kb + D.so_q0) / 4;
  // 0/1 columns of x_n (res_x, res_y, top, 1 - top): min-max normalisation of a constant column gives 0
  auto flag = [&](int n, int c) -> int { return c == 2 ? res[2 * n] != 0 : c == 3 ? res[2 * n + 1] != 0 : c == 5 ? top[n] != 0 : top[n] == 0; };
  bool any0[13] = {}, any1[13] = {};
  for (int n = 0; n < N; ++n)
    for (int c : {2, 3, 5, 6}) (flag(n, c) ? any1[c] : any0[c]) = true;
  const int dyn_of[13] = {0, 1, -1, -1, 2, -1, -1, 3, 4, 5, 6, 7, 8};
  std::vector<uint16_t> txn, tnxn, tnxe, tmat;
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < 13; ++c)
      txn.push_back((uint16_t)(dyn_of[c] < 0   ? (flag(n, c) && any0[c] ? C1 : ZERO)
                               : dyn_of[c] < 4 ? D.b_nna + 4 * n + dyn_of[c]
                               : dyn_of[c] < 8 ? D.b_nnb + 4 * n + dyn_of[c] - 4
                                               : D.b_nn8 + n));
  for (int n = 0; n < N; ++n) {
    const int nr = D.b_nraw + 4 * n;   // loaded, target / y, |dy|, violated
    const int src[12] = {fX + n, fY + n, res[2 * n] ? ONE : ZERO, res[2 * n + 1] ? ONE : ZERO, nr + 0, top[n] ? ONE : ZERO,
                         top[n] ? ZERO : ONE, fMU + n, fMD + n, nr + 1, nr + 2, nr + 3};
    for (int c = 0; c < 12; ++c) tnxn.push_back((uint16_t)src[c]);
  }
  for (int e = 0; e < E; ++e) {
    const int er = D.b_erec + 4 * e, er2 = D.b_erec2 + 2 * e;   // (sec, area, length, tension), (compression, violated)
    const int own[7] = {er + 0, er + 1, er + 2, er + 3, er2 + 0, fQ0 + e, er2 + 1};
    for (int c = 0; c < 7; ++c) tnxe.push_back((uint16_t)own[c]);
    for (int q = 0; q < 2; ++q) {
      const int n = conn[2 * e + q];
      const int nr = D.b_nraw + 4 * n;
      const int nd[7] = {fX + n, fY + n, res[2 * n] ? ONE : ZERO, res[2 * n + 1] ? ONE : ZERO, nr + 0, nr + 2, nr + 3};
      for (int c = 0; c < 7; ++c) tnxe.push_back((uint16_t)nd[c]);
    }
  }
  tmat.assign((size_t)N * N, (uint16_t)E);   // row-major = chunk order
  for (int e = 0; e < E; ++e) {
    tmat[(size_t)conn[2 * e] * N + conn[2 * e + 1]] = (uint16_t)e;
    tmat[(size_t)conn[2 * e + 1] * N + conn[2 * e]] = (uint16_t)e;
  }
  D.nc_xn = (int32_t)txn.size() / 4;
  D.nc_nxn = (int32_t)tnxn.size() / 4;
  D.nxe_cw = (E & 3) == 0 ? 4 : (E & 1) == 0 ? 2 : 1;    // 21 E floats per env: 16-, 8- or 4-byte aligned rows
  D.nc_nxe = (int32_t)tnxe.size() / D.nxe_cw;
  D.nc_mat = (int32_t)tmat.size() / 4;
  D.mat_stride4 = D.nc_mat;
  // the same table over the N Kc cells of the compact rows (TRUSS_F_OBS_COMPACT): slot t of row i is the element joining
  // (i, nbr[i][t]); the diagonal and the unused slots have none.  N % 4 == 0, so N Kc / 4 is whole.
  const int Kc = t->k_nbr;
  std::vector<uint16_t> tmatc((size_t)N * Kc, (uint16_t)E);
  for (int i = 0; i < N; ++i)
    for (int s = 0; s < Kc; ++s) {
      const int j = t->nbr[(size_t)i * Kc + s];
      if (j >= 0 && j != i) tmatc[(size_t)i * Kc + s] = tmat[(size_t)i * N + j];
    }
  t->nc_mat_c = (int32_t)tmatc.size() / 4;
  // pad to `iters` iterations of G chunks (entries past the end repeat the last chunk); chunk q = iteration q / G, lane q % G
  auto padded = [&](const std::vector<uint16_t> &v, int iters) {
    const size_t nc = v.size() / 4;
    std::vector<uint16_t> out((size_t)iters * G * 4);
    for (size_t q = 0; q < (size_t)iters * G; ++q)
      for (int j = 0; j < 4; ++j) out[4 * q + j] = v[4 * std::min(q, nc - 1) + j];
    return out;
  };
  // register tables: [pair][G][2]: the entries of iterations (2p, 2p+1) of a lane are adjacent
  auto paired = [&](const std::vector<uint16_t> &v, int iters) {
    const int ip = (iters + 1) / 2;
    std::vector<uint16_t> lin = padded(v, 2 * ip), out(lin.size());
    for (int p2 = 0; p2 < ip; ++p2)
      for (int g = 0; g < G; ++g)
        for (int h = 0; h < 2; ++h)
          for (int j = 0; j < 4; ++j) out[(((size_t)p2 * G + g) * 2 + h) * 4 + j] = lin[((size_t)(2 * p2 + h) * G + g) * 4 + j];
    return out;
  };
  std::vector<char> tab;
  D.et_xn = tb_push(tab, paired(txn, IX));
  D.et_nxn = tb_push(tab, paired(tnxn, IN_));
  D.et_mat = tb_push(tab, paired(tmat, IM));
  t->et_mat_c = tb_push(tab, paired(tmatc, IM));   // Kc <= N: never more chunks than the dense matrix
  tab.resize((tab.size() + 15) & ~size_t(15));
  t->etab = tb_dev_alloc(tab.size());   // t's from here on, whatever becomes of the upload
  if (!t->etab || !tb_dev_upload(t->etab, tab.data(), tab.size())) return false;
  D.etab = (const char *)t->etab;
  D.f_tnxe = tb_push(blob, D.nxe_cw == 4 ? padded(tnxe, IE) : tnxe);   // LDS-resident, staged by EMIT launches only
  blob.resize((blob.size() + 15) & ~size_t(15));
  D.emit_ok = 1;
  return true;
}

// --- DOF numbering, FEM_2Dtruss.py:227-261 (nsc: free DOFs first), and every element's four DOFs, :311-317 (ttnsc) ---
static void tb_dof_numbering(truss_topo &t, const int32_t *conn, const uint8_t *res) {
  const int N = t.N;
  t.nsc.assign(2 * N, 0);
  int c = 1;
  for (int i = 0; i < 2 * N; ++i)
    if (res[i] == 0) t.nsc[i] = c++;
  t.ndof = c - 1;
  for (int i = 0; i < 2 * N; ++i)
    if (res[i] != 0) t.nsc[i] = c++;
  t.n_rest = 2 * N - t.ndof;
  t.ttnsc.resize(4 * t.E);
  for (int e = 0; e < t.E; ++e)
    for (int q = 0; q < 4; ++q) t.ttnsc[4 * e + q] = t.nsc[2 * conn[2 * e + (q >> 1)] + (q & 1)];
}

// half bandwidth (in DOFs) of K when nodes are visited in `order`
static int tb_bandwidth(const std::vector<int> &order, const uint8_t *res, const int32_t *conn, int N, int E,
                        std::vector<int> *dofpos_out) {
  std::vector<int> pos(2 * N, -1);
  int c = 0;
  for (int i = 0; i < N; ++i) {
    int n = order[i];
    for (int k = 0; k < 2; ++k)
      if (res[2 * n + k] == 0) pos[2 * n + k] = c++;
  }
  int bw = 0;
  for (int n = 0; n < N; ++n)
    if (pos[2 * n] >= 0 && pos[2 * n + 1] >= 0) bw = std::max(bw, std::abs(pos[2 * n] - pos[2 * n + 1]));
  for (int e = 0; e < E; ++e) {
    int a = conn[2 * e], b = conn[2 * e + 1];
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j) {
        int pa = pos[2 * a + i], pb = pos[2 * b + j];
        if (pa >= 0 && pb >= 0) bw = std::max(bw, std::abs(pa - pb));
      }
  }
  if (dofpos_out) *dofpos_out = pos;
  return bw;
}

// reverse Cuthill-McKee from `start` on the node graph
static std::vector<int> tb_rcm(int start, const std::vector<std::vector<int>> &adj, int N) {
  std::vector<int> order;
  std::vector<char> seen(N, 0);
  auto bfs = [&](int s) {
    std::queue<int> q;
    q.push(s);
    seen[s] = 1;
    while (!q.empty()) {
      int u = q.front();
      q.pop();
      order.push_back(u);
      std::vector<int> nb;
      for (int v : adj[u])
        if (!seen[v]) {
          seen[v] = 1;
          nb.push_back(v);
        }
      std::sort(nb.begin(), nb.end(), [&](int a, int b) {
        return adj[a].size() != adj[b].size() ? adj[a].size() < adj[b].size() : a < b;
      });
      for (int v : nb) q.push(v);
    }
  };
  bfs(start);
  for (int i = 0; i < N; ++i)
    if (!seen[i]) bfs(i);
  std::reverse(order.begin(), order.end());
  return order;
}

extern "C" int truss_abi_version(void) { return TRUSS_ABI_VERSION; }
extern "C" const char *truss_last_error(void) { return g_truss_err.c_str(); }
extern "C" const char *truss_backend(void) { return TRUSS_BACKEND_NAME; }

// ================= truss_topo_create: the phases, in the order they run =================
// what the caller passed (the arguments of truss_topo_create behind `out`, in their order)
struct TbInput {
  int N, E;
  const int32_t *conn;
  const uint8_t *res, *top;
  const int32_t *pair;
  const uint8_t *load_mask;
  int n_sym_nodes;
  const int32_t *sym_nodes;
  int n_sym_elems;
  const int32_t *sym_elems;
  int n_sections;
  const double *sections;
  double e_mod, long_stress;
  const int32_t *node_order;
};

// ---- argument checks ----
static int tb_check_args(truss_topo_t **out, const TbInput &in) {
  const int N = in.N, E = in.E;
  const int32_t *conn = in.conn;
  if (!out || !conn || !in.res || !in.top || !in.sections) return tb_fail(TRUSS_EINVAL, "NULL argument");
  if (N < 2 || E < 1 || N > 16000) return tb_fail(TRUSS_EINVAL, "bad N/E");
  if (in.n_sections < 1) return tb_fail(TRUSS_EINVAL, "need at least one section");
  if ((in.n_sym_nodes > 0 && !in.sym_nodes) || (in.n_sym_elems > 0 && !in.sym_elems)) return tb_fail(TRUSS_EINVAL, "sym table NULL");
  for (int e = 0; e < E; ++e)
    if (conn[2 * e] < 0 || conn[2 * e] >= N || conn[2 * e + 1] < 0 || conn[2 * e + 1] >= N || conn[2 * e] == conn[2 * e + 1])
      return tb_fail(TRUSS_EINVAL, "conn out of range");
  for (int i = 0; i < in.n_sym_nodes * 2; ++i)
    if (in.sym_nodes[i] < 0 || in.sym_nodes[i] >= N) return tb_fail(TRUSS_EINVAL, "sym_nodes out of range");
  for (int i = 0; i < in.n_sym_elems * 2; ++i)
    if (in.sym_elems[i] < 0 || in.sym_elems[i] >= E) return tb_fail(TRUSS_EINVAL, "sym_elems out of range");
  for (int e = 0; e < E; ++e)
    for (int f = e + 1; f < E; ++f)
      if ((conn[2 * e] == conn[2 * f] && conn[2 * e + 1] == conn[2 * f + 1]) ||
          (conn[2 * e] == conn[2 * f + 1] && conn[2 * e + 1] == conn[2 * f]))
        return tb_fail(TRUSS_EUNSUPPORTED, "two elements join the same pair of nodes (parallel members are not supported)");
  return TRUSS_OK;
}

// ---- vertical pairs: the (lo, hi) list; false when pair[] is not an involution without fixed points ----
static bool tb_vertical_pairs(const int32_t *pair, int N, std::vector<int16_t> &pairs) {
  for (int i = 0; pair && i < N; ++i) {
    const int j = pair[i];
    if (j < 0 || j >= N || j == i || pair[j] != i) return false;
    if (i < j) {
      pairs.push_back((int16_t)i);
      pairs.push_back((int16_t)j);
    }
  }
  return true;
}

// ---- neighbour table: per node the columns in which a node-graph adjacency can be non-zero -- the node itself and the far ends
// of its members -- ascending, padded with -1 to the widest row (the rule of TrussTopology.neighbor_table()) ----
static void tb_neighbor_table(const TbInput &in, std::vector<int16_t> &nbr, int &k_nbr) {
  std::vector<std::vector<int>> cols(in.N);
  for (int n = 0; n < in.N; ++n) cols[n].push_back(n);
  for (int e = 0; e < in.E; ++e) {
    cols[in.conn[2 * e]].push_back(in.conn[2 * e + 1]);
    cols[in.conn[2 * e + 1]].push_back(in.conn[2 * e]);
  }
  k_nbr = 0;
  for (auto &c : cols) {
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
    k_nbr = std::max(k_nbr, (int)c.size());
  }
  nbr.assign((size_t)in.N * k_nbr, (int16_t)-1);
  for (int n = 0; n < in.N; ++n)
    for (size_t s = 0; s < cols[n].size(); ++s) nbr[(size_t)n * k_nbr + s] = (int16_t)cols[n][s];
}

// ---- node ordering for the banded solver: hint, natural, RCM from every start; the first candidate with the smallest
// half-bandwidth `bw` gives dofpos (solver position of node*2+comp, -1 = restrained).  false: the hint is no permutation ----
static bool tb_node_ordering(const TbInput &in, int &bw, std::vector<int> &dofpos) {
  const int N = in.N, E = in.E;
  std::vector<std::vector<int>> adj(N);
  for (int e = 0; e < E; ++e) {
    adj[in.conn[2 * e]].push_back(in.conn[2 * e + 1]);
    adj[in.conn[2 * e + 1]].push_back(in.conn[2 * e]);
  }
  std::vector<std::vector<int>> cands;
  if (in.node_order) {
    std::vector<int> o(in.node_order, in.node_order + N);
    std::vector<char> seen(N, 0);
    for (int v : o) {
      if (v < 0 || v >= N || seen[v]) return false;
      seen[v] = 1;
    }
    cands.push_back(o);
  }
  cands.emplace_back(N);
  for (int i = 0; i < N; ++i) cands.back()[i] = i;
  for (int s = 0; s < N && N <= 1024; ++s) cands.push_back(tb_rcm(s, adj, N));
  int best = -1, best_bw = 1 << 30;
  for (size_t i = 0; i < cands.size(); ++i) {
    int b = tb_bandwidth(cands[i], in.res, in.conn, N, E, nullptr);
    if (b < best_bw) {
      best_bw = b;
      best = (int)i;
    }
  }
  bw = tb_bandwidth(cands[best], in.res, in.conn, N, E, &dofpos);
  return true;
}

// ---- kernel variant (index into kVariants, -1 = none compiled): the narrowest window that holds the band; 16 lanes per
// env (4 envs per wave) so that a 4096-env batch puts a wave on every SIMD.  TRUSS_LANES / TRUSS_WLANES / TRUSS_RPL / TRUSS_EPL override ----
static int tb_pick_variant(int bw, int E) {
  int want_G = tb_env_int("TRUSS_LANES", 0), want_WL = tb_env_int("TRUSS_WLANES", 0), want_RPL = tb_env_int("TRUSS_RPL", 0),
      want_EPL = tb_env_int("TRUSS_EPL", 0);
  int pick = -1;
  auto score = [](const TbVariant &v) {
    int W = v.WL * v.RPL;
    int pref = (v.G == 16 && v.WL == 8) ? 0 : (v.G == 8 && v.WL == 8) ? 1 : (v.G == 16) ? 2 : 3;
    return W * 10000 + v.RPL * 1000 + pref * 100 + v.EPL;
  };
  for (int i = 0; i < kNumVariants; ++i) {
    const TbVariant &v = kVariants[i];
    int W = v.WL * v.RPL;
    if (W <= bw) continue;
    if ((E + v.G - 1) / v.G > v.EPL) continue;
    if (want_G && v.G != want_G) continue;
    if (want_WL && v.WL != want_WL) continue;
    if (want_RPL && v.RPL != want_RPL) continue;
    if (want_EPL && v.EPL != want_EPL) continue;
    if (pick < 0 || score(v) < score(kVariants[pick])) pick = i;
  }
  return pick;
}

// ---- solver geometry (see TopoDev): one team, or two that eliminate from both ends (TRUSS_ONE_SIDED: diagnostic) ----
// The band of one layout: rows KS doubles apart (tb_band_stride: W, or W + 2 where rows are padded), team A's rows first, team B's
// from kb_b (tb_band_team_b, the function the kernel takes it from; tools/lds_conflict_model.cpp sets other values to compare them).
struct TbGeometry {
  int nteams, W, KS, n, KA, mid, rowsA, rowsB, zlen, dlen, zslot, kb_b;
  bool padded() const { return KS != W; }
  TbGeometry(const truss_topo &t, int ks) : W(t.W), KS(ks), n(t.ndof) {
    nteams = (t.G / t.WL >= 2 && t.RPL == 1 && !tb_env_int("TRUSS_ONE_SIDED", 0)) ? 2 : 1;
    if (nteams == 2) {
      KA = n > W ? (n - W + 1) / 2 : 0;
      mid = n - 2 * KA;
      rowsA = KA + 2 * W;
      rowsB = KA + W;
      zlen = dlen = KA + 2 * W;
      zslot = n + 2 * W;
    } else {
      KA = t.n_pad;
      mid = 0;
      rowsA = t.n_pad + W;
      rowsB = 0;
      zlen = dlen = t.n_pad + W;
      zslot = t.n_pad;
    }
    kb_b = tb_band_team_b(rowsA, KS, W);   // one team (rowsB = 0): where the trash slot lies
  }
  // offset (in doubles) of the lower-band entry (r, c), r >= c, original solver positions.  A band row
  // stores its W entries by COLUMN RESIDUE in the owning team's frame: entry (row, col) at row*KS + col%W
  // (distinct for the W consecutive columns of a row), which is the order of the solver's window registers.
  int band_off(int r, int c) const {
    if (nteams == 1 || r < n - KA) return r * KS + (c % W);             // team A: its part + middle rows
    int rb = n - 1 - r, cb = n - 1 - c;                                    // team B frame: cb >= rb
    return kb_b + cb * KS + (rb % W);
  }
  // a spare double right behind the band: sink for entries on restrained DOFs
  int trash_off() const { return kb_b + rowsB * KS; }
};

// ---- topology tables ----
// solver position -> reference DOF (t.perm, 0-based) and node*2+comp; node*2+comp -> solver position / reaction slot
static void tb_position_tables(truss_topo &t, const std::vector<int> &dofpos, std::vector<int16_t> &posnode,
                               std::vector<int16_t> &dofpos16, std::vector<int16_t> &restslot) {
  t.perm.assign(t.ndof, -1);
  posnode.assign(t.n_pad, -1);
  dofpos16.assign(2 * t.N, -1);
  restslot.assign(2 * t.N, -1);
  for (int i = 0; i < 2 * t.N; ++i) {
    if (dofpos[i] >= 0) {
      t.perm[dofpos[i]] = t.nsc[i] - 1;
      posnode[dofpos[i]] = (int16_t)i;
      dofpos16[i] = (int16_t)dofpos[i];
    } else {
      restslot[i] = (int16_t)(t.nsc[i] - t.ndof - 1);
    }
  }
}

// band offsets of every element's four off-diagonal entries (FEM_2Dtruss.py:320-324 restricted to the lower band); the
// node-diagonal blocks go through tb_diag_offsets.  false: an entry lies outside the window or its offset beyond int16
static bool tb_asm_codes(const TbGeometry &g, const TbInput &in, const std::vector<int> &dofpos, std::vector<int16_t> &asm_code) {
  asm_code.assign(4 * (size_t)in.E, -1);
  bool band_ok = true;
  for (int e = 0; e < in.E; ++e) {
    const int *pa = &dofpos[2 * in.conn[2 * e]], *pb = &dofpos[2 * in.conn[2 * e + 1]];
    const int rc[4][2] = {{pa[0], pb[0]}, {pa[1], pb[1]}, {pa[0], pb[1]}, {pa[1], pb[0]}};
    for (int q = 0; q < 4; ++q) {
      int r = rc[q][0], c = rc[q][1], code = g.trash_off();
      if (r >= 0 && c >= 0) {
        if (r < c) std::swap(r, c);
        if (r - c >= g.W) band_ok = false;
        code = g.band_off(r, c);
        if (code > 32767) band_ok = false;
      }
      asm_code[4 * (size_t)e + q] = (int16_t)code;
    }
  }
  for (int nd = 0; nd < in.N; ++nd)   // a node's own x/y pair must fit the band too
    if (dofpos[2 * nd] >= 0 && dofpos[2 * nd + 1] >= 0 && std::abs(dofpos[2 * nd] - dofpos[2 * nd + 1]) >= g.W) band_ok = false;
  return band_ok;
}

// band offsets of the node-diagonal 2x2 block entries (x,x), (y,y), (x,y)
static std::vector<int16_t> tb_diag_offsets(const TbGeometry &g, int N, const std::vector<int> &dofpos) {
  std::vector<int16_t> diagoff(3 * (size_t)N, (int16_t)g.trash_off());
  for (int nd = 0; nd < N; ++nd) {
    int px = dofpos[2 * nd], py = dofpos[2 * nd + 1];
    if (px >= 0) diagoff[3 * nd + 0] = (int16_t)g.band_off(px, px);
    if (py >= 0) diagoff[3 * nd + 1] = (int16_t)g.band_off(py, py);
    if (px >= 0 && py >= 0) diagoff[3 * nd + 2] = (int16_t)g.band_off(std::max(px, py), std::min(px, py));
  }
  return diagoff;
}

static std::vector<uint8_t> tb_node_flags(const TbInput &in) {
  const int N = in.N;
  std::vector<uint8_t> nflags(N, 0);
  for (int n = 0; n < N; ++n) {
    uint8_t f = 0;
    if (in.top[n]) f |= TF_TOP;
    if (in.res[2 * n]) f |= TF_RESX;
    if (in.res[2 * n + 1]) f |= TF_RESY;
    // loaded as a bridge / as a roof: the caller's mask, else truss2D_GEN.py:421-430
    if (in.load_mask ? in.load_mask[n] != 0 : !in.top[n] && in.res[2 * n + 1] == 0) f |= TF_LOAD_BRIDGE;
    if (in.load_mask ? in.load_mask[N + n] != 0 : in.top[n] != 0) f |= TF_LOAD_ROOF;
    nflags[n] = f;
  }
  return nflags;
}

// elements incident to each node (ascending element index), padded to 8 with E = "zero slot"; false: a node joins more
static bool tb_adjacency8(const TbInput &in, std::vector<int16_t> &adj8) {
  adj8.assign((size_t)in.N * 8, (int16_t)in.E);
  for (int n = 0; n < in.N; ++n) {
    int c = 0;
    for (int e = 0; e < in.E; ++e)
      if (in.conn[2 * e] == n || in.conn[2 * e + 1] == n) {
        if (c >= 8) return false;
        adj8[(size_t)n * 8 + c++] = (int16_t)e;
      }
  }
  return true;
}

// load code of every z/P slot in team frames (see TopoDev::f_zcode)
static std::vector<uint8_t> tb_load_codes(const TbGeometry &g, const std::vector<int16_t> &posnode, const std::vector<uint8_t> &nflags) {
  std::vector<uint8_t> zcode((size_t)g.zlen * g.nteams, 0);
  for (int tm = 0; tm < g.nteams; ++tm)
    for (int pz = 0; pz < g.zlen; ++pz) {
      int orig = -1;
      if (g.nteams == 1) orig = pz < g.n ? pz : -1;
      else if (tm == 0) orig = pz < g.n - g.KA ? pz : -1;
      else orig = pz < g.KA ? g.n - 1 - pz : -1;
      if (orig < 0) continue;
      int nd = posnode[orig];
      if (nd < 0) continue;
      uint8_t fl = nflags[nd >> 1];
      zcode[(size_t)tm * g.zlen + pz] = (uint8_t)((nd & 1) | ((fl & TF_LOAD_BRIDGE) ? 2 : 0) | ((fl & TF_LOAD_ROOF) ? 4 : 0));
    }
  return zcode;
}

// slots of every element's four end displacements in the solution vector (restrained -> the zero slot)
static std::vector<int16_t> tb_solution_slots(const TbGeometry &g, const TbInput &in, const std::vector<int> &dofpos) {
  std::vector<int16_t> exs(4 * (size_t)in.E);
  for (int e = 0; e < in.E; ++e)
    for (int q = 0; q < 4; ++q) {
      const int dp = dofpos[2 * in.conn[2 * e + (q >> 1)] + (q & 1)];
      exs[4 * (size_t)e + q] = (int16_t)(dp < 0 ? g.zslot : dp);
    }
  return exs;
}

static std::vector<int16_t> tb_int16(const int32_t *p, size_t n) { return std::vector<int16_t>(p, p + n); }

// every table of the step kernel for the band of `g`, packed into `blob`; the ORDER of the pushes is the blob layout.  Fills the
// counts, the solver geometry and the f_* offsets of D (the plain launches' or the EMIT launches' TopoDev).  Refuses (band guard, then node degree) before anything is pushed.
static int tb_build_tables(truss_topo &t, TopoDev &D, const TbGeometry &g, const TbInput &in, const std::vector<int> &dofpos,
                           const std::vector<int16_t> &pairs, std::vector<char> &blob, std::vector<int32_t> &band_offsets) {
  const int S = in.n_sections;
  std::vector<int16_t> posnode, dofpos16, restslot, asm_code, adj8;
  tb_position_tables(t, dofpos, posnode, dofpos16, restslot);
  if (!tb_asm_codes(g, in, dofpos, asm_code))
    return tb_fail(TRUSS_EUNSUPPORTED, "internal: band wider than window / offsets beyond int16");
  if (!tb_adjacency8(in, adj8)) return tb_fail(TRUSS_EUNSUPPORTED, "a node joins more than 8 elements");
  const std::vector<uint8_t> nflags = tb_node_flags(in);
  std::vector<double> area(S), isr(S);
  std::vector<float> areaf(S), vsf(S);
  for (int i = 0; i < S; ++i) {
    area[i] = in.sections[2 * i];
    isr[i] = 1.0 / (area[i] * in.long_stress);
    areaf[i] = (float)area[i];
    vsf[i] = (float)(area[i] / in.sections[2 * (S - 1)]);   // truss2D_ENV.py:86-87 (area / truss[-1] area)
  }
  const std::vector<int16_t> diagoff = tb_diag_offsets(g, t.N, dofpos);
  band_offsets.clear();     // what the two tables say about the band (truss_topo_lds_info): every entry that is not the trash slot
  for (int16_t c : asm_code)
    if (c != g.trash_off()) band_offsets.push_back(c);
  for (int16_t c : diagoff)
    if (c != g.trash_off()) band_offsets.push_back(c);
  D.N = t.N;
  D.E = t.E;
  D.NP = t.NP;
  D.ndof = t.ndof;
  D.n_pad = t.n_pad;
  D.n_rest = t.n_rest;
  D.n_sym_nodes = in.n_sym_nodes;
  D.n_sym_elems = in.n_sym_elems;
  D.n_sections = S;
  D.has_pairs = t.NP > 0 && 2 * t.NP == t.N;
  D.nteams = g.nteams;
  D.KA = g.KA;
  D.mid = g.mid;
  D.rowsA = g.rowsA;
  D.rowsB = g.rowsB;
  D.zlen = g.zlen;
  D.dlen = g.dlen;
  D.zslot = g.zslot;
  D.e_mod = in.e_mod;
  D.long_stress = in.long_stress;
  D.f_conn = tb_push(blob, tb_int16(in.conn, 2 * (size_t)t.E));
  D.f_pairs = tb_push(blob, pairs);
  D.f_nflags = tb_push(blob, nflags);
  D.f_dofpos = tb_push(blob, dofpos16);
  D.f_restslot = tb_push(blob, restslot);
  D.f_asm = tb_push(blob, asm_code);
  D.f_posnode = tb_push(blob, posnode);
  D.f_symn = tb_push(blob, tb_int16(in.sym_nodes, 2 * (size_t)in.n_sym_nodes));
  D.f_syme = tb_push(blob, tb_int16(in.sym_elems, 2 * (size_t)in.n_sym_elems));
  D.f_area = tb_push(blob, area);
  D.f_isr = tb_push(blob, isr);
  D.f_areaf = tb_push(blob, areaf);
  D.f_vsf = tb_push(blob, vsf);
  D.f_adj8 = tb_push(blob, adj8);
  D.f_diagoff = tb_push(blob, diagoff);
  D.f_zcode = tb_push(blob, tb_load_codes(g, posnode, nflags));
  D.f_exs = tb_push(blob, tb_solution_slots(g, in, dofpos));
  blob.resize((blob.size() + 15) & ~size_t(15));
  D.blob_bytes = (int32_t)blob.size();
  return TRUSS_OK;
}

// ---- LDS layout: [copy of the tables][env 0][env 1]...; every array 16-byte aligned.  Fills o_*, so_*, env_stride and o_env0
// of D for the band of `g` and returns the bytes per workgroup; early / late: the dead bytes of an env for the bank of the fused observation writer (tb_build_emit) ----
struct TbCarve {   // byte offsets of arrays laid out one behind the other
  size_t off = 0;
  int32_t operator()(size_t bytes) {
    size_t o = off;
    off = (off + bytes + 15) & ~size_t(15);
    return (int32_t)o;
  }
  void at_least(size_t o0, size_t need) {   // the region that began at o0 holds `need` bytes or more
    if (off - o0 < need) off = (o0 + need + 15) & ~size_t(15);
  }
};
// Two orders.  Dense bands (every EMIT layout among them, whose early / late fragments are placed from it):
//   [band][solver scratch | EV][par][y][x][tg][geo tac | merge scratch][sec]
// the element values (EV, 3 (E + 1) doubles, live from phase_elements to phase_assemble_nodes) lie over the solver scratch, which is
// smaller, so the region is as long as EV.  Padded bands have no bytes to spare for that:
//   [band][solver scratch][geo tac | merge scratch][par][y][x][tg][sec]
// the action rows are dead from the end of phase_sizing until rollout_stash / merge_post, both behind the assembly, so EV runs on
// from the solver scratch into them and nothing is carved for EV alone.
static size_t tb_lds_layout(const truss_topo &t, TopoDev &D, const TbGeometry &g, size_t table_bytes, std::vector<TbFrag> &early,
                            std::vector<TbFrag> &late, TbLayoutInfo &info) {
  const int N = t.N, E = t.E, W = g.W;
  const size_t ev_bytes = sizeof(double) * 3 * ((size_t)E + 1);
  TbCarve carve;
  // band region; after the back substitution it is reused as the output staging area
  {
    const size_t band = sizeof(double) * ((size_t)g.trash_off() + 2);  // + trash slot
    TbCarve sub;
    D.so_q0 = sub(sizeof(float) * E);
    D.so_sr = sub(sizeof(float) * E);
    D.so_disp = sub(sizeof(float) * 2 * N);
    D.so_mu = sub(sizeof(float) * N);
    D.so_md = sub(sizeof(float) * N);
    D.so_comp = sub((size_t)E);
    const size_t red_off = sub.off;   // objective partials live behind the staging rows (the band is dead by then)
    const size_t so = red_off + sizeof(double) * TRUSS_NRED * (size_t)t.G;
    D.o_kb = carve(std::max(band, so));
    D.o_red = D.o_kb + (int32_t)red_off;
    early.push_back({(size_t)D.o_kb + so, (size_t)D.o_kb + std::max(band, so)});
    info.band = {(size_t)D.o_kb, (size_t)D.o_kb + band};
  }
  // solver scratch; before the solver the same bytes hold the per-element (k cc, k cs, k ss), after
  // the back substitution `red` (objective partials) reuses the z vectors
  const size_t scratch0 = carve.off;
  D.o_zs = carve(sizeof(double) * (size_t)g.zlen * g.nteams);  // z vector per team (zlen is even)
  D.o_xsol = carve(sizeof(double) * (g.zslot + 4));  // + zero slot, dummy slot, 16-byte fill
  D.o_rbuf = carve(sizeof(double) * std::max(t.n_rest, 1));
  D.o_zring = carve(sizeof(double) * W * g.nteams);   // per-lane trash slots
  D.o_ev = (int32_t)scratch0;
  info.ev = {scratch0, scratch0 + ev_bytes};
  auto actions = [&]() {
    const size_t o0 = carve.off;
    D.o_geo = carve(sizeof(float) * 2 * N);
    D.o_tac = carve(sizeof(float) * 3 * N);
    D.o_mrg = (int32_t)o0;  // merge scratch of the two-sided solver: the actions are dead by then
    carve.at_least(o0, g.nteams == 2 ? sizeof(double) * (size_t)(W * W + W) : 0);
    early.push_back({o0, carve.off});
  };
  auto rows = [&]() {
    D.o_par = carve(sizeof(double) * 8);
    D.o_y = carve(sizeof(float) * N);
    D.o_x = carve(sizeof(float) * N);
    D.o_tg = carve(sizeof(float) * N);
    info.live_with_ev.push_back({(size_t)D.o_par, carve.off});
  };
  if (g.padded()) {
    actions();
    carve.at_least(scratch0, ev_bytes);
    late.push_back({scratch0, (size_t)D.o_rbuf});
    late.push_back({(size_t)D.o_zring, (size_t)D.o_geo});
    rows();
  } else {
    carve.at_least(scratch0, ev_bytes);
    late.push_back({scratch0, (size_t)D.o_rbuf});                // z vectors, solution vector
    late.push_back({(size_t)D.o_zring, carve.off});              // behind the reactions
    rows();
    actions();
  }
  D.o_sec = carve(sizeof(int32_t) * E);
  info.live_with_ev.push_back({(size_t)D.o_sec, carve.off});
  // Env regions are staggered across the LDS banks.  Dense bands: stride = 64 B (mod 256 B).  Padded bands: 128 B (mod 256 B) --
  // a 16-lane group of the pivot column's broadcast read (ds_read_b128, banks mod 64) holds the two teams of two neighbouring envs,
  // four addresses that must lie on four different 16-byte bank quads: team B is 64 B (mod 128 B) behind team A (TbGeometry), the
  // next env 128 B (mod 256 B) behind this one.  The 32-lane groups of the entering column's read (ds_read_b64: four runs of 64 B)
  // then tile the 256 bytes of the banks as well.  tools/lds_conflict_model.cpp counts every row-structured access for both.
  const size_t stagger = g.padded() ? 128 : 64;
  const size_t stride = ((carve.off + 255) & ~size_t(255)) + stagger;
  info.live_with_ev.push_back({stride - 4, stride});   // the parked symmetry coin (StepLane::coinsh)
  D.env_stride = (int32_t)stride;
  D.o_env0 = (int32_t)((table_bytes + 255) & ~size_t(255));
  return D.o_env0 + stride * (64 / t.G);
}

extern "C" int truss_topo_create(truss_topo_t **out, int32_t N, int32_t E, const int32_t *conn, const uint8_t *res,
                                 const uint8_t *top, const int32_t *pair, const uint8_t *load_mask,
                                 int32_t n_sym_nodes, const int32_t *sym_nodes, int32_t n_sym_elems,
                                 const int32_t *sym_elems, int32_t n_sections, const double *sections, double e_mod,
                                 double long_stress, const int32_t *node_order) {
  const TbInput in{N, E, conn, res, top, pair, load_mask, n_sym_nodes, sym_nodes, n_sym_elems, sym_elems, n_sections, sections,
                   e_mod, long_stress, node_order};
  if (int rc = tb_check_args(out, in)) return rc;
  std::unique_ptr<truss_topo> t(new truss_topo());   // every refusal below just returns: ~truss_topo frees what exists by then
  t->N = N;
  t->E = E;
  t->n_sections = n_sections;
  tb_neighbor_table(in, t->nbr, t->k_nbr);
  tb_dof_numbering(*t, conn, res);
  if (t->ndof < 1) return tb_fail(TRUSS_EINVAL, "no free DOF");
  std::vector<int16_t> pairs;
  if (!tb_vertical_pairs(pair, N, pairs)) return tb_fail(TRUSS_EINVAL, "pair[] must be an involution without fixed points");
  t->NP = (int)pairs.size() / 2;
  std::vector<int> dofpos;
  if (!tb_node_ordering(in, t->bw, dofpos)) return tb_fail(TRUSS_EINVAL, "node_order is not a permutation");
  t->variant = tb_pick_variant(t->bw, E);
  if (t->variant < 0) {
    char buf[256];
    snprintf(buf, sizeof buf,
             "no compiled kernel for half-bandwidth %d with %d elements (windows: 8, 16; up to 640 elements)", t->bw, E);
    return tb_fail(TRUSS_EUNSUPPORTED, buf);
  }
  const TbVariant &v = kVariants[t->variant];
  t->G = v.G;
  t->WL = v.WL;
  t->RPL = v.RPL;
  t->EPL = v.EPL;
  t->W = v.WL * v.RPL;
  t->n_pad = ((t->ndof + t->W - 1) / t->W) * t->W;
  // Two sets of tables and two layouts: the plain step and the persistent rollout with the band rows of their instantiation
  // (tb_band_stride), the EMIT instantiation with dense rows.  One device allocation holds [plain tables][EMIT tables].
  const TbGeometry g(*t, tb_band_stride(t->G, t->WL, t->RPL, t->EPL, false)), ge(*t, tb_band_stride(t->G, t->WL, t->RPL, t->EPL, true));
  TopoDev &D = t->dev, &DE = t->dev_emit;
  std::vector<char> blob, blob_e;
  if (int rc = tb_build_tables(*t, D, g, in, dofpos, pairs, blob, t->band_offsets[0])) return rc;
  std::vector<TbFrag> fr_early, fr_late;
  t->lds_bytes = tb_lds_layout(*t, D, g, blob.size(), fr_early, fr_late, t->layout[0]);
  // the neighbour table of the observation kernel's compact rows: uploaded with the tables, behind the D.blob_bytes that the step
  // kernels stage (their LDS layout stands as computed above)
  D.f_nbr = tb_push(blob, t->nbr);
  D.k_nbr = t->k_nbr;
  D.mat_stride4 = N * N / 4;
  blob.resize((blob.size() + 15) & ~size_t(15));
  if (tb_variant_emits(t->G, t->WL, t->RPL, t->EPL)) {
    if (int rc = tb_build_tables(*t, DE, ge, in, dofpos, pairs, blob_e, t->band_offsets[1])) return rc;
    fr_early.clear();
    fr_late.clear();
    tb_lds_layout(*t, DE, ge, blob_e.size(), fr_early, fr_late, t->layout[1]);
    tb_build_emit(t.get(), DE, conn, res, top, fr_early, fr_late, blob_e);   // may append the LDS-resident nN_x_e table to the blob
  }
  const size_t emit_at = (blob.size() + 255) & ~size_t(255);
  t->blob = tb_dev_alloc(emit_at + blob_e.size());
  if (!t->blob || !tb_dev_upload(t->blob, blob.data(), blob.size()) ||
      (!blob_e.empty() && !tb_dev_upload((char *)t->blob + emit_at, blob_e.data(), blob_e.size())))
    return tb_fail(TRUSS_ENOMEM, "device allocation/upload of topology tables failed");
  const size_t stride = (size_t)D.env_stride;
  D.blob = (const char *)t->blob;
  if (DE.emit_ok) {
    DE.blob = (const char *)t->blob + emit_at;
    DE.blob_bytes = (int32_t)blob_e.size();
    DE.o_flag = (int32_t)blob_e.size();   // progress word right behind the staged tables
    DE.o_env0 = (int32_t)((blob_e.size() + 16 + 255) & ~size_t(255));
    t->lds_bytes_emit = DE.o_env0 + (size_t)DE.env_stride * (64 / t->G);
    if (t->lds_bytes_emit > 160 * 1024) DE.emit_ok = 0;
  }
  if (!DE.emit_ok) {     // no EMIT launch will be asked for (tb_step_dispatch goes by dev.emit_ok)
    DE = D;
    t->lds_bytes_emit = t->lds_bytes;
  }
  D.emit_ok = DE.emit_ok;
  if (DE.emit_ok) {      // the twin of TRUSS_F_OBS_COMPACT launches: what a backend's tb_launch_step reads of a topology
    truss_topo *c = new truss_topo();
    t->compact.reset(c);
    c->N = t->N;
    c->E = t->E;
    c->G = t->G;
    c->WL = t->WL;
    c->RPL = t->RPL;
    c->EPL = t->EPL;
    c->W = t->W;
    c->variant = t->variant;
    c->lds_bytes = t->lds_bytes;
    c->lds_bytes_emit = t->lds_bytes_emit;
    c->dev = D;
    c->dev_emit = DE;
    c->dev_emit.et_mat = t->et_mat_c;
    c->dev_emit.nc_mat = t->nc_mat_c;
    c->dev_emit.mat_stride4 = t->nc_mat_c;
  }
  if (tb_env_int("TRUSS_VERBOSE", 0))
    fprintf(stderr,
            "[truss_mi355] N=%d E=%d ndof=%d bw=%d | G=%d WL=%d RPL=%d EPL=%d teams=%d KA=%d mid=%d | band rows %d B apart, tables %d B, "
            "env %zu B, LDS/workgroup %zu B (%zu workgroups/CU), fused observation writer %s\n",
            N, E, t->ndof, t->bw, t->G, t->WL, t->RPL, t->EPL, g.nteams, g.KA, g.mid, 8 * g.KS, D.blob_bytes, stride, t->lds_bytes,
            (size_t)(160 * 1024) / t->lds_bytes, D.emit_ok ? "yes" : "no");
  if (tb_env_int("TRUSS_VERBOSE", 0) && D.emit_ok)
    fprintf(stderr, "[truss_mi355]   fused launch: tables %d B, LDS/workgroup %zu B (%zu workgroups/CU)\n", t->dev_emit.blob_bytes,
            t->lds_bytes_emit, (size_t)(160 * 1024) / t->lds_bytes_emit);
  if (t->lds_bytes > 160 * 1024) return tb_fail(TRUSS_EUNSUPPORTED, "topology needs more than 160 KiB of LDS per workgroup");
  *out = t.release();
  return TRUSS_OK;
}

extern "C" int truss_topo_destroy(truss_topo_t *t) {
  delete t;
  return TRUSS_OK;
}

extern "C" int truss_topo_dofs(const truss_topo_t *t, int32_t *nsc, int32_t *ttnsc) {
  if (!t) return tb_fail(TRUSS_EINVAL, "NULL topology");
  if (nsc) memcpy(nsc, t->nsc.data(), t->nsc.size() * sizeof(int32_t));
  if (ttnsc) memcpy(ttnsc, t->ttnsc.data(), t->ttnsc.size() * sizeof(int32_t));
  return t->ndof;
}

extern "C" int truss_topo_solver_info(const truss_topo_t *t, int32_t *perm, int32_t *half_bandwidth,
                                      int32_t *lanes_per_env, int32_t *rows_per_lane) {
  if (!t) return tb_fail(TRUSS_EINVAL, "NULL topology");
  if (perm) memcpy(perm, t->perm.data(), t->perm.size() * sizeof(int32_t));
  if (half_bandwidth) *half_bandwidth = t->bw;
  if (lanes_per_env) *lanes_per_env = t->G;
  if (rows_per_lane) *rows_per_lane = t->RPL;
  return TRUSS_OK;
}

extern "C" int truss_topo_fused_obs(const truss_topo_t *t) { return t && t->dev.emit_ok ? 1 : 0; }

extern "C" int truss_topo_neighbors(const truss_topo_t *t, int16_t *out, int32_t cap, int32_t *k_nbr) {
  if (!t) return tb_fail(TRUSS_EINVAL, "NULL topology");
  if (k_nbr) *k_nbr = t->k_nbr;
  if (out) {
    if (cap < (int32_t)t->nbr.size()) return tb_fail(TRUSS_EINVAL, "truss_topo_neighbors: out holds fewer than n_nodes * k_nbr entries");
    memcpy(out, t->nbr.data(), t->nbr.size() * sizeof(int16_t));
  }
  return TRUSS_OK;
}

extern "C" int truss_topo_lds_info(const truss_topo_t *t, int32_t emit, int32_t *info, int32_t *live, int32_t cap_live,
                                   int32_t *band_offsets, int32_t cap_offsets) {
  if (!t || !info) return tb_fail(TRUSS_EINVAL, "NULL argument");
  const int which = emit && t->dev.emit_ok ? 1 : 0;
  const TopoDev &D = which ? t->dev_emit : t->dev;
  const TbLayoutInfo &I = t->layout[which];
  const TbGeometry g(*t, tb_band_stride(t->G, t->WL, t->RPL, t->EPL, which != 0));
  const int32_t v[TRUSS_LDS_INFO_LEN] = {(int32_t)(which ? t->lds_bytes_emit : t->lds_bytes), D.o_env0, D.env_stride, 64 / t->G, g.W, g.KS,
                                         g.rowsA, g.rowsB, g.kb_b, g.trash_off(), (int32_t)I.band.lo, (int32_t)I.band.hi,
                                         (int32_t)I.ev.lo, (int32_t)I.ev.hi, (int32_t)I.live_with_ev.size(),
                                         (int32_t)t->band_offsets[which].size()};
  memcpy(info, v, sizeof v);
  for (int i = 0; live && i < cap_live && i < (int)I.live_with_ev.size(); ++i) {
    live[2 * i] = (int32_t)I.live_with_ev[i].lo;
    live[2 * i + 1] = (int32_t)I.live_with_ev[i].hi;
  }
  for (int i = 0; band_offsets && i < cap_offsets && i < (int)t->band_offsets[which].size(); ++i) band_offsets[i] = t->band_offsets[which][i];
  return TRUSS_OK;
}

static int tb_make_step_args(const truss_topo_t *t, const truss_step_args_t *a, StepArgsDev &D) {
  if (!t || !a) return tb_fail(TRUSS_EINVAL, "NULL argument");
  if (a->struct_size != sizeof(truss_step_args_t)) return tb_fail(TRUSS_EINVAL, "truss_step_args_t size mismatch (ABI)");
  if (a->n_envs < 1) return tb_fail(TRUSS_EINVAL, "n_envs < 1");
  const bool decode = !(a->flags & TRUSS_F_NO_DECODE);
  if (!a->x || !a->y_in || !a->sec_in || !a->target || !a->env_params || !a->y_out || !a->disp || !a->q0 || !a->sr ||
      !a->comp || !a->point)
    return tb_fail(TRUSS_EINVAL, "a required device pointer is NULL");
  if (((size_t)a->point & 15) != 0 || ((size_t)a->obj & 7) != 0) return tb_fail(TRUSS_EINVAL, "point must be 16-byte aligned, obj 8-byte aligned");
  if (decode && (!a->a_geo || !a->a_topo)) return tb_fail(TRUSS_EINVAL, "actions are NULL");
  if (decode && !t->dev.has_pairs) return tb_fail(TRUSS_EINVAL, "action decode needs a vertical-pair table");
  if ((a->max_up_in == nullptr) != (a->max_down_in == nullptr)) return tb_fail(TRUSS_EINVAL, "max_up_in/max_down_in must come together");
  if ((a->max_up_out == nullptr) != (a->max_down_out == nullptr)) return tb_fail(TRUSS_EINVAL, "max_up_out/max_down_out must come together");
  if (decode && t->dev.n_sym_nodes + t->dev.n_sym_elems > 0 && !a->coin) return tb_fail(TRUSS_EINVAL, "symmetric topology needs coin[]");
  D.B = a->n_envs;
  D.flags = a->flags;
  D.x = a->x;
  D.y_in = a->y_in;
  D.sec_in = a->sec_in;
  D.mu_in = a->max_up_in;
  D.md_in = a->max_down_in;
  D.a_geo = a->a_geo;
  D.a_topo = a->a_topo;
  D.coin = a->coin;
  D.target = a->target;
  D.env_params = a->env_params;
  D.y_out = a->y_out;
  D.sec_out = a->sec_out;
  D.mu_out = a->max_up_out;
  D.md_out = a->max_down_out;
  D.disp = a->disp;
  D.q0 = a->q0;
  D.sr = a->sr;
  D.comp = a->comp;
  D.point = a->point;
  D.obj = a->obj;
  D.disp64 = a->disp_f64;
  D.q064 = a->q0_f64;
  D.energy = a->energy;
  D.react = a->reactions;
  D.status = a->status;
  D.x_n = a->x_n;
  D.A_s = a->A_s;
  D.A_ts = a->A_n_ts;
  D.A_cs = a->A_n_cs;
  D.nxn = a->nN_x_n;
  D.nxe = a->nN_x_e;
  if ((a->flags & TRUSS_F_OBS_COMPACT) && !(a->flags & TRUSS_F_EMIT_OBS))
    return tb_fail(TRUSS_EINVAL, "TRUSS_F_OBS_COMPACT is a layout of TRUSS_F_EMIT_OBS: set both");
  if ((a->flags & TRUSS_F_OBS_COMPACT) && t->dev.emit_ok && !t->compact)
    return tb_fail(TRUSS_EUNSUPPORTED, "internal: no compact image for the fused observation writer");
  if (a->flags & TRUSS_F_EMIT_OBS) {
    if (!a->sec_out || !a->max_up_out) return tb_fail(TRUSS_EINVAL, "TRUSS_F_EMIT_OBS needs sec_out and max_up_out / max_down_out");
    if (!t->dev.emit_ok && tb_obs_lds_bytes(t->N) > 160 * 1024) return tb_fail(TRUSS_EUNSUPPORTED, "N too large for the observation kernel");
  }
  return TRUSS_OK;
}

// Arguments of an observation launch: `O` lists B, flags and the tensors in the order of ObsArgsDev's fields; the row tiling of the
// N x N matrices (tile_rows / n_split, the two fields behind them) is decided here
static ObsArgsDev tb_obs_args(int N, ObsArgsDev O) {
  O.tile_rows = tb_obs_tile_rows(N);
  O.n_split = tb_obs_splits(N) ? (N + O.tile_rows - 1) / O.tile_rows : 1;
  return O;
}

// One step; with TRUSS_F_EMIT_OBS the observation tensors come from the same launch where the topology allows
// it (dev.emit_ok) and from the observation kernel, launched right behind the step on the same stream, elsewhere.
static int tb_step_dispatch(const truss_topo *t, const StepArgsDev &D, void *stream) {
  if (!(D.flags & TB_EMIT_OBS)) return tb_launch_step(t, D, false, stream);
  // the layout of the fused writer is a property of the image: a compact launch is the same kernel on the twin's image
  if (t->dev.emit_ok) return tb_launch_step((D.flags & TB_OBS_COMPACT) ? t->compact.get() : t, D, true, stream);
  int rc = tb_launch_step(t, D, false, stream);
  if (rc != TRUSS_OK) return rc;
  return tb_launch_obs(t, tb_obs_args(t->N, {D.B, D.flags & TB_OBS_COMPACT, D.x, D.y_out, D.sec_out, D.mu_out, D.md_out, D.target, D.disp, D.q0, D.sr, D.comp,
                                             D.env_params, D.x_n, D.A_s, D.A_ts, D.A_cs, D.nxn, D.nxe}), stream);
}

// the persistent rollout kernel keeps rows in LDS with the staging fast path's 16-byte accesses: same conditions
static bool tb_rollout_one_launch(const truss_topo *t, const StepArgsDev &D) {
  if (tb_env_int("TRUSS_ROLLOUT_LAUNCHES", 0)) return false;          // diagnostic: one launch per step, as in round 1
  if ((D.flags & (TB_NO_DECODE | TB_EMIT_OBS | TB_CLAMP_INPLACE)) || !D.a_geo) return false;
  if (!tb_variant_rolls(t->G, t->WL, t->RPL, t->EPL)) return false;
  const int NPL = (2 * t->EPL + 4) / 5, ncap = std::max(t->G * NPL, 64), ecap = std::max(t->G * t->EPL, 128);
  return (t->N & 3) == 0 && t->N <= ncap && t->E <= ecap && t->dev.blob_bytes <= 20 * 64 * 16;
}

extern "C" int truss_topo_persistent_rollout(const truss_topo_t *t) {
  if (!t) return 0;
  StepArgsDev D{};
  D.a_geo = (float *)1;   // "decode steps with actions": what the query is about
  return tb_rollout_one_launch(t, D) ? 1 : 0;
}

extern "C" int truss_step(const truss_topo_t *t, const truss_step_args_t *a, void *stream) {
  StepArgsDev D;
  int rc = tb_make_step_args(t, a, D);
  if (rc != TRUSS_OK) return rc;
  return tb_step_dispatch(t, D, stream);
}

extern "C" int truss_rollout(const truss_topo_t *t, const truss_step_args_t *a, int32_t n_steps, int32_t n_action_sets,
                             void *stream) {
  StepArgsDev D;
  int rc = tb_make_step_args(t, a, D);
  if (rc != TRUSS_OK) return rc;
  if (n_steps < 1 || n_action_sets < 1) return tb_fail(TRUSS_EINVAL, "n_steps/n_action_sets < 1");
  if (!a->sec_out) return tb_fail(TRUSS_EINVAL, "rollout needs sec_out");
  if (a->max_up_in) return tb_fail(TRUSS_EINVAL, "rollout recomputes move ranges; pass max_up_in = NULL");
  if (tb_rollout_one_launch(t, D)) return tb_launch_rollout(t, D, n_steps, n_action_sets, stream);
  const float *ybuf[2] = {a->y_in, a->y_out};
  const int32_t *sbuf[2] = {a->sec_in, a->sec_out};
  const size_t gstride = (size_t)a->n_envs * t->N * 2, tstride = (size_t)a->n_envs * t->N * 3;
  for (int s = 0; s < n_steps; ++s) {
    StepArgsDev S = D;
    S.y_in = ybuf[s & 1];
    S.y_out = (float *)ybuf[(s + 1) & 1];
    S.sec_in = sbuf[s & 1];
    S.sec_out = (int32_t *)sbuf[(s + 1) & 1];
    if (D.a_geo) {
      S.a_geo = D.a_geo + (size_t)(s % n_action_sets) * gstride;
      S.a_topo = D.a_topo + (size_t)(s % n_action_sets) * tstride;
    }
    rc = tb_step_dispatch(t, S, stream);
    if (rc != TRUSS_OK) return rc;
  }
  return TRUSS_OK;
}

extern "C" int truss_obs(const truss_topo_t *t, const truss_obs_args_t *a, void *stream) {
  if (!t || !a) return tb_fail(TRUSS_EINVAL, "NULL argument");
  if (a->struct_size != sizeof(truss_obs_args_t)) return tb_fail(TRUSS_EINVAL, "truss_obs_args_t size mismatch (ABI)");
  if (a->n_envs < 1) return tb_fail(TRUSS_EINVAL, "n_envs < 1");
  if (!a->x || !a->y || !a->sec || !a->max_up || !a->max_down || !a->target || !a->disp || !a->q0 || !a->sr || !a->comp ||
      !a->env_params)
    return tb_fail(TRUSS_EINVAL, "a required device pointer is NULL");
  if (tb_obs_lds_bytes(t->N) > 160 * 1024) return tb_fail(TRUSS_EUNSUPPORTED, "N too large for the observation kernel");
  // (with row tiles that is N > ~3000)
  return tb_launch_obs(t, tb_obs_args(t->N, {a->n_envs, a->flags, a->x, a->y, a->sec, a->max_up, a->max_down, a->target, a->disp, a->q0,
                                             a->sr, a->comp, a->env_params, a->x_n, a->A_s, a->A_n_ts, a->A_n_cs, a->nN_x_n, a->nN_x_e}),
                       stream);
}
