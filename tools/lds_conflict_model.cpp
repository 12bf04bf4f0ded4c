// lds_conflict_model.cpp -- host-only model of the LDS-array cycles and bank-conflict cycles of one workgroup of the step kernel,
// for dense band rows (row stride W) and padded ones (W + 2), built from the same host code as the library (truss_host.h): the
// tables, band offsets and LDS layout are the real ones, only the lanes' address streams are written out again here.
//
// Covered: the row-structured and table-driven accesses of phase_elements (connectivity, sections, band offsets, coordinates,
// section constants, EV stores, band scatter), phase_assemble_nodes (adjacency, diagonal offsets, EV gather, diagonal stores,
// identity rows), solver_scratch_init, the factorisation (solver_init, own-row fetches, pivot write / column read / entering
// column, z stores, merge, pivot check), the back substitution (own-row fetches, flushes, hand-over) and the solution gather and
// result stores of phase_post_elements.  Not covered: staging, decode, sizing, post_nodes, the result rows' read-out.
// Banking per instruction as measured on CDNA4: lane groups {2 x 32 | 4 x 16 | 8 x 8}, banks of 4 bytes mod 32 (stores, 4-byte
// reads) or mod 64 (8- and 16-byte reads); a group takes as many LDS cycles as its busiest bank has distinct dwords.
// What it cannot know: which stores and loads the compiler merges or splits, and the sections a batch holds (a hash here).
//
//   python3 - > metric.topo <<'PY'            # the arrays truss_topo_create receives, as text
//   import sys; sys.path[:0] = ["mop-truss-marl_amd"]
//   from truss_mi355 import synthetic
//   t = synthetic.bench_topology(16, 4)
//   f = lambda a: " ".join(str(v) for v in a.ravel().tolist())
//   print(t.N, t.E, t.sections.shape[0], t.e_mod, t.long_stress)
//   for a in (t.conn, t.res, t.top, t.pair, t.load_mask, t.sections, t.node_order): print(f(a))
//   PY
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -o lds_conflict_model tools/lds_conflict_model.cpp
//   ./lds_conflict_model metric.topo            # the table: dense | padded, per phase
//   ./lds_conflict_model metric.topo sweep      # padded rows: solver conflict cycles for every (team, env) stagger
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <vector>

#define TRUSS_HD inline
#define TRUSS_UNROLL
#define TB_STREAM_STORE(p, v) (*(p) = (v))
#define TB_OBS_STORE(p, v) (*(p) = (v))
static inline void tb_lds_add(double *p, double v) { *p += v; }
static inline double tb_rcp(double d) { return 1.0 / d; }
static inline double tb_rsqrt(double x) { return 1.0 / sqrt(x); }
static inline float tb_rcpf(float d) { return 1.0f / d; }
#include "../mop-truss-marl_amd/csrc/truss_body.h"

#define TRUSS_BACKEND_NAME "model"
struct truss_topo;
static void *tb_dev_alloc(size_t n) { return malloc(n); }
static void tb_dev_free(void *p) { free(p); }
static bool tb_dev_upload(void *dst, const void *src, size_t n) {
  memcpy(dst, src, n);
  return true;
}
static int tb_launch_step(const truss_topo *, const StepArgsDev &, bool, void *) { return -1; }
static int tb_launch_obs(const truss_topo *, const ObsArgsDev &, void *) { return -1; }
static int tb_launch_rollout(const truss_topo *, const StepArgsDev &, int, int, void *) { return -1; }
#include "../mop-truss-marl_amd/csrc/truss_host.h"

// ---- the LDS array ----
enum Kind { R32, R64, R128, W32, W64, W128 };
struct Count {
  long inst = 0, cyc = 0, conf = 0;
};
static const int kGroups128[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                      {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                      {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
struct Wave {   // one wave-instruction: the byte address of every lane, -1 = lane masked off
  long a[64];
  Wave() {
    for (long &v : a) v = -1;
  }
};
static void issue(Kind k, const Wave &w, Count &c) {
  const int dwords = (k == R64 || k == W64) ? 2 : (k == R128 || k == W128) ? 4 : 1;
  const int banks = (k == R64 || k == R128) ? 64 : 32;
  const int gsize = (k == R128 || k == W64) ? 16 : (k == W128) ? 8 : 32;
  bool any = false;
  for (int g0 = 0; g0 < 64 / gsize; ++g0) {
    std::map<int, std::set<long>> per_bank;
    for (int j = 0; j < gsize; ++j) {
      const int lane = k == R128 ? kGroups128[g0][j] : g0 * gsize + j;
      if (w.a[lane] < 0) continue;
      for (int d = 0; d < dwords; ++d) {
        const long dw = w.a[lane] / 4 + d;
        per_bank[(int)(dw % banks)].insert(dw);
      }
    }
    if (per_bank.empty()) continue;
    size_t worst = 1;
    for (auto &b : per_bank) worst = std::max(worst, b.second.size());
    c.cyc += (long)worst;
    c.conf += (long)worst - 1;
    any = true;
  }
  if (any) c.inst += 1;
}

// ---- one layout of one topology ----
struct Layout {
  TopoDev D{};
  std::vector<char> blob;
  int G, WL, EPL, NPL, W, KS, kb_b;
  template <class T>
  const T *tab(int32_t off) const { return (const T *)(blob.data() + off); }
};
struct Phases {
  Count elements, assemble, scratch, factor, backsub, post;
};

// every lane's address of one access: f(lane, g, grp) -> byte address in LDS or -1
template <class F>
static void all_lanes(Kind k, Count &c, const Layout &Y, F f) {
  Wave w;
  for (int l = 0; l < 64; ++l) w.a[l] = f(l, l % Y.G, l / Y.G);
  issue(k, w, c);
}

static Phases run_model(const Layout &Y, int n_sections) {
  const TopoDev &T = Y.D;
  const int G = Y.G, WL = Y.WL, W = Y.W, KS = Y.KS, EPL = Y.EPL, NPL = Y.NPL, E = T.E, N = T.N;
  Phases P;
  auto Lb = [&](int grp) { return (long)T.o_env0 + (long)grp * T.env_stride; };
  auto team_of = [&](int g) { return T.nteams == 2 ? (g / WL) & 1 : 0; };
  auto Kt = [&](int g, int grp) { return Lb(grp) + T.o_kb + 8L * team_of(g) * Y.kb_b; };
  auto Zt = [&](int g, int grp) { return Lb(grp) + T.o_zs + 8L * team_of(g) * T.zlen; };
  auto ZRt = [&](int g, int grp) { return Lb(grp) + T.o_zring + 8L * team_of(g) * W; };
  auto sec_of = [&](int grp, int e) { return (int)((2654435761u * (unsigned)(grp * 977 + e + 1)) >> 16) % n_sections; };
  const int16_t *CN = Y.tab<int16_t>(T.f_conn), *AC = Y.tab<int16_t>(T.f_asm), *AD = Y.tab<int16_t>(T.f_adj8),
                *DO = Y.tab<int16_t>(T.f_diagoff), *EX = Y.tab<int16_t>(T.f_exs);
  auto elem = [&](int g, int i) { return std::min(g + G * i, E - 1); };
  auto node = [&](int g, int i) { return std::min(g + G * i, N - 1); };

  // ---- phase_elements ----
  {
    Count &c = P.elements;
    for (int j = 0; j < 3; ++j) all_lanes(W64, c, Y, [&](int, int g, int grp) { return g == 0 ? Lb(grp) + T.o_ev + 8L * (3 * E + j) : -1L; });
    for (int i = 0; i < EPL; ++i) {
      all_lanes(R32, c, Y, [&](int, int g, int) { return (long)T.f_conn + 4L * elem(g, i); });
      all_lanes(R32, c, Y, [&](int, int g, int grp) { return Lb(grp) + T.o_sec + 4L * elem(g, i); });
      all_lanes(R64, c, Y, [&](int, int g, int) { return (long)T.f_asm + 8L * elem(g, i); });
    }
    for (int i = 0; i < EPL; ++i) {
      for (int q = 0; q < 4; ++q)
        all_lanes(R32, c, Y, [&](int, int g, int grp) { return Lb(grp) + ((q & 2) ? T.o_y : T.o_x) + 4L * CN[2 * elem(g, i) + (q & 1)]; });
      all_lanes(R64, c, Y, [&](int, int g, int grp) { return (long)T.f_area + 8L * sec_of(grp, elem(g, i)); });
    }
    for (int i = 0; i < EPL; ++i) {
      all_lanes(R64, c, Y, [&](int, int g, int grp) { return (long)T.f_isr + 8L * sec_of(grp, elem(g, i)); });
      for (int j = 0; j < 3; ++j) all_lanes(W64, c, Y, [&](int, int g, int grp) { return Lb(grp) + T.o_ev + 8L * (3 * elem(g, i) + j); });
      for (int q : {0, 1, 2, 3}) all_lanes(W64, c, Y, [&](int, int g, int grp) { return Lb(grp) + T.o_kb + 8L * AC[4 * elem(g, i) + (q == 1 ? 2 : q == 2 ? 1 : q)]; });
    }
  }
  // ---- phase_assemble_nodes ----
  {
    Count &c = P.assemble;
    for (int i = 0; i < NPL; ++i) {
      all_lanes(R128, c, Y, [&](int, int g, int) { return (long)T.f_adj8 + 16L * node(g, i); });
      for (int j = 0; j < 3; ++j) all_lanes(R32, c, Y, [&](int, int g, int) { return ((long)T.f_diagoff + 2L * (3 * node(g, i) + j)) & ~3L; });
    }
    for (int h = 0; h < 2; ++h)
      for (int i = 0; i < NPL; ++i)
        for (int a = 0; a < 4; ++a)
          for (int j = 0; j < 3; ++j)
            all_lanes(R64, c, Y, [&](int, int g, int grp) { return Lb(grp) + T.o_ev + 8L * (3 * AD[node(g, i) * 8 + 4 * h + a] + j); });
    for (int i = 0; i < NPL; ++i)
      for (int j = 0; j < 3; ++j) all_lanes(W64, c, Y, [&](int, int g, int grp) { return Lb(grp) + T.o_kb + 8L * DO[3 * node(g, i) + j]; });
    const int idA = T.nteams == 1 ? T.ndof : T.ndof - T.KA;
    for (int r0 = idA; r0 < T.rowsA; r0 += G)
      all_lanes(W64, c, Y, [&](int, int g, int grp) { return r0 + g < T.rowsA ? Lb(grp) + T.o_kb + 8L * ((r0 + g) * KS + (r0 + g) % W) : -1L; });
    for (int r0 = T.KA + T.mid; r0 < T.rowsB; r0 += G)
      all_lanes(W64, c, Y, [&](int, int g, int grp) { return r0 + g < T.rowsB ? Lb(grp) + T.o_kb + 8L * (Y.kb_b + (r0 + g) * KS + (r0 + g) % W) : -1L; });
  }
  // ---- solver_scratch_init ----
  {
    Count &c = P.scratch;
    const int zt = T.zlen * T.nteams;
    for (int r0 = 0; r0 < std::max(zt, 6 * G); r0 += G) {
      const bool unrolled = r0 < 6 * G;
      all_lanes(R32, c, Y, [&](int, int g, int) { return unrolled || r0 + g < zt ? ((long)T.f_zcode + std::min(r0 + g, zt - 1)) & ~3L : -1L; });
      all_lanes(W64, c, Y, [&](int, int g, int grp) { return unrolled || r0 + g < zt ? Lb(grp) + T.o_zs + 8L * std::min(r0 + g, zt - 1) : -1L; });
    }
    for (int r0 = 0; r0 < (T.zslot + 2) / 2; r0 += G)
      all_lanes(W128, c, Y, [&](int, int g, int grp) { return r0 + g < (T.zslot + 2) / 2 ? Lb(grp) + T.o_xsol + 16L * (r0 + g) : -1L; });
    for (int r0 = 0; r0 < T.n_rest; r0 += G)
      all_lanes(W64, c, Y, [&](int, int g, int grp) { return r0 + g < T.n_rest ? Lb(grp) + T.o_rbuf + 8L * (r0 + g) : -1L; });
  }
  if (T.nteams != 2 || W > 8) {
    fprintf(stderr, "the solver model covers the two-team, window-8 schedule only\n");
    return P;
  }
  // ---- factorisation (TRUSS_STEP_SCHEDULE, two teams, W <= 8) ----
  {
    Count &c = P.factor;
    auto fetch = [&](int kb) {
      for (int i = 0; i < W / 2; ++i) all_lanes(R128, c, Y, [&](int, int g, int grp) { return Kt(g, grp) + 8L * (kb + W + g % WL) * KS + 16L * i; });
      all_lanes(R64, c, Y, [&](int, int g, int grp) { return Zt(g, grp) + 8L * (kb + W + g % WL); });
    };
    auto pivot = [&](int k) {
      all_lanes(W64, c, Y, [&](int, int g, int grp) { return Kt(g, grp) + 8L * (k * KS + g % WL); });
      all_lanes(R64, c, Y, [&](int, int g, int grp) { return Kt(g, grp) + 8L * ((k + W) * KS + g % WL); });
      for (int i = 0; i < W / 2; ++i) all_lanes(R128, c, Y, [&](int, int g, int grp) { return Kt(g, grp) + 8L * k * KS + 16L * i; });
    };
    auto z_store = [&](int kb, int c0, int cnt) {
      all_lanes(W64, c, Y, [&](int, int g, int grp) {
        const int off = (g % WL - c0 + W) % W;
        return off < cnt ? Zt(g, grp) + 8L * (kb + off) : ZRt(g, grp) + 8L * (g % WL);
      });
    };
    for (int cc = 0; cc < W; ++cc) all_lanes(R64, c, Y, [&](int, int g, int grp) { const int r = g % WL; return Kt(g, grp) + 8L * (cc <= r ? r * KS + cc : cc * KS + r); });
    all_lanes(R64, c, Y, [&](int, int g, int grp) { return Zt(g, grp) + 8L * (g % WL); });
    int kb = 0;
    for (; kb + W <= T.KA; kb += W) {
      fetch(kb);
      for (int kk = 0; kk < W; ++kk) pivot(kb + kk);
      z_store(kb, 0, W);
    }
    const int c0 = T.KA % W;
    if (c0 > 0) fetch(kb);
    for (int kk = 0; kk < c0; ++kk) pivot(kb + kk);
    if (c0 > 0) z_store(kb, 0, c0);
    for (int j = 0; j <= W; ++j)   // merge_post: team B's window rows and right-hand sides; merge_take: team A reads them
      all_lanes(W64, c, Y, [&](int, int g, int grp) { return team_of(g) == 1 ? Lb(grp) + T.o_mrg + 8L * (j < W ? (g % WL) * W + j : W * W + g % WL) : -1L; });
    auto win_row = [&](int slot) { return T.KA + ((slot - T.KA % W + W) % W); };
    for (int j = 0; j <= W; ++j)
      all_lanes(R64, c, Y, [&](int, int g, int grp) {
        if (team_of(g) != 0) return -1L;
        const int lim = T.ndof - T.KA, p = win_row(g % WL), pb = T.ndof - 1 - p;
        if (j == W) return Lb(grp) + T.o_mrg + 8L * (W * W + (p < lim ? pb % W : 0));
        const int cw = win_row(j), cb = T.ndof - 1 - cw;
        return Lb(grp) + T.o_mrg + 8L * ((p < lim && cw < lim) ? (pb % W) * W + cb % W : 0);
      });
    for (int i = 0; i < W; ++i) {
      if ((c0 + i) % W == 0) fetch(T.KA + i);
      pivot(T.KA + i);
    }
    z_store(T.KA, c0, W);
    for (int k0 = 0; k0 < T.KA + W; k0 += WL)
      all_lanes(R64, c, Y, [&](int, int g, int grp) {
        const int lim = team_of(g) == 1 ? T.KA : T.KA + W, k = k0 + g % WL;
        return k < lim ? Kt(g, grp) + 8L * (k * KS + k % W) : -1L;
      });
  }
  // ---- back substitution ----
  {
    Count &c = P.backsub;
    auto fetch = [&](int kb) {
      for (int i = 0; i < W / 2; ++i) all_lanes(R128, c, Y, [&](int, int g, int grp) { return Kt(g, grp) + 8L * std::max(kb + g % WL, 0) * KS + 16L * i; });
      all_lanes(R64, c, Y, [&](int, int g, int grp) { return Zt(g, grp) + 8L * std::max(kb + g % WL, 0); });
      all_lanes(R64, c, Y, [&](int, int g, int grp) { const int pc = std::max(kb + g % WL, 0); return Kt(g, grp) + 8L * (pc * KS + pc % W); });
    };
    auto owns = [&](int tm, int p) { return tm == 0 ? p < T.ndof - T.KA : p < T.KA; };
    auto flush = [&](int kb) {
      all_lanes(W64, c, Y, [&](int, int g, int grp) {
        const int tm = team_of(g), p = kb + g % WL;
        return Lb(grp) + T.o_xsol + 8L * (owns(tm, p) ? (tm ? T.ndof - 1 - p : p) : T.zslot + 1);
      });
    };
    auto win_row = [&](int slot) { return T.KA + ((slot - T.KA % W + W) % W); };
    const int kend = T.KA + W, c0 = T.KA % W;
    int kb = ((kend - 1) / W) * W;
    fetch(kb);
    fetch(kb - W);
    for (int i = W - 1; i >= 0; --i)
      if ((c0 + i) % W == 0 && i > 0) {
        kb -= W;
        fetch(kb - W);
      }
    all_lanes(W64, c, Y, [&](int, int g, int grp) {   // backsub_flush_mid
      const int p = win_row(g % WL);
      return Lb(grp) + T.o_xsol + 8L * ((team_of(g) == 0 && owns(0, p)) ? p : T.zslot + 1);
    });
    for (int j = 0; j < W; ++j)                      // backsub_reload
      all_lanes(R64, c, Y, [&](int, int g, int grp) {
        const int p = win_row(j), o = team_of(g) ? T.ndof - 1 - p : p;
        return Lb(grp) + T.o_xsol + 8L * ((o >= 0 && o < T.ndof) ? o : T.zslot);
      });
    if (c0 > 0) flush(kb);
    kb -= W;
    for (; kb >= 0; kb -= W) {
      fetch(kb - W);
      flush(kb);
    }
  }
  // ---- phase_post_elements ----
  {
    Count &c = P.post;
    for (int i = 0; i < EPL; ++i) all_lanes(R64, c, Y, [&](int, int g, int) { return (long)T.f_exs + 8L * elem(g, i); });
    for (int i = 0; i < EPL; ++i)
      for (int q = 0; q < 4; ++q) all_lanes(R64, c, Y, [&](int, int g, int grp) { return Lb(grp) + T.o_xsol + 8L * EX[4 * elem(g, i) + q]; });
    for (int i = 0; i < EPL; ++i) {
      all_lanes(W32, c, Y, [&](int, int g, int grp) { return Lb(grp) + T.o_kb + T.so_q0 + 4L * elem(g, i); });
      all_lanes(W32, c, Y, [&](int, int g, int grp) { return Lb(grp) + T.o_kb + T.so_sr + 4L * elem(g, i); });
      all_lanes(W32, c, Y, [&](int, int g, int grp) { return (Lb(grp) + T.o_kb + T.so_comp + elem(g, i)) & ~3L; });
    }
  }
  return P;
}

template <class T>
static std::vector<T> read_n(std::ifstream &f, size_t n) {
  std::vector<T> v(n);
  for (auto &x : v) {
    double d = 0;
    f >> d;
    x = (T)d;
  }
  return v;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <topology dump> [sweep]\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1]);
  int N = 0, E = 0, S = 0;
  double e_mod = 0, long_stress = 0;
  f >> N >> E >> S >> e_mod >> long_stress;
  if (!f || N < 2 || E < 1 || S < 1) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  const auto conn = read_n<int32_t>(f, 2 * (size_t)E);
  const auto res = read_n<uint8_t>(f, 2 * (size_t)N), top = read_n<uint8_t>(f, N);
  const auto pair = read_n<int32_t>(f, N);
  const auto load_mask = read_n<uint8_t>(f, 2 * (size_t)N);
  const auto sections = read_n<double>(f, 2 * (size_t)S);
  const auto order = read_n<int32_t>(f, N);
  if (!f) {
    fprintf(stderr, "%s is shorter than its header says\n", argv[1]);
    return 2;
  }
  const TbInput in{N, E, conn.data(), res.data(), top.data(), pair.data(), load_mask.data(), 0, nullptr, 0, nullptr, S, sections.data(),
                   e_mod, long_stress, order.data()};
  truss_topo t;   // the first phases of truss_topo_create
  t.N = N;
  t.E = E;
  t.n_sections = S;
  tb_dof_numbering(t, conn.data(), res.data());
  std::vector<int16_t> pairs;
  std::vector<int> dofpos;
  if (!tb_vertical_pairs(pair.data(), N, pairs) || !tb_node_ordering(in, t.bw, dofpos) || (t.variant = tb_pick_variant(t.bw, E)) < 0) {
    fprintf(stderr, "topology refused\n");
    return 1;
  }
  t.NP = (int)pairs.size() / 2;
  const TbVariant &v = kVariants[t.variant];
  t.G = v.G, t.WL = v.WL, t.RPL = v.RPL, t.EPL = v.EPL, t.W = v.WL * v.RPL;
  t.n_pad = ((t.ndof + t.W - 1) / t.W) * t.W;
  if (t.RPL != 1) {
    fprintf(stderr, "one row per lane only\n");
    return 1;
  }
  // team_stagger / env_stagger < 0: what the library lays out for this row stride
  auto layout = [&](int ks, int team_stagger, int env_stagger) {
    Layout Y;
    TbGeometry g(t, ks);
    if (team_stagger >= 0) g.kb_b = g.rowsA * ks + ((team_stagger - g.rowsA * ks * 8) & 127) / 8;
    std::vector<int32_t> offs;
    std::vector<TbFrag> early, late;
    TbLayoutInfo info;
    if (tb_build_tables(t, Y.D, g, in, dofpos, pairs, Y.blob, offs) != TRUSS_OK) exit(1);
    const size_t bytes = tb_lds_layout(t, Y.D, g, Y.blob.size(), early, late, info);
    if (env_stagger >= 0) Y.D.env_stride = (Y.D.env_stride & ~255) + env_stagger;
    Y.G = t.G, Y.WL = t.WL, Y.EPL = t.EPL, Y.NPL = (2 * t.EPL + 4) / 5, Y.W = t.W, Y.KS = ks, Y.kb_b = g.kb_b;
    if (team_stagger < 0 && env_stagger < 0)
      printf("row stride %2d doubles: team B %d B behind team A (%d mod 128), env stride %d B (%d mod 256), LDS per workgroup %zu B\n", ks,
             8 * g.kb_b, (8 * g.kb_b) % 128, Y.D.env_stride, Y.D.env_stride % 256, bytes);
    return Y;
  };
  if (argc > 2 && !strcmp(argv[2], "sweep")) {
    printf("padded rows (stride %d): conflict cycles of factorisation + back substitution per workgroup\nteam stagger (B mod 128) down, env stagger (B mod 256) across\n      ", t.W + 2);
    for (int es = 0; es < 256; es += 16) printf("%6d", es);
    printf("\n");
    for (int ts = 0; ts < 128; ts += 16) {
      printf("%6d", ts);
      for (int es = 0; es < 256; es += 16) {
        const Phases P = run_model(layout(t.W + 2, ts, es), S);
        printf("%6ld", P.factor.conf + P.backsub.conf);
      }
      printf("\n");
    }
    return 0;
  }
  printf("N=%d E=%d ndof=%d | G=%d WL=%d EPL=%d | one workgroup (%d envs)\n", N, E, t.ndof, t.G, t.WL, t.EPL, 64 / t.G);
  const Phases A = run_model(layout(t.W, -1, -1), S), B = run_model(layout(t.W + 2, -1, -1), S);
  printf("%-22s %28s | %28s\n%-22s %8s %9s %9s | %8s %9s %9s\n", "", "dense rows", "padded rows", "phase", "cycles", "conflict", "ratio", "cycles",
         "conflict", "ratio");
  struct Row {
    const char *name;
    const Count Phases::*m;
  };
  const Row rows[] = {{"elements", &Phases::elements}, {"assemble_nodes", &Phases::assemble}, {"scratch_init", &Phases::scratch},
                      {"factorisation", &Phases::factor}, {"back substitution", &Phases::backsub}, {"post_elements", &Phases::post}};
  Count ta, tb;
  for (const Row &r : rows) {
    const Count &a = A.*(r.m), &b = B.*(r.m);
    printf("%-22s %8ld %9ld %9.2f | %8ld %9ld %9.2f\n", r.name, a.cyc, a.conf, a.cyc ? (double)a.conf / a.cyc : 0.0, b.cyc, b.conf,
           b.cyc ? (double)b.conf / b.cyc : 0.0);
    ta.cyc += a.cyc, ta.conf += a.conf, tb.cyc += b.cyc, tb.conf += b.conf;
  }
  printf("%-22s %8ld %9ld %9.2f | %8ld %9ld %9.2f\n", "all of the above", ta.cyc, ta.conf, (double)ta.conf / ta.cyc, tb.cyc, tb.conf,
         (double)tb.conf / tb.cyc);
  return 0;
}
