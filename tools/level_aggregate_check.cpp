// level_aggregate_check.cpp -- the argument check of truss_gcn_level_aggregate (csrc/truss_gcn_level_agg.h, the part outside
// __HIPCC__) driven by a stand-alone host program, for a sanitizer build: no GPU, no Python.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/level_aggregate_check.cpp -o /tmp/level_aggregate_check
//   /tmp/level_aggregate_check        (prints one line per case; exit status 0 iff every case returned what it must)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "truss_mi355.h"

static std::string g_last;
static int tb_fail(int code, const std::string &msg) {
  g_last = msg;
  return code;
}
#include "../mop-truss-marl_amd/csrc/truss_gcn_level_agg.h"

int main() {
  const int B = 2, N = 66, C = 8, K = 6;
  std::vector<float> x(2 * B * N * C), adj((size_t)B * N * N), y(B * N * C);
  std::vector<int16_t> nbr(N * K, -1);
  auto item = [&] {
    truss_gcn_agg_t a{};
    a.struct_size = sizeof a;
    a.x = x.data(), a.adj = adj.data(), a.a_batch_stride = N * N, a.nbr = nbr.data(), a.y = y.data();
    a.n_batch = B, a.n_nodes = N, a.n_ch = C, a.k_nbr = K, a.transpose = 0;
    return a;
  };
  struct Case {
    const char *name;
    truss_gcn_agg_t a;
    int want;
  };
  std::vector<Case> cases;
  auto add = [&](const char *name, int want, auto &&edit) {
    truss_gcn_agg_t a = item();
    edit(a);
    cases.push_back({name, a, want});
  };
  add("good", TRUSS_OK, [](truss_gcn_agg_t &) {});
  add("x NULL", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.x = nullptr; });
  add("adj NULL", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.adj = nullptr; });
  add("nbr NULL", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.nbr = nullptr; });
  add("y NULL", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.y = nullptr; });
  add("k_nbr 0", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.k_nbr = 0; });
  add("k_nbr 17", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.k_nbr = 17; });
  add("k_nbr 16", TRUSS_OK, [](truss_gcn_agg_t &a) { a.k_nbr = 16; });
  add("n_ch 0", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.n_ch = 0; });
  add("n_nodes 0", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.n_nodes = 0; });
  add("n_nodes 32768", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.n_nodes = 32768; });
  add("n_batch -1", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.n_batch = -1; });
  add("a_batch_stride -1", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.a_batch_stride = -1; });
  add("struct_size", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.struct_size -= 4; });
  add("y is x", TRUSS_EINVAL, [&](truss_gcn_agg_t &a) { a.y = x.data(); });
  add("y overlaps the end of x", TRUSS_EINVAL, [&](truss_gcn_agg_t &a) { a.y = x.data() + B * N * C - 1; });
  add("y behind x", TRUSS_OK, [&](truss_gcn_agg_t &a) { a.y = x.data() + B * N * C; });
  add("2^38 elements and one more row", TRUSS_EINVAL, [](truss_gcn_agg_t &a) { a.n_batch = 1 << 30, a.n_nodes = 257, a.n_ch = 1; });
  add("empty item, nothing else set", TRUSS_OK, [](truss_gcn_agg_t &a) {
    a = truss_gcn_agg_t{};
    a.struct_size = sizeof a;
  });
  int bad = 0;
  for (const Case &c : cases) {
    g_last.clear();
    const truss_gcn_agg_t two[2] = {item(), c.a};      // behind a good item: the whole call is refused
    const int rc = tb_gcn_level_aggregate_check(two, 2);
    std::printf("%-34s -> %d  %s\n", c.name, rc, g_last.c_str());
    bad += rc != c.want;
  }
  bad += tb_gcn_level_aggregate_check(nullptr, 0) != TRUSS_OK;
  bad += tb_gcn_level_aggregate_check(nullptr, 1) != TRUSS_EINVAL;
  bad += tb_gcn_level_aggregate_check(nullptr, -1) != TRUSS_EINVAL;
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
