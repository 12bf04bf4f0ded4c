// truss_torch_ops.cpp -- PyTorch custom operators in front of the C ABI of include/truss_mi355.h: one operator of
// torch.ops.truss_mi355 per line of TRUSS_OPERATOR_ENTRIES below.
//
// The reference's hot path runs inside TensorFlow ops on its side of the loop (truss2D_RL.py:328-354); here the env
// step itself is an operator of the host framework: tensors in, tensors mutated in place, launched on the stream the
// caller names (torch's current stream), capturable in a hipGraph, traceable (Meta kernels).  The operators do no
// arithmetic: they check tensors (device, dtype, contiguity, sizes), fill the ABI's argument block with data
// pointers and call the entry point of the native library the caller bound (`lib`: the HIP product library, or the
// CPU lane emulator of the test-suite) -- the same entry points a ctypes / cffi binding would call.
// Built by csrc/Makefile with g++ against the installed libtorch; no HIP headers needed.
#include <torch/library.h>
#include <ATen/ATen.h>

#include <dlfcn.h>

#include <array>
#include <cstring>
#include <vector>
#include <string>

#include "../../include/truss_mi355.h"

// THE table of native entry points: X(field, symbol, required).  `field` is the member of Backend and, for the
// operator entries, the name of the operator (and of the function below that implements it); `symbol` is looked up by
// name in the bound library, its pointer type comes from the header's declaration.  A library may lack the optional
// ones (the CPU lane emulator does): their operators then fail with "the bound native library has no <symbol>".
#define TRUSS_OPERATOR_ENTRIES(X)                                \
  X(step, truss_step, true)                                      \
  X(rollout, truss_rollout, true)                                \
  X(obs, truss_obs, true)                                        \
  X(front, truss_front, true)                                    \
  X(gcn_aggregate, truss_gcn_aggregate, true)                    \
  X(gcn_aggregate_sparse, truss_gcn_aggregate_sparse, true)      \
  X(gcn_layer, truss_gcn_layer, true)                            \
  X(gcn_split_w, truss_gcn_split_w, true)                        \
  X(gcn_level, truss_gcn_level, true)                            \
  X(gcn_level_backward, truss_gcn_level_backward, false)         \
  X(replay_scatter, truss_replay_scatter, false)                 \
  X(replay_gather, truss_replay_gather, false)                   \
  X(reward, truss_reward, false)                                 \
  X(archive_merge, truss_archive_merge, false)                   \
  X(gcn_layer_fused, truss_gcn_layer_fused, false)               \
  X(gcn_layer_terms, truss_gcn_layer_terms, false)               \
  X(gcn_layer_group, truss_gcn_layer_group, false)               \
  X(pair_setup, truss_pair_setup, false)                         \
  X(gcn_level_aggregate, truss_gcn_level_aggregate, false)        \
  X(optim_step, truss_optim_step, false)                         \
  X(critic_tail, truss_critic_tail, false)                       \
  X(critic_tail_backward, truss_critic_tail_backward, false)     \
  X(target_update, truss_target_update, false)
#define TRUSS_ENTRY_POINTS(X) TRUSS_OPERATOR_ENTRIES(X) X(last_error, truss_last_error, true)

namespace {

struct Backend {
#define X(field, symbol, required) decltype(&symbol) field = nullptr;
  TRUSS_ENTRY_POINTS(X)
#undef X
  bool device = false;   // true: the HIP library (tensors must be on a cuda device)
  decltype(&truss_topo_neighbors) topo_neighbors = nullptr;   // no operator of its own: the width of the compact observation rows
};
std::array<Backend, 8> g_backends;

const Backend &backend(int64_t lib) {
  TORCH_CHECK(lib >= 0 && lib < (int64_t)g_backends.size() && g_backends[lib].step, "truss_mi355: native library ", lib,
              " is not bound (truss_mi355.ops binds it when it loads the library)");
  return g_backends[lib];
}

void check_rc(const Backend &b, int rc, const char *what) {
  TORCH_CHECK(rc == TRUSS_OK, what, " failed (", rc, "): ", b.last_error ? b.last_error() : "?");
}

using OT = c10::optional<at::Tensor>;
bool present(const OT &t) { return t.has_value() && t->defined(); }
OT at_or_none(const c10::List<OT> &l, size_t i) { return l.empty() ? OT() : l.get(i); }   // an empty list: no entry for any layer

// data pointer of a tensor the ABI will read / write as `dtype`, nullptr for an absent optional
template <typename T>
T *ptr(const Backend &b, const at::Tensor &t, at::ScalarType dtype, const char *name, int64_t min_numel = 0) {
  TORCH_CHECK(t.scalar_type() == dtype, "truss_mi355: ", name, " must be ", dtype, ", got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), "truss_mi355: ", name, " must be contiguous");
  TORCH_CHECK(b.device ? t.is_cuda() : t.is_cpu(), "truss_mi355: ", name, " is on ", t.device(), ", the bound library needs ",
              b.device ? "a cuda (ROCm) device" : "the cpu");
  TORCH_CHECK(t.numel() >= min_numel, "truss_mi355: ", name, " has ", t.numel(), " elements, needs ", min_numel);
  return (T *)t.data_ptr();
}
template <typename T>
T *ptr(const Backend &b, const OT &t, at::ScalarType dtype, const char *name, int64_t min_numel = 0) {
  return present(t) ? ptr<T>(b, *t, dtype, name, min_numel) : nullptr;
}

// an optional entry point of the bound library
template <typename F>
void need(F fn, const char *symbol) {
  TORCH_CHECK(fn, "truss_mi355: the bound native library has no ", symbol);
}

#define STEP_TENSOR_PARAMS                                                                                                     \
  const at::Tensor &x, const at::Tensor &y_in, const at::Tensor &sec_in, const OT &max_up_in, const OT &max_down_in,          \
      const OT &a_geo, const OT &a_topo, const OT &coin, const at::Tensor &target, const at::Tensor &env_params,              \
      const at::Tensor &y_out, const OT &sec_out, const OT &max_up_out, const OT &max_down_out, const at::Tensor &disp,       \
      const at::Tensor &q0, const at::Tensor &sr, const at::Tensor &comp, const at::Tensor &point, const OT &obj,             \
      const OT &disp_f64, const OT &q0_f64, const OT &energy, const OT &reactions, const OT &status, const OT &x_n,           \
      const OT &A_s, const OT &A_n_ts, const OT &A_n_cs, const OT &nN_x_n, const OT &nN_x_e
#define STEP_TENSOR_ARGS                                                                                                       \
  x, y_in, sec_in, max_up_in, max_down_in, a_geo, a_topo, coin, target, env_params, y_out, sec_out, max_up_out, max_down_out,  \
      disp, q0, sr, comp, point, obj, disp_f64, q0_f64, energy, reactions, status, x_n, A_s, A_n_ts, A_n_cs, nN_x_n, nN_x_e

// floats per env of A_s / A_n_ts / A_n_cs: N N, or N Kc in the compact layout (the library's own table width)
int64_t adj_floats(const Backend &b, int64_t topo, int64_t N, bool compact) {
  if (!compact) return N * N;
  need(b.topo_neighbors, "truss_topo_neighbors");
  int32_t k = 0;
  check_rc(b, b.topo_neighbors((const truss_topo_t *)topo, nullptr, 0, &k), "truss_topo_neighbors");
  return N * (int64_t)k;
}

void fill_step(const Backend &b, int64_t topo, truss_step_args_t &a, int64_t flags, int64_t n_envs, int64_t N, int64_t E, int64_t sets,
               STEP_TENSOR_PARAMS) {
  TORCH_CHECK(n_envs >= 1 && N >= 2 && E >= 1, "truss_mi355: bad n_envs / n_nodes / n_elems");
  const int64_t B = n_envs, BN = B * N, BE = B * E;
  const auto f32 = at::kFloat, f64 = at::kDouble, i32 = at::kInt, u8 = at::kByte;
  a = truss_step_args_t{};
  a.struct_size = sizeof(truss_step_args_t);
  a.n_envs = (int32_t)B;
  a.flags = (uint32_t)flags;
  a.x = ptr<const float>(b, x, f32, "x", BN);
  a.y_in = ptr<const float>(b, y_in, f32, "y_in", BN);
  a.sec_in = ptr<const int32_t>(b, sec_in, i32, "sec_in", BE);
  a.max_up_in = ptr<const float>(b, max_up_in, f32, "max_up_in", BN);
  a.max_down_in = ptr<const float>(b, max_down_in, f32, "max_down_in", BN);
  a.a_geo = ptr<float>(b, a_geo, f32, "a_geo", sets * BN * 2);
  a.a_topo = ptr<float>(b, a_topo, f32, "a_topo", sets * BN * 3);
  a.coin = ptr<const uint8_t>(b, coin, u8, "coin", B);
  a.target = ptr<const float>(b, target, f32, "target", BN);
  a.env_params = ptr<const double>(b, env_params, f64, "env_params", B * TRUSS_NPARAM);
  a.y_out = ptr<float>(b, y_out, f32, "y_out", BN);
  a.sec_out = ptr<int32_t>(b, sec_out, i32, "sec_out", BE);
  a.max_up_out = ptr<float>(b, max_up_out, f32, "max_up_out", BN);
  a.max_down_out = ptr<float>(b, max_down_out, f32, "max_down_out", BN);
  a.disp = ptr<float>(b, disp, f32, "disp", BN * 2);
  a.q0 = ptr<float>(b, q0, f32, "q0", BE);
  a.sr = ptr<float>(b, sr, f32, "sr", BE);
  a.comp = ptr<uint8_t>(b, comp, u8, "comp", BE);
  a.point = ptr<float>(b, point, f32, "point", B * 4);
  a.obj = ptr<float>(b, obj, f32, "obj", B * 2);
  a.disp_f64 = ptr<double>(b, disp_f64, f64, "disp_f64", BN * 2);
  a.q0_f64 = ptr<double>(b, q0_f64, f64, "q0_f64", BE);
  a.energy = ptr<double>(b, energy, f64, "energy", B);
  a.reactions = ptr<double>(b, reactions, f64, "reactions", B);
  a.status = ptr<int32_t>(b, status, i32, "status", B);
  a.x_n = ptr<float>(b, x_n, f32, "x_n", BN * 13);
  const int64_t BA = B * adj_floats(b, topo, N, (flags & TRUSS_F_OBS_COMPACT) != 0);
  a.A_s = ptr<float>(b, A_s, f32, "A_s", BA);
  a.A_n_ts = ptr<float>(b, A_n_ts, f32, "A_n_ts", BA);
  a.A_n_cs = ptr<float>(b, A_n_cs, f32, "A_n_cs", BA);
  a.nN_x_n = ptr<float>(b, nN_x_n, f32, "nN_x_n", BN * 12);
  a.nN_x_e = ptr<float>(b, nN_x_e, f32, "nN_x_e", BE * 21);
}

// One Game_research04._game_modify per env (truss2D_ENV.py:370-525) == truss_step
void step(int64_t lib, int64_t topo, int64_t stream, int64_t flags, int64_t n_envs, int64_t n_nodes, int64_t n_elems,
          STEP_TENSOR_PARAMS) {
  const Backend &b = backend(lib);
  truss_step_args_t a;
  fill_step(b, topo, a, flags, n_envs, n_nodes, n_elems, 1, STEP_TENSOR_ARGS);
  check_rc(b, b.step((const truss_topo_t *)topo, &a, (void *)stream), "truss_step");
}
// n_steps chained transitions (truss_rollout); a_geo / a_topo hold n_action_sets action sets
void rollout(int64_t lib, int64_t topo, int64_t stream, int64_t flags, int64_t n_envs, int64_t n_nodes, int64_t n_elems,
             int64_t n_steps, int64_t n_action_sets, STEP_TENSOR_PARAMS) {
  const Backend &b = backend(lib);
  truss_step_args_t a;
  fill_step(b, topo, a, flags, n_envs, n_nodes, n_elems, n_action_sets, STEP_TENSOR_ARGS);
  check_rc(b, b.rollout((const truss_topo_t *)topo, &a, (int32_t)n_steps, (int32_t)n_action_sets, (void *)stream), "truss_rollout");
}

// state_data + state_data_not_norm (truss2D_ENV.py:40-193) == truss_obs
void obs_flags(int64_t lib, int64_t topo, int64_t stream, int64_t flags, int64_t n_envs, int64_t N, int64_t E, const at::Tensor &x, const at::Tensor &y,
         const at::Tensor &sec, const at::Tensor &max_up, const at::Tensor &max_down, const at::Tensor &target, const at::Tensor &disp,
         const at::Tensor &q0, const at::Tensor &sr, const at::Tensor &comp, const at::Tensor &env_params, const OT &x_n, const OT &A_s,
         const OT &A_n_ts, const OT &A_n_cs, const OT &nN_x_n, const OT &nN_x_e) {
  const Backend &b = backend(lib);
  TORCH_CHECK(n_envs >= 1, "truss_mi355: n_envs < 1");
  const int64_t B = n_envs, BN = B * N, BE = B * E;
  const auto f32 = at::kFloat;
  truss_obs_args_t a{};
  a.struct_size = sizeof(truss_obs_args_t);
  a.n_envs = (int32_t)B;
  a.flags = (uint32_t)flags;
  a.x = ptr<const float>(b, x, f32, "x", BN);
  a.y = ptr<const float>(b, y, f32, "y", BN);
  a.sec = ptr<const int32_t>(b, sec, at::kInt, "sec", BE);
  a.max_up = ptr<const float>(b, max_up, f32, "max_up", BN);
  a.max_down = ptr<const float>(b, max_down, f32, "max_down", BN);
  a.target = ptr<const float>(b, target, f32, "target", BN);
  a.disp = ptr<const float>(b, disp, f32, "disp", BN * 2);
  a.q0 = ptr<const float>(b, q0, f32, "q0", BE);
  a.sr = ptr<const float>(b, sr, f32, "sr", BE);
  a.comp = ptr<const uint8_t>(b, comp, at::kByte, "comp", BE);
  a.env_params = ptr<const double>(b, env_params, at::kDouble, "env_params", B * TRUSS_NPARAM);
  a.x_n = ptr<float>(b, x_n, f32, "x_n", BN * 13);
  const int64_t BA = B * adj_floats(b, topo, N, (flags & TRUSS_OBS_F_COMPACT) != 0);
  a.A_s = ptr<float>(b, A_s, f32, "A_s", BA);
  a.A_n_ts = ptr<float>(b, A_n_ts, f32, "A_n_ts", BA);
  a.A_n_cs = ptr<float>(b, A_n_cs, f32, "A_n_cs", BA);
  a.nN_x_n = ptr<float>(b, nN_x_n, f32, "nN_x_n", BN * 12);
  a.nN_x_e = ptr<float>(b, nN_x_e, f32, "nN_x_e", BE * 21);
  check_rc(b, b.obs((const truss_topo_t *)topo, &a, (void *)stream), "truss_obs");
}
// the same with flags = 0: the dense layout
void obs(int64_t lib, int64_t topo, int64_t stream, int64_t n_envs, int64_t N, int64_t E, const at::Tensor &x, const at::Tensor &y,
         const at::Tensor &sec, const at::Tensor &max_up, const at::Tensor &max_down, const at::Tensor &target, const at::Tensor &disp,
         const at::Tensor &q0, const at::Tensor &sr, const at::Tensor &comp, const at::Tensor &env_params, const OT &x_n, const OT &A_s,
         const OT &A_n_ts, const OT &A_n_cs, const OT &nN_x_n, const OT &nN_x_e) {
  obs_flags(lib, topo, stream, 0, n_envs, N, E, x, y, sec, max_up, max_down, target, disp, q0, sr, comp, env_params, x_n, A_s, A_n_ts, A_n_cs,
            nN_x_n, nN_x_e);
}

// Pareto cull + 2-D hypervolume of B small point sets (utils.py:11-342) == truss_front
void front(int64_t lib, int64_t stream, int64_t max_front, int64_t flags, const at::Tensor &points, const at::Tensor &n_points,
           const OT &ref_points, const OT &front_idx, const OT &n_front, const OT &hv_front, const OT &hv_all, const OT &metrics) {
  const Backend &b = backend(lib);
  TORCH_CHECK(points.dim() == 3 && points.size(2) == 4, "truss_mi355: points must be [B, P, 4]");
  const int64_t B = points.size(0), P = points.size(1);
  truss_front_args_t a{};
  a.struct_size = sizeof(truss_front_args_t);
  a.n_envs = (int32_t)B;
  a.max_points = (int32_t)P;
  a.max_front = (int32_t)max_front;
  a.flags = (uint32_t)flags;
  a.points = ptr<const double>(b, points, at::kDouble, "points");
  a.n_points = ptr<const int32_t>(b, n_points, at::kInt, "n_points", B);
  a.ref_points = ptr<const double>(b, ref_points, at::kDouble, "ref_points", B * 2);
  a.front_idx = ptr<int32_t>(b, front_idx, at::kInt, "front_idx", B * P);
  a.n_front = ptr<int32_t>(b, n_front, at::kInt, "n_front", B);
  a.hv_front = ptr<double>(b, hv_front, at::kDouble, "hv_front", B);
  a.hv_all = ptr<double>(b, hv_all, at::kDouble, "hv_all", B);
  a.metrics = ptr<double>(b, metrics, at::kDouble, "metrics", B * 5);
  if (B == 0) return;
  check_rc(b, b.front(&a, (void *)stream), "truss_front");
}

// ---- what the GCN operators share ----
void check_adj(const at::Tensor &adj, int64_t B, int64_t N) {
  TORCH_CHECK((adj.dim() == 2 || adj.dim() == 3) && adj.size(-1) == N && adj.size(-2) == N && (adj.dim() == 2 || adj.size(0) == B),
              "truss_mi355: adj must be [N, N] or [B, N, N]");
}
// the argument block of one layer: sizes, activation, x (absent in the backward), the adjacency with its optional sparsity
// pattern, the weights; bias / out and the rest are the caller's
// adj_layout 1: adj holds the compact rows [N, Kc] / [B, N, Kc] of its table nbr [N, Kc]; any other value passes with the dense shapes
// and the library judges it
truss_gcn_layer_args_t layer_args(const Backend &b, int64_t B, int64_t N, int64_t K, int64_t C, int64_t act, const at::Tensor *x,
                                  const at::Tensor &adj, const OT &nbr, const at::Tensor &w, int64_t adj_layout = 0) {
  const bool compact = adj_layout == TRUSS_GCN_ADJ_COMPACT;
  if (compact) {
    TORCH_CHECK(present(nbr) && nbr->dim() == 2, "truss_mi355: a compact adj needs its table nbr [N, Kc]");
    TORCH_CHECK((adj.dim() == 2 || adj.dim() == 3) && adj.size(-1) == nbr->size(1) && adj.size(-2) == N && (adj.dim() == 2 || adj.size(0) == B),
                "truss_mi355: a compact adj must be [N, Kc] or [B, N, Kc] with nbr [N, Kc]");
  } else {
    check_adj(adj, B, N);
  }
  TORCH_CHECK(adj_layout >= INT32_MIN && adj_layout <= INT32_MAX, "truss_mi355: adj_layout out of range");
  truss_gcn_layer_args_t a{};
  a.adj_layout = (int32_t)adj_layout;
  a.struct_size = sizeof a;
  a.n_batch = (int32_t)B;
  a.n_nodes = (int32_t)N;
  a.k_in = (int32_t)K;
  a.c_out = (int32_t)C;
  a.act = (int32_t)act;
  if (x) a.x = ptr<const float>(b, *x, at::kFloat, "x");
  a.adj = ptr<const float>(b, adj, at::kFloat, "adj");
  a.a_batch_stride = adj.dim() == 3 ? N * adj.size(-1) : 0;
  if (present(nbr)) {
    TORCH_CHECK(nbr->dim() == 2 && nbr->size(0) == N, "truss_mi355: nbr must be [N, K]");
    a.nbr = ptr<const int16_t>(b, *nbr, at::kShort, "nbr");
    a.k_nbr = (int32_t)nbr->size(1);
  }
  a.w = ptr<const float>(b, w, at::kFloat, "w");
  return a;
}
// the same for a forward layer of operator `op`, from its tensors: shapes checked, bias and out filled in
truss_gcn_layer_args_t forward_args(const Backend &b, const char *op, const at::Tensor &x, const at::Tensor &adj, const OT &nbr,
                                    const at::Tensor &w, const OT &bias, const at::Tensor &out, int64_t act, int64_t adj_layout = 0) {
  TORCH_CHECK(x.dim() == 3 && out.dim() == 3 && w.dim() == 2, "truss_mi355: x [B, N, K], w [C, K], out [B, N, C]");
  const int64_t B = x.size(0), N = x.size(1), K = x.size(2), C = w.size(0);
  TORCH_CHECK(w.size(1) == K && out.size(0) == B && out.size(1) == N && out.size(2) == C, "truss_mi355: ", op, " shapes do not match");
  truss_gcn_layer_args_t a = layer_args(b, B, N, K, C, act, &x, adj, nbr, w, adj_layout);
  a.bias = ptr<const float>(b, bias, at::kFloat, "bias", C);
  a.out = ptr<float>(b, out, at::kFloat, "out");
  return a;
}

// act(A @ H + bias) of a GCN layer for B small graphs (truss2D_RL.py:49-120, inference) == truss_gcn_aggregate
void gcn_aggregate(int64_t lib, int64_t stream, const at::Tensor &adj, const at::Tensor &h, const OT &bias, const at::Tensor &out,
                   int64_t act) {
  const Backend &b = backend(lib);
  TORCH_CHECK(h.dim() == 3 && out.sizes() == h.sizes(), "truss_mi355: h / out must be [B, N, C] of equal shape");
  const int64_t B = h.size(0), N = h.size(1), C = h.size(2);
  check_adj(adj, B, N);
  const float *pa = ptr<const float>(b, adj, at::kFloat, "adj");
  const float *ph = ptr<const float>(b, h, at::kFloat, "h");
  const float *pb = ptr<const float>(b, bias, at::kFloat, "bias", C);
  float *po = ptr<float>(b, out, at::kFloat, "out");
  check_rc(b, b.gcn_aggregate(pa, adj.dim() == 3 ? N * N : 0, ph, pb, po, (int32_t)B, (int32_t)N, (int32_t)C, (int32_t)act, (void *)stream),
           "truss_gcn_aggregate");
}

// the same over a fixed sparsity pattern (nbr [N, K] int16: the columns that may be non-zero in row i) == truss_gcn_aggregate_sparse
void gcn_aggregate_sparse(int64_t lib, int64_t stream, const at::Tensor &adj, const at::Tensor &nbr, const at::Tensor &h, const OT &bias,
                          const at::Tensor &out, int64_t act) {
  const Backend &b = backend(lib);
  TORCH_CHECK(h.dim() == 3 && out.sizes() == h.sizes(), "truss_mi355: h / out must be [B, N, C] of equal shape");
  const int64_t B = h.size(0), N = h.size(1), C = h.size(2);
  check_adj(adj, B, N);
  TORCH_CHECK(nbr.dim() == 2 && nbr.size(0) == N, "truss_mi355: nbr must be [N, K]");
  const float *pa = ptr<const float>(b, adj, at::kFloat, "adj");
  const int16_t *pn = ptr<const int16_t>(b, nbr, at::kShort, "nbr");
  const float *ph = ptr<const float>(b, h, at::kFloat, "h");
  const float *pb = ptr<const float>(b, bias, at::kFloat, "bias", C);
  float *po = ptr<float>(b, out, at::kFloat, "out");
  check_rc(b, b.gcn_aggregate_sparse(pa, adj.dim() == 3 ? N * N : 0, pn, (int32_t)nbr.size(1), ph, pb, po, (int32_t)B, (int32_t)N, (int32_t)C,
                           (int32_t)act, (void *)stream),
           "truss_gcn_aggregate_sparse");
}

// one whole GCN layer, out = act(adj @ (x @ w^T) + bias) [+ out], on the matrix cores == truss_gcn_layer
void gcn_layer(int64_t lib, int64_t stream, const at::Tensor &x, const at::Tensor &adj, const OT &nbr, const at::Tensor &w, const OT &bias,
               const at::Tensor &out, int64_t act, bool accumulate, const OT &w_split, int64_t adj_layout) {
  const Backend &b = backend(lib);
  truss_gcn_layer_args_t a = forward_args(b, "gcn_layer", x, adj, nbr, w, bias, out, act, adj_layout);
  a.accumulate = accumulate ? 1 : 0;
  a.w_bf16x3 = (const uint16_t *)ptr<const int16_t>(b, w_split, at::kShort, "w_split", 3 * 224 * ((a.k_in + 15) / 16 * 16));
  check_rc(b, b.gcn_layer(&a, (void *)stream), "truss_gcn_layer");
}

// the same layer with a consumer of its output V in the epilogue of the launch: kind 1 (head) out2 = act2(adj2 @ (V @ w2^T) + bias2),
// kind 2 (pool) pool = V.sum(dim=1); out (V itself) is optional == truss_gcn_layer_fused
// (the argument blocks of the two operators that take an epilogue)
void fused_args(const Backend &b, truss_gcn_layer_args_t &a, truss_gcn_epilogue_t &e, const at::Tensor &x, const at::Tensor &adj, const OT &nbr,
                const at::Tensor &w, const OT &bias, const OT &out, int64_t act, const OT &w_split, int64_t kind, const OT &w2, const OT &bias2,
                const OT &adj2, const OT &nbr2, int64_t act2, const OT &out2, const OT &pool, int64_t adj_layout) {
  TORCH_CHECK(x.dim() == 3 && w.dim() == 2 && w.size(1) == x.size(2), "truss_mi355: gcn_layer_fused: x [B, N, K], w [C, K]");
  const int64_t B = x.size(0), N = x.size(1), K = x.size(2), C = w.size(0);
  a = layer_args(b, B, N, K, C, act, &x, adj, nbr, w, adj_layout);
  a.bias = ptr<const float>(b, bias, at::kFloat, "bias", C);
  TORCH_CHECK(!present(out) || (out->dim() == 3 && out->size(0) == B && out->size(1) == N && out->size(2) == C),
              "truss_mi355: gcn_layer_fused: out must be [B, N, C]");
  a.out = ptr<float>(b, out, at::kFloat, "out");
  a.w_bf16x3 = (const uint16_t *)ptr<const int16_t>(b, w_split, at::kShort, "w_split", 3 * 224 * ((K + 15) / 16 * 16));
  e = truss_gcn_epilogue_t{};
  e.struct_size = sizeof e;
  e.kind = (int32_t)kind;
  e.act2 = (int32_t)act2;
  if (present(w2)) {
    TORCH_CHECK(w2->dim() == 2 && w2->size(1) == C, "truss_mi355: gcn_layer_fused: w2 must be [c2, C]");
    e.w2 = ptr<const float>(b, *w2, at::kFloat, "w2");
    e.c2 = (int32_t)w2->size(0);
  }
  e.bias2 = ptr<const float>(b, bias2, at::kFloat, "bias2", e.c2);
  if (present(adj2)) {
    check_adj(*adj2, B, N);
    e.adj2 = ptr<const float>(b, *adj2, at::kFloat, "adj2");
    e.a2_batch_stride = adj2->dim() == 3 ? N * N : 0;
  }
  if (present(nbr2)) {
    TORCH_CHECK(nbr2->dim() == 2 && nbr2->size(0) == N, "truss_mi355: nbr2 must be [N, K]");
    e.nbr2 = ptr<const int16_t>(b, *nbr2, at::kShort, "nbr2");
    e.k_nbr2 = (int32_t)nbr2->size(1);
  }
  TORCH_CHECK(!present(out2) || (out2->dim() == 3 && out2->size(0) == B && out2->size(1) == N && out2->size(2) == e.c2),
              "truss_mi355: gcn_layer_fused: out2 must be [B, N, c2]");
  e.out2 = ptr<float>(b, out2, at::kFloat, "out2");
  TORCH_CHECK(!present(pool) || (pool->dim() == 2 && pool->size(0) == B && pool->size(1) == C), "truss_mi355: gcn_layer_fused: pool must be [B, C]");
  e.pool = ptr<float>(b, pool, at::kFloat, "pool");
}
void gcn_layer_fused(int64_t lib, int64_t stream, const at::Tensor &x, const at::Tensor &adj, const OT &nbr, const at::Tensor &w, const OT &bias,
                     const OT &out, int64_t act, const OT &w_split, int64_t kind, const OT &w2, const OT &bias2, const OT &adj2, const OT &nbr2,
                     int64_t act2, const OT &out2, const OT &pool, int64_t adj_layout) {
  const Backend &b = backend(lib);
  need(b.gcn_layer_fused, "truss_gcn_layer_fused");
  truss_gcn_layer_args_t a;
  truss_gcn_epilogue_t e;
  fused_args(b, a, e, x, adj, nbr, w, bias, out, act, w_split, kind, w2, bias2, adj2, nbr2, act2, out2, pool, adj_layout);
  check_rc(b, b.gcn_layer_fused(&a, &e, (void *)stream), "truss_gcn_layer_fused");
}

// the split-weight layer on the first `terms` bf16 terms of both operands (3: bf16x3, 2: bf16x2, 1: bf16); kind 0: the plain layer
// (out required, accumulate allowed), kind 1 / 2: with the epilogue of gcn_layer_fused == truss_gcn_layer_terms
void gcn_layer_terms(int64_t lib, int64_t stream, const at::Tensor &x, const at::Tensor &adj, const OT &nbr, const at::Tensor &w, const OT &bias,
                     const OT &out, int64_t act, const OT &w_split, int64_t kind, const OT &w2, const OT &bias2, const OT &adj2, const OT &nbr2,
                     int64_t act2, const OT &out2, const OT &pool, bool accumulate, int64_t terms, int64_t adj_layout) {
  const Backend &b = backend(lib);
  need(b.gcn_layer_terms, "truss_gcn_layer_terms");
  truss_gcn_layer_args_t a;
  truss_gcn_epilogue_t e;
  fused_args(b, a, e, x, adj, nbr, w, bias, out, act, w_split, kind, w2, bias2, adj2, nbr2, act2, out2, pool, adj_layout);
  TORCH_CHECK(kind != 0 || present(out), "truss_mi355: gcn_layer_terms: out must be [B, N, C] for a plain layer (kind 0)");
  a.accumulate = accumulate ? 1 : 0;
  TORCH_CHECK(terms >= INT32_MIN && terms <= INT32_MAX, "truss_mi355: gcn_layer_terms: terms out of range");
  check_rc(b, b.gcn_layer_terms(&a, kind == 0 ? nullptr : &e, (int32_t)terms, (void *)stream), "truss_gcn_layer_terms");
}

// several split-weight layers in one launch: the lists hold one entry per layer, chain-major ([n_chains][steps_per_chain]); layer i
// is what gcn_layer_terms takes.  kind 0: plain layers (out required, the epilogue lists empty); kind 1 / 2: one step per chain, each
// with the epilogue of gcn_layer_fused (out optional) == truss_gcn_layer_group
void gcn_layer_group(int64_t lib, int64_t stream, at::TensorList x, at::TensorList adj, const c10::List<OT> &nbr, at::TensorList w,
                     const c10::List<OT> &bias, const c10::List<OT> &out, at::IntArrayRef act, const c10::List<bool> &accumulate,
                     at::TensorList w_split, int64_t steps_per_chain, int64_t kind, const c10::List<OT> &w2, const c10::List<OT> &bias2,
                     const c10::List<OT> &adj2, const c10::List<OT> &nbr2, at::IntArrayRef act2, const c10::List<OT> &out2,
                     const c10::List<OT> &pool, int64_t terms, at::IntArrayRef adj_layout) {
  const Backend &b = backend(lib);
  need(b.gcn_layer_group, "truss_gcn_layer_group");
  const size_t L = x.size();
  auto per_layer = [L](const c10::List<OT> &l) { return l.empty() || l.size() == L; };
  TORCH_CHECK(adj.size() == L && w.size() == L && act.size() == L && accumulate.size() == L && w_split.size() == L && per_layer(nbr) &&
                  per_layer(bias) && out.size() == L,
              "truss_mi355: gcn_layer_group takes one entry per layer in every list");
  TORCH_CHECK(adj_layout.empty() || adj_layout.size() == L, "truss_mi355: gcn_layer_group: adj_layout is empty (dense) or holds one entry per layer");
  TORCH_CHECK(kind != 0 ? (per_layer(w2) && per_layer(bias2) && per_layer(adj2) && per_layer(nbr2) && act2.size() == L && per_layer(out2) &&
                           per_layer(pool))
                        : (w2.empty() && bias2.empty() && adj2.empty() && nbr2.empty() && act2.empty() && out2.empty() && pool.empty()),
              "truss_mi355: gcn_layer_group: the epilogue lists hold one entry per layer, or are empty without an epilogue (kind 0)");
  TORCH_CHECK(steps_per_chain >= INT32_MIN && steps_per_chain <= INT32_MAX && terms >= INT32_MIN && terms <= INT32_MAX && L <= INT32_MAX,
              "truss_mi355: gcn_layer_group: steps_per_chain / terms out of range");
  TORCH_CHECK(steps_per_chain < 1 || L % (size_t)steps_per_chain == 0, "truss_mi355: gcn_layer_group: ", L, " layers are not whole chains of ",
              steps_per_chain);
  std::vector<truss_gcn_layer_args_t> args(L);
  std::vector<truss_gcn_epilogue_t> epi(L);
  for (size_t i = 0; i < L; ++i) {
    fused_args(b, args[i], epi[i], x[i], adj[i], at_or_none(nbr, i), w[i], at_or_none(bias, i), out.get(i), act[i], OT(w_split[i]), kind,
               at_or_none(w2, i), at_or_none(bias2, i), at_or_none(adj2, i), at_or_none(nbr2, i), kind != 0 ? act2[i] : 0, at_or_none(out2, i),
               at_or_none(pool, i), adj_layout.empty() ? 0 : adj_layout[i]);
    TORCH_CHECK(kind != 0 || present(out.get(i)), "truss_mi355: gcn_layer_group: out must be [B, N, C] for a plain layer (kind 0)");
    args[i].accumulate = accumulate.get(i) ? 1 : 0;
  }
  const int32_t chains = steps_per_chain >= 1 ? (int32_t)(L / (size_t)steps_per_chain) : (int32_t)L;
  check_rc(b, b.gcn_layer_group(args.data(), kind == 0 ? nullptr : epi.data(), chains, (int32_t)steps_per_chain, (int32_t)terms, (void *)stream),
           "truss_gcn_layer_group");
}

// a whole level of GCN layers in one launch: out[i] = act[i](adj[i] @ (x[i] @ w[i]^T) + bias[i]); x_agg (empty, or one tensor per
// layer) receives adj[i] @ x[i] == truss_gcn_level
void gcn_level(int64_t lib, int64_t stream, at::TensorList x, at::TensorList adj, const c10::List<OT> &nbr, at::TensorList w, at::TensorList bias,
               at::TensorList out, at::TensorList x_agg, at::IntArrayRef act) {
  const Backend &b = backend(lib);
  const size_t L = x.size();
  TORCH_CHECK(adj.size() == L && w.size() == L && bias.size() == L && out.size() == L && act.size() == L && (x_agg.empty() || x_agg.size() == L) &&
                  (nbr.empty() || nbr.size() == L),
              "truss_mi355: gcn_level takes one entry per layer in every list");
  std::vector<truss_gcn_layer_args_t> args(L);
  std::vector<float *> xa(L, nullptr);
  for (size_t i = 0; i < L; ++i) {
    args[i] = forward_args(b, "gcn_level", x[i], adj[i], at_or_none(nbr, i), w[i], bias[i], out[i], act[i]);
    if (!x_agg.empty()) {
      TORCH_CHECK(x_agg[i].numel() == x[i].numel(), "truss_mi355: x_agg[i] must hold B * N * K elements");
      xa[i] = ptr<float>(b, x_agg[i], at::kFloat, "x_agg");
    }
  }
  check_rc(b, b.gcn_level(args.data(), (int32_t)L, x_agg.empty() ? nullptr : xa.data(), (void *)stream), "truss_gcn_level");
}

// the backward of such a level in one launch: d_b[i] = sum_rows dZ, d_w[i] = dZ^T x_agg[i], d_x[i] = adj[i]^T (dZ w[i]) with
// dZ = d_out[i] * act[i]'(out[i]); the lists of optional tensors are empty or hold one entry per layer (None: not wanted)
// == truss_gcn_level_backward
void gcn_level_backward(int64_t lib, int64_t stream, at::TensorList adj, at::TensorList w, at::IntArrayRef act, at::TensorList d_out,
                        at::TensorList out, const c10::List<OT> &x_agg, const c10::List<OT> &d_w, const c10::List<OT> &d_b,
                        const c10::List<OT> &d_x) {
  const Backend &b = backend(lib);
  need(b.gcn_level_backward, "truss_gcn_level_backward");
  const size_t L = d_out.size();
  auto per_layer = [L](const c10::List<OT> &l) { return l.empty() || l.size() == L; };
  TORCH_CHECK(adj.size() == L && w.size() == L && act.size() == L && out.size() == L && per_layer(x_agg) && per_layer(d_w) && per_layer(d_b) &&
                  per_layer(d_x),
              "truss_mi355: gcn_level_backward takes one entry per layer in every list");
  std::vector<truss_gcn_layer_args_t> args(L);
  std::vector<truss_gcn_level_bwd_t> bw(L);
  for (size_t i = 0; i < L; ++i) {
    TORCH_CHECK(d_out[i].dim() == 3 && w[i].dim() == 2 && out[i].sizes() == d_out[i].sizes(),
                "truss_mi355: d_out / out [B, N, C] of equal shape, w [C, K]");
    const int64_t B = d_out[i].size(0), N = d_out[i].size(1), C = d_out[i].size(2), K = w[i].size(1);
    TORCH_CHECK(w[i].size(0) == C, "truss_mi355: gcn_level_backward shapes do not match");
    args[i] = layer_args(b, B, N, K, C, act[i], nullptr, adj[i], OT(), w[i]);
    truss_gcn_level_bwd_t &g = bw[i];
    g.d_out = ptr<const float>(b, d_out[i], at::kFloat, "d_out");
    g.out = ptr<const float>(b, out[i], at::kFloat, "out");
    g.x_agg = ptr<const float>(b, at_or_none(x_agg, i), at::kFloat, "x_agg", B * N * K);
    const OT dw = at_or_none(d_w, i), db = at_or_none(d_b, i), dx = at_or_none(d_x, i);
    TORCH_CHECK(!present(dw) || dw->numel() == C * K, "truss_mi355: d_w[i] must hold C * K elements");
    TORCH_CHECK(!present(db) || db->numel() == C, "truss_mi355: d_b[i] must hold C elements");
    TORCH_CHECK(!present(dx) || dx->numel() == B * N * K, "truss_mi355: d_x[i] must hold B * N * K elements");
    g.d_w = ptr<float>(b, dw, at::kFloat, "d_w");
    g.d_b = ptr<float>(b, db, at::kFloat, "d_b");
    g.d_x = ptr<float>(b, dx, at::kFloat, "d_x");
  }
  check_rc(b, b.gcn_level_backward(args.data(), (int32_t)L, bw.data(), (void *)stream), "truss_gcn_level_backward");
}

// the neighbour sums of a level through the node table, every item one slice of one launch: y[i] = adj[i] x[i], or adj[i]^T x[i]
// with transpose[i], over the entries of nbr[i] [N, Kn] only; x[i] / y[i] [B, N, n_ch] (or [B N, n_ch]) contiguous, adj[i] [N, N]
// (one for the batch) or [B, N, N] == truss_gcn_level_aggregate
void gcn_level_aggregate(int64_t lib, int64_t stream, at::TensorList x, at::TensorList adj, at::TensorList nbr, at::TensorList y,
                         const c10::List<bool> &transpose) {
  const Backend &b = backend(lib);
  need(b.gcn_level_aggregate, "truss_gcn_level_aggregate");
  const size_t L = x.size();
  TORCH_CHECK(adj.size() == L && nbr.size() == L && y.size() == L && transpose.size() == L,
              "truss_mi355: gcn_level_aggregate takes one entry per item in every list");
  std::vector<truss_gcn_agg_t> items(L);
  for (size_t i = 0; i < L; ++i) {
    TORCH_CHECK(nbr[i].dim() == 2 && (x[i].dim() == 2 || x[i].dim() == 3) && x[i].sizes() == y[i].sizes(),
                "truss_mi355: gcn_level_aggregate: x / y [B, N, n_ch] of equal shape, nbr [N, Kn]");
    const int64_t N = nbr[i].size(0), C = x[i].size(-1), rows = x[i].numel() / (C > 0 ? C : 1);
    TORCH_CHECK(N >= 1 && C >= 1 && rows % N == 0 && (x[i].dim() == 2 || x[i].size(1) == N), "truss_mi355: gcn_level_aggregate: rows of x are not whole graphs of nbr's N nodes");
    const int64_t B = rows / N;
    TORCH_CHECK(B <= INT32_MAX && N <= INT32_MAX && C <= INT32_MAX && nbr[i].size(1) <= INT32_MAX, "truss_mi355: gcn_level_aggregate: sizes beyond int32");
    const bool shared = adj[i].dim() == 2;
    TORCH_CHECK((shared || adj[i].dim() == 3) && adj[i].size(-1) == N && adj[i].size(-2) == N && (shared || adj[i].size(0) == B),
                "truss_mi355: gcn_level_aggregate: adj must be [N, N] or [B, N, N]");
    truss_gcn_agg_t &a = items[i];
    a = truss_gcn_agg_t{};
    a.struct_size = sizeof(truss_gcn_agg_t);
    a.x = ptr<const float>(b, x[i], at::kFloat, "x");
    a.adj = ptr<const float>(b, adj[i], at::kFloat, "adj");
    a.a_batch_stride = shared ? 0 : N * N;
    a.nbr = ptr<const int16_t>(b, nbr[i], at::kShort, "nbr");
    a.y = ptr<float>(b, y[i], at::kFloat, "y");
    a.n_batch = (int32_t)B, a.n_nodes = (int32_t)N, a.n_ch = (int32_t)C, a.k_nbr = (int32_t)nbr[i].size(1);
    a.transpose = transpose.get(i) ? 1 : 0;
  }
  check_rc(b, b.gcn_level_aggregate(items.data(), (int32_t)L, (void *)stream), "truss_gcn_level_aggregate");
}

// one optimiser step over the list `params` (each contiguous float32, updated in place): the gradient of params[i] is the slice of
// the flat vector `grad` behind those of params[< i] -- the offsets are the running sum of the sizes -- clipped to L2 norm <= 1 on
// its own; then Adam on the flat moments exp_avg / exp_avg_sq at step number *step (a float64 tensor the caller has already
// incremented), or, with mode 1, the first step of a fresh Adam (no moments, no step).  partials: float64 scratch of one element
// per chunk of TRUSS_OPTIM_CHUNK elements of every tensor; clipped (flat like grad) / norms ([len(params)]): optional outputs
// == truss_optim_step
void optim_step(int64_t lib, int64_t stream, int64_t mode, at::TensorList params, const at::Tensor &grad, const OT &exp_avg,
                const OT &exp_avg_sq, const OT &step, double lr, double beta1, double beta2, double eps, const at::Tensor &partials,
                const OT &clipped, const OT &norms) {
  const Backend &b = backend(lib);
  need(b.optim_step, "truss_optim_step");
  const size_t L = params.size();
  TORCH_CHECK(L <= (size_t)INT32_MAX, "truss_mi355: optim_step: too many tensors");
  std::vector<truss_optim_tensor_t> ts(L);
  int64_t total = 0, chunks = 0;
  for (size_t i = 0; i < L; ++i) {
    ts[i].p = ptr<float>(b, params[i], at::kFloat, "params[i]", 1);
    ts[i].offset = total;
    ts[i].numel = params[i].numel();
    total += ts[i].numel;
    chunks += (ts[i].numel + TRUSS_OPTIM_CHUNK - 1) / TRUSS_OPTIM_CHUNK;
  }
  TORCH_CHECK(grad.numel() == total, "truss_mi355: optim_step: grad has ", grad.numel(), " elements, the parameters ", total);
  TORCH_CHECK(!present(exp_avg) || exp_avg->numel() == total, "truss_mi355: optim_step: exp_avg must hold ", total, " elements");
  TORCH_CHECK(!present(exp_avg_sq) || exp_avg_sq->numel() == total, "truss_mi355: optim_step: exp_avg_sq must hold ", total, " elements");
  TORCH_CHECK(!present(clipped) || clipped->numel() == total, "truss_mi355: optim_step: clipped must hold ", total, " elements");
  truss_optim_args_t a{};
  a.struct_size = sizeof(truss_optim_args_t);
  a.mode = (int32_t)mode;
  a.n_tensors = (int32_t)L;
  a.tensors = ts.data();
  a.grad = ptr<const float>(b, grad, at::kFloat, "grad");
  a.exp_avg = ptr<float>(b, exp_avg, at::kFloat, "exp_avg");
  a.exp_avg_sq = ptr<float>(b, exp_avg_sq, at::kFloat, "exp_avg_sq");
  a.step = ptr<const double>(b, step, at::kDouble, "step", 1);
  a.lr = lr, a.beta1 = beta1, a.beta2 = beta2, a.eps = eps;
  a.partials = ptr<double>(b, partials, at::kDouble, "partials", chunks);
  a.clipped = ptr<float>(b, clipped, at::kFloat, "clipped");
  a.norms = ptr<float>(b, norms, at::kFloat, "norms", (int64_t)L);
  check_rc(b, b.optim_step(&a, (void *)stream), "truss_optim_step");
}

// targets[i] (contiguous float32, updated in place) follows sources[i] (as many elements, not modified): lerp(target, source, tau)
// where *step mod period == 0 -- `step` a float64 tensor read on the device; None: always -- nothing written otherwise
// == truss_target_update
void target_update(int64_t lib, int64_t stream, at::TensorList targets, at::TensorList sources, double tau, int64_t period, const OT &step) {
  const Backend &b = backend(lib);
  need(b.target_update, "truss_target_update");
  const size_t L = targets.size();
  TORCH_CHECK(sources.size() == L, "truss_mi355: target_update: ", L, " targets, ", sources.size(), " sources");
  TORCH_CHECK(L <= (size_t)INT32_MAX, "truss_mi355: target_update: too many tensors");
  std::vector<truss_target_pair_t> ps(L);
  // `ptr` with the tensor's index in its name; the name is only built for a tensor that `ptr` will refuse
  auto at_ptr = [&](const at::Tensor &t, const char *list, size_t i) {
    if (t.scalar_type() == at::kFloat && t.is_contiguous() && (b.device ? t.is_cuda() : t.is_cpu()) && t.numel() >= 1) return (float *)t.data_ptr();
    const std::string name = std::string(list) + "[" + std::to_string(i) + "]";
    return ptr<float>(b, t, at::kFloat, name.c_str(), 1);
  };
  for (size_t i = 0; i < L; ++i) {
    ps[i].t = at_ptr(targets[i], "targets", i);
    ps[i].p = at_ptr(sources[i], "sources", i);
    ps[i].numel = targets[i].numel();
    TORCH_CHECK(sources[i].numel() == ps[i].numel, "truss_mi355: target_update: targets[", i, "] has ", ps[i].numel, " elements, sources[", i,
                "] ", sources[i].numel());
  }
  truss_target_args_t a{};
  a.struct_size = sizeof(truss_target_args_t);
  a.n_pairs = (int32_t)L;
  a.pairs = ps.data();
  a.tau = tau;
  a.period = period;
  a.step = ptr<const double>(b, step, at::kDouble, "step", 1);
  check_rc(b, b.target_update(&a, (void *)stream), "truss_target_update");
}

// the tails of several critic passes (items) in one call: item j pools its n_layers[j] level outputs o [B, N, H] -- the lists of all
// items one after the other in `o` -- over the nodes, concatenates them and applies relu(w1 . + b1) [Q, L H], relu(w2 . + b2) [Q, Q],
// w3 . + b3 [1, Q] -> q[j] [B, 1]; p / z1 / z2: empty lists, or per item None or the tensors [B, L H], [B, Q], [B, Q] the backward
// reads (all three or none) == truss_critic_tail
void critic_tail(int64_t lib, int64_t stream, at::TensorList o, at::IntArrayRef n_layers, at::TensorList w1, at::TensorList b1, at::TensorList w2,
                 at::TensorList b2, at::TensorList w3, at::TensorList b3, at::TensorList q, const c10::List<OT> &p, const c10::List<OT> &z1,
                 const c10::List<OT> &z2) {
  const Backend &b = backend(lib);
  need(b.critic_tail, "truss_critic_tail");
  const size_t J = n_layers.size();
  auto per_item = [J](const c10::List<OT> &l) { return l.empty() || l.size() == J; };
  TORCH_CHECK(w1.size() == J && b1.size() == J && w2.size() == J && b2.size() == J && w3.size() == J && b3.size() == J && q.size() == J &&
                  per_item(p) && per_item(z1) && per_item(z2) && J <= (size_t)INT32_MAX,
              "truss_mi355: critic_tail takes one entry per item in every list");
  std::vector<truss_critic_tail_args_t> items(J);
  size_t pos = 0;
  for (size_t j = 0; j < J; ++j) {
    const int64_t L = n_layers[j];
    TORCH_CHECK(L >= 1 && L <= TRUSS_CRITIC_TAIL_MAX_LAYERS && pos + (size_t)L <= o.size(), "truss_mi355: critic_tail: n_layers[j] must be 1..",
                TRUSS_CRITIC_TAIL_MAX_LAYERS, " and o must hold the layers of every item");
    const at::Tensor &o0 = o[pos];
    TORCH_CHECK(o0.dim() == 3 && w1[j].dim() == 2 && w2[j].dim() == 2, "truss_mi355: critic_tail: o [B, N, H], w1 [Q, L H], w2 [Q, Q]");
    const int64_t B = o0.size(0), N = o0.size(1), H = o0.size(2), Q = w1[j].size(0);
    TORCH_CHECK(B <= INT32_MAX && N <= INT32_MAX && H <= INT32_MAX && Q <= INT32_MAX, "truss_mi355: critic_tail: sizes beyond int32");
    TORCH_CHECK(w1[j].size(1) == L * H && w2[j].size(0) == Q && w2[j].size(1) == Q, "truss_mi355: critic_tail: w1 must be [Q, L H], w2 [Q, Q]");
    truss_critic_tail_args_t &a = items[j];
    a = truss_critic_tail_args_t{};
    a.struct_size = sizeof(truss_critic_tail_args_t);
    a.n_batch = (int32_t)B, a.n_nodes = (int32_t)N, a.n_layers = (int32_t)L, a.n_hidden = (int32_t)H, a.n_q = (int32_t)Q;
    for (int64_t i = 0; i < L; ++i) {
      TORCH_CHECK(o[pos + i].sizes() == o0.sizes(), "truss_mi355: critic_tail: the layers of an item must have one shape [B, N, H]");
      a.o[i] = ptr<const float>(b, o[pos + i], at::kFloat, "o");
    }
    pos += (size_t)L;
    a.w1 = ptr<const float>(b, w1[j], at::kFloat, "w1");
    a.b1 = ptr<const float>(b, b1[j], at::kFloat, "b1", Q);
    a.w2 = ptr<const float>(b, w2[j], at::kFloat, "w2");
    a.b2 = ptr<const float>(b, b2[j], at::kFloat, "b2", Q);
    a.w3 = ptr<const float>(b, w3[j], at::kFloat, "w3", Q);
    a.b3 = ptr<const float>(b, b3[j], at::kFloat, "b3", 1);
    TORCH_CHECK(b1[j].numel() == Q && b2[j].numel() == Q && w3[j].numel() == Q && b3[j].numel() == 1 && q[j].numel() == B,
                "truss_mi355: critic_tail: b1, b2, w3 must hold Q elements, b3 one, q B");
    a.q = ptr<float>(b, q[j], at::kFloat, "q");
    const OT pj = at_or_none(p, j), z1j = at_or_none(z1, j), z2j = at_or_none(z2, j);
    TORCH_CHECK(present(pj) == present(z1j) && present(pj) == present(z2j), "truss_mi355: critic_tail: p, z1 and z2 of an item come together");
    if (present(pj)) {
      TORCH_CHECK(pj->numel() == B * L * H && z1j->numel() == B * Q && z2j->numel() == B * Q,
                  "truss_mi355: critic_tail: p must hold B L H elements, z1 and z2 B Q");
      a.save = 1;
      a.p = ptr<float>(b, pj, at::kFloat, "p");
      a.z1 = ptr<float>(b, z1j, at::kFloat, "z1");
      a.z2 = ptr<float>(b, z2j, at::kFloat, "z2");
    }
  }
  TORCH_CHECK(pos == o.size(), "truss_mi355: critic_tail: o holds ", o.size(), " tensors, n_layers asks for ", pos);
  check_rc(b, b.critic_tail(items.data(), (int32_t)J, (void *)stream), "truss_critic_tail");
}

float *view_ptr(const Backend &b, const at::Tensor &t, const char *name);   // (below: a tensor that need not be contiguous)

// the backward of such tails: per item dq [B, 1] (of any stride over the samples) and the saved z1, z2 (p: only read for d_w1; o: empty, or
// what the forward pooled, laid out like d_o: not read, only held against the outputs) -> d_o (the layers of all items one
// after the other, None: not wanted; an empty list: none at all) and the six parameter gradients (empty lists, or per item None or
// a tensor of the parameter's size); dz1 / dz2 [B, Q]: scratch of the items with a parameter gradient == truss_critic_tail_backward
void critic_tail_backward(int64_t lib, int64_t stream, at::IntArrayRef n_layers, at::IntArrayRef n_nodes, at::TensorList dq, const c10::List<OT> &p,
                          at::TensorList z1, at::TensorList z2, at::TensorList w1, at::TensorList w2, at::TensorList w3, const c10::List<OT> &o, const c10::List<OT> &d_o,
                          const c10::List<OT> &dz1, const c10::List<OT> &dz2, const c10::List<OT> &d_w1, const c10::List<OT> &d_b1,
                          const c10::List<OT> &d_w2, const c10::List<OT> &d_b2, const c10::List<OT> &d_w3, const c10::List<OT> &d_b3) {
  const Backend &b = backend(lib);
  need(b.critic_tail_backward, "truss_critic_tail_backward");
  const size_t J = n_layers.size();
  auto per_item = [J](const c10::List<OT> &l) { return l.empty() || l.size() == J; };
  TORCH_CHECK(n_nodes.size() == J && dq.size() == J && per_item(p) && z1.size() == J && z2.size() == J && w1.size() == J && w2.size() == J &&
                  w3.size() == J && per_item(dz1) && per_item(dz2) && per_item(d_w1) && per_item(d_b1) && per_item(d_w2) && per_item(d_b2) &&
                  per_item(d_w3) && per_item(d_b3) && J <= (size_t)INT32_MAX,
              "truss_mi355: critic_tail_backward takes one entry per item in every list");
  std::vector<truss_critic_tail_bwd_t> items(J);
  size_t pos = 0;
  for (size_t j = 0; j < J; ++j) {
    const int64_t L = n_layers[j], N = n_nodes[j];
    TORCH_CHECK(L >= 1 && L <= TRUSS_CRITIC_TAIL_MAX_LAYERS && (d_o.empty() || pos + (size_t)L <= d_o.size()) &&
                    (o.empty() || pos + (size_t)L <= o.size()),
                "truss_mi355: critic_tail_backward: n_layers[j] must be 1..", TRUSS_CRITIC_TAIL_MAX_LAYERS, " and d_o empty or one entry per layer");
    TORCH_CHECK(z1[j].dim() == 2 && w1[j].dim() == 2 && w2[j].dim() == 2, "truss_mi355: critic_tail_backward: z1 [B, Q], w1 [Q, L H], w2 [Q, Q]");
    const int64_t B = z1[j].size(0), Q = z1[j].size(1), K1 = w1[j].size(1), H = K1 / L;
    TORCH_CHECK(B <= INT32_MAX && N >= 1 && N <= INT32_MAX && K1 <= INT32_MAX && Q <= INT32_MAX, "truss_mi355: critic_tail_backward: sizes beyond int32");
    TORCH_CHECK(H * L == K1 && w1[j].size(0) == Q && w2[j].size(0) == Q && w2[j].size(1) == Q && w3[j].numel() == Q && dq[j].numel() == B &&
                    z2[j].numel() == B * Q,
                "truss_mi355: critic_tail_backward: dq [B], z1 / z2 [B, Q], w1 [Q, L H], w2 [Q, Q], w3 [Q]");
    truss_critic_tail_bwd_t &a = items[j];
    a = truss_critic_tail_bwd_t{};
    a.struct_size = sizeof(truss_critic_tail_bwd_t);
    a.n_batch = (int32_t)B, a.n_nodes = (int32_t)N, a.n_layers = (int32_t)L, a.n_hidden = (int32_t)H, a.n_q = (int32_t)Q;
    TORCH_CHECK((dq[j].dim() == 1 || (dq[j].dim() == 2 && dq[j].size(1) == 1)) && (B <= 1 || (dq[j].stride(0) >= 0 && dq[j].stride(0) <= INT32_MAX)), "truss_mi355: critic_tail_backward: dq must be [B] or [B, 1]");
    a.dq = view_ptr(b, dq[j], "dq");
    a.dq_stride = B > 1 ? (int32_t)dq[j].stride(0) : 1;
    a.p = ptr<const float>(b, at_or_none(p, j), at::kFloat, "p", B * K1);
    a.z1 = ptr<const float>(b, z1[j], at::kFloat, "z1");
    a.z2 = ptr<const float>(b, z2[j], at::kFloat, "z2");
    a.w1 = ptr<const float>(b, w1[j], at::kFloat, "w1");
    a.w2 = ptr<const float>(b, w2[j], at::kFloat, "w2");
    a.w3 = ptr<const float>(b, w3[j], at::kFloat, "w3");
    for (int64_t i = 0; i < L && !o.empty(); ++i) a.o[i] = ptr<const float>(b, o.get(pos + i), at::kFloat, "o", B * N * H);
    for (int64_t i = 0; i < L && !d_o.empty(); ++i) {
      const OT d = d_o.get(pos + i);
      TORCH_CHECK(!present(d) || d->numel() == B * N * H, "truss_mi355: critic_tail_backward: d_o[i] must hold B N H elements");
      a.d_o[i] = ptr<float>(b, d, at::kFloat, "d_o");
    }
    pos += (size_t)L;
    auto out = [&](const c10::List<OT> &l, int64_t numel, const char *name) {
      const OT t = at_or_none(l, j);
      TORCH_CHECK(!present(t) || t->numel() == numel, "truss_mi355: critic_tail_backward: ", name, " must hold ", numel, " elements");
      return ptr<float>(b, t, at::kFloat, name);
    };
    a.dz1 = out(dz1, B * Q, "dz1"), a.dz2 = out(dz2, B * Q, "dz2");
    a.d_w1 = out(d_w1, Q * K1, "d_w1"), a.d_b1 = out(d_b1, Q, "d_b1"), a.d_w2 = out(d_w2, Q * Q, "d_w2"), a.d_b2 = out(d_b2, Q, "d_b2");
    a.d_w3 = out(d_w3, Q, "d_w3"), a.d_b3 = out(d_b3, 1, "d_b3");
  }
  TORCH_CHECK(d_o.empty() || pos == d_o.size(), "truss_mi355: critic_tail_backward: d_o holds ", d_o.size(), " entries, n_layers asks for ", pos);
  check_rc(b, b.critic_tail_backward(items.data(), (int32_t)J, (void *)stream), "truss_critic_tail_backward");
}

// w [C, K] float32 -> out [3, 224, KP] int16 (bfloat16 bit patterns, zero rows / columns beyond C / K): the exact three-term split of the bf16x3 path == truss_gcn_split_w
void gcn_split_w(int64_t lib, int64_t stream, const at::Tensor &w, const at::Tensor &out) {
  const Backend &b = backend(lib);
  TORCH_CHECK(w.dim() == 2 && out.dim() == 3 && out.size(0) == 3 && out.size(1) == 224 && w.size(0) <= 224 && out.size(2) == (w.size(1) + 15) / 16 * 16,
              "truss_mi355: gcn_split_w: w [C <= 224, K], out [3, 224, (K + 15) / 16 * 16]");
  check_rc(b, b.gcn_split_w(ptr<const float>(b, w, at::kFloat, "w"), (int32_t)w.size(0), (int32_t)w.size(1),
                          (uint16_t *)ptr<int16_t>(b, out, at::kShort, "out"), (void *)stream), "truss_gcn_split_w");
}

// float32 tensor of the bound library's device that need not be contiguous (a view read in place)
float *view_ptr(const Backend &b, const at::Tensor &t, const char *name) {
  TORCH_CHECK(t.scalar_type() == at::kFloat, "truss_mi355: ", name, " must be ", at::kFloat, ", got ", t.scalar_type());
  TORCH_CHECK(b.device ? t.is_cuda() : t.is_cpu(), "truss_mi355: ", name, " is on ", t.device(), ", the bound library needs ",
              b.device ? "a cuda (ROCm) device" : "the cpu");
  return (float *)t.data_ptr();
}
bool dense_from(const at::Tensor &t, int64_t d0) {   // dims d0.. laid out contiguously
  int64_t want = 1;
  for (int64_t d = t.dim() - 1; d >= d0; --d) {
    if (t.size(d) != 1 && t.stride(d) != want) return false;
    want *= t.size(d);
  }
  return true;
}
// descriptor of one field: ring [capacity, ...] contiguous, ext [rows, ...] of the same row shape (pattern: [rows, n, n] against
// ring [capacity, n, k_nbr]); a plain ext may be strided over its rows and over dim 1 (a permuted view)
truss_replay_field_t replay_field(const Backend &b, const at::Tensor &ring, const at::Tensor &ext, const OT &nbr, int64_t capacity, int64_t group) {
  truss_replay_field_t f{};
  TORCH_CHECK(ring.dim() >= 1 && ring.size(0) == capacity && capacity >= 1, "truss_mi355: a replay ring tensor must be [capacity, ...]");
  TORCH_CHECK(ext.dim() == ring.dim(), "truss_mi355: replay field: ring and outside tensor must have the same number of dims");
  f.ring = ptr<float>(b, ring, at::kFloat, "ring");
  f.ext = view_ptr(b, ext, "replay field");
  f.ext_rows = ext.size(0);
  f.ext_row_stride = ext.size(0) > 1 ? ext.stride(0) : 0;
  f.group = (int32_t)group;
  const int64_t row = ring.numel() / capacity;
  if (present(nbr)) {
    TORCH_CHECK(ring.dim() == 3 && nbr->dim() == 2 && nbr->size(0) == ring.size(1) && nbr->size(1) == ring.size(2) && ext.size(1) == ring.size(1) &&
                    ext.size(2) == ring.size(1) && dense_from(ext, 1),
                "truss_mi355: replay pattern field: ring [capacity, n, k_nbr], nbr [n, k_nbr], outside tensor [rows, n, n] with contiguous matrices");
    f.nbr = ptr<const int16_t>(b, *nbr, at::kShort, "nbr");
    f.n = (int32_t)ring.size(1);
    f.k_nbr = (int32_t)ring.size(2);
  } else {
    TORCH_CHECK(ext.sizes().slice(1) == ring.sizes().slice(1), "truss_mi355: replay plain field: ring and outside tensor rows differ in shape");
    TORCH_CHECK(row >= 1 && row <= INT32_MAX, "truss_mi355: replay plain field: bad row length");
    if (dense_from(ext, 1)) {
      f.parts = 1;
      f.part_len = (int32_t)row;
    } else {
      TORCH_CHECK(ext.dim() >= 2 && dense_from(ext, 2) && ext.stride(1) >= 0,
                  "truss_mi355: replay plain field: the outside tensor may be strided over dims 0 and 1 only");
      f.parts = (int32_t)ext.size(1);
      f.part_len = (int32_t)(row / ext.size(1));
      f.ext_part_stride = ext.stride(1);
    }
  }
  TORCH_CHECK(f.ext_row_stride >= 0, "truss_mi355: replay field: negative stride");
  return f;
}

// append: ring row (head + r) % capacity of every field <- row rows[group[i]][r] of src[i], r < k == truss_replay_scatter
void replay_scatter(int64_t lib, int64_t stream, at::TensorList ring, at::TensorList src, const c10::List<OT> &nbr, at::IntArrayRef group,
                    const at::Tensor &rows, int64_t k, int64_t head, int64_t capacity) {
  const Backend &b = backend(lib);
  need(b.replay_scatter, "truss_replay_scatter");
  const size_t F = ring.size();
  TORCH_CHECK(src.size() == F && nbr.size() == F && group.size() == F, "truss_mi355: replay_scatter takes one entry per field in every list");
  TORCH_CHECK(k >= 0 && k <= INT32_MAX && rows.dim() == 2 && rows.size(0) == 4 && rows.size(1) == k, "truss_mi355: rows must be [4, k]");
  std::vector<truss_replay_field_t> f(F);
  for (size_t i = 0; i < F; ++i) f[i] = replay_field(b, ring[i], src[i], nbr.get(i), capacity, group[i]);
  const int64_t *pr = ptr<const int64_t>(b, rows, at::kLong, "rows");
  check_rc(b, b.replay_scatter(f.data(), (int32_t)F, pr, (int32_t)k, head, capacity, (void *)stream), "truss_replay_scatter");
}

// sample: row r of out[i] <- ring row idx[r] of every field (a pattern field: the whole dense matrix) == truss_replay_gather
void replay_gather(int64_t lib, int64_t stream, at::TensorList ring, at::TensorList out, const c10::List<OT> &nbr, const at::Tensor &idx,
                   int64_t capacity) {
  const Backend &b = backend(lib);
  need(b.replay_gather, "truss_replay_gather");
  const size_t F = ring.size();
  TORCH_CHECK(out.size() == F && nbr.size() == F, "truss_mi355: replay_gather takes one entry per field in every list");
  TORCH_CHECK(idx.dim() == 1 && idx.numel() <= INT32_MAX, "truss_mi355: idx must be [batch]");
  const int64_t batch = idx.numel();
  std::vector<truss_replay_field_t> f(F);
  for (size_t i = 0; i < F; ++i) {
    TORCH_CHECK(out[i].dim() >= 1 && out[i].size(0) == batch, "truss_mi355: replay_gather outputs must be [batch, ...]");
    f[i] = replay_field(b, ring[i], out[i], nbr.get(i), capacity, 0);
  }
  const int64_t *pi = ptr<const int64_t>(b, idx, at::kLong, "idx");
  check_rc(b, b.replay_gather(f.data(), (int32_t)F, pi, (int32_t)batch, capacity, (void *)stream), "truss_replay_gather");
}

// the difference reward of K (env, member) pairs in one launch (master_DDPG_truss2D_MO.py:263-368) == truss_reward
void reward(int64_t lib, int64_t stream, int64_t max_front, const at::Tensor &front_no, const at::Tensor &n_front_no, const at::Tensor &pf_hv,
            const at::Tensor &n_pf_hv, const at::Tensor &parent, const at::Tensor &points, const at::Tensor &ref_points, const at::Tensor &n_pf,
            const at::Tensor &R, const at::Tensor &G_U, const at::Tensor &xmax, const at::Tensor &ymax, const OT &parts) {
  const Backend &b = backend(lib);
  need(b.reward, "truss_reward");
  TORCH_CHECK(front_no.dim() == 3 && front_no.size(2) == 4, "truss_mi355: front_no must be [K, P, 4]");
  const int64_t K = front_no.size(0), P = front_no.size(1);
  TORCH_CHECK(pf_hv.sizes() == front_no.sizes(), "truss_mi355: pf_hv must be [K, P, 4] like front_no");
  TORCH_CHECK(P >= 1 && P + 3 <= 64, "truss_mi355: reward takes 1..61 archive rows per pair (P + 3 <= 64), got P = ", P);
  TORCH_CHECK(max_front >= 0 && max_front <= INT32_MAX, "truss_mi355: max_front must be 0 or >= 2");
  auto is1d = [K](const at::Tensor &t) { return t.dim() == 1 && t.size(0) == K; };
  auto is2d = [K](const at::Tensor &t, int64_t c) { return t.dim() == 2 && t.size(0) == K && t.size(1) == c; };
  TORCH_CHECK(is1d(n_front_no) && is1d(n_pf_hv) && is1d(n_pf), "truss_mi355: n_front_no / n_pf_hv / n_pf must be [K]");
  TORCH_CHECK(is2d(parent, 2) && is2d(ref_points, 2), "truss_mi355: parent / ref_points must be [K, 2]");
  TORCH_CHECK(points.dim() == 3 && points.size(0) == K && points.size(1) == 3 && points.size(2) == 4, "truss_mi355: points must be [K, 3, 4]");
  TORCH_CHECK(is2d(R, 3), "truss_mi355: R must be [K, 3]");
  TORCH_CHECK(is1d(G_U) && is1d(xmax) && is1d(ymax), "truss_mi355: G_U / xmax / ymax must be [K]");
  TORCH_CHECK(!present(parts) || is2d(*parts, 8), "truss_mi355: parts must be [K, 8]");
  truss_reward_args_t a{};
  a.struct_size = sizeof(truss_reward_args_t);
  a.n_sets = (int32_t)K;
  a.max_points = (int32_t)P;
  a.max_front = (int32_t)max_front;
  a.front_no = ptr<const double>(b, front_no, at::kDouble, "front_no");
  a.n_front_no = ptr<const int32_t>(b, n_front_no, at::kInt, "n_front_no");
  a.pf_hv = ptr<const double>(b, pf_hv, at::kDouble, "pf_hv");
  a.n_pf_hv = ptr<const int32_t>(b, n_pf_hv, at::kInt, "n_pf_hv");
  a.parent = ptr<const double>(b, parent, at::kDouble, "parent");
  a.points = ptr<const double>(b, points, at::kDouble, "points");
  a.ref_points = ptr<const double>(b, ref_points, at::kDouble, "ref_points");
  a.n_pf = ptr<const int32_t>(b, n_pf, at::kInt, "n_pf");
  a.R = ptr<double>(b, R, at::kDouble, "R");
  a.G_U = ptr<double>(b, G_U, at::kDouble, "G_U");
  a.xmax = ptr<double>(b, xmax, at::kDouble, "xmax");
  a.ymax = ptr<double>(b, ymax, at::kDouble, "ymax");
  a.parts = ptr<double>(b, parts, at::kDouble, "parts");
  TORCH_CHECK(K <= INT32_MAX, "truss_mi355: too many pairs");
  if (K == 0) return;
  check_rc(b, b.reward(&a, (void *)stream), "truss_reward");
}

// the archive update of a game step for B envs in one launch: cull of the archive rows + the candidate slots, truncation, gather of
// the surviving designs, accepted flags (master_DDPG_truss2D_MO.py:372-436) == truss_archive_merge
void archive_merge(int64_t lib, int64_t stream, int64_t max_front, int64_t n_slots, const at::Tensor &pts_in, const at::Tensor &n_in,
                   const at::Tensor &y_in, const at::Tensor &sec_in, const OT &slot_row, const at::Tensor &cand_points, const at::Tensor &cand_y,
                   const at::Tensor &cand_sec, const at::Tensor &pts_out, const at::Tensor &y_out, const at::Tensor &sec_out, const at::Tensor &n_out,
                   const OT &accepted, const OT &front_idx, const OT &hv_front, const OT &metrics) {
  const Backend &b = backend(lib);
  need(b.archive_merge, "truss_archive_merge");
  TORCH_CHECK(pts_in.dim() == 3 && pts_in.size(2) == 4, "truss_mi355: pts_in must be [B, P, 4]");
  const int64_t B = pts_in.size(0), P = pts_in.size(1), C = n_slots;
  TORCH_CHECK(y_in.dim() == 3 && y_in.size(0) == B && y_in.size(1) == P, "truss_mi355: y_in must be [B, P, n_y]");
  TORCH_CHECK(sec_in.dim() == 3 && sec_in.size(0) == B && sec_in.size(1) == P, "truss_mi355: sec_in must be [B, P, n_sec]");
  const int64_t ny = y_in.size(2), ns = sec_in.size(2);
  TORCH_CHECK(n_in.dim() == 1 && n_in.size(0) == B, "truss_mi355: n_in must be [B]");
  TORCH_CHECK(C >= 0 && C <= INT32_MAX, "truss_mi355: n_slots must be >= 0");
  TORCH_CHECK(!present(slot_row) || (slot_row->dim() == 2 && slot_row->size(0) == B && slot_row->size(1) == C), "truss_mi355: slot_row must be [B, n_slots]");
  TORCH_CHECK(cand_points.dim() == 2 && cand_points.size(1) == 4, "truss_mi355: cand_points must be [R, 4]");
  const int64_t R = cand_points.size(0);
  TORCH_CHECK(cand_y.dim() == 2 && cand_y.size(0) == R && cand_y.size(1) == ny, "truss_mi355: cand_y must be [R, n_y] like y_in's rows");
  TORCH_CHECK(cand_sec.dim() == 2 && cand_sec.size(0) == R && cand_sec.size(1) == ns, "truss_mi355: cand_sec must be [R, n_sec] like sec_in's rows");
  TORCH_CHECK(pts_out.dim() == 3 && pts_out.size(0) == B && pts_out.size(2) == 4, "truss_mi355: pts_out must be [B, max_out, 4]");
  const int64_t O = pts_out.size(1);
  TORCH_CHECK(y_out.dim() == 3 && y_out.size(0) == B && y_out.size(1) == O && y_out.size(2) == ny, "truss_mi355: y_out must be [B, max_out, n_y]");
  TORCH_CHECK(sec_out.dim() == 3 && sec_out.size(0) == B && sec_out.size(1) == O && sec_out.size(2) == ns, "truss_mi355: sec_out must be [B, max_out, n_sec]");
  TORCH_CHECK(n_out.dim() == 1 && n_out.size(0) == B, "truss_mi355: n_out must be [B]");
  TORCH_CHECK(!present(accepted) || (accepted->dim() == 2 && accepted->size(0) == B && accepted->size(1) == C), "truss_mi355: accepted must be [B, n_slots]");
  TORCH_CHECK(!present(front_idx) || (front_idx->dim() == 2 && front_idx->size(0) == B && front_idx->size(1) == O), "truss_mi355: front_idx must be [B, max_out]");
  TORCH_CHECK(!present(hv_front) || (hv_front->dim() == 1 && hv_front->size(0) == B), "truss_mi355: hv_front must be [B]");
  TORCH_CHECK(!present(metrics) || (metrics->dim() == 2 && metrics->size(0) == B && metrics->size(1) == 5), "truss_mi355: metrics must be [B, 5]");
  TORCH_CHECK(B <= INT32_MAX && P <= INT32_MAX && O <= INT32_MAX && R <= INT32_MAX && ny <= INT32_MAX && ns <= INT32_MAX && max_front >= INT32_MIN &&
                  max_front <= INT32_MAX, "truss_mi355: archive_merge: a size does not fit 32 bits");
  truss_archive_args_t a{};
  a.struct_size = sizeof(truss_archive_args_t);
  a.n_envs = (int32_t)B;
  a.max_points = (int32_t)P;
  a.n_slots = (int32_t)C;
  a.max_front = (int32_t)max_front;
  a.max_out = (int32_t)O;
  a.n_y = (int32_t)ny;
  a.n_sec = (int32_t)ns;
  a.n_cand_rows = (int32_t)R;
  a.pts_in = ptr<const double>(b, pts_in, at::kDouble, "pts_in");
  a.n_in = ptr<const int32_t>(b, n_in, at::kInt, "n_in");
  a.y_in = ptr<const float>(b, y_in, at::kFloat, "y_in");
  a.sec_in = ptr<const int32_t>(b, sec_in, at::kInt, "sec_in");
  a.slot_row = ptr<const int32_t>(b, slot_row, at::kInt, "slot_row");
  a.cand_points = ptr<const double>(b, cand_points, at::kDouble, "cand_points");
  a.cand_y = ptr<const float>(b, cand_y, at::kFloat, "cand_y");
  a.cand_sec = ptr<const int32_t>(b, cand_sec, at::kInt, "cand_sec");
  a.pts_out = ptr<double>(b, pts_out, at::kDouble, "pts_out");
  a.y_out = ptr<float>(b, y_out, at::kFloat, "y_out");
  a.sec_out = ptr<int32_t>(b, sec_out, at::kInt, "sec_out");
  a.n_out = ptr<int32_t>(b, n_out, at::kInt, "n_out");
  a.accepted = ptr<uint8_t>(b, accepted, at::kByte, "accepted");
  a.front_idx = ptr<int32_t>(b, front_idx, at::kInt, "front_idx");
  a.hv_front = ptr<double>(b, hv_front, at::kDouble, "hv_front");
  a.metrics = ptr<double>(b, metrics, at::kDouble, "metrics");
  check_rc(b, b.archive_merge(&a, (void *)stream), "truss_archive_merge");
}

// the set-up of K (env, member) pairs of a game step in one launch: design rows of the parents and (three times) the candidates,
// the step-start archive, the Pareto-graph observation (rep copies) and the design game's coins == truss_pair_setup.
// K = idx.numel(); the outputs may hold more rows than the call writes (the env objects' resident buffers)
void pair_setup(int64_t lib, int64_t stream, int64_t rep, int64_t seed, int64_t game_step, at::ArrayRef<double> dtab, const at::Tensor &idx,
                const at::Tensor &ms, const at::Tensor &pts, const at::Tensor &n, const at::Tensor &arch_y, const at::Tensor &arch_sec,
                const at::Tensor &c_x, const at::Tensor &c_target, const at::Tensor &c_params, const at::Tensor &ref_points, const OT &env_ids,
                const OT &frac_tab, const at::Tensor &par_x, const at::Tensor &par_target, const at::Tensor &par_params, const at::Tensor &par_y,
                const at::Tensor &par_sec, const at::Tensor &cand_x, const at::Tensor &cand_target, const at::Tensor &cand_params,
                const at::Tensor &cand_y, const at::Tensor &cand_sec, const at::Tensor &p0, const at::Tensor &nn0, const at::Tensor &parent_obj,
                const at::Tensor &ref, const at::Tensor &x_p, const at::Tensor &A_p, const OT &coin) {
  const Backend &b = backend(lib);
  need(b.pair_setup, "truss_pair_setup");
  TORCH_CHECK(pts.dim() == 3 && pts.size(2) == 4, "truss_mi355: pair_setup: pts must be [B, P, 4]");
  const int64_t B = pts.size(0), P = pts.size(1);
  TORCH_CHECK(idx.dim() == 1 && ms.dim() == 1 && ms.size(0) == idx.size(0), "truss_mi355: pair_setup: idx / ms must be [K]");
  const int64_t K = idx.size(0);
  TORCH_CHECK(arch_y.dim() == 3 && arch_y.size(0) == B && arch_y.size(1) == P, "truss_mi355: pair_setup: arch_y must be [B, P, N]");
  TORCH_CHECK(arch_sec.dim() == 3 && arch_sec.size(0) == B && arch_sec.size(1) == P, "truss_mi355: pair_setup: arch_sec must be [B, P, E]");
  const int64_t N = arch_y.size(2), E = arch_sec.size(2);
  TORCH_CHECK(c_params.dim() == 2 && c_params.size(0) == B, "truss_mi355: pair_setup: c_params must be [B, NPARAM]");
  const int64_t NP = c_params.size(1);
  auto rows_of = [](const at::Tensor &t, int64_t rows, int64_t width) { return t.dim() == 2 && t.size(0) == rows && t.size(1) == width; };
  TORCH_CHECK(n.dim() == 1 && n.size(0) == B && rows_of(c_x, B, N) && rows_of(c_target, B, N) && rows_of(ref_points, B, 2),
              "truss_mi355: pair_setup: n [B], c_x / c_target [B, N], ref_points [B, 2]");
  TORCH_CHECK(!present(env_ids) || (env_ids->dim() == 1 && env_ids->size(0) == B), "truss_mi355: pair_setup: env_ids must be [B]");
  TORCH_CHECK(!present(frac_tab) || (frac_tab->dim() == 1 && frac_tab->size(0) == P + 1), "truss_mi355: pair_setup: frac_tab must be [P + 1]");
  TORCH_CHECK(rep == 1 || rep == 3, "truss_mi355: pair_setup: rep must be 1 or 3");
  TORCH_CHECK(dtab.size() == 4, "truss_mi355: pair_setup: dtab must hold 4 values");
  TORCH_CHECK(K <= INT32_MAX / 3 && B <= INT32_MAX && P <= INT32_MAX && N <= INT32_MAX && E <= INT32_MAX && NP <= INT32_MAX,
              "truss_mi355: pair_setup: a size does not fit 32 bits");
  // outputs: at least the rows the call writes, with the row shape of the input they copy
  auto out_rows = [](const at::Tensor &t, int64_t rows, at::IntArrayRef row, const char *name) {
    TORCH_CHECK(t.dim() == (int64_t)row.size() + 1 && t.size(0) >= rows && t.sizes().slice(1) == row, "truss_mi355: pair_setup: ", name, " must be [>= ",
                rows, ", ...] with rows of shape ", row);
  };
  out_rows(par_x, K, {N}, "par_x"); out_rows(par_target, K, {N}, "par_target"); out_rows(par_params, K, {NP}, "par_params");
  out_rows(par_y, K, {N}, "par_y"); out_rows(par_sec, K, {E}, "par_sec");
  out_rows(cand_x, 3 * K, {N}, "cand_x"); out_rows(cand_target, 3 * K, {N}, "cand_target"); out_rows(cand_params, 3 * K, {NP}, "cand_params");
  out_rows(cand_y, 3 * K, {N}, "cand_y"); out_rows(cand_sec, 3 * K, {E}, "cand_sec");
  out_rows(p0, K, {P, 4}, "p0"); out_rows(nn0, K, {}, "nn0"); out_rows(parent_obj, K, {2}, "parent_obj"); out_rows(ref, K, {2}, "ref");
  out_rows(x_p, rep * K, {P, 4}, "x_p"); out_rows(A_p, rep * K, {P, P}, "A_p");
  if (present(coin)) out_rows(*coin, 3 * K, {}, "coin");
  const auto f32 = at::kFloat, f64 = at::kDouble, i32 = at::kInt, i64 = at::kLong;
  truss_pair_args_t a{};
  a.struct_size = sizeof(truss_pair_args_t);
  a.n_pairs = (int32_t)K;
  a.n_envs = (int32_t)B;
  a.max_points = (int32_t)P;
  a.n_y = (int32_t)N;
  a.n_sec = (int32_t)E;
  a.n_param = (int32_t)NP;
  a.rep = (int32_t)rep;
  a.seed = seed;
  a.game_step = game_step;
  for (int i = 0; i < 4; ++i) a.dtab[i] = (float)dtab[i];
  a.idx = ptr<const int64_t>(b, idx, i64, "idx");
  a.ms = ptr<const int64_t>(b, ms, i64, "ms");
  a.pts = ptr<const double>(b, pts, f64, "pts");
  a.n = ptr<const int32_t>(b, n, i32, "n");
  a.arch_y = ptr<const float>(b, arch_y, f32, "arch_y");
  a.arch_sec = ptr<const int32_t>(b, arch_sec, i32, "arch_sec");
  a.c_x = ptr<const float>(b, c_x, f32, "c_x");
  a.c_target = ptr<const float>(b, c_target, f32, "c_target");
  a.c_params = ptr<const double>(b, c_params, f64, "c_params");
  a.ref_points = ptr<const double>(b, ref_points, f64, "ref_points");
  a.env_ids = ptr<const int64_t>(b, env_ids, i64, "env_ids");
  a.frac_tab = ptr<const float>(b, frac_tab, f32, "frac_tab");
  a.par_x = ptr<float>(b, par_x, f32, "par_x");
  a.par_target = ptr<float>(b, par_target, f32, "par_target");
  a.par_params = ptr<double>(b, par_params, f64, "par_params");
  a.par_y = ptr<float>(b, par_y, f32, "par_y");
  a.par_sec = ptr<int32_t>(b, par_sec, i32, "par_sec");
  a.cand_x = ptr<float>(b, cand_x, f32, "cand_x");
  a.cand_target = ptr<float>(b, cand_target, f32, "cand_target");
  a.cand_params = ptr<double>(b, cand_params, f64, "cand_params");
  a.cand_y = ptr<float>(b, cand_y, f32, "cand_y");
  a.cand_sec = ptr<int32_t>(b, cand_sec, i32, "cand_sec");
  a.p0 = ptr<double>(b, p0, f64, "p0");
  a.nn0 = ptr<int32_t>(b, nn0, i32, "nn0");
  a.parent_obj = ptr<double>(b, parent_obj, f64, "parent_obj");
  a.ref = ptr<double>(b, ref, f64, "ref");
  a.x_p = ptr<float>(b, x_p, f32, "x_p");
  a.A_p = ptr<float>(b, A_p, f32, "A_p");
  a.coin = ptr<uint8_t>(b, coin, at::kByte, "coin");
  if (K == 0) return;
  check_rc(b, b.pair_setup(&a, (void *)stream), "truss_pair_setup");
}

// every operator on meta tensors (tracing): nothing to compute, the schema says what is mutated
void noop_boxed(const c10::OperatorHandle &op, torch::jit::Stack *s) { torch::jit::drop(*s, op.schema().arguments().size()); }

}  // namespace

// Bind the entry points of a native library that is already loaded in this process (ctypes did that), looked up by name in the
// image at `path`, under the small index `lib`.  0, or: -1 `lib` is not an index of the table of libraries, -2 no such image is loaded,
// -3 the library lacks a required symbol (*missing names it; a missing optional entry just stays null).
extern "C" int truss_torch_bind(int lib, const char *path, const char **missing) {
  if (lib < 0 || lib >= (int)g_backends.size()) return -1;
  void *h = path ? dlopen(path, RTLD_NOW | RTLD_NOLOAD) : nullptr;
  if (!h) return -2;
  Backend b;
  const char *lacks = nullptr;   // the first required symbol the library does not export
  auto find = [&](const char *symbol, bool required) {
    void *fn = dlsym(h, symbol);
    if (!fn && required && !lacks) lacks = symbol;
    return fn;
  };
#define X(field, symbol, required) b.field = (decltype(b.field))find(#symbol, required);
  TRUSS_ENTRY_POINTS(X)
#undef X
  b.topo_neighbors = (decltype(b.topo_neighbors))find("truss_topo_neighbors", false);
  auto backend_name = (decltype(&truss_backend))find("truss_backend", true);
  dlclose(h);                    // only the reference taken above: the caller keeps the image loaded
  if (lacks) {
    if (missing) *missing = lacks;
    return -3;
  }
  b.device = std::strcmp(backend_name(), "hip") == 0;
  g_backends[lib] = b;
  return 0;
}

// the symbols of the table, comma-joined (the test-suite holds them against the header)
extern "C" const char *truss_torch_entries(void) {
#define X(field, symbol, required) "," #symbol
  return &(TRUSS_ENTRY_POINTS(X))[1];
#undef X
}

#define STEP_SCHEMA_TENSORS                                                                                                          \
  "Tensor x, Tensor y_in, Tensor sec_in, Tensor? max_up_in, Tensor? max_down_in, Tensor(a!)? a_geo, Tensor(b!)? a_topo, "            \
  "Tensor? coin, Tensor target, Tensor env_params, Tensor(c!) y_out, Tensor(d!)? sec_out, Tensor(e!)? max_up_out, "                  \
  "Tensor(f!)? max_down_out, Tensor(g!) disp, Tensor(h!) q0, Tensor(i!) sr, Tensor(j!) comp, Tensor(k!) point, Tensor(l!)? obj, "    \
  "Tensor(m!)? disp_f64, Tensor(n!)? q0_f64, Tensor(o!)? energy, Tensor(p!)? reactions, Tensor(q!)? status, Tensor(r!)? x_n, "        \
  "Tensor(s!)? A_s, Tensor(t!)? A_n_ts, Tensor(u!)? A_n_cs, Tensor(v!)? nN_x_n, Tensor(w!)? nN_x_e) -> ()"

TORCH_LIBRARY(truss_mi355, m) {
  m.def("step(int lib, int topo, int stream, int flags, int n_envs, int n_nodes, int n_elems, " STEP_SCHEMA_TENSORS);
  m.def("rollout(int lib, int topo, int stream, int flags, int n_envs, int n_nodes, int n_elems, int n_steps, int n_action_sets, "
        STEP_SCHEMA_TENSORS);
  m.def("obs(int lib, int topo, int stream, int n_envs, int n_nodes, int n_elems, Tensor x, Tensor y, Tensor sec, Tensor max_up, "
        "Tensor max_down, Tensor target, Tensor disp, Tensor q0, Tensor sr, Tensor comp, Tensor env_params, Tensor(a!)? x_n, "
        "Tensor(b!)? A_s, Tensor(c!)? A_n_ts, Tensor(d!)? A_n_cs, Tensor(e!)? nN_x_n, Tensor(f!)? nN_x_e) -> ()");
  m.def("obs_flags(int lib, int topo, int stream, int flags, int n_envs, int n_nodes, int n_elems, Tensor x, Tensor y, Tensor sec, Tensor max_up, "
        "Tensor max_down, Tensor target, Tensor disp, Tensor q0, Tensor sr, Tensor comp, Tensor env_params, Tensor(a!)? x_n, "
        "Tensor(b!)? A_s, Tensor(c!)? A_n_ts, Tensor(d!)? A_n_cs, Tensor(e!)? nN_x_n, Tensor(f!)? nN_x_e) -> ()");   // truss_obs with args->flags
  m.def("front(int lib, int stream, int max_front, int flags, Tensor points, Tensor n_points, Tensor? ref_points, "
        "Tensor(a!)? front_idx, Tensor(b!)? n_front, Tensor(c!)? hv_front, Tensor(d!)? hv_all, Tensor(e!)? metrics) -> ()");
  m.def("gcn_aggregate(int lib, int stream, Tensor adj, Tensor h, Tensor? bias, Tensor(a!) out, int act) -> ()");
  m.def("gcn_aggregate_sparse(int lib, int stream, Tensor adj, Tensor nbr, Tensor h, Tensor? bias, Tensor(a!) out, int act) -> ()");
  m.def("gcn_layer(int lib, int stream, Tensor x, Tensor adj, Tensor? nbr, Tensor w, Tensor? bias, Tensor(a!) out, int act, bool accumulate, "
        "Tensor? w_split, int adj_layout=0) -> ()");
  m.def("gcn_split_w(int lib, int stream, Tensor w, Tensor(a!) out) -> ()");
  m.def("gcn_level(int lib, int stream, Tensor[] x, Tensor[] adj, Tensor?[] nbr, Tensor[] w, Tensor[] bias, Tensor(a!)[] out, Tensor(b!)[] x_agg, "
        "int[] act) -> ()");
  m.def("gcn_level_backward(int lib, int stream, Tensor[] adj, Tensor[] w, int[] act, Tensor[] d_out, Tensor[] out, Tensor?[] x_agg, "
        "Tensor(a!)?[] d_w, Tensor(b!)?[] d_b, Tensor(c!)?[] d_x) -> ()");
  m.def("replay_scatter(int lib, int stream, Tensor(a!)[] ring, Tensor[] src, Tensor?[] nbr, int[] group, Tensor rows, int k, int head, "
        "int capacity) -> ()");
  m.def("replay_gather(int lib, int stream, Tensor[] ring, Tensor(a!)[] out, Tensor?[] nbr, Tensor idx, int capacity) -> ()");
  m.def("reward(int lib, int stream, int max_front, Tensor front_no, Tensor n_front_no, Tensor pf_hv, Tensor n_pf_hv, Tensor parent, Tensor points, "
        "Tensor ref_points, Tensor n_pf, Tensor(a!) R, Tensor(b!) G_U, Tensor(c!) xmax, Tensor(d!) ymax, Tensor(e!)? parts) -> ()");
  m.def("archive_merge(int lib, int stream, int max_front, int n_slots, Tensor pts_in, Tensor n_in, Tensor y_in, Tensor sec_in, Tensor? slot_row, "
        "Tensor cand_points, Tensor cand_y, Tensor cand_sec, Tensor(a!) pts_out, Tensor(b!) y_out, Tensor(c!) sec_out, Tensor(d!) n_out, "
        "Tensor(e!)? accepted, Tensor(f!)? front_idx, Tensor(g!)? hv_front, Tensor(h!)? metrics) -> ()");
  m.def("gcn_layer_fused(int lib, int stream, Tensor x, Tensor adj, Tensor? nbr, Tensor w, Tensor? bias, Tensor(a!)? out, int act, Tensor? w_split, "
        "int kind, Tensor? w2, Tensor? bias2, Tensor? adj2, Tensor? nbr2, int act2, Tensor(b!)? out2, Tensor(c!)? pool, int adj_layout=0) -> ()");
  m.def("gcn_layer_terms(int lib, int stream, Tensor x, Tensor adj, Tensor? nbr, Tensor w, Tensor? bias, Tensor(a!)? out, int act, Tensor? w_split, "
        "int kind, Tensor? w2, Tensor? bias2, Tensor? adj2, Tensor? nbr2, int act2, Tensor(b!)? out2, Tensor(c!)? pool, bool accumulate, "
        "int terms, int adj_layout=0) -> ()");
  m.def("gcn_layer_group(int lib, int stream, Tensor[] x, Tensor[] adj, Tensor?[] nbr, Tensor[] w, Tensor?[] bias, Tensor(a!)?[] out, int[] act, "
        "bool[] accumulate, Tensor[] w_split, int steps_per_chain, int kind, Tensor?[] w2, Tensor?[] bias2, Tensor?[] adj2, Tensor?[] nbr2, "
        "int[] act2, Tensor(b!)?[] out2, Tensor(c!)?[] pool, int terms, int[] adj_layout=[]) -> ()");
  m.def("pair_setup(int lib, int stream, int rep, int seed, int game_step, float[] dtab, Tensor idx, Tensor ms, Tensor pts, Tensor n, Tensor arch_y, "
        "Tensor arch_sec, Tensor c_x, Tensor c_target, Tensor c_params, Tensor ref_points, Tensor? env_ids, Tensor? frac_tab, Tensor(a!) par_x, Tensor(b!) par_target, "
        "Tensor(c!) par_params, Tensor(d!) par_y, Tensor(e!) par_sec, Tensor(f!) cand_x, Tensor(g!) cand_target, Tensor(h!) cand_params, "
        "Tensor(i!) cand_y, Tensor(j!) cand_sec, Tensor(k!) p0, Tensor(l!) nn0, Tensor(m!) parent_obj, Tensor(n!) ref, Tensor(o!) x_p, "
        "Tensor(p!) A_p, Tensor(q!)? coin) -> ()");
  m.def("gcn_level_aggregate(int lib, int stream, Tensor[] x, Tensor[] adj, Tensor[] nbr, Tensor(a!)[] y, bool[] transpose) -> ()");
  m.def("optim_step(int lib, int stream, int mode, Tensor(a!)[] params, Tensor grad, Tensor(b!)? exp_avg, Tensor(c!)? exp_avg_sq, Tensor? step, "
        "float lr, float beta1, float beta2, float eps, Tensor(d!) partials, Tensor(e!)? clipped, Tensor(f!)? norms) -> ()");
  m.def("critic_tail(int lib, int stream, Tensor[] o, int[] n_layers, Tensor[] w1, Tensor[] b1, Tensor[] w2, Tensor[] b2, Tensor[] w3, Tensor[] b3, "
        "Tensor(a!)[] q, Tensor(b!)?[] p, Tensor(c!)?[] z1, Tensor(d!)?[] z2) -> ()");
  m.def("critic_tail_backward(int lib, int stream, int[] n_layers, int[] n_nodes, Tensor[] dq, Tensor?[] p, Tensor[] z1, Tensor[] z2, Tensor[] w1, "
        "Tensor[] w2, Tensor[] w3, Tensor?[] o, Tensor(a!)?[] d_o, Tensor(b!)?[] dz1, Tensor(c!)?[] dz2, Tensor(d!)?[] d_w1, Tensor(e!)?[] d_b1, "
        "Tensor(f!)?[] d_w2, Tensor(g!)?[] d_b2, Tensor(h!)?[] d_w3, Tensor(i!)?[] d_b3) -> ()");
  m.def("target_update(int lib, int stream, Tensor(a!)[] targets, Tensor[] sources, float tau, int period, Tensor? step) -> ()");
}
static void register_operators(torch::Library &m) {
#define X(field, symbol, required) m.impl(#field, field);
  TRUSS_OPERATOR_ENTRIES(X)
#undef X
  m.impl("obs_flags", obs_flags);   // a second operator of truss_obs: no table line of its own
}
TORCH_LIBRARY_IMPL(truss_mi355, CPU, m) { register_operators(m); }    // the emulator library of the test-suite binds here
TORCH_LIBRARY_IMPL(truss_mi355, CUDA, m) { register_operators(m); }   // = HIP on ROCm: the product library
TORCH_LIBRARY_IMPL(truss_mi355, Meta, m) {                            // tracing: every operator only mutates its outputs
#define X(field, symbol, required) m.impl(#field, torch::CppFunction::makeFromBoxedFunction<&noop_boxed>());
  TRUSS_OPERATOR_ENTRIES(X)
#undef X
  m.impl("obs_flags", torch::CppFunction::makeFromBoxedFunction<&noop_boxed>());
}
