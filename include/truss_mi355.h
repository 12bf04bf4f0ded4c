/*
 * truss_mi355.h -- C ABI of the MI355X-native batched 2-D truss FEM environment step.
 *
 * This is the drop-in boundary for the hot path of kupc25648/MOP-truss-MARL.
 * The reference has no FFI of its own: its boundary is Python duck typing between
 * master_DDPG_truss2D_MO.py and truss2D_ENV.Game_research04.  The entry points below are what a
 * binding for that path needs; each one cites the reference interface it replaces
 * (paths relative to the reference checkout, train/code/ unless a test copy is named).
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature; `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream).
 *   - every pointer inside truss_step_args_t is DEVICE memory owned by the caller; the library
 *     never allocates per call and never synchronises the stream (safe inside hipGraph capture).
 *   - all functions return TRUSS_OK (0) or a negative error code; truss_last_error() gives text.
 *   - batch layout is struct-of-arrays with the env index outermost: a[B][N], a[B][E], ...
 *   - heights/actions/observations are float32 exactly as in the reference's state arrays; the
 *     stiffness assembly and the solve are float64 (SURVEY.md §7 "Precision").
 */
#ifndef TRUSS_MI355_H
#define TRUSS_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRUSS_ABI_VERSION 3

#define TRUSS_OK 0
#define TRUSS_EINVAL (-1)       /* bad argument (NULL, size mismatch, pair table not an involution ...) */
#define TRUSS_EUNSUPPORTED (-2) /* topology outside the compiled kernel envelope (bandwidth, N, E) */
#define TRUSS_EHIP (-3)         /* a HIP runtime call failed */
#define TRUSS_ENOMEM (-4)

/* flags for truss_step_args_t.flags */
#define TRUSS_F_NO_DECODE 0x1u     /* analysis only: y_out = y_in, sec_out = sec_in (reset path) */
#define TRUSS_F_CLAMP_INPLACE 0x2u /* write the clamped actions back into a_geo / a_topo
                                      (truss2D_ENV.py:376-388 mutates the caller's arrays) */
#define TRUSS_F_EMIT_OBS 0x4u      /* also write the observation tensors of the NEW design (x_n ... nN_x_e below):
                                      _game_modify builds them in the same call (truss2D_ENV.py:497-500).  One
                                      launch where the topology allows it (truss_topo_fused_obs), otherwise the
                                      observation kernel is queued behind the step on the same stream */
#define TRUSS_F_OBS_COMPACT 0x8u   /* layout of the three node-graph adjacencies that TRUSS_F_EMIT_OBS writes (valid only
                                      together with it; TRUSS_EINVAL otherwise): A_s, A_n_ts and A_n_cs are [B][N][Kc] rows
                                      through the topology's neighbour table (truss_topo_neighbors) instead of [B][N][N]:
                                        Ac[b][i][t] = A[b][i][nbr[i][t]]  where nbr[i][t] >= 0,  +0.0 in the unused slots
                                      float32, contiguous, Kc exactly the table's width.  Every value is the one the dense
                                      layout holds in that cell; x_n, nN_x_n and nN_x_e are unchanged.  The same rows are
                                      what the GCN layer kernels pick through `nbr` and what the compact replay ring holds */
/* flag of truss_obs_args_t.flags with the same meaning for truss_obs */
#define TRUSS_OBS_F_COMPACT 0x8u

/* columns of env_params[B][TRUSS_NPARAM] (float64) */
#define TRUSS_NPARAM 8
#define TRUSS_P_YMAX 0    /* gen_model.y_max            truss2D_GEN.py:80  */
#define TRUSS_P_DMIN 1    /* gen_model.d_min            truss2D_GEN.py:82  */
#define TRUSS_P_MAXDEF 2  /* gen_model.max_deformation  truss2D_GEN.py:78  */
#define TRUSS_P_LOADX 3   /* Load.size[0]               truss2D_GEN.py:362-364 */
#define TRUSS_P_LOADY 4   /* Load.size[1] */
#define TRUSS_P_INTOBJ1 5 /* Game_research04.int_obj1   truss2D_ENV.py:273 */
#define TRUSS_P_INTOBJ2 6 /* Game_research04.int_obj2   truss2D_ENV.py:274 */
#define TRUSS_P_ISROOF 7  /* truss_type == 'roof' (1.0) / 'bridge' (0.0)  truss2D_GEN.py:70 */

typedef struct truss_topo truss_topo_t; /* opaque: host + device tables of one topology */

/* ---- library ---------------------------------------------------------------------------- */
int truss_abi_version(void);
const char *truss_last_error(void);
/* "hip" for the product library; the CPU lane emulator used by the build's own tests says "emu". */
const char *truss_backend(void);

/* ---- topology (reset time) ----------------------------------------------------------------
 * Replaces Model.add_node/add_element + gen_nsc/gen_tnsc/gen_ndof + the ttnsc half of gen_ssm
 * (FEM_2Dtruss.py:189-198, 227-261, 310-317) and the static output of gen_model.generate
 * (truss2D_GEN.py:241-434): connectivity, supports, top_node, vertical_pair, load placement.
 *
 *   conn[E][2]        0-based node indices (element.nodes[0], element.nodes[1])
 *   res[N][2]         Node.res (1 = restrained)
 *   top[N]            Node.top_node
 *   pair[N]           index of Node.vertical_pair[0]; must be an involution without fixed points when
 *                     the action decode is used; may be NULL for analysis-only topologies
 *   load_mask[2][N]   nodes that carry the load for bridge (row 0) / roof (row 1)
 *                     (truss2D_GEN.py:421-430); NULL = derive by that rule from top/res
 *   sym_nodes[n][2]   (dst, src): y[dst] = y[src] when coin != 0, y[src] = y[dst] when coin == 0
 *                     (hard-coded mirror blocks of test/<star>/code/truss2D_ENV.py:459-553 / :459-675);
 *                     n = 0 for the train copy
 *   sym_elems[n][2]   both elements take min(section) (same blocks)
 *   sections[S][2]    area [m^2], inertia [m^4]  (section_data/01_brace_rod2.csv * 1e-4 / 1e-8,
 *                     truss2D_GEN.py:63-64, 291-292)
 *   node_order[N]     optional hint: node ordering for the banded solver (NULL = library chooses)
 */
int truss_topo_create(truss_topo_t **out, int32_t n_nodes, int32_t n_elems, const int32_t *conn,
                      const uint8_t *res, const uint8_t *top, const int32_t *pair,
                      const uint8_t *load_mask, int32_t n_sym_nodes, const int32_t *sym_nodes,
                      int32_t n_sym_elems, const int32_t *sym_elems, int32_t n_sections,
                      const double *sections, double e_mod, double long_stress,
                      const int32_t *node_order);
int truss_topo_destroy(truss_topo_t *t);

/* DOF numbering exactly as the reference computes it (bit-exact integers):
 *   nsc[2N]    Model.nsc   (FEM_2Dtruss.py:227-245), 1-based, free DOFs first
 *   ttnsc[E][4] Model.ttnsc (FEM_2Dtruss.py:311-317)
 * returns ndof (FEM_2Dtruss.py:255-261) or a negative error. Host pointers, may be NULL. */
int truss_topo_dofs(const truss_topo_t *t, int32_t *nsc, int32_t *ttnsc);

/* Solver view of the same system: perm[ndof] = reference DOF id (0-based) at solver position i,
 * half_bandwidth of K under that ordering, and the kernel window (lanes-per-env x rows-per-lane)
 * that was selected.  Host pointers, may be NULL. */
int truss_topo_solver_info(const truss_topo_t *t, int32_t *perm, int32_t *half_bandwidth,
                           int32_t *lanes_per_env, int32_t *rows_per_lane);

/* 1 when truss_step writes the observation tensors from the step's own launch for this topology
 * (TRUSS_F_EMIT_OBS), 0 when it queues the observation kernel behind it.  Same results either way. */
int truss_topo_fused_obs(const truss_topo_t *t);

/* The topology's neighbour table, built at truss_topo_create from conn: out[N][k_nbr] int16, per node the columns in which a
 * node-graph adjacency (A_s, A_n_ts, A_n_cs, A_n) can be non-zero -- the node itself and the far ends of its members --
 * ascending, -1 in the unused slots; k_nbr = the widest row.  It is the table of the compact observation layout
 * (TRUSS_F_OBS_COMPACT).  Host pointers; out may be NULL (then only *k_nbr is set), cap = entries `out` holds (TRUSS_EINVAL when
 * fewer than N * k_nbr).  Optional entry: a caller that wants the compact layout checks that it exists and that the table
 * equals its own before it trusts the layout. */
int truss_topo_neighbors(const truss_topo_t *t, int16_t *out, int32_t cap, int32_t *k_nbr);

/* LDS layout of the step launches of this topology, for tests and tools.  emit = 0: the plain step and the persistent
 * rollout; 1: the launch that also writes the observations (where truss_topo_fused_obs() is 0 it has none and the plain
 * layout is reported).  info[TRUSS_LDS_INFO_LEN], in this order: bytes per workgroup, offset of env 0, bytes between envs,
 * envs per workgroup; window width W and band row stride, in doubles; band rows of team A and of team B; offset of team B's
 * rows and of the trash slot from the band's start, in doubles; then byte ranges [lo, hi) inside one env: the band, the
 * element-value buffer; the number of ranges in `live` and of entries in `band_offsets`.
 * live[2 * cap_live]: (lo, hi) of everything that holds a value still to be read while the element-value buffer is in use.
 * band_offsets[cap_offsets]: every offset (doubles from the band's start) the assembly tables store to, trash slot left out.
 * Host pointers; live and band_offsets may be NULL. */
#define TRUSS_LDS_INFO_LEN 16
int truss_topo_lds_info(const truss_topo_t *t, int32_t emit, int32_t *info, int32_t *live, int32_t cap_live,
                        int32_t *band_offsets, int32_t cap_offsets);

/* ---- the batched environment step ----------------------------------------------------------
 * One Game_research04._game_modify(set_node, set_element, nC_e, actions) per env
 * (truss2D_ENV.py:370-525): clamp -> _set_model -> geometry move -> supports/round -> section
 * +-1 -> sequential height repairs -> [symmetry] -> set_moveRange -> Model.gen_all -> objectives.
 * With TRUSS_F_NO_DECODE it is Model.restore(); Model.gen_all() + the objective sums of
 * Game_research04.__init__ (truss2D_ENV.py:264-274) = the reset path (_game_get_1_state :336-340).
 *
 * status[env] describes the LAST step only: every step (every step of truss_rollout too) overwrites it, so a design
 * that one step flags and the next step's decode repairs comes back with 0 and correct results.  The float outputs
 * of an env flagged TRUSS_STATUS_NOT_SPD (disp, q0, sr, point, obj, energy, reactions, the float64 copies and its
 * slices of the observation tensors) are unspecified -- NaN as a rule; its design outputs (y_out, sec_out, move
 * ranges) are valid.  The other envs of the batch are unaffected, bit for bit, whether they share a wavefront
 * with the flagged env or not (tests/test_step_status.py).
 */
#define TRUSS_STATUS_NOT_SPD 1
#define TRUSS_STATUS_OBS_TIMEOUT 2

typedef struct truss_step_args {
  size_t struct_size; /* = sizeof(truss_step_args_t), ABI guard */
  int32_t n_envs;     /* B */
  uint32_t flags;

  /* design state in (device) */
  const float *x;         /* [B][N]   node x (Node.coord[0]) */
  const float *y_in;      /* [B][N]   set_node[:,1]   (truss2D_ENV.py:362) */
  const int32_t *sec_in;  /* [B][E]   set_element[:,0] (truss2D_ENV.py:366) */
  const float *max_up_in; /* [B][N] or NULL. The reference uses the move ranges left on its model by
                             the PREVIOUS analysis (truss2D_ENV.py:402,407); NULL = recompute from
                             y_in (the ranges the parent design itself has, nN_x_n[:,7:9]) */
  const float *max_down_in;
  float *a_geo;           /* [B][N][2] actions[0]; written only with TRUSS_F_CLAMP_INPLACE */
  float *a_topo;          /* [B][N][3] actions[1] */
  const uint8_t *coin;    /* [B] or NULL: 1 when random.random() >= 0.5 (test copies :459) */
  const float *target;    /* [B][N]   Node.target of top nodes (truss2D_GEN.py:369-374) */
  const double *env_params; /* [B][TRUSS_NPARAM] */

  /* design state out */
  float *y_out;        /* [B][N] */
  int32_t *sec_out;    /* [B][E] */
  float *max_up_out;   /* [B][N] or NULL  set_moveRange of the new design (truss2D_GEN.py:118-133) */
  float *max_down_out; /* [B][N] or NULL */

  /* analysis results */
  float *disp;      /* [B][N][2] Node.global_d (FEM_2Dtruss.py:341-352); restrained DOFs = 0 */
  float *q0;        /* [B][E]    Element.e_q[0][0] (FEM_2Dtruss.py:383-386) */
  float *sr;        /* [B][E]    Element.prop_yeield (FEM_2Dtruss.py:414-431) */
  uint8_t *comp;    /* [B][E]    Element.iscompress */
  float *point;     /* [B][4]    [obj1/int_obj1, obj2/int_obj2, con1, con2] (truss2D_ENV.py:518-523); 16-byte aligned (one store per env) */
  float *obj;       /* [B][2] or NULL: raw obj1, obj2 (= int_obj1/2 when called at reset) */
  double *disp_f64; /* [B][N][2] or NULL: float64 copy for solver-level parity checks */
  double *q0_f64;   /* [B][E] or NULL */
  double *energy;   /* [B] or NULL: Model.U_full (FEM_2Dtruss.py:374-379) */
  double *reactions; /* [B][2N-ndof] or NULL: Model.r[ndof:] (FEM_2Dtruss.py:393-411) */
  int32_t *status;  /* [B] or NULL: bit mask, 0 = ok.
                       TRUSS_STATUS_NOT_SPD (1): non-positive pivot (K not SPD: the reference would raise
                         numpy.linalg.LinAlgError from FEM_2Dtruss.py:337 or return garbage);
                       TRUSS_STATUS_OBS_TIMEOUT (2): TRUSS_F_EMIT_OBS only -- the wavefront that streams the observation
                         tensors gave up waiting for the step's results (bounded wait: the launch always drains); the
                         observation tensors of this env were NOT (completely) written by this call */

  /* observation tensors of the new design, written with TRUSS_F_EMIT_OBS (needs sec_out and max_up_out /
   * max_down_out); same contents and layouts as truss_obs_args_t below; any of them may be NULL.  With
   * TRUSS_F_OBS_COMPACT the three [B][N][N] matrices are [B][N][Kc] */
  float *x_n;     /* [B][N][13]  state_data          truss2D_ENV.py:50-102 */
  float *A_s;     /* [B][N][N]                       :86-87 */
  float *A_n_ts;  /* [B][N][N]                       :92-97 */
  float *A_n_cs;  /* [B][N][N]                       :98-100 */
  float *nN_x_n;  /* [B][N][12]  state_data_not_norm :134-146 */
  float *nN_x_e;  /* [B][E][21]                      :148-169 */
} truss_step_args_t;

int truss_step(const truss_topo_t *t, const truss_step_args_t *args, void *stream);

/* Run `n_steps` chained steps without returning to the host in between: step s reads design
 * state from buffer (s & 1) and writes buffer ((s+1) & 1); actions for step s are taken at
 * a_geo + (s % n_action_sets) * B*N*2 (resp. a_topo ... *3).  args->y_in/sec_in = buffer 0, y_out/sec_out =
 * buffer 1; all other outputs are overwritten every step (every step writes them: the last step's survive).
 * This is the `for sol in Pf: for agent: _game_modify(...)` chain of run() (master…:211-260) with the actions known
 * up front.  Where truss_topo_persistent_rollout() says so the whole chain is ONE launch: every workgroup plays its
 * envs through all steps with the design state, the per-env constants and the topology tables resident in LDS and
 * the next step's actions prefetched during the solve (envs are independent: nothing crosses workgroups); otherwise
 * one launch per step.  Same results either way (bit for bit). */
int truss_rollout(const truss_topo_t *t, const truss_step_args_t *args, int32_t n_steps,
                  int32_t n_action_sets, void *stream);
/* 1 when truss_rollout runs plain decode steps of this topology as one persistent launch (0: one launch per step;
 * also 0 with the environment variable TRUSS_ROLLOUT_LAUNCHES=1, a diagnostic switch read at every call). */
int truss_topo_persistent_rollout(const truss_topo_t *t);

/* ---- observation tensors ---------------------------------------------------------------------
 * state_data + state_data_not_norm (truss2D_ENV.py:40-193) for the design/analysis a truss_step
 * just produced.  A_n, mask and nC_e are topology-static and are NOT written per env (the host
 * mirror builds them once).  All outputs float32, any of them may be NULL.
 * flags: 0, or TRUSS_OBS_F_COMPACT: A_s, A_n_ts and A_n_cs are [B][N][Kc] (see TRUSS_F_OBS_COMPACT).
 */
typedef struct truss_obs_args {
  size_t struct_size;
  int32_t n_envs;
  uint32_t flags;
  const float *x;          /* [B][N] */
  const float *y;          /* [B][N]  (truss_step y_out) */
  const int32_t *sec;      /* [B][E] */
  const float *max_up;     /* [B][N] */
  const float *max_down;   /* [B][N] */
  const float *target;     /* [B][N] */
  const float *disp;       /* [B][N][2] */
  const float *q0;         /* [B][E] */
  const float *sr;         /* [B][E] */
  const uint8_t *comp;     /* [B][E] */
  const double *env_params; /* [B][TRUSS_NPARAM] */
  float *x_n;     /* [B][N][13]  normalised node features (truss2D_ENV.py:50-102) */
  float *A_s;     /* [B][N][N]   area / max area on edges (:86-87) */
  float *A_n_ts;  /* [B][N][N]   tension stress ratio on edges (:92-97) */
  float *A_n_cs;  /* [B][N][N]   compression stress ratio on edges (:98-100) */
  float *nN_x_n;  /* [B][N][12]  raw node features (:134-146) */
  float *nN_x_e;  /* [B][E][21]  raw element features (:148-169) */
} truss_obs_args_t;

int truss_obs(const truss_topo_t *t, const truss_obs_args_t *args, void *stream);

/* ---- Pareto front + hypervolume of a batch of small point sets --------------------------------
 * replaces: utils.simple_cull / simple_cull_final (train copy utils.py:11-217, test copies :220-403) and
 * utils.union_rectangles_fastest (:275-342), which the reward block of master_DDPG_truss2D_MO.run()
 * (:263-368) calls 5 + 6 times per archived solution, for B envs at once.
 *
 * Per env: n_points[b] rows [obj1, obj2, con1, con2] (n <= max_points <= 256: one wave per env up to 64 rows,
 *           one 256-thread workgroup per env above; the same rules and the same results either way).
 *   feasible  = not (con1 > 1 or con2 > 1)                                   (utils.py:18-22)
 *   front     = feasible rows no other feasible row beats in BOTH objectives (strict), identical rows once,
 *               sorted by obj1 (ties: obj2, then input order -- the reference's tie order is a set order)
 *   truncation (flags & TRUSS_FRONT_TRUNCATE, train copy): fronts longer than max_front keep both ends and
 *               the max_front-2 interior points of largest crowding distance, in obj1 order.  DEVIATION:
 *               the reference draws the interior points with random.sample (utils.py:118-123) and keeps
 *               them in draw order; a batched kernel has no Python RNG stream to follow.
 *   metrics   = [max_distance, dis_distance, p_norm_inv_cd, sum_distance, std_cd]  (utils.py:126-214)
 *   hv_front  = union_rectangles_fastest(front, ref_point); hv_all = the same over ALL input rows
 *               (the reference also calls it on raw archives).  Closed form over the x-sorted points
 *               instead of the sweep + segment tree: same area, summation order differs (<= 1e-12).
 * All pointers are device memory; outputs may be NULL to skip them.
 */
#define TRUSS_FRONT_TRUNCATE 0x1u
#define TRUSS_FRONT_MAXP 256

typedef struct truss_front_args {
  size_t struct_size;
  int32_t n_envs;
  int32_t max_points;      /* P: row stride of points / front_idx (<= TRUSS_FRONT_MAXP) */
  int32_t max_front;       /* MAX_FRONT (utils.py:6-7: 20 train, 50 test); used with TRUSS_FRONT_TRUNCATE */
  uint32_t flags;
  const double *points;    /* [B][P][4] */
  const int32_t *n_points; /* [B] */
  const double *ref_points;/* [B][2] or NULL = (1, 1) */
  int32_t *front_idx;      /* [B][P]  input row of the k-th front point, -1 beyond n_front */
  int32_t *n_front;        /* [B] */
  double *hv_front;        /* [B] */
  double *hv_all;          /* [B] */
  double *metrics;         /* [B][5] */
} truss_front_args_t;

int truss_front(const truss_front_args_t *args, void *stream);

/* ---- difference reward of a game step, one launch for K (env, member) pairs ------------------------
 * replaces: the reward block of master_DDPG_truss2D_MO.run() (:263-368, difference_reward): per pair the hypervolume of the
 * archive plus the feasible new points with agent 0 / 1 / 2 left out and with all three (four culls), the archive's own
 * hypervolume with and without the reference point, and the sums that turn them into the three agents' rewards, G_U and the
 * running maxima -- what truss_mi355/reward.py::difference_reward assembles from three truss_front launches and about thirty
 * element-wise operators.
 *
 * Per pair k:
 *   agent j is feasible iff all four entries of points[k][j] are <= 1 (a NaN is infeasible)
 *   set s (0..2) = the first n_front_no[k] rows of front_no[k] (clamped to [0, P]) + the feasible points of the agents other
 *                  than s, in agent order; set 3 = the archive rows + all feasible points
 *   every set goes through the cull, ordering, truncation and closed-form hypervolume of truss_front (above; max_front == 0:
 *                  no truncation, else as TRUSS_FRONT_TRUNCATE) with the reference point ref_points[k]
 *   sum_distance, std_cd = metrics [3], [4] of set 3
 *   compareV / real_compareV = hv_all (truss_front) of the first n_pf_hv[k] rows of pf_hv[k] with ref_points[k] / with (1, 1)
 *   R, G_U, xmax, ymax as in reward.py::difference_reward, float64, the same operations in the same order; no special case for
 *                  n_pf == 0 or empty sets (IEEE results)
 * DEVIATIONS from the per-env host path, both those of reward.py: (1) fronts longer than max_front are truncated
 * deterministically (crowding distance), not with random.sample; (2) the final sum is float64 throughout, the reference's is
 * float32 where an agent is feasible (NEP-50), so R agrees to ~1e-6 relative there.
 * One workgroup per pair, the four sets on its four waves: P + 3 <= 64.  Device pointers; the library neither allocates nor
 * synchronises (capturable in a hipGraph).  TRUSS_EINVAL: bad struct_size, n_sets < 0, max_points outside 1..61, max_front == 1
 * (or < 0), a NULL input or R / G_U / xmax / ymax NULL; nothing is launched then.  n_sets == 0: TRUSS_OK, no launch.
 * Optional symbol: a library of this ABI version may lack it. */
typedef struct truss_reward_args {
  size_t struct_size;
  int32_t n_sets;            /* K: (env, member) pairs */
  int32_t max_points;        /* P: row stride of front_no / pf_hv; P + 3 <= 64 */
  int32_t max_front;         /* 0: no truncation; else as TRUSS_FRONT_TRUNCATE with this MAX_FRONT (>= 2) */
  uint32_t flags;            /* 0 */
  const double *front_no;    /* [K][P][4]  current non-dominated archive rows */
  const int32_t *n_front_no; /* [K] */
  const double *pf_hv;       /* [K][P][4]  archive rows the step started from; may alias front_no */
  const int32_t *n_pf_hv;    /* [K] */
  const double *parent;      /* [K][2]     (obj1, obj2) of the solution the agents acted on */
  const double *points;      /* [K][3][4]  the three agents' new points */
  const double *ref_points;  /* [K][2] */
  const int32_t *n_pf;       /* [K]        len(Pf) */
  double *R;                 /* [K][3] */
  double *G_U, *xmax, *ymax; /* [K] */
  double *parts;             /* [K][8] or NULL: hv(-0), hv(-1), hv(-2), hv(all), compareV, real_compareV, sum_distance, std_cd
                                (the four hv BEFORE compareV is subtracted and clamped) */
} truss_reward_args_t;
int truss_reward(const truss_reward_args_t *args, void *stream);

/* ---- archive update of a game step, one launch for B envs ---------------------------------------------
 * replaces: the archive block of master_DDPG_truss2D_MO.run() (:372-436: append the feasible candidates to Pf, simple_cull,
 * clip the objectives) as truss_mi355/marl.py assembles it around one truss_front launch -- candidate buffers, scatters, two
 * concatenations of the whole archive, gathers of the surviving designs and the accepted flags.
 *
 * Per env b the cull sees P + C rows [obj1, obj2, con1, con2]:
 *   row i < P      archive row pts_in[b][i]; rows i >= clamp(n_in[b], 0, P) are dead: the cull sees their con1 as 2.0
 *   row P + c      candidate slot c < C: row r = slot_row[b][c] of the caller's candidate arrays (cand_points / cand_y /
 *                  cand_sec), r outside [0, n_cand_rows) (-1 by convention) = empty slot; slot_row == NULL: r = b C + c (dense
 *                  step-wide buffers).  A candidate is ok iff con1 <= 1 && con2 <= 1 (a NaN is not ok).  An empty slot is the
 *                  infeasible row [0, 0, 2, 0]; a candidate that is not ok keeps its values with con1 = 2.0
 * The cull, the order (obj1, obj2, input order) and, with max_front >= 2, the truncation by crowding distance are those of
 * truss_front (above; max_front == 0: no truncation) with the reference point (1, 1): the same selection, bit for bit.
 * Outputs, rows in front order, every row j >= n_out[b] written as zeros:
 *   pts_out    the selected row, obj1 / obj2 clamped to <= 1.0 (:434-436)
 *   y_out / sec_out  the selected design: archive row i of y_in / sec_in, or row r of cand_y / cand_sec (n_y / n_sec words each)
 *   n_out      size of the front (at most max_front when truncating)
 *   accepted   [B][C] 1 iff slot c's row is in the new archive (NULL: skipped)
 *   front_idx  [B][max_out] input row (i, or P + c) of the k-th front point, -1 beyond n_out; hv_front [B], metrics [B][5] as
 *              truss_front's (each NULL: skipped)
 * One workgroup per env: one wave for P + C <= 64, 256 threads up to P + C <= 256.  No atomics, every output element has one
 * owner.  Device pointers; the library neither allocates nor synchronises (capturable in a hipGraph).
 * TRUSS_EINVAL, with nothing launched or written: bad struct_size, n_envs < 0, P < 1, C < 0, P + C > 256, max_front == 1 or < 0,
 * max_out < max_front (truncating) or < P + C (not), n_y < 1, n_sec < 1, n_cand_rows < 0 (< B C with slot_row == NULL), a NULL
 * required pointer (the candidate arrays are required when C > 0), an output range that overlaps an input range or another output
 * -- the archive cannot be updated in place: the caller keeps two sets of buffers.  n_envs == 0: TRUSS_OK, no launch.
 * Optional symbol: a library of this ABI version may lack it. */
#define TRUSS_ARCHIVE_MAXROWS 256
typedef struct truss_archive_args {
  size_t struct_size;
  int32_t n_envs;            /* B */
  int32_t max_points;        /* P: rows of the archive per env */
  int32_t n_slots;           /* C: candidate slots per env; P + C <= TRUSS_ARCHIVE_MAXROWS */
  int32_t max_front;         /* 0: no truncation; else as TRUSS_FRONT_TRUNCATE with this MAX_FRONT (>= 2) */
  int32_t max_out;           /* row stride of the outputs: >= max_front when truncating, >= P + C otherwise */
  int32_t n_y, n_sec;        /* words per design row of y / sec */
  int32_t n_cand_rows;       /* R: rows of the candidate arrays */
  uint32_t flags;            /* 0 */
  uint32_t reserved;
  const double *pts_in;      /* [B][P][4] */
  const int32_t *n_in;       /* [B] */
  const float *y_in;         /* [B][P][n_y] */
  const int32_t *sec_in;     /* [B][P][n_sec] */
  const int32_t *slot_row;   /* [B][C] or NULL */
  const double *cand_points; /* [R][4] */
  const float *cand_y;       /* [R][n_y] */
  const int32_t *cand_sec;   /* [R][n_sec] */
  double *pts_out;           /* [B][max_out][4] */
  float *y_out;              /* [B][max_out][n_y] */
  int32_t *sec_out;          /* [B][max_out][n_sec] */
  int32_t *n_out;            /* [B] */
  uint8_t *accepted;         /* [B][C] or NULL */
  int32_t *front_idx;        /* [B][max_out] or NULL */
  double *hv_front;          /* [B] or NULL */
  double *metrics;           /* [B][5] or NULL */
} truss_archive_args_t;
int truss_archive_merge(const truss_archive_args_t *args, void *stream);

/* ---- set-up of a chunk of (env, member) pairs of a game step, one launch for K pairs ------------------
 * replaces: the block of indexing operators with which truss_mi355/marl.py starts every chunk of a game step (the prologue of
 * master_DDPG_truss2D_MO.run() :211-260 per archive member, batched): the gathers of the step-start archive and the per-env
 * constants, the copies into the parent and candidate env objects, truss2D_ENV.pareto_state_data (:19-38) padded to P nodes, and
 * the symmetry coins of the design game.  Nothing is computed beyond one conversion, one division or one product per element.
 *
 * Pair k < K is (env idx[k], member ms[k]); idx and ms are int64 (what the framework's nonzero returns), idx may repeat an env any
 * number of times and need not be sorted.  With b = idx[k], m = ms[k], n = clamp(n[b], 0, P):
 *   par_x / par_target / par_params / par_y / par_sec   row k       = c_x[b], c_target[b], c_params[b], arch_y[b][m], arch_sec[b][m]
 *   cand_x / cand_target / cand_params / cand_y / cand_sec  rows a K + k, a = 0..2 = the same five rows (agent-major)
 *   p0 [K][P][4] = pts[b]     nn0 [K] = n[b] (as stored)     parent_obj [K][2] = pts[b][m][0:2]     ref [K][2] = ref_points[b]
 *   x_p [rep K][P][4] float32, row i < n: [ (float)pts[b][i][0], (float)pts[b][i][1], i == m ? 1 : 0, frac ]
 *                     (conversions round to nearest); rows i >= n: exact zeros.  frac = (float)n / (float)P, ONE float32 division
 *                     -- or, with frac_tab, the caller's frac_tab[n]: a framework that divides a tensor by a host scalar as a
 *                     product with the rounded reciprocal (two roundings: 49 / 50 comes out one ulp lower) is matched by handing
 *                     over the table it computes, as with dtab
 *   A_p [rep K][P][P] float32: dtab[deg_i] * dtab[deg_j] (ONE float32 product) for |i - j| <= 1 and i, j < n, else exact zero,
 *                     deg_i = 1 + [i > 0] + [i + 1 < n]: the path over the n members with self loops, symmetrically normalised.
 *                     dtab[d] is the caller's float32 value of d^-1/2 for d = 1, 2, 3 (dtab[0] is not read): the caller decides how
 *                     that is rounded, so that A_p carries the bits of whatever host computation it stands in for
 *   rows a K + k of x_p / A_p are equal for every a < rep (rep = 3: the candidates' next states see their parent's front)
 *   coin [3 K] uint8 or NULL: coin[a K + k] = top bit of splitmix64(splitmix64(seed) ^ (env_ids[b] << 26 | game_step << 10 | m << 2 | a))
 *                     in 64-bit wrap-around arithmetic
 * Only rows [0, K) (3 K, rep K) of the outputs are written.  Two workgroups per pair (the design rows; everything else); plain
 * vector loads and stores, 16 bytes where both the piece and the address allow it; no LDS, no atomics, every output word has one
 * owner.  Device pointers; the library neither allocates nor synchronises (capturable in a hipGraph).
 * idx[k] outside [0, n_envs) or ms[k] outside [0, P) is the caller's error and is not detected (that would need a synchronisation):
 * both are clamped into range before they index anything, so such a pair reads some env's rows and writes its own rows only.
 * TRUSS_EINVAL, naming the argument, with nothing launched or written: bad struct_size, n_pairs < 0, n_envs < 0 (< 1 with pairs),
 * max_points outside 1..TRUSS_PAIR_MAXP, n_y / n_sec / n_param < 1, rep outside {1, 3}, flags != 0, 3 n_pairs (or n_envs max_points) times the
 * widest row (max(P P, 8 P, n_y, n_sec, 2 n_param) words) above 2^31 - 1, a NULL pointer (coin and frac_tab may be NULL; env_ids may be
 * NULL when coin is), a pointer not aligned to its element type, an output range that overlaps an input range or another output.
 * n_pairs == 0: TRUSS_OK, no launch.  Optional symbol: a library of this ABI version may lack it. */
#define TRUSS_PAIR_MAXP 256
typedef struct truss_pair_args {
  size_t struct_size;
  int32_t n_pairs;           /* K */
  int32_t n_envs;            /* B */
  int32_t max_points;        /* P: rows of the archive per env */
  int32_t n_y, n_sec;        /* N, E: words per design row of y / sec (x and target rows have n_y words too) */
  int32_t n_param;           /* doubles per row of c_params (TRUSS_NPARAM) */
  int32_t rep;               /* 1 or 3: copies of the Pareto graph */
  uint32_t flags;            /* 0 */
  int64_t seed;              /* the coin's seed */
  int64_t game_step;         /* the coin's step field */
  float dtab[4];             /* [0, 1^-1/2, 2^-1/2, 3^-1/2] as the caller rounds them */
  const int64_t *idx;        /* [K] */
  const int64_t *ms;         /* [K] */
  const double *pts;         /* [B][P][4] */
  const int32_t *n;          /* [B] */
  const float *arch_y;       /* [B][P][n_y] */
  const int32_t *arch_sec;   /* [B][P][n_sec] */
  const float *c_x;          /* [B][n_y] */
  const float *c_target;     /* [B][n_y] */
  const double *c_params;    /* [B][n_param] */
  const double *ref_points;  /* [B][2] */
  const int64_t *env_ids;    /* [B]; may be NULL when coin is */
  const float *frac_tab;     /* [P + 1] or NULL: column 3 of x_p for n = 0..P instead of (float)n / (float)P */
  float *par_x, *par_target; /* [K][n_y] */
  double *par_params;        /* [K][n_param] */
  float *par_y;              /* [K][n_y] */
  int32_t *par_sec;          /* [K][n_sec] */
  float *cand_x, *cand_target; /* [3 K][n_y] */
  double *cand_params;       /* [3 K][n_param] */
  float *cand_y;             /* [3 K][n_y] */
  int32_t *cand_sec;         /* [3 K][n_sec] */
  double *p0;                /* [K][P][4] */
  int32_t *nn0;              /* [K] */
  double *parent_obj;        /* [K][2] */
  double *ref;               /* [K][2] */
  float *x_p;                /* [rep K][P][4] */
  float *A_p;                /* [rep K][P][P] */
  uint8_t *coin;             /* [3 K] or NULL */
} truss_pair_args_t;
int truss_pair_setup(const truss_pair_args_t *args, void *stream);

/* ---- GCN neighbourhood aggregation for the actors' inference in batched rollouts -----------------
 * replaces (inference only): the `A @ (X W) + b` + activation half of spektral GCNConv as used by
 * truss2D_RL.multimodes_actor (truss2D_RL.py:49-120): out[b][i][c] = act(sum_j A[b][i][j] H[b][j][c] + bias[c])
 * with H = X W computed by the caller (one large GEMM, rocBLAS).  float32; n_nodes <= 64.
 * a_batch_stride = n_nodes * n_nodes for per-env adjacencies, 0 for one adjacency shared by the batch.
 * act: 0 none, 1 relu, 2 sigmoid.  Device pointers; `out` may alias `h`.
 */
int truss_gcn_aggregate(const float *adj, int64_t a_batch_stride, const float *h, const float *bias, float *out,
                        int32_t n_batch, int32_t n_nodes, int32_t n_channels, int32_t act, void *stream);

/* The same aggregation for graphs whose adjacency is known to be zero outside a fixed sparsity pattern -- the truss's own
 * connectivity plus the diagonal, which is the pattern of every node-graph adjacency the reference builds (A_n, A_s, A_n_ts,
 * A_n_cs: truss2D_ENV.py:40-193): out[b][i][c] = act(sum_k A[b][i][nbr[i][k]] H[b][nbr[i][k]][c] + bias[c]), k < k_nbr,
 * instead of a sum over all n_nodes columns (256-node trusses: 9 terms instead of 256).  `adj` stays the DENSE [n_nodes][n_nodes]
 * matrix (per env or shared, as above): only the listed entries are read.  nbr: int16 [n_nodes][k_nbr] device table, ascending
 * column indices per row, -1 = unused slot; k_nbr <= 16.  n_channels must be a multiple of 4, h / out / bias 16-byte aligned.
 * Any n_nodes <= 32767.  `out` must NOT alias `h` (rows are read by their neighbours' threads).
 */
int truss_gcn_aggregate_sparse(const float *adj, int64_t a_batch_stride, const int16_t *nbr, int32_t k_nbr, const float *h,
                               const float *bias, float *out, int32_t n_batch, int32_t n_nodes, int32_t n_channels, int32_t act,
                               void *stream);

/* ---- one whole GCN layer on the matrix cores -------------------------------------------------------------
 * replaces: spektral GCNConv as the reference's actors / critics call it (truss2D_RL.py:49-127; 13 layers per actor, 21 per
 * critic): out[b] = act(A[b] (X[b] W^T) + bias) for a batch of small graphs, float32 throughout.  Evaluated as ((A X) W^T): the
 * neighbourhood sum is applied to the input rows on their way into LDS, the product with W^T runs on MFMA (v_mfma_f32_32x32x2_f32,
 * float32 accumulation), bias / activation / accumulation are the epilogue -- H = X W never exists in HBM.  Same value as the
 * reference's order of operations up to float32 rounding (<= 2e-5 relative against the float32 PyTorch layer in the tests).
 *   x    [n_batch][n_nodes][k_in], rows x_row_stride floats apart (0 = k_in)
 *   adj  dense [n_nodes][n_nodes] per graph (a_batch_stride = n_nodes^2) or one for all (0)
 *   nbr  optional sparsity pattern as for truss_gcn_aggregate_sparse: int16 [n_nodes][k_nbr], -1 = unused, k_nbr <= 16;
 *        NULL = dense, n_nodes <= 64 (the Pareto graph)
 *   w    [c_out][k_in], k contiguous (the layout of torch.nn.Linear.weight), c_out <= 224; bias [c_out] or NULL
 *   out  [n_batch][n_nodes][c_out], rows out_row_stride floats apart (0 = c_out); must not alias x
 *   act  0 none, 1 relu, 2 sigmoid;  accumulate != 0: out += act(...) (the sum of the five second-level layers of the actor)
 * n_nodes <= 256.  Device pointers. */
#define TRUSS_GCN_ADJ_DENSE 0
#define TRUSS_GCN_ADJ_COMPACT 1
typedef struct truss_gcn_layer_args {
  size_t struct_size;
  int32_t n_batch, n_nodes, k_in, c_out, act, accumulate, k_nbr;
  int32_t adj_layout;  /* TRUSS_GCN_ADJ_DENSE (0): adj as above.  TRUSS_GCN_ADJ_COMPACT (1): adj holds the rows of the compact
                          observation layout (TRUSS_F_OBS_COMPACT) -- [n_nodes][k_nbr] per graph, a_batch_stride = n_nodes * k_nbr
                          or 0; nbr is required; term t of row i is adj[i * k_nbr + t] instead of adj[i * n_nodes + nbr[i][t]], its
                          source row still nbr[i][t].  Same coefficients in the same order: the output is bit for bit that of the
                          dense call.  Every entry that takes this block honours it for the layer's own adjacency (an epilogue's
                          adj2 stays dense); truss_gcn_level takes dense adjacencies only.  Any other value: TRUSS_EINVAL */
  const float *x;
  int64_t x_row_stride;
  const float *adj;
  int64_t a_batch_stride;
  const int16_t *nbr;
  const float *w;
  const float *bias;
  float *out;
  int64_t out_row_stride;
  const uint16_t *w_bf16x3; /* NULL: the product runs on the float32 matrix cores.  Otherwise: `w` split into three bfloat16 terms by
                               truss_gcn_split_w ([3][224][kp], kp = k_in rounded up to 16); the product then runs on the bf16
                               matrix cores as six partial products with float32 accumulation ("bf16x3": every float32 operand is
                               split EXACTLY into three bf16 terms, the three dropped cross terms are below 2^-24 |a||b|) -- 2.7 x
                               fewer matrix-core cycles at float32 accuracy.  Hidden layers only: c_out 33..224, k_in % 4 == 0, x
                               16-byte aligned, <= 9 terms per row; other shapes are refused with this pointer set. */
} truss_gcn_layer_args_t;

int truss_gcn_layer(const truss_gcn_layer_args_t *args, void *stream);

/* The same layer with a CONSUMER of its output in the epilogue of the same launch, for the three activations of the actor's
 * inference that are written to HBM only to be read back once (truss2D_RL.py:86-120).  With V = act(A (X W^T) + bias), the layer's
 * output:
 *   TRUSS_GCN_EPI_HEAD  out2 = act2(A2 (V W2^T) + bias2): a second, narrow GCN layer (an action head: gcn_l3_x + gcn_l4_x).
 *       w2   [c2][c_out] float32 as it lies in nn.Linear.weight, 1 <= c2 <= 8; bias2 [c2] or NULL; act2 as act
 *       adj2 / a2_batch_stride / nbr2 / k_nbr2: the head's own adjacency over the same n_nodes, as adj / a_batch_stride / nbr / k_nbr
 *       out2 [n_batch][n_nodes][c2], rows out2_row_stride floats apart (0 = c2)
 *   TRUSS_GCN_EPI_POOL  pool[b][c] = sum over ALL n_nodes rows n of V[b][n][c] (GlobalSumPool: gcn_l1_4 over the Pareto graph)
 *       pool [n_batch][c_out], rows pool_row_stride floats apart (0 = c_out)
 * `layer` is what truss_gcn_layer takes (both products), except that layer->out may be NULL -- V is then never written, which is
 * the point -- and layer->accumulate must be 0.  out2 / pool must not overlap x, out or each other.  One owner per output element,
 * fixed summation order, no atomics: results are bitwise reproducible.  Neither allocates nor synchronises; capturable.
 * Optional entry of ABI version 3 (a library may lack it). */
#define TRUSS_GCN_EPI_HEAD 1
#define TRUSS_GCN_EPI_POOL 2
typedef struct truss_gcn_epilogue {
  uint32_t struct_size;
  int32_t kind;
  /* HEAD */
  const float *w2;
  const float *bias2;
  const float *adj2;
  int64_t a2_batch_stride;
  const int16_t *nbr2;
  int32_t k_nbr2, c2, act2;
  float *out2;
  int64_t out2_row_stride;
  /* POOL */
  float *pool;
  int64_t pool_row_stride;
} truss_gcn_epilogue_t;
int truss_gcn_layer_fused(const truss_gcn_layer_args_t *layer, const truss_gcn_epilogue_t *epi, void *stream);

/* The split-weight layer at REDUCED precision, for inference that does not need float32 products (rollout actions get exploration
 * noise on top and are decoded to a 0.01 grid / +-1 sections).  `layer` and `epi` are exactly what truss_gcn_layer /
 * truss_gcn_layer_fused take, with the same checks; epi == NULL is the plain layer.  layer->w_bf16x3 must be set (TRUSS_EINVAL
 * otherwise: this entry is the split-weight path only, with its envelope), and the same [3][224][kp] image serves every value of
 *   bf16_terms  3  "bf16x3": the six partial products x_i w_j, i + j <= 2 -- the very kernels the two entries above launch
 *               2  "bf16x2": x1 w0 + x0 w1 + x0 w0, operands truncated to two bf16 terms (16 significant bits)
 *               1  "bf16"  : x0 w0, operands truncated to one bf16 term (8 significant bits)
 *               anything else: TRUSS_EINVAL.
 * Accumulation stays float32; bias, activation, accumulation into out and the epilogues (the head's own product included) are
 * float32 as before.  Operands are TRUNCATED, not rounded to nearest (that is what lets one weight image serve all three): every
 * product is therefore biased towards zero, by up to 2^-6 of its size with one term and 2^-13 with two.  Against float64, with
 * Mag = |A| (|X| |W|^T) + |b| (+ |out0|):  |out - ref| <= (tau + 1e-6) Mag,  tau = 2^-13 (two terms), 2^-6 (one term).
 * n_batch == 0: TRUSS_OK, no launch.  Launches nothing and writes nothing on any refusal; neither allocates nor synchronises;
 * capturable; bitwise reproducible.  Optional entry of ABI version 3 (a library may lack it). */
int truss_gcn_layer_terms(const truss_gcn_layer_args_t *layer, const truss_gcn_epilogue_t *epi, int32_t bf16_terms, void *stream);

/* SEVERAL split-weight layers in ONE launch: the layers of one depth of the actors' inference, for all agents (truss2D_RL.py:86-120
 * evaluated for three actors that read the same observations: 9 input layers, 3 Pareto layers, 3 x 5 second-level layers, 6 head
 * layers).  layers is [n_chains][steps_per_chain]; the result is that of
 *   truss_gcn_layer_terms(&layers[c * S + s], s == S - 1 && epis ? &epis[c] : NULL, bf16_terms, stream)
 * for c = 0 .. n_chains - 1, s = 0 .. S - 1 (S = steps_per_chain) in that order, BIT FOR BIT: every output element is computed by
 * the same instructions in the same order; only which workgroup runs which layer differs.  Grid = (row tiles, chains): a workgroup
 * owns one row tile of one chain and runs the chain's steps one after the other.
 *   chains  do not depend on each other: no output (out, out2, pool) of one chain may overlap anything another chain reads or
 *           writes (TRUSS_EINVAL).
 *   steps   of a chain write the same out (out, out_row_stride and c_out agree), each with its own accumulate flag: the five
 *           second-level layers of an actor, which add into one tensor.  A step accumulates onto what the SAME THREAD stored in
 *           the step before.  No step may read, as its x, rows of the chain's out (TRUSS_EINVAL): those would be rows other
 *           threads wrote.  k_in, act, accumulate, adj / a_batch_stride / nbr, w, bias and x may differ from step to step.
 *   epis    NULL, or one epilogue per chain, all of one kind; then steps_per_chain must be 1.
 * All layers share n_batch, n_nodes, table-or-dense and the kernel instantiation truss_gcn_layer_terms would choose for them (at
 * most 6 terms per row, or 7..9) -- TRUSS_EINVAL otherwise -- and each passes every check of truss_gcn_layer_terms, with that
 * entry's codes.  TRUSS_EINVAL as well: n_chains < 0, steps_per_chain < 1, more than TRUSS_GCN_GROUP_MAX_STEPS layers, more than
 * TRUSS_GCN_GROUP_MAX_EPI chains with epilogues, bf16_terms outside 1..3.  n_chains == 0 or n_batch == 0: TRUSS_OK, no launch.
 * The layers' descriptors travel in the kernel arguments: the entry allocates nothing, copies nothing, does not synchronise and
 * launches nothing and writes nothing on any refusal; capturable; bitwise reproducible.  Optional entry of ABI version 3 (a
 * library may lack it). */
#define TRUSS_GCN_GROUP_MAX_STEPS 16   /* n_chains * steps_per_chain, plain layers */
#define TRUSS_GCN_GROUP_MAX_EPI    8   /* n_chains when epilogues are given */
int truss_gcn_layer_group(const truss_gcn_layer_args_t *layers,   /* [n_chains][steps_per_chain] */
                          const truss_gcn_epilogue_t *epis,       /* NULL, or [n_chains] */
                          int32_t n_chains, int32_t steps_per_chain, int32_t bf16_terms, void *stream);

/* A whole LEVEL of GCN layers in one launch: layers[i] as for truss_gcn_layer, for n_layers layers that do not depend on each other
 * -- the layers of one depth of the reference's actor / critic graphs (truss2D_RL.py:86-103, 116-133), of one network or of
 * several.  replaces: the forward passes of the MADDPG update (truss2D_RL.py:561-629: 19 network passes of 13 / 21 GCN layers at
 * batch 32), which are bound by their kernel count when run layer by layer.  Grid = (row tiles, layers, 32-column blocks).
 * float32 product only (w_bf16x3 = NULL, accumulate = 0), n_nodes <= 128 (dense: <= 64), any mix of shapes within one call.
 *   x_agg  NULL, or n_layers pointers (entries may be NULL): where given, the kernel also stores X' = A X of that layer,
 *          [n_batch * n_nodes][k_in] contiguous -- what the backward pass of the layer needs (dW = dZ^T X'). */
int truss_gcn_level(const truss_gcn_layer_args_t *layers, int32_t n_layers, float *const *x_agg, void *stream);

/* The BACKWARD of such a level in one launch: for every layer i of layers[] (shapes, adj, a_batch_stride, w and act as the forward
 * took them; x, bias and out of layers[i] are not read), from the gradient of the layer's output,
 *   dZ = d_out * act'(out)   (relu: out > 0, sigmoid: out (1 - out), none: 1; never stored)
 *   d_b = sum over rows of dZ,   d_w = dZ^T X',   d_x = A^T (dZ W)
 * float32 with float32 accumulation on MFMA (v_mfma_f32_32x32x2_f32).  replaces: the backward half of the MADDPG update
 * (truss2D_RL.py:561-689) as TensorFlow's autodiff runs it through the GCN layers of the actors / critics -- per layer a
 * ReluGrad / SigmoidGrad, three MatMuls, a BiasAddGrad -- which is bound by its kernel count at batch 32.  Every output element has
 * one owner and every sum a fixed order (no atomics): results are bitwise reproducible from call to call.  More than 24 layers are
 * run as consecutive launches, as in the forward.
 *   d_out  [n_batch * n_nodes][c_out] contiguous       out    the same: the layer's forward output
 *   x_agg  [n_batch * n_nodes][k_in]: X' = A X as truss_gcn_level stored it; required iff d_w is asked for
 *   d_w [c_out][k_in], d_b [c_out], d_x [n_batch * n_nodes][k_in]: each written in full where given, NULL = not wanted (a layer
 *   with all three NULL costs nothing).  d_x must not alias d_out / out (TRUSS_EINVAL), nor may outputs overlap each other.
 * Envelope: dense adjacency (nbr == NULL; a sparsity pattern is refused), n_nodes <= 64, c_out <= 224, k_in <= 256, float32
 * (w_bf16x3 == NULL, accumulate == 0), any n_batch; anything else TRUSS_EUNSUPPORTED with nothing written.  Device pointers. */
typedef struct truss_gcn_level_bwd {
  const float *d_out;
  const float *out;
  const float *x_agg;
  float *d_w;
  float *d_b;
  float *d_x;
} truss_gcn_level_bwd_t;
int truss_gcn_level_backward(const truss_gcn_layer_args_t *layers, int32_t n_layers, const truss_gcn_level_bwd_t *bwd, void *stream);

/* The NEIGHBOUR SUMS of a level through the node table, for graphs beyond the 64 nodes of the two entries above: for up to
 * TRUSS_GCN_AGG_MAX independent items per launch (more run as consecutive launches, as in truss_gcn_level), per graph g and row i
 *   transpose == 0:  y[g,i] = sum_t adj[g][i][j_t] x[g,j_t]        transpose != 0:  y[g,i] = sum_t adj[g][j_t][i] x[g,j_t]
 * over the entries j_t = nbr[i][t] >= 0 of row i of the table, in table order, float32 fmaf from 0.  The first is A x for an
 * adjacency that is zero outside the table; the second is A^T x exactly when the table is structurally symmetric (j in row i iff
 * i in row j) -- which this entry cannot check on a device table and does not; the caller does (truss2D_RL.NodePattern).
 * replaces: the N x N products X' = A X and dX = A^T (dZ W) of the MADDPG update (truss2D_RL.py:561-689) where a truss node has at
 * most 9 neighbours: 2 k N n_ch flop per graph instead of 2 N^2 n_ch, and no [n B, N, N] stack of adjacencies.  The dense products
 * of the level (X' W^T, dZ^T X', dZ W) stay with the library.
 *   x    [n_batch * n_nodes][n_ch], rows contiguous            y    the same shape; must not overlap x
 *   adj  dense [n_nodes][n_nodes] per graph, a_batch_stride floats apart (0: one adjacency for all); read only at the table's columns
 *   nbr  [n_nodes][k_nbr] int16, -1 = no entry (as for truss_gcn_aggregate_sparse; entries need not be ascending)
 * n_nodes 1..32767, k_nbr 1..16, any n_ch >= 1: 16-byte accesses where n_ch % 4 == 0 and x / y are 16-byte aligned, element by
 * element otherwise (the update has n_ch of 2, 3, 13 and 4: actions, node features, the front).  An item with n_batch == 0 passes
 * unread; n_items == 0: TRUSS_OK, no launch.  TRUSS_EINVAL: a NULL pointer, a wrong struct_size, sizes outside the above, y
 * overlapping x -- nothing is launched or written on any refusal.  The items' descriptors travel in the kernel arguments: the entry
 * allocates nothing, does not synchronise; capturable.  Every output element has one owner and a fixed order of summation (no
 * atomics): results are bitwise reproducible from call to call.  Device pointers.  Optional entry of ABI version 3 (a library may
 * lack it). */
#define TRUSS_GCN_AGG_MAX 24   /* items per launch */
typedef struct truss_gcn_agg {
  uint32_t struct_size;
  const float *x;
  const float *adj;
  int64_t a_batch_stride;
  const int16_t *nbr;
  float *y;
  int32_t n_batch, n_nodes, n_ch, k_nbr, transpose;
} truss_gcn_agg_t;
int truss_gcn_level_aggregate(const truss_gcn_agg_t *items, int32_t n_items, void *stream);

/* w [c_out <= 224][k_in] float32 -> w_bf16x3 [3][224][kp] bfloat16 bit patterns (kp = (k_in + 15) & ~15; rows >= c_out and columns >=
 * k_in are written as zeros: the layer kernel reads whole 224 x 16 slabs by LDS-DMA): the exact
 * three-term split the bf16x3 path of truss_gcn_layer reads.  Once per weight version; device pointers, 16-byte aligned output. */
int truss_gcn_split_w(const float *w, int32_t c_out, int32_t k_in, uint16_t *w_bf16x3, void *stream);

/* ---- replay buffer: append and sample, every field of a transition in one launch -------------------------------
 * replaces: MADDPG.remember (truss2D_RL.py:458-460: one deque append per transition) and the batch assembly at the top of
 * MADDPG.train (truss2D_RL.py:463 onward: random.sample + one np.array per field), for a replay that lives in device memory as
 * one ring tensor per FIELD of a transition ([capacity][row]; today 27 fields: 6 observation tensors x (state + 3 next states),
 * the two action tensors and the rewards).  Data is only moved: bit patterns survive (NaN payloads, -0.0).  A field is
 *   plain    (nbr == NULL): a ring row of parts x part_len floats.  The tensor outside the ring may be strided in two levels --
 *            rows ext_row_stride floats apart, the parts of a row ext_part_stride apart -- so that a permuted view [K, 3, N, c] of
 *            an agent-major [3, K, N, c] tensor is read in place, the accepted rows only;
 *   pattern  (nbr != NULL): a dense [n][n] matrix outside the ring, [n][k_nbr] inside it, through the table nbr[n][k_nbr] of the
 *            columns that may be non-zero in each row (as for truss_gcn_aggregate_sparse: int16, ascending, -1 = unused slot,
 *            k_nbr <= 16).  Unused slots are stored as +0.0.  Lossless iff the matrix is zero outside the table.
 * truss_replay_scatter (append): for r < k, ring row (head + r) % capacity of every field <- row rows[group][r] of its `ext`
 *   (rows: int64 [4][k]: list 0 for the state's fields, 1 + a for agent a's next state; an index outside [0, ext_rows) skips the row).
 * truss_replay_gather (sample): for r < batch, row r of every field's `ext` <- ring row idx[r] (outside [0, capacity): skipped).  A
 *   pattern field writes the WHOLE dense row: zeros, then the listed entries.
 * Rows move in 16-byte pieces where addresses and lengths allow, element by element otherwise.  Every output element has one
 * owner (no atomics); ring rows that are not addressed keep their contents.  More than 32 fields are run as consecutive launches.
 * k == 0 / batch == 0 / n_fields == 0: nothing to do.  TRUSS_EINVAL: a NULL pointer, capacity < 1, head outside [0, capacity),
 * k > capacity, bad sizes; TRUSS_EUNSUPPORTED: k_nbr > 16 (or rows x row pieces >= 2^31 in one field); nothing is written then.
 * The library neither allocates nor synchronises: both entries may be captured in a hipGraph.  Device pointers.  Optional
 * symbols: a library of this ABI version may lack them. */
typedef struct truss_replay_field {
  float *ring;              /* [capacity][parts * part_len] (plain) or [capacity][n][k_nbr] (pattern), contiguous */
  float *ext;               /* the tensor outside the ring: read by scatter (never written), written by gather */
  const int16_t *nbr;       /* NULL: plain field */
  int64_t ext_rows;         /* rows of ext */
  int64_t ext_row_stride;   /* floats between rows of ext */
  int64_t ext_part_stride;  /* plain: floats between the parts of one row of ext (not read when parts == 1) */
  int32_t parts, part_len;  /* plain */
  int32_t n, k_nbr;         /* pattern; the dense matrix itself is contiguous */
  int32_t group;            /* scatter: the list of `rows` (0..3) this field takes its source rows from */
  int32_t reserved;
} truss_replay_field_t;
int truss_replay_scatter(const truss_replay_field_t *fields, int32_t n_fields, const int64_t *rows, int32_t k, int64_t head,
                         int64_t capacity, void *stream);
int truss_replay_gather(const truss_replay_field_t *fields, int32_t n_fields, const int64_t *idx, int32_t batch, int64_t capacity,
                        void *stream);

/* ---- optimiser step: per-tensor gradient clip and Adam over a list of parameter tensors, two launches ------------------
 * replaces: the critic's Adam and the fresh Adam every actor update builds, both with clipnorm=1 (truss2D_RL.py:629/658/688 and the
 * critic optimisers created with the agents): Keras clips every gradient tensor to L2 norm <= 1 on its own, then applies Adam.
 * One call is one optimiser step over n_tensors parameter tensors whose gradients, and moments, lie in FLAT float32 vectors:
 * tensor i owns the elements [offset, offset + numel) of grad / exp_avg / exp_avg_sq / clipped and the numel contiguous floats at p.
 * Per tensor, with g its slice of grad (u = 2^-24 roundings as written, nothing contracted, correctly rounded / and sqrt):
 *   s = sum g_j^2 in float64 (a float32 square is exact there), norm = (float) sqrt(s), fac = min(1.0f, 1.0f / (norm + 1e-12f)),
 *   c_j = g_j * fac                                                                                        -- then, all float32,
 *   TRUSS_OPTIM_ADAM        m' = m + (1 - beta1) (c - m);  v' = v beta2 + ((1 - beta2) c) c;
 *                           den = sqrtf(v') / (float) sqrt(1 - beta2^t) + eps;  w' = w + ((1 / den) m') (float)(-lr / (1 - beta1^t))
 *                           with beta^t in float64 from t = *step, the step number (>= 1) the CALLER has already incremented: the
 *                           kernels only read it;
 *   TRUSS_OPTIM_FIRST_STEP  w' = w + (float)(-lr) (c / (|c| + eps)): step 1 of an Adam with zero moments; exp_avg, exp_avg_sq
 *                           and step are not read (NULL).
 * Two launches per TRUSS_OPTIM_MAX_TENSORS tensors (longer lists run as consecutive pairs), one 256-thread workgroup per chunk of
 * TRUSS_OPTIM_CHUNK elements of a tensor in both: the first writes every chunk's float64 sum of squares to partials[chunk], the
 * second adds its tensor's partials in chunk order, forms fac and updates its chunk.  16-byte accesses where every address of the
 * chunk allows and its length is a multiple of 4, word by word otherwise (the sums do not depend on which).  The descriptors travel in the kernel arguments: the entry
 * allocates nothing and does not synchronise; capturable.  Every output element has one owner and every sum a fixed order (no
 * atomics): two calls on equal inputs give equal bits.
 *   tensors   HOST array [n_tensors]: p device pointer (contiguous), numel 1..2^31-1, ranges ascending and disjoint
 *   grad      device, read only       exp_avg, exp_avg_sq  device, updated in place (ADAM)       step  device double (ADAM)
 *   partials  device scratch of sum_i ceil(numel_i / TRUSS_OPTIM_CHUNK) doubles, the caller's
 *   clipped   NULL, or flat float32 like grad: c as the kernel used it, the tensors' ranges only    norms  NULL, or float32 [n_tensors]
 * TRUSS_EINVAL, with nothing launched or written: bad struct_size, unknown mode, n_tensors < 0, a NULL tensors / grad / partials /
 * p, exp_avg / exp_avg_sq / step missing in ADAM mode, numel outside 1..2^31-1, ranges not ascending and disjoint, lr / eps / betas
 * not finite or betas outside [0, 1), an output (p, exp_avg, exp_avg_sq, clipped, norms, partials) overlapping the tensors' span
 * of grad.  n_tensors == 0: TRUSS_OK, no launch.  Optional entry of ABI version 3 (a library may lack it). */
#define TRUSS_OPTIM_ADAM 0
#define TRUSS_OPTIM_FIRST_STEP 1
#define TRUSS_OPTIM_CHUNK 4096         /* elements per workgroup */
#define TRUSS_OPTIM_MAX_TENSORS 160    /* tensors per launch pair */
typedef struct truss_optim_tensor {
  float *p;
  int64_t offset;
  int64_t numel;
} truss_optim_tensor_t;
typedef struct truss_optim_args {
  size_t struct_size;
  int32_t mode;
  int32_t n_tensors;
  const truss_optim_tensor_t *tensors;
  const float *grad;
  float *exp_avg;
  float *exp_avg_sq;
  const double *step;
  double lr, beta1, beta2, eps;
  double *partials;
  float *clipped;
  float *norms;
} truss_optim_args_t;
int truss_optim_step(const truss_optim_args_t *args, void *stream);

/* ---- critic tail: the 11 sum pools, their concatenation and the three dense layers of a critic pass, forward and backward ----
 * replaces: the end of truss2D_RL._critic_steps behind the second GCN level (torch.stack(o, 1).sum(2).flatten(1), dense_1 / relu,
 * dense_2 / relu, dense_out) and its autograd backward.  One ITEM is one critic pass; a call takes any number of independent items
 * that may differ in every size.  Item sizes: B samples, N nodes, L layers of H channels, Q dense units; K1 = L H.  All float32,
 * u = 2^-24 roundings as written, nothing contracted.  Forward, for sample b:
 *   p[b][i H + c] = ((O_i[b][0][c] + O_i[b][1][c]) + O_i[b][2][c]) + ...           over the N nodes in ascending order
 *   a1 = W1 p + b1 (W1 [Q][K1]), z1 = max(a1, 0);  a2 = W2 z1 + b2 (W2 [Q][Q]), z2 = max(a2, 0);  q = w3 . z2 + b3
 *   every dot product of a row w with x over K terms: lane l of 64 owns the element quads l, l + 64, ... and adds w_k x_k to its own
 *   partial sum (from 0) in ascending k; the 64 partials are added pairwise -- lanes 2m and 2m + 1, then pairs of those, six levels;
 *   the bias is added last.
 * A workgroup owns TRUSS_CRITIC_TAIL_SAMPLES consecutive samples of one item end to end; one launch per TRUSS_CRITIC_TAIL_MAX items
 * (longer lists run as consecutive launches).  16-byte loads where the row length (H, K1, Q) is a multiple of 4 and the pointers
 * are 16-byte aligned, word by word otherwise: the same sums either way.
 *   o[i]   device [B][N][H] contiguous, i < n_layers           w1 [Q][K1], b1 [Q], w2 [Q][Q], b2 [Q], w3 [Q], b3 [1]  device
 *   q      device [B], written
 *   save   != 0: p [B][K1], z1 [B][Q], z2 [B][Q] are written too (what the backward reads); == 0: they are not touched (may be NULL)
 * Backward of an item, from dq (sample b at dq[b dq_stride]) and the saved p, z1, z2 -- launch A, per sample:
 *   dz2_k = (dq w3_k) [z2_k > 0]                                                    one rounding
 *   dz1_j = (sum_k dz2_k W2[k][j]) [z1_j > 0],   dp_m = sum_j dz1_j W1[j][m]         from 0, ascending k / j, one owner per element
 *   d_o[i][b][n][c] = dp[b][i H + c] for every node n, for the layers whose d_o[i] is not NULL
 * and, when any parameter gradient is asked for, dz1 / dz2 [B][Q] go to the caller's scratch and launch B adds over the samples in
 * ascending b, from 0, one owner per element -- each of the six is optional (NULL: not wanted):
 *   d_w1 = dz1^T p   d_b1 = sum_b dz1   d_w2 = dz2^T z1   d_b2 = sum_b dz2   d_w3 = sum_b dq z2   d_b3 = sum_b dq
 * An item that asks for nothing (no d_o, no parameter gradient) is skipped.  p is read only for d_w1.
 * o[i] (optional) names the level outputs [B][N][H] the forward pooled: the backward does not read them, but whoever produced them
 * still does, so an output of the call that overlaps one of them is refused like an overlap with an input.
 * The descriptors travel in the kernel arguments: the entries allocate nothing and do not synchronise; capturable.  Every output
 * element has one owner and every sum a fixed order (no atomics): two calls on equal inputs give equal bits.
 * With nothing launched or written -- TRUSS_EINVAL: NULL items with n_items > 0, n_items < 0, a bad struct_size, a size < 1
 * (n_batch < 0, dq_stride < 0), a NULL required pointer (forward: o[i], the six parameters, q, and p / z1 / z2 with save; backward: dq, z1, z2, w1,
 * w2, w3, p with d_w1, dz1 and dz2 with any parameter gradient), an output of the call overlapping an input or another output of
 * the call (any item); TRUSS_EUNSUPPORTED: n_layers > TRUSS_CRITIC_TAIL_MAX_LAYERS, n_hidden > 256, n_q > 256, K1 > 4096,
 * n_nodes > 2^23 - 1.
 * n_items == 0: TRUSS_OK, no launch; an item with n_batch == 0 is skipped.  Optional entries of ABI version 3 (a library may
 * lack them). */
#define TRUSS_CRITIC_TAIL_MAX 4            /* items per launch */
#define TRUSS_CRITIC_TAIL_MAX_LAYERS 16
#ifndef TRUSS_CRITIC_TAIL_SAMPLES
#define TRUSS_CRITIC_TAIL_SAMPLES 1        /* samples per workgroup (a build-time choice: 1 .. 8) */
#endif
typedef struct truss_critic_tail_args {
  size_t struct_size;
  int32_t n_batch, n_nodes, n_layers, n_hidden, n_q;
  int32_t save;
  const float *o[TRUSS_CRITIC_TAIL_MAX_LAYERS];
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  float *q;
  float *p, *z1, *z2;
} truss_critic_tail_args_t;
typedef struct truss_critic_tail_bwd {
  size_t struct_size;
  int32_t n_batch, n_nodes, n_layers, n_hidden, n_q;
  int32_t dq_stride;             /* floats between the samples of dq, >= 0 (0: one value for every sample) */
  const float *dq;
  const float *p, *z1, *z2;
  const float *w1, *w2, *w3;
  const float *o[TRUSS_CRITIC_TAIL_MAX_LAYERS];   /* NULL, or what the forward pooled: never read, only held against the outputs */
  float *d_o[TRUSS_CRITIC_TAIL_MAX_LAYERS];
  float *dz1, *dz2;
  float *d_w1, *d_b1, *d_w2, *d_b2, *d_w3, *d_b3;
} truss_critic_tail_bwd_t;
int truss_critic_tail(const truss_critic_tail_args_t *items, int32_t n_items, void *stream);
int truss_critic_tail_backward(const truss_critic_tail_bwd_t *items, int32_t n_items, void *stream);

/* ---- target update: the target networks of the MADDPG update follow their online networks, gated on the device ------------
 * replaces: nothing that runs today -- the reference's soft update never fires (truss2D_RL.py:392-400, :692-699) and the default of
 * this project keeps that; MADDPG(target_update="polyak" / "hard") asks for targets that track, and this is their native path.
 * One call moves n_pairs target tensors t towards their source tensors p, all float32, u = 2^-24, per element, with the two
 * branches of torch.lerp (the product may or may not be contracted into an FMA):
 *   tau < 0.5        t' = t + (float) tau (p - t)
 *   0.5 <= tau < 1   t' = p - (p - t) (float) (1 - tau)
 *   tau == 1         t' = p, a copy of the bits
 * The gate: with step != NULL the call changes something iff fmod(*step, (double) period) == 0, where *step is read ON THE DEVICE
 * by every workgroup before its first store -- one captured call fires on some replays and not on others.  A gate that does not
 * fire stores nothing.  step == NULL: always fires.
 * One 256-thread workgroup per chunk of TRUSS_TARGET_CHUNK elements of a pair, one launch per TRUSS_TARGET_MAX_PAIRS pairs (longer
 * lists run as consecutive launches).  16-byte accesses where both addresses of the chunk are 16-byte aligned and its length is a
 * multiple of 4, word by word otherwise, the same elements either way.  The descriptors travel in the kernel arguments: the entry
 * allocates nothing and does not synchronise; capturable.  Every element has one owner (no atomics).
 *   pairs  HOST array [n_pairs]: t, p device pointers (contiguous), numel 1..2^31-1        step  device double, or NULL
 * TRUSS_EINVAL, with nothing launched or written: bad struct_size, n_pairs < 0, NULL pairs with n_pairs > 0, a NULL t or p, numel
 * outside 1..2^31-1, tau not in (0, 1], period < 1, a target range overlapping a source range or another target range.
 * n_pairs == 0: TRUSS_OK, no launch.  Optional entry of ABI version 3 (a library may lack it). */
#define TRUSS_TARGET_CHUNK 4096        /* elements per workgroup */
#define TRUSS_TARGET_MAX_PAIRS 160     /* pairs per launch */
typedef struct truss_target_pair {
  float *t;
  const float *p;
  int64_t numel;
} truss_target_pair_t;
typedef struct truss_target_args {
  size_t struct_size;
  int32_t n_pairs;
  const truss_target_pair_t *pairs;
  double tau;
  int64_t period;
  const double *step;            /* NULL: always fires */
} truss_target_args_t;
int truss_target_update(const truss_target_args_t *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRUSS_MI355_H */
