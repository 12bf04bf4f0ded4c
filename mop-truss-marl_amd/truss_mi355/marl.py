"""Batched multi-agent rollout + training loop (BASELINE configs 3-5: thousands of envs with the MADDPG
agents in the loop).  The reference's `run()` (master_DDPG_truss2D_MO.py:164-705) plays ONE truss: per game
step it lets the three agents modify every member of the Pareto archive, scores the moves with the
hypervolume-difference reward, culls the archive and trains.  Here the same game step runs for B trusses at
once, every piece on the device:

    pair set-up                       pairs.py: gathers + pareto_graph    (pair_path="hip": pairs.pair_setup, truss_pair_setup)
    parents' analysis + observation   BatchedTruss.analyze / observe     (truss_step, truss_obs kernels)
    three agents' actions             gcn.actor_infer / actors_infer      (truss_gcn_layer kernels; "grouped": truss_gcn_layer_group)
    the 3 B candidate designs         one truss_step launch over 3 B envs (+ truss_obs for the next states)
    rewards                           reward.difference_reward            (truss_front kernel; reward_path="hip": truss_reward)
    archive update                    reward.front_hv + gathers           (archive_path="hip": reward.archive_merge)
    replay + MADDPG update            replay.DeviceReplay, MADDPG.train_on_batch (its GCN levels: gcn.level_forward / level_backward)

This module holds the two engines, `BatchedMARL` and `MixedMARL`; the names of gcn.py, pairs.py and replay.py that callers
have always reached through it are imported below.

One game step is ONE flat pass over all live (env, archive member) pairs (member-major list, in chunks of at most
`pair_capacity` pairs): one parent analysis, one actor pass per agent, one candidate launch, one reward evaluation for
all of them -- not one pass per member index, whose later, thin iterations were bound by launch overhead.

Differences from the per-env loop, all forced by batching and documented here:
  D1  the archive is culled once per chunk of pairs -- for an archive of up to 14 members (MAX_FRONT 20: the front
      kernel takes 64 rows = 20 archive rows + the 3 x 14 candidates of 14 members) that is once per game step, like the
      reference (:430); larger archives are folded in two rounds (the Pareto front of a union is the front of the
      partial fronts, so the set is the same unless the MAX_FRONT truncation intervenes); rewards use the front at
      the START of the game step, like the reference (front_no / Pf_HV, :263-368);
  D2  a transition enters the replay when its candidate is in the archive after that cull (the reference remembers the
      candidates that survive the end-of-step cull, :595-621);
  D3  truncation to MAX_FRONT is deterministic (largest crowding distance), see include/truss_mi355.h;
  D4  when an agent's move is infeasible its next state in the replay is the first feasible agent's
      (the reference draws a random survivor, :380-407); the Pareto-graph inputs (x_p, A_p) of the next
      states are those of the step-start front;
  D5  exploration noise is drawn on the device (same law as truss2D_RL.OUNoise: theta (mu - a) dt + sigma N(0,1));
  D6  (design game) the symmetry coin of each move is the top bit of a splitmix64 hash of (engine seed, global env id, game
      step, member index in the step-start archive, agent) -- `design_coins` -- instead of the reference's random.random()
      >= 0.5 per _game_modify call (test/*/truss2D_ENV.py:459-553): the same Bernoulli(0.5) law, reproducible by a host
      model and independent of `pair_capacity` and of the chunk order.

The design game (`game="test"`, the reference's test copies test/0?_*/code): trained agents modify mirror-symmetric
designs with a coin per move, the archive keeps up to MAX_FRONT = 50 members, nothing is trained (train_period = 0) and
the last step culls the archive plus all of that step's candidates WITHOUT truncation (simple_cull_final, master…:424-428).
Every chunk's candidates are collected into step-wide buffers (slot = 3 member + agent) and the step ends with ONE cull over
the P archive rows + 3 P candidates (the wide front kernel takes up to 256 rows): D1 does not apply to this game.
`design_episode` plays a whole episode.
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from . import _lib
from . import reward as RW
from .batched import BatchedTruss
from .gcn import (PRECISIONS, actor_infer, actors_infer, gcn_aggregate, gcn_layer, gcn_layer_group, gcn_layer_head, gcn_layer_pool,  # noqa: F401
                  level_aggregate, level_backward, level_forward, refresh_actor_caches, split_weights)
from .critic_tail import tail_hook
from .optim import optimizer_step
from .target import target_hook
from .pairs import design_coins, pair_dtab, pair_frac_tab, pair_setup, pareto_graph, path_graph_table  # noqa: F401
from .replay import DeviceReplay
from .topology import TrussTopology

_level_backward_hook = level_backward        # (BatchedMARL's argument of the same name shadows the function)


_TUNE_UPDATE_GEMMS = False


def enable_gemm_tuning(max_ms_per_shape: int = 30, filename: str | None = None):
    """Let PyTorch's TunableOp choose the library GEMM for the shapes of the MADDPG UPDATE (fixed: batch 32), timed once
    during the eager warm-up updates that precede the hipGraph capture (BatchedMARL._train).  The weight gradients of the
    GCN layers (200 x 200 outputs, K = 32 x 16 = 512) otherwise get a single 256 x 224 tile from the library's heuristic:
    118 us each, half of an update.  The inference GEMMs are left alone: their row count (live (env, member) pairs x nodes)
    changes every game step and every new shape would be tuned again (11 s for four game steps when tried).
    No-op on the CPU backend."""
    global _TUNE_UPDATE_GEMMS
    if not torch.cuda.is_available():
        return False
    t = torch.cuda.tunable
    t.enable(True)                 # use tuned solutions where a shape has one
    t.tuning_enable(False)         # ... but time new shapes only inside the update's warm-up
    t.set_max_tuning_duration(int(max_ms_per_shape))
    t.set_max_tuning_iterations(20)
    filename = filename or os.environ.get("TRUSS_GEMM_TUNE_FILE")   # keep / reuse the choices (a profiled run reads them: no tuning)
    if filename:
        t.set_filename(filename)
        if hasattr(t, "write_file_on_exit"):
            t.write_file_on_exit(True)
    elif hasattr(t, "write_file_on_exit"):
        t.write_file_on_exit(False)    # no tunableop_results*.csv in the caller's working directory
    _TUNE_UPDATE_GEMMS = True
    return True


def _option(name, value, env, allowed, env_values=(), default=None):
    """An engine option: the argument; None: what the environment variable `env` says, else the default (allowed[0] unless given).
    env_values: the variable's values that count, mapped to the option's (default: the option's own non-default values); any other
    value means the default.  env_values=None: the variable's value is taken as it is, and validated like the argument."""
    default = allowed[0] if default is None else default
    if value is None:
        value = os.environ.get(env, default)
        if env_values is not None:
            value = dict(env_values or {v: v for v in allowed}).get(value, default)
    if value not in allowed:
        names = [repr(v) for v in allowed]
        raise ValueError(f"{name} must be " + ("one of " + ", ".join(names) if len(names) > 3 else ", ".join(names[:-1]) + " or " + names[-1])
                         + f", got {value!r}")
    return value


class BatchedMARL:
    """game: "train" (the train copy: MAX_FRONT 20, no coin, culls of at most 64 rows, D1) or "test" (the design game of the
    test copies, see the module docstring: needs a topology built with `symmetry=`; MAX_FRONT 50 unless max_front says
    otherwise).  env_ids: global ids of the B envs (the coin's env field; default 0..B-1).
    pair_path: how a game step sets up a chunk of (env, member) pairs -- "torch" (gathers of the step-start archive, copies into the
    env objects, `pareto_graph`, `design_coins`: framework operators, the default) or "hip" (one `truss_pair_setup` launch per chunk;
    needs a library with that entry); None: "hip" if the environment has TRUSS_PAIRS=hip, else "torch".  Both play the same game,
    bit for bit.
    actor_precision: the product of the actors' hidden layers in the ROLLOUT (`actor_infer(precision=...)`): "bf16x3" (float32
    accuracy, the default), "f32", or the reduced "bf16x2" / "bf16" (two terms / one term of the bf16 split, truncated: errors of
    up to 2^-13 / 2^-6 of a layer's magnitude, every product biased towards zero; need a library with `truss_gcn_layer_terms`);
    None: the environment's TRUSS_ACTOR_PRECISION, else "bf16x3".  Composes with actor_path; the update is not affected (it
    evaluates the actors in float32 from the replayed states).
    actor_path: how the rollout evaluates an actor -- "layers" (13 launches of the fused layer kernel, the default) or "fused"
    (`actor_infer(fused=True)`: the Pareto pool and the two action heads run in the epilogues of the layers that feed them, 11
    launches; needs a library with `truss_gcn_layer_fused`) or "grouped" (`actors_infer`: the fused path for all three actors at
    once, every depth of their layers ONE launch of `truss_gcn_layer_group` -- four launches per call instead of 33, the same bits
    as "fused"; needs a library with that entry); None: the environment's TRUSS_ACTOR if it is "fused" or "grouped", else "layers".
    archive_path: how a game step updates the archives -- "torch" (candidate buffers, one `truss_front` launch and gathers by
    framework operators, the default) or "hip" (one `truss_archive_merge` launch per chunk, per step in the design game; needs a
    library with that entry; the archive then lives in two sets of buffers that swap roles); None: "hip" if the environment has
    TRUSS_ARCHIVE=hip, else "torch".  Both play the same game, bit for bit.
    reward_path: how a game step computes the difference reward of a chunk of pairs -- "torch" (three `truss_front` launches plus
    element-wise operators, the default) or "hip" (one `truss_reward` launch; needs max_front + 3 <= 64 and a library with that
    entry); None: "hip" if the environment has TRUSS_REWARD=hip, else "torch".
    replay_storage: "dense" (the default) or "compact" (`DeviceReplay`: adjacencies stored through the neighbour tables, one
    launch per append / sample on the GPU); None: "compact" if the environment has TRUSS_REPLAY_STORAGE=compact, else "dense".
    obs_layout: how the step / observation kernels hand over the node-graph adjacencies A_s, A_n_ts, A_n_cs of a game step -- "dense"
    ([., N, N], the default) or "compact" ([., N, Kc] rows through `topo.neighbor_table()`, TRUSS_F_OBS_COMPACT: the actors' layer
    kernels read the rows as they are, the replay takes them as plain fields; needs a library with `truss_topo_neighbors`, and in the
    train game replay_storage="compact" -- ValueError otherwise); None: "compact" if the environment has TRUSS_OBS_LAYOUT=compact,
    else "dense".  Both play the same game, bit for bit; the update reads dense samples either way.
    level_backward: how the update differentiates a level of GCN layers on the GPU -- "library" (batched library GEMMs, the
    default) or "hip" (one `truss_gcn_level_backward` launch per level); None: "hip" if the environment has
    TRUSS_LEVEL_BACKWARD=1, else "library".  The choice is installed process-wide for cuda tensors (like the level forward)
    and is part of an update graph from the moment it is captured.
    level_adjacency: how the update's levels apply the node-graph adjacencies of a truss of MORE than 64 nodes (up to 64 the fused
    level kernels own whole graphs and this option changes nothing) -- "dense" (batched library GEMMs over stacked N x N
    adjacencies, the default) or "table" (sums over the entries of `topo.neighbor_table()`, one `truss_gcn_level_aggregate` launch
    per level and direction on the GPU; needs a library with that entry; the sampled adjacencies are zero outside the table by
    construction); None: "table" if the environment has TRUSS_LEVEL_ADJACENCY=table, else "dense".
    optimizer_path: how the update takes its four optimiser steps (the three critics' shared Adam, one fresh Adam per actor, each with
    the per-tensor gradient clip) -- "torch" (`_clip_flat` + `SharedStepAdam.step` / `_fresh_adam_step`: 35 and 13
    launches, the default) or "hip" (one `truss_optim_step` call, two launches, per step: `optim.optimizer_step`; needs
    a library with that entry); None: "hip" if the environment has TRUSS_OPTIMIZER=hip, else "torch".  Installed process-wide for
    cuda tensors like level_backward, and removed again by an engine built with "torch".  The optimiser's state stays with
    `SharedStepAdam` either way.
    critic_tail: how the update evaluates the end of a critic pass, behind the second GCN level (11 sum pools, their concatenation,
    three dense layers; nine passes per update) -- "torch" (framework operators and autograd, the default) or "hip" (`truss_critic_tail`
    / `truss_critic_tail_backward`: one launch forward for all critics that run together, two backward, `critic_tail.tail_hook`; needs
    a library with those entries); None: "hip" if the environment has TRUSS_CRITIC_TAIL=hip, else "torch".  Installed process-wide for
    cuda tensors like optimizer_path, and removed again by an engine built with "torch".
    target_path: how the update moves the target networks where the MADDPG asks for it (`MADDPG(target_update="polyak" / "hard")`: the
    mode, tau and period are the MADDPG's, the engine only chooses the path; with the default mode no path runs) -- "torch"
    (`truss2D_RL._target_update_torch`: a fixed number of multi-tensor operations, the default) or "hip" (one `truss_target_update` call,
    two launches for the 222 parameter tensors: `target.target_hook`; needs a library with that entry); None: "hip" if the
    environment has TRUSS_TARGET_PATH=hip, else "torch".  Either way the gate "every k-th update" is decided on the device, so one
    captured update fires on some replays and not on others.  Installed process-wide for cuda tensors like optimizer_path, and
    removed again by an engine built with "torch"."""

    def __init__(self, topo: TrussTopology, n_envs: int, maddpg, *, max_front: int | None = None, lib=None, device=None,
                 replay_capacity: int = 32768, batch_size: int = 32, hv_margin: float = 0.2, seed: int = 0,
                 pair_capacity: int | None = None, tune_update_gemms: bool = True, game: str = "train", env_ids=None,
                 level_backward: str | None = None, replay_storage: str | None = None, reward_path: str | None = None,
                 archive_path: str | None = None, actor_path: str | None = None, actor_precision: str | None = None,
                 pair_path: str | None = None, level_adjacency: str | None = None, optimizer_path: str | None = None,
                 critic_tail: str | None = None, obs_layout: str | None = None, target_path: str | None = None):
        if game not in ("train", "test"):
            raise ValueError(f"game must be 'train' or 'test', got {game!r}")
        if game == "test" and len(topo.sym_nodes) == 0:
            raise ValueError("game='test' modifies mirror-symmetric designs: build the topology with symmetry='small' or 'large'")
        if max_front is None:
            max_front = 50 if game == "test" else 20
        self.game = game
        self.topo, self.B, self.P = topo, int(n_envs), int(max_front)
        self.rl = maddpg
        if tune_update_gemms and (device is None or torch.device(device).type == "cuda"):
            enable_gemm_tuning()      # library GEMM per (fixed) shape of the update, chosen during its warm-up (23 -> 14 ms per update)
        if game == "test":
            # one cull per game step over the P archive rows + the 3 candidates of every member
            if 4 * self.P > _lib.FRONT_MAXP:
                raise ValueError(f"game='test': max_front {self.P} needs {4 * self.P} rows per cull, the front kernel takes {_lib.FRONT_MAXP}")
            self.Gm = self.P
        else:
            # members whose candidates fit one cull: P archive rows + 3 candidates per member <= the front kernel's 64 rows
            self.Gm = max(1, min(self.P, (64 - self.P) // 3))
        # (env, member) pairs per pass: the env objects below hold that many designs (3 x as many candidates)
        self.cap = int(pair_capacity) if pair_capacity else min(self.B * self.Gm, 4 * self.B)
        self.cap = max(self.cap, self.B)
        self.envP = BatchedTruss(topo, self.cap, device=device, lib=lib)          # archive members under study
        self.envC = BatchedTruss(topo, 3 * self.cap, device=device, lib=lib)      # their candidates, agent-major
        self.lib, self.device = self.envP.lib, self.envP.device
        if self.device.type == "cuda" and os.environ.get("TRUSS_LEVEL_FORWARD", "1") != "0":
            import truss2D_RL
            truss2D_RL.set_level_forward(level_forward(self.lib), "cuda")   # the update's forward passes: one launch per level
        self._options(level_backward, replay_storage, reward_path, archive_path, pair_path, actor_path, actor_precision, level_adjacency,
                      optimizer_path, critic_tail, obs_layout, target_path)
        self._arch_spare = None       # archive_path="hip": the set of archive buffers the next merge writes (see _merge_archive)
        self._pair_dtab = self._pair_frac = None   # pair_path="hip": deg^-1/2 and n / P as the framework rounds them on this device
        #                                             (pair_dtab, pair_frac_tab; made at the first step)
        if self.device.type == "cuda":
            import truss2D_RL
            truss2D_RL.set_level_backward(_level_backward_hook(self.lib) if self.level_backward == "hip" else None, "cuda")
            truss2D_RL.set_optimizer_step(optimizer_step(self.lib) if self.optimizer_path == "hip" else None, "cuda")
            truss2D_RL.set_critic_tail(tail_hook(self.lib) if self.critic_tail == "hip" else None, "cuda")
            truss2D_RL.set_target_update(target_hook(self.lib) if self.target_path == "hip" else None, "cuda")
        # level_adjacency="table": the node table of this truss, current during every update of this engine (`_train`); the table's
        # device tensor stays with the pattern, i.e. with the engine: a captured update holds its address
        self.pattern = None
        if self.level_adjacency == "table":
            import truss2D_RL
            self.pattern = truss2D_RL.NodePattern(topo.neighbor_table()).to(self.device)
            if self.device.type == "cuda":
                truss2D_RL.set_level_aggregate(level_aggregate(self.lib), "cuda")
        dev, B, P, N, E = self.device, self.B, self.P, topo.N, topo.E
        A_n, mask = topo.normalized_adjacency()
        self.A_n = torch.tensor(A_n, device=dev)[None]
        self.mask = torch.tensor(mask, device=dev)[None]
        self.nbr = torch.tensor(topo.neighbor_table(), device=dev)     # sparsity pattern of every node-graph adjacency (actor inference)
        self.nbr_p = torch.tensor(path_graph_table(P), device=dev)     # ... and of the Pareto graph (a path over the front's members)
        self.pts = torch.zeros((B, P, 4), dtype=torch.float64, device=dev)
        self.arch_y = torch.zeros((B, P, N), dtype=torch.float32, device=dev)
        self.arch_sec = torch.zeros((B, P, E), dtype=torch.int32, device=dev)
        self.n = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.ref_points = torch.ones((B, 2), dtype=torch.float64, device=dev)
        self.replay = DeviceReplay(replay_capacity, N, P, dev, storage=self.replay_storage, nbr=self.nbr, nbr_p=self.nbr_p, lib=self.lib)
        self.batch_size, self.hv_margin = batch_size, hv_margin
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        self.seed = int(seed)
        self.env_ids = (torch.arange(B, dtype=torch.int64, device=dev) if env_ids is None else
                        torch.as_tensor(np.asarray(env_ids, np.int64), device=dev))
        assert self.env_ids.shape == (B,)
        self.end_step = None           # design game: the game step whose cull is the final one (design_episode sets it)
        self.final = None              # design game: the final front after that step (see _design_cull)
        self.game_step = 1
        self._steps_dev = torch.zeros((), dtype=torch.int64, device=self.device)
        self._synced = False
        self._tg, self.use_train_graph = None, True
        self.profile = None            # set to {} to accumulate synchronised wall time per segment (diagnostic)

    def _options(self, level_backward, replay_storage, reward_path, archive_path, pair_path, actor_path, actor_precision, level_adjacency,
                 optimizer_path=None, critic_tail=None, obs_layout=None, target_path=None):
        # (see the class) argument, else environment, else default; then what the choice needs of the library and of max_front
        def lib_has(flag, what, entry):
            if not flag:
                raise ValueError(f"{what}: {self.lib.path} has no {entry}")

        self.level_backward = _option("level_backward", level_backward, "TRUSS_LEVEL_BACKWARD", ("library", "hip"), {"1": "hip"})
        self.level_adjacency = _option("level_adjacency", level_adjacency, "TRUSS_LEVEL_ADJACENCY", ("dense", "table"))
        if self.level_adjacency == "table":
            lib_has(self.lib.has_level_aggregate, "level_adjacency='table'", "truss_gcn_level_aggregate")
        self.optimizer_path = _option("optimizer_path", optimizer_path, "TRUSS_OPTIMIZER", ("torch", "hip"))
        if self.optimizer_path == "hip":
            lib_has(self.lib.has_optim_step, "optimizer_path='hip'", "truss_optim_step")
        self.critic_tail = _option("critic_tail", critic_tail, "TRUSS_CRITIC_TAIL", ("torch", "hip"))
        if self.critic_tail == "hip":
            lib_has(self.lib.has_critic_tail, "critic_tail='hip'", "truss_critic_tail")
        self.target_path = _option("target_path", target_path, "TRUSS_TARGET_PATH", ("torch", "hip"))
        if self.target_path == "hip":
            lib_has(self.lib.has_target_update, "target_path='hip'", "truss_target_update")
        self.replay_storage = _option("replay_storage", replay_storage, "TRUSS_REPLAY_STORAGE", ("dense", "compact"))
        self.obs_layout = _option("obs_layout", obs_layout, "TRUSS_OBS_LAYOUT", ("dense", "compact"))
        if self.obs_layout == "compact":
            lib_has(self.lib.has_obs_compact, "obs_layout='compact'", "truss_topo_neighbors")
            if self.game == "train" and self.replay_storage != "compact":
                raise ValueError("obs_layout='compact' in the train game needs replay_storage='compact': a dense ring holds [N, N] adjacencies")
            self.envP.obs_width("compact")                        # the library's table against the topology's, once, here
        # what the layout adds to the calls that carry it; the dense engine calls everything exactly as it always did
        compact = self.obs_layout == "compact"
        self._kw_obs = dict(obs_layout="compact") if compact else {}
        self._kw_act = dict(compact=True) if compact else {}
        self._kw_add = dict(compact_in=True) if compact else {}
        self.reward_path = _option("reward_path", reward_path, "TRUSS_REWARD", ("torch", "hip"))
        if self.reward_path == "hip":
            lib_has(self.lib.has_reward, "reward_path='hip'", "truss_reward")
            if self.P + 3 > 64:
                raise ValueError(f"reward_path='hip': max_front {self.P} + 3 new points exceed the 64 rows of a wave (truss_reward)")
        self.archive_path = _option("archive_path", archive_path, "TRUSS_ARCHIVE", ("torch", "hip"))
        if self.archive_path == "hip":
            lib_has(self.lib.has_archive, "archive_path='hip'", "truss_archive_merge")
            if self.P + 3 * self.Gm > _lib.ARCHIVE_MAXROWS:
                raise ValueError(f"archive_path='hip': max_front {self.P} + {3 * self.Gm} candidate slots exceed the "
                                 f"{_lib.ARCHIVE_MAXROWS} rows of truss_archive_merge")
        self.pair_path = _option("pair_path", pair_path, "TRUSS_PAIRS", ("torch", "hip"))
        if self.pair_path == "hip":
            lib_has(self.lib.has_pair_setup, "pair_path='hip'", "truss_pair_setup")
            if self.P > _lib.PAIR_MAXP:
                raise ValueError(f"pair_path='hip': max_front {self.P} exceeds the {_lib.PAIR_MAXP} rows of truss_pair_setup")
        self.actor_path = actor_path = _option("actor_path", actor_path, "TRUSS_ACTOR", ("layers", "fused", "grouped"))
        if actor_path == "grouped":
            lib_has(self.lib.has_gcn_group, "actor_path='grouped'", "truss_gcn_layer_group")
        if actor_path in ("fused", "grouped"):                        # (a level outside the group's envelope runs fused)
            lib_has(self.lib.has_gcn_fused, f"actor_path={actor_path!r}", "truss_gcn_layer_fused")
        self.actor_precision = _option("actor_precision", actor_precision, "TRUSS_ACTOR_PRECISION", PRECISIONS, None, "bf16x3")
        if self.actor_precision in ("bf16x2", "bf16"):
            lib_has(self.lib.has_gcn_terms, f"actor_precision={self.actor_precision!r}", "truss_gcn_layer_terms")

    def _tick(self, name, t0):
        if self.profile is None:
            return t0
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        t1 = time.perf_counter()
        self.profile[name] = self.profile.get(name, 0.0) + (t1 - t0)
        return t1

    @property
    def env_steps(self):
        """agent modifications evaluated so far (3 per live archive member per game step)"""
        return int(self._steps_dev.item())

    # ---- episode set-up (Game_research04.__init__ / ENV.reset / run() prologue, :164-196) ----
    def reset(self, x, target, y_max, d_min, max_def, load_x, load_y, is_roof, y0, sec0):
        def tiled(a, rep):                                   # per-env arrays [B] / [B, N] -> [rep B, ...]; scalars as they are
            a = np.asarray(a, np.float64)
            if a.ndim == 0:
                return a
            a = np.broadcast_to(a, (self.B,) + a.shape[1:]) if a.shape[0] != self.B else a
            return np.tile(a, (rep,) + (1,) * (a.ndim - 1))
        # the reset analysis of the B designs (normalisers int_obj1 / int_obj2, :264-274) on a B-env object
        e0 = BatchedTruss(self.topo, self.B, device=self.device, lib=self.lib)
        e0.set_constants(*[tiled(a, 1) for a in (x, target, y_max, d_min, max_def, load_x, load_y, is_roof)])
        e0.set_design(y0, sec0)
        e0.analyze(set_normalisers=True)
        # per-env constants of the whole batch: the pair-sized env objects are re-filled with the constants of the LIVE
        # (env, member) pairs of every pass, compacted to the front (BatchedTruss n_active)
        self.c_x, self.c_target, self.c_params = e0.x.clone(), e0.target.clone(), e0.env_params.clone()
        self._y_reset, self._sec_reset = e0.y.clone(), e0.sec.clone()
        self.pts.zero_(); self.arch_y.zero_(); self.arch_sec.zero_()
        self.pts[:, 0, 0:2] = 1.0                                    # Pf = [[1, 1, 0, 0, S0, ...]] (:168)
        self.arch_y[:, 0] = self._y_reset
        self.arch_sec[:, 0] = self._sec_reset
        self.n.fill_(1)
        self.ref_points.fill_(1.0)
        self.game_step = 1
        self.final = None

    # ---- observation tensors in the networks' order ----
    def _obs(self, env, pts0, n0, index, rep=1, k=None, o=None, graph=None):
        """o: observation tensors the analysis / step call has already written (TRUSS_F_EMIT_OBS); None = observation kernel.
        graph: (x_p, A_p) of the same (pts0, n0, index) if the caller has them already (the candidates see their parent's front)"""
        k = env.B if k is None else k
        if o is None:
            o = env.observe(n_active=k, **self._kw_obs)
        x_p, A_p = graph if graph is not None else pareto_graph(pts0, n0, index, self.P)
        if rep > 1:
            x_p, A_p = x_p.repeat(rep, 1, 1), A_p.repeat(rep, 1, 1)
        # views of the env's own observation buffers: the caller is done with them (actor inference, replay rows) before the same env
        # object analyses / steps again
        c = lambda key: o[key][:k]
        return dict(x_n=c("x_n"), A_s=c("A_s"), A_n_ts=c("A_n_ts"), A_n_cs=c("A_n_cs"), x_p=x_p, A_p=A_p)

    def _net_state(self, S):
        b = S["x_n"].shape[0]
        return [S["x_n"], self.A_n.expand(b, -1, -1), S["A_s"], S["A_n_ts"], S["A_n_cs"], self.mask.expand(b, -1, -1), S["x_p"], S["A_p"]]

    def _noise_vectors(self, noises):
        """(theta dt, mu, sigma) of a list of OUNoise objects as per-column device vectors (cached on the list's first object)"""
        hit = getattr(noises[0], "_dev_vectors", None)
        if hit is None or hit[0].device != self.device:
            f = lambda vals: torch.tensor(vals, dtype=torch.float32, device=self.device)
            hit = (f([nz.theta * nz.dt for nz in noises]), f([nz.mu for nz in noises]), f([nz.sigma for nz in noises]))
            noises[0]._dev_vectors = hit
        return hit

    def _act(self, S, explore):
        ins = self._net_state(S)
        actor_in = [ins[0], ins[1], ins[2], ins[3], ins[4], ins[6], ins[7]]
        geo, topo = [], []
        net_in = [actor_in[0], self.A_n[0], actor_in[2], actor_in[3], actor_in[4], actor_in[5], actor_in[6]]
        with torch.no_grad():
            grouped = None
            if self.actor_path == "grouped":                          # every actor's layers of a depth in one launch, before any noise
                grouped = actors_infer(self.lib, [ag.actor_model for ag in self.rl.agents], net_in, nbr=self.nbr, nbr_p=self.nbr_p,
                                       precision=self.actor_precision, **self._kw_act)
            for i, ag in enumerate(self.rl.agents):
                g, t = grouped[i] if grouped is not None else actor_infer(
                    self.lib, ag.actor_model, net_in, nbr=self.nbr, nbr_p=self.nbr_p, fused=self.actor_path == "fused",
                    precision=self.actor_precision, **self._kw_act)
                if explore:                                          # truss2D_RL.OUNoise.gen_noise per scalar (:41-48), all columns at once
                    for out, noises in ((g, ag.noise_geo), (t, ag.noise_topo)):
                        th_dt, mu, sg = self._noise_vectors(noises)
                        out.addcmul_(th_dt, mu - out).addcmul_(sg, torch.randn(out.shape, device=out.device, generator=self.gen))
                geo.append(g.float().contiguous())
                topo.append(t.float().contiguous())
        return geo, topo

    # ---- the MADDPG update: eager, or (one GPU) replayed as a hipGraph ----
    def _train(self, S, NS, A, R):
        """`_update` with this engine's node table current (level_adjacency="table"): the eager updates, the warm-up, the capture"""
        if self.pattern is None:
            return self._update(S, NS, A, R)
        import truss2D_RL
        with truss2D_RL.node_pattern(self.pattern):
            return self._update(S, NS, A, R)

    def _update(self, S, NS, A, R):
        """The update is thousands of small kernels at batch 32 -- launch-bound.  On the GPU it is captured once into a hipGraph
        (static input buffers, capturable Adam) and replayed -- data-parallel too: the gradient all-reduces (RCCL; one flat
        buffer for the three critics, one per actor) are captured WITH the update, every rank replaying its own copy of the same
        graph.  On the CPU backend (gloo tests) it runs eagerly."""
        if self.device.type != "cuda" or not self.use_train_graph:
            return self.rl.train_on_batch(S, NS, A, R)
        flat_in = list(S) + [t for ns in NS for t in ns] + [t for a in A for t in a] + [R]
        if self._tg is None:
            try:
                # static input buffers of the graph.  Inputs that are broadcast constants (the shared adjacency A_n, the mask: stride 0
                # over the batch) are captured as they are -- nothing to copy per update, and the passes see ONE shared adjacency
                bufs = [t if (t.dim() and t.stride(0) == 0) else t.clone() for t in flat_in]
                nS = len(S)

                def unpack(b):
                    s_ = b[:nS]
                    ns_ = [b[nS * (1 + k): nS * (2 + k)] for k in range(3)]
                    a_ = b[4 * nS: 4 * nS + 6]
                    return s_, ns_, [(a_[0], a_[1]), (a_[2], a_[3]), (a_[4], a_[5])], b[4 * nS + 6]

                # the warm-up runs real updates: weights and optimiser moments are put back afterwards (in place,
                # the graph holds their addresses), so that training is what it would have been without capture
                nets = [n for ag_ in self.rl.agents for n in (ag_.actor_model, ag_.critic_model, ag_.target_actor_model,
                                                                ag_.target_critic_model)]
                self.rl._ensure_ready(S, [A[0][0], A[0][1], A[1][0], A[1][1], A[2][0], A[2][1]])
                # the inference caches of every actor (split images, padded input weights) exist before capture: the captured
                # update rewrites them in place at its end, so that the rollout acts with the weights each replay wrote
                with torch.no_grad():
                    for ag_ in self.rl.agents:
                        actor_infer(self.lib, ag_.actor_model, [S[0][:1], self.A_n[0], S[2][:1], S[3][:1], S[4][:1], S[6][:1], S[7][:1]],
                                    nbr=self.nbr, nbr_p=self.nbr_p, fused=self.actor_path != "layers",   # (grouped: the same caches)
                                    precision=self.actor_precision)
                snap =[[p.detach().clone() for p in n.parameters()] for n in nets]
                osnap = [t.clone() for t in self.rl.critics_opt.state_tensors()]    # [] = no step taken yet (one optimiser for the three critics)
                n_loss = [len(ag_.c_loss) for ag_ in self.rl.agents]
                side = torch.cuda.Stream(device=self.device)
                side.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(side):
                    if _TUNE_UPDATE_GEMMS:
                        torch.cuda.tunable.tuning_enable(True)           # the update's GEMM shapes are fixed: pick their kernels now
                    try:
                        for _ in range(3):                               # warm-up on the capture stream
                            self.rl.train_on_batch(*unpack(bufs))
                    finally:
                        if _TUNE_UPDATE_GEMMS:
                            torch.cuda.tunable.tuning_enable(False)
                torch.cuda.current_stream(self.device).wait_stream(side)
                torch.cuda.synchronize(self.device)
                d_ = getattr(self.rl, "dist", None)
                if d_ is not None and d_.is_initialized():
                    # The process group's watchdog thread polls the events of every eagerly enqueued collective until it has seen
                    # it complete (about every 100 ms).  A poll that lands inside the capture below, on an event of the stream the
                    # captured collectives run on, aborts the process (hipErrorCapturedEvent; this PyTorch build does not hold a
                    # capture back for pending polls).  The warm-up's collectives have completed (synchronize above): wait until
                    # the watchdog has retired them.
                    time.sleep(0.5)

                def restore():      # weights, Adam moments and loss log back to the state before the warm-up
                    with torch.no_grad():
                        for n, sp in zip(nets, snap):
                            for p, v in zip(n.parameters(), sp):
                                p.copy_(v)
                        for k, t in enumerate(self.rl.critics_opt.state_tensors()):
                            t.copy_(osnap[k]) if osnap else t.zero_()
                    for ag_, nl in zip(self.rl.agents, n_loss):
                        del ag_.c_loss[nl:]

                g = torch.cuda.CUDAGraph()
                try:
                    with torch.cuda.graph(g, stream=side):
                        self.rl.train_on_batch(*unpack(bufs))
                        with torch.no_grad():
                            for ag_ in self.rl.agents:
                                refresh_actor_caches(self.lib, ag_.actor_model)
                finally:
                    restore()       # captured or not: training continues from the pre-warm-up state
                self._tg = (g, bufs)
            except RuntimeError as e:                                    # capture is an optimisation, never a requirement
                print(f"[marl] hipGraph capture of the MADDPG update failed ({type(e).__name__}: {e}); running eagerly")
                self.use_train_graph = False
                torch.cuda.synchronize(self.device)
                return self.rl.train_on_batch(S, NS, A, R)
        g, bufs = self._tg
        # broadcast constants were captured by address: a call that brings another one (or a shape the graph was not captured
        # for) runs eagerly -- never a copy into an expanded buffer, never the captured adjacency in its place
        if any(b.dim() and b.stride(0) == 0 and (t.data_ptr() != b.data_ptr() or t.stride() != b.stride() or t.shape != b.shape)
               for b, t in zip(bufs, flat_in)):
            return self.rl.train_on_batch(S, NS, A, R)
        pairs = [(b, t) for b, t in zip(bufs, flat_in) if b is not t and b.data_ptr() != t.data_ptr()]
        torch._foreach_copy_([b for b, _ in pairs], [t for _, t in pairs])    # multi-tensor launches for the ~30 input tensors
        g.replay()

    # ---- one game step of every env (run() :198-705) ----
    def game_step_all(self, train: bool | None = None, explore: bool = True, train_iters: int = 1, update: bool = True):
        """train: push accepted transitions to the replay and (with `update`) run `train_iters` MADDPG updates from it
        (default: True in the train game; the design game does not train); update=False leaves the updates to the caller
        (MixedMARL: one set of agents over several size classes).
        Design game: every move gets its coin (D6), the step ends with one cull of the archive and all candidates, truncated to
        max_front -- or, at game step `end_step`, not truncated: the final front (`self.final`).  The result adds G_U [B]."""
        test = self.game == "test"
        if train is None:
            train = not test
        if test and train:
            raise ValueError("the design game (game='test') does not train (train_period = 0)")
        B, P, Gm, dev = self.B, self.P, self.Gm, self.device
        start = dict(pts=self.pts.clone(), n=self.n.clone(), y=self.arch_y.clone(), sec=self.arch_sec.clone())   # front_no / Pf_HV (:203-209)
        added = 0
        rsum = torch.zeros((B, 3), dtype=torch.float64, device=dev)
        tk = time.perf_counter()
        arP = self._const("arP", lambda: torch.arange(P, device=dev))
        n_max = int(start["n"].max().item())
        if test:                      # step-wide candidate buffers, slot = 3 member + agent
            gsum = torch.zeros((B,), dtype=torch.float64, device=dev)
            step_cand = self._empty_candidates(3 * P)
        for g0 in range(0, n_max, Gm):                                # member groups whose candidates fit one cull
            # live (env, member) pairs of this group, member-major: pair k = (env pb[k], member pm[k])
            livemask = (arP[None, g0:g0 + Gm] < start["n"][:, None])  # [B, Gm]
            pm_all, pb_all = torch.nonzero(livemask.t(), as_tuple=True)
            pm_all = pm_all + g0
            for c0 in range(0, int(pb_all.numel()), self.cap):
                tk = self._tick("other", tk)
                idx, ms = pb_all[c0:c0 + self.cap], pm_all[c0:c0 + self.cap]
                K = int(idx.numel())
                pq = (self._pairs_hip if self.pair_path == "hip" else self._pairs_torch)(idx, ms, K, start, test)
                tk = self._tick("parent analysis + obs", tk)
                geo, topo = self._act(pq["S"], explore)
                tk = self._tick("actors", tk)
                a_geo, a_topo, NSall = self._candidate_step(pq, geo, topo, ms, K, test)
                tk = self._tick("candidate step + obs", tk)
                cand, R, G_U = self._reward(pq, idx, K, rsum)
                tk = self._tick("reward", tk)
                cand["ok"] = (cand["points"][:, :, 2:4] <= 1).all(dim=2)                         # archive candidates (:372)
                if test:                                              # collected; culled once after the last chunk
                    gsum.index_add_(0, idx, G_U)
                    self._collect_candidates(step_cand, cand, idx, ms)
                    tk = self._tick("archive update", tk)
                    continue
                # archive update (D1): front of (working archive + the feasible candidates of this chunk's members)
                slot = ((ms - g0) * 3)[:, None] + self._const("ar3", lambda: torch.arange(3, device=dev)[None, :])   # [K, 3] candidate slot of (pair, agent)
                accepted = (self._archive_hip if self.archive_path == "hip" else self._archive_torch)(pq, cand, idx, slot, K, want_accepted=train)
                tk = self._tick("archive update", tk)
                if train:
                    added += self._replay_append(pq["S"], NSall, a_geo, a_topo, R, cand["ok"], accepted, K)
                tk = self._tick("replay", tk)
        # ---- end of the game step (:430-473, 642) ----
        if test:
            final = self.end_step is not None and self.game_step >= self.end_step
            fin = self._design_cull(*step_cand, final)
            tk = self._tick("archive update", tk)
        if test and final:
            hv = dict(hv_front=fin["hv"], metrics=fin["metrics"])
            n_out = fin["n"].clone()
        else:
            hv = RW.front_hv(self.pts.contiguous(), self.n, None, 0, self.lib)
            n_out = self.n.clone()
        self.ref_points = torch.clamp(self.ref_points + self.hv_margin, max=1.0)
        self.game_step += 1
        if update:
            self.train_from_replay(train_iters if train else 0)
        tk = self._tick("train", tk)
        out = dict(hv=hv["hv_front"], n_front=n_out, sum_distance=hv["metrics"][:, 3], reward=rsum, replay_added=added,
                   replay_size=self.replay.size)
        if test:
            out["G_U"] = gsum
        return out

    # ---- the phases of a chunk of K (env, member) pairs: env idx[k], member ms[k] of the step-start archive `start` ----
    # Pair set-up, two variants that write the same bits: the design rows of the parents (envP) and their candidates (envC, three copies,
    # agent-major) in the env objects, the parents' state S, and per pair the step-start front p0 / nn0, the parent's objectives, the
    # reference point, the Pareto graph x_p / A_p ([K, ...], or [3 K, ...]: the candidates' copies too) and the design game's coins (D6)
    def _pairs_torch(self, idx, ms, K, start, test):
        """framework operators: gathers of the step-start archive, copies into the env objects, `pareto_graph`, `design_coins`"""
        eP, eC = self.envP, self.envC
        ark = torch.arange(K, device=self.device)
        p0, nn0 = start["pts"][idx].contiguous(), start["n"][idx].contiguous()
        py, ps = start["y"][idx, ms], start["sec"][idx, ms]
        cx, ct, cp = self.c_x[idx], self.c_target[idx], self.c_params[idx]
        # parents: the members of the step-start archive (:211-221)
        eP.x[:K], eP.target[:K], eP.env_params[:K] = cx, ct, cp
        eP.y[:K], eP.sec[:K] = py, ps
        S = self._obs(eP, p0, nn0, ms, k=K, o=eP.analyze(n_active=K, obs=True, **self._kw_obs))          # analysis + observations: one launch
        # the three agents modify the SAME parent (:249-260)
        eC.x[:3 * K], eC.target[:3 * K], eC.env_params[:3 * K] = cx.repeat(3, 1), ct.repeat(3, 1), cp.repeat(3, 1)
        eC.y[:3 * K], eC.sec[:3 * K] = py.repeat(3, 1), ps.repeat(3, 1)
        coin = design_coins(self.seed, self.env_ids[idx], self.game_step, ms).t().contiguous().view(-1) if test else None
        return dict(p0=p0, nn0=nn0, parent_obj=p0[ark, ms, :2].contiguous(), ref=self.ref_points[idx].contiguous(), x_p=S["x_p"], A_p=S["A_p"],
                    coin=coin, S=S, ark=ark)

    def _pairs_hip(self, idx, ms, K, start, test):
        """one `truss_pair_setup` launch (the Pareto graph three times over for the next states of the train game), then the analysis"""
        eP, eC = self.envP, self.envC
        if self._pair_dtab is None:
            self._pair_dtab, self._pair_frac = pair_dtab(self.device), pair_frac_tab(self.P, self.device)
        env_rows = lambda e: dict(x=e.x, target=e.target, params=e.env_params, y=e.y, sec=e.sec)
        pq = pair_setup(self.lib, idx, ms, start["pts"], start["n"], start["y"], start["sec"], self.c_x, self.c_target, self.c_params,
                        self.ref_points, rep=1 if test else 3, dtab=self._pair_dtab, frac_tab=self._pair_frac, par=env_rows(eP), cand=env_rows(eC),
                        coins=(self.seed, self.env_ids, self.game_step) if test else None)
        pq["S"] = self._obs(eP, pq["p0"], pq["nn0"], ms, k=K, o=eP.analyze(n_active=K, obs=True, **self._kw_obs), graph=(pq["x_p"][:K], pq["A_p"][:K]))
        pq["ark"] = torch.arange(K, device=self.device) if self.archive_path == "hip" and not test else None    # (for the merge's table of rows)
        return pq

    def _candidate_step(self, pq, geo, topo, ms, K, test):
        """the 3 K candidates of the chunk: one launch over the candidate env, agent-major (step + next-state observations; the design
        game observes nothing, it has no replay).  Returns the clamped actions (they go to the replay, :375) and the next states."""
        eC = self.envC
        a_geo, a_topo = torch.cat(geo, 0).contiguous(), torch.cat(topo, 0).contiguous()
        oC = eC.step(a_geo, a_topo, pq["coin"], clamp_inplace=True, n_active=3 * K, obs=not test, **self._kw_obs)
        self._steps_dev += 3 * K
        # the candidates see their parent's front: its Pareto graph, repeated per agent unless the set-up wrote the copies
        return a_geo, a_topo, None if test else self._obs(eC, pq["p0"], pq["nn0"], ms, rep=3 * K // pq["x_p"].shape[0], k=3 * K, o=oC,
                                                          graph=(pq["x_p"], pq["A_p"]))

    def _reward(self, pq, idx, K, rsum):
        """the difference reward of the chunk, added to the step's sum per env; the candidates pair-major: points [K, 3, 4] float64,
        y, sec (views of the candidate env's rows); the caller adds ok [K, 3]"""
        eC, p0, nn0 = self.envC, pq["p0"], pq["nn0"]
        points = eC.point[:3 * K].view(3, K, 4).permute(1, 0, 2).double().contiguous()
        cand = dict(points=points, y=eC.y[:3 * K].view(3, K, -1).permute(1, 0, 2), sec=eC.sec[:3 * K].view(3, K, -1).permute(1, 0, 2))
        R, G_U, _, _ = RW.difference_reward(p0, nn0, p0, nn0, pq["parent_obj"], points, pq["ref"], nn0, max_front=self.P, lib=self.lib,
                                            path=self.reward_path)
        rsum.index_add_(0, idx, R)
        return cand, R, G_U

    def _empty_candidates(self, C):
        """candidate buffers (points, y, sec) of C slots per env; an empty slot is the infeasible row [0, 0, 2, 0]"""
        B, dev = self.B, self.device
        empty = self._const(f"empty{C}", lambda: torch.tensor([0.0, 0.0, 2.0, 0.0], dtype=torch.float64, device=dev).expand(B, C, 4))
        z = lambda width, dt: torch.zeros((B, C, width), dtype=dt, device=dev)
        return empty.clone(), z(self.topo.N, torch.float32), z(self.topo.E, torch.int32)

    def _collect_candidates(self, step_cand, cand, idx, ms):
        """design game: the chunk's candidates into the step-wide buffers, slot = 3 member + agent, the infeasible ones marked"""
        (stepP, stepY, stepS), points, ok = step_cand, cand["points"], cand["ok"]
        slot = (ms * 3)[:, None] + self._const("ar3", lambda: torch.arange(3, device=self.device)[None, :])
        stepP[idx[:, None], slot] = torch.cat([points[:, :, :2], torch.where(ok, points[:, :, 2], 2.0)[:, :, None], points[:, :, 3:]], dim=2)
        stepY[idx[:, None], slot] = cand["y"]
        stepS[idx[:, None], slot] = cand["sec"]

    # Archive update of the train game, two variants: cull of the working archive + the chunk's candidates; accepted [K, 3] on request
    def _archive_hip(self, pq, cand, idx, slot, K, want_accepted):
        """one launch: the candidates are handed over as they lie (agent-major rows a K + k of the candidate env's tensors) through a
        [B, C3] table of rows, -1 = empty slot"""
        eC, dev, ark = self.envC, self.device, pq["ark"]
        slot_row = torch.full((self.B, 3 * self.Gm), -1, dtype=torch.int32, device=dev)
        slot_row[idx[:, None], slot] = (self._const("ar3", lambda: torch.arange(3, device=dev)[None, :]) * K + ark[:, None]).int()
        acc = self._merge_archive(eC.point[:3 * K].double(), eC.y[:3 * K], eC.sec[:3 * K], slot_row, 3 * self.Gm, accepted=want_accepted)
        return acc[idx[:, None], slot].bool() if want_accepted else None                    # one gather from the kernel's flags

    def _archive_torch(self, pq, cand, idx, slot, K, want_accepted):
        """candidate buffers, one `truss_front` launch and gathers (`_cull`)"""
        candP, candY, candS = self._empty_candidates(3 * self.Gm)
        pmark = cand["points"].clone()
        pmark[:, :, 2] = torch.where(cand["ok"], pmark[:, :, 2], 2.0)
        candP[idx[:, None], slot] = pmark
        candY[idx[:, None], slot] = cand["y"]
        candS[idx[:, None], slot] = cand["sec"]
        new, take, live = self._cull(candP, candY, candS, self.P)
        self.pts, self.arch_y, self.arch_sec, self.n = new["points"], new["y"], new["sec"], new["n"].clamp(max=self.P)   # (int32 already)
        if want_accepted:
            infront = torch.zeros((self.B, self.P + 3 * self.Gm), dtype=torch.bool, device=self.device)
            infront.scatter_(1, take, live[:, :, 0])
            return infront[idx[:, None], self.P + slot] & cand["ok"]

    def _replay_append(self, S, NSall, a_geo, a_topo, R, ok, accepted, K):
        """replay (D2): one row per pair with an accepted candidate.  Next state of agent a = its own candidate where that is feasible,
        else the first feasible one (D4): the rows are picked from the agent-major candidate tensors inside `add`, for the accepted
        pairs only."""
        first_ok = torch.argmax(ok.int(), dim=1)                                   # D4
        src = torch.where(ok, torch.arange(3, device=self.device)[None, :], first_ok[:, None])   # [K, 3]
        NSv = {k: NSall[k].view(3, K, *NSall[k].shape[1:]) for k in DeviceReplay.KEYS}
        ag = a_geo.view(3, K, -1, 2).permute(1, 0, 2, 3)
        at = a_topo.view(3, K, -1, 3).permute(1, 0, 2, 3)
        return self.replay.add(accepted.any(dim=1), S, NSv, ag, at, R.float(), src=src, **self._kw_add)

    def _cull(self, candP, candY, candS, max_front):
        """The torch cull: the front of the archive (P rows, dead rows marked infeasible) + C candidate slots, truncated to
        `max_front` (D3; 0: not at all), gathered in front order by framework operators.  Returns dict(points (objectives clipped to
        <= 1, :434-436), y, sec, n, hv, metrics), rows beyond n zero, and take [B, rows] / live [B, rows, 1]: the source row of
        every output row among the P + C, and whether there is one.  The archive itself is left to the caller."""
        B, P, dev = self.B, self.P, self.device
        total = P + candP.shape[1]
        arP = self._const("arP", lambda: torch.arange(P, device=dev))
        origp = torch.cat([self.pts, candP], dim=1)
        allp = origp.clone()
        allp[:, :P, 2] = torch.where(arP[None, :] >= self.n[:, None], 2.0, allp[:, :P, 2])      # infeasible marker
        fr = RW.front_hv(allp, self._const(f"rows{total}", lambda: torch.full((B,), total, dtype=torch.int32, device=dev)), None,
                         max_front=max_front, lib=self.lib)
        fidx = (fr["front_idx"][:, :max_front] if max_front else fr["front_idx"]).long()
        take, live = fidx.clamp(min=0), (fidx >= 0)[:, :, None]
        rows = self._const("rows", lambda: torch.arange(B, device=dev)[:, None])
        newp = torch.where(live, origp[rows, take], 0.0)
        newp[:, :, 0:2].clamp_(max=1.0)
        newy = torch.where(live, torch.cat([self.arch_y, candY], dim=1)[rows, take], 0.0)
        news = torch.where(live, torch.cat([self.arch_sec, candS], dim=1)[rows, take], 0)
        return dict(points=newp, y=newy, sec=news, n=fr["n_front"], hv=fr["hv_front"], metrics=fr["metrics"]), take, live

    def _design_cull(self, candP, candY, candS, final):
        """Design game: the ONE cull of a game step, over the archive (P rows, dead rows marked infeasible) + the step's 3 P
        candidate slots.  Truncated to max_front (D3) and written to the archive; at the final step not truncated (simple_cull_final,
        master…:424-428, 680): the archive is left as it was and `self.final` = dict(points [B, 4P, 4] (objectives clipped to <= 1
        like the archive's, :683-686), y [B, 4P, N], sec [B, 4P, E], n [B], hv [B], metrics [B, 5]), rows beyond n zero."""
        B, P = self.B, self.P
        if self.archive_path == "hip":          # one launch on the dense step-wide buffers: slot c of env b is row b 3P + c
            N, E = candY.shape[2], candS.shape[2]
            cand = (candP.view(B * 3 * P, 4), candY.view(B * 3 * P, N), candS.view(B * 3 * P, E))
            if not final:
                self._merge_archive(*cand, None, 3 * P, accepted=False)
                return None
            fr = RW.archive_merge(self.pts.contiguous(), self.n, self.arch_y.contiguous(), self.arch_sec.contiguous(), *cand, None, n_slots=3 * P,
                                  max_front=0, max_out=4 * P, accepted=False, extras=True, lib=self.lib)
            self.final = dict(points=fr["points"], y=fr["y"], sec=fr["sec"], n=fr["n"], hv=fr["hv_front"], metrics=fr["metrics"])
            return self.final
        new, _, _ = self._cull(candP, candY, candS, 0 if final else P)
        if final:
            self.final = new
            return new
        self.pts, self.arch_y, self.arch_sec, self.n = new["points"], new["y"], new["sec"], new["n"]

    def _merge_archive(self, cand_points, cand_y, cand_sec, slot_row, n_slots, accepted):
        """archive_path="hip": one `truss_archive_merge` launch from the current archive buffers into the spare set, truncated to
        max_front; the two sets then swap roles (the entry refuses to write over its inputs).  Returns accepted [B, n_slots] uint8
        (None unless asked for)."""
        P = self.P
        cur = dict(points=self.pts.contiguous(), y=self.arch_y.contiguous(), sec=self.arch_sec.contiguous(), n=self.n)
        if self._arch_spare is None:
            self._arch_spare = {k: torch.empty_like(v) for k, v in cur.items()}
        res = RW.archive_merge(cur["points"], cur["n"], cur["y"], cur["sec"], cand_points, cand_y, cand_sec, slot_row, n_slots=n_slots,
                               max_front=P, max_out=P, accepted=accepted, out=self._arch_spare, lib=self.lib)
        self.pts, self.arch_y, self.arch_sec, self.n = res["points"], res["y"], res["sec"], res["n"]
        self._arch_spare = cur
        return res.get("accepted")

    def design_episode(self, end_step: int = 500, explore: bool = True):
        """One episode of the design game (game="test") from the state `reset` left: game steps game_step .. end_step, the last
        one ending in the untruncated final cull.  Returns device tensors: hv [T, B] and n_front [T, B] per step (hyperS and
        numHV of master…:662-664; the last row is the final front's), R [B, 3] and G_U [B] summed over the episode (R0..R2, Gr of
        cal_success.py), and final = dict(points, y, sec, n, hv, metrics) (see _design_cull)."""
        if self.game != "test":
            raise ValueError("design_episode plays the design game: build the engine with game='test'")
        T = int(end_step) - self.game_step + 1
        if T < 1:
            raise ValueError(f"end_step {end_step} is before the current game step {self.game_step}")
        B, dev = self.B, self.device
        hv = torch.empty((T, B), dtype=torch.float64, device=dev)
        nf = torch.empty((T, B), dtype=torch.int32, device=dev)
        R = torch.zeros((B, 3), dtype=torch.float64, device=dev)
        G_U = torch.zeros((B,), dtype=torch.float64, device=dev)
        self.end_step = int(end_step)
        try:
            for t in range(T):
                o = self.game_step_all(train=False, explore=explore)
                hv[t], nf[t] = o["hv"], o["n_front"]
                R += o["reward"]
                G_U += o["G_U"]
        finally:
            self.end_step = None
        return dict(hv=hv, n_front=nf, R=R, G_U=G_U, final=self.final)

    def _const(self, name, make):
        """small constant device tensors of the game step (index ranges, fill patterns), made once"""
        c = self.__dict__.setdefault("_consts", {})
        if name not in c:
            c[name] = make()
        return c[name]

    def train_from_replay(self, train_iters: int = 1):
        """`train_iters` MADDPG updates on batches sampled from this engine's replay (when it holds a batch; collective
        decision under data parallelism).  Returns the number of updates run."""
        train = train_iters > 0
        ready = train and self.replay.size >= self.batch_size
        d = getattr(self.rl, "dist", None)
        if train and d is not None and d.is_initialized() and d.get_world_size() > 1:
            # data parallel: every rank plays its own envs and replay; the update is collective
            # (fused gradient all-reduce inside train_on_batch), so all ranks must agree to run it
            flag = torch.tensor([1 if ready else 0], device=self.device)
            d.all_reduce(flag, op=d.ReduceOp.MIN)
            ready = bool(flag.item())
        if ready:
            if not self._synced:
                with torch.no_grad():                                     # materialise lazy layers, then one broadcast
                    S, NS, ag, at, R = self.replay.sample(2, self.gen)
                    A = [(ag[:, a].contiguous(), at[:, a].contiguous()) for a in range(3)]
                    st = self._net_state(S)
                    self.rl._ensure_ready(st, [A[0][0], A[0][1], A[1][0], A[1][1], A[2][0], A[2][1]])
                self.rl.sync_parameters()
                self._synced = True
            for _ in range(train_iters):
                S, NS, ag, at, R = self.replay.sample(self.batch_size, self.gen)
                A = [(ag[:, a].contiguous(), at[:, a].contiguous()) for a in range(3)]
                self._train(self._net_state(S), [self._net_state(ns) for ns in NS], A, R)
            return train_iters
        return 0


class MixedMARL:
    """The batched rollout over a MIX of truss sizes with ONE set of agents (BASELINE configs[4]; the reference trains one
    MADDPG on a different truss every episode, master…:807-825; its GCN layers do not depend on the node count).

    One `BatchedMARL` engine per size class -- archives, env objects and replay have the class's shapes -- all sharing
    `maddpg`.  Envs are dealt to ranks in buckets like `MixedTrussPool` (pool.deal_buckets): every rank plays the same
    class mix.  A game step plays every class; the updates of the step then draw their batches from the classes'
    replays in turn (a batch is of one class: its tensors have that class's shapes).
    Tracking targets (`MADDPG(target_update=...)`) need nothing special here: each class's update is a `train_on_batch` call, so
    the targets move once per update of any class, counted by the one shared step counter of the critics' optimiser."""

    def __init__(self, classes, maddpg, *, bucket_envs=64, rank=0, world=1, **engine_kw):
        """engine_kw go to every class's BatchedMARL (game="test": every class brings its own symmetric topology; the coin's env
        field is the env's global id, `global_ids`, where class c's envs are numbered after those of classes 0..c-1)"""
        from .pool import deal_buckets
        self.classes = [(t, int(n)) for t, n in classes]
        self.share = deal_buckets([n for _, n in self.classes], bucket_envs, world)
        self.class_ids, self.ranges, self.engines = [], [], []
        for c, (topo, _) in enumerate(self.classes):
            n_local = sum(hi - lo for lo, hi in self.share[rank][c])
            if n_local:
                self.class_ids.append(c)
                self.ranges.append(self.share[rank][c])
                kw = dict(engine_kw)
                if kw.get("game", "train") == "test":
                    kw["env_ids"] = sum(n for _, n in self.classes[:c]) + self.global_ids(len(self.engines))
                self.engines.append(BatchedMARL(topo, n_local, maddpg, **kw))
        self.rl = maddpg
        self._turn = 0

    def global_ids(self, k):
        return np.concatenate([np.arange(lo, hi) for lo, hi in self.ranges[k]])

    @property
    def env_steps(self):
        return sum(e.env_steps for e in self.engines)

    def reset(self, per_class):
        """per_class[k]: dict(x, target, y_max, d_min, max_def, load_x, load_y, is_roof, y, sec) of this rank's k-th class"""
        for e, b in zip(self.engines, per_class):
            e.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])

    def design_episode(self, end_step: int = 500, explore: bool = True):
        """BatchedMARL.design_episode of every class (game="test"): per_class = their results; hv / n_front [T, B_local] and
        R / G_U concatenated over the classes in engine order"""
        outs = [e.design_episode(end_step=end_step, explore=explore) for e in self.engines]
        cat = lambda k, d: torch.cat([o[k] for o in outs], dim=d)
        return dict(per_class=outs, hv=cat("hv", 1), n_front=cat("n_front", 1), R=cat("R", 0), G_U=cat("G_U", 0))

    def game_step_all(self, train: bool | None = None, explore: bool = True, train_iters: int = 1):
        if train is None:
            train = self.engines[0].game != "test"
        outs = [e.game_step_all(train=train, explore=explore, update=False) for e in self.engines]
        done = 0
        if train:
            for _ in range(train_iters):                       # one class per update, in turn
                for _try in range(len(self.engines)):
                    e = self.engines[self._turn % len(self.engines)]
                    self._turn += 1
                    if e.train_from_replay(1):
                        done += 1
                        break
        return dict(per_class=outs, updates=done, hv=torch.cat([o["hv"] for o in outs]), n_front=torch.cat([o["n_front"] for o in outs]))
