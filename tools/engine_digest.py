#!/usr/bin/env python3
"""Diagnostic: SHA-256 digests of small games played by the batched engine, to compare one tree of this repository with another
(a refactor with its parent): the same digests = the same bits in the archives, the per-step results and the replay.

   tools/engine_digest.py TREE [--emu] [--update]

TREE    the checkout to import the engine from (its mop-truss-marl_amd/ and its built libraries)
--emu   play on the CPU lane emulator (TREE/tests/emu/libtruss_emu.so; defaults only: it has no fused / terms / group / reward /
        archive / pair entries); otherwise the native library on cuda, once per option combination
--update  one more line: the train game WITH MADDPG updates (digest over the networks' parameters too).  Library GEMM selection and
        the captured graph may make it differ between two runs of ONE tree: compare trees only if a tree agrees with itself.

Only the public engine API is used, so this file runs unchanged against either tree."""
import contextlib
import hashlib
import io
import os
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = {a for a in sys.argv[1:] if a.startswith("--")}
if len(args) != 1 or flags - {"--emu", "--update"}:
    sys.exit(__doc__)
TREE = os.path.abspath(args[0])
sys.path[:0] = [os.path.join(TREE, "mop-truss-marl_amd"), TREE]
import torch                                                   # noqa: E402
import truss_mi355 as tm                                       # noqa: E402
from truss_mi355 import marl, synthetic                        # noqa: E402
import master_DDPG_truss2D_MO as M                             # noqa: E402
import truss2D_RL as RL                                        # noqa: E402

EMU = "--emu" in flags
DEVICE = "cpu" if EMU else "cuda"
LIB = tm.load(os.path.join(TREE, "tests", "emu", "libtruss_emu.so")) if EMU else tm.load()
COMBINATIONS = {"defaults": {}} if EMU else {
    "defaults": {},
    "all-hip": dict(reward_path="hip", archive_path="hip", pair_path="hip", replay_storage="compact", actor_path="grouped"),
    "fused bf16x2": dict(actor_path="fused", actor_precision="bf16x2"),
}
HIDDEN = 40                                                    # above 32: the hidden layers are inside the split-weight envelope


def engine(topo, B, seed, **kw):
    torch.manual_seed(seed)
    rl = RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, HIDDEN, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=DEVICE)
    eng = marl.BatchedMARL(topo, B, rl, lib=LIB, device=DEVICE, seed=seed, tune_update_gemms=False, **kw)
    b = synthetic.random_batch(topo, B, seed)
    eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
    return eng


class Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, *values):
        for v in values:
            if isinstance(v, dict):
                self.add(*[v[k] for k in sorted(v)])
            elif isinstance(v, (list, tuple)):
                self.add(*v)
            elif torch.is_tensor(v):
                self.h.update(v.detach().cpu().contiguous().numpy().tobytes())
            else:
                self.h.update(repr(v).encode())

    def engine(self, eng):
        r = eng.replay
        self.add(eng.pts, eng.n, eng.arch_y, eng.arch_sec, eng.ref_points, r.size, r.head, r.S, r.NS, r.a_geo, r.a_topo, r.R)
        return f"{self.h.hexdigest()}  replay {r.size}, archive sizes {eng.n.tolist()}"


def train_game(update=False, **kw):
    """grid(6), 5 envs, max_front 20, pair_capacity 5 (the smallest: several chunks per step once the archives grow), 6 steps"""
    if update:
        kw = dict(kw, batch_size=8, replay_capacity=64)
    eng = engine(tm.TrussTopology.grid(6), 5, 3, max_front=20, pair_capacity=5, **kw)
    d = Digest()
    for _ in range(6):
        o = eng.game_step_all(train=True, update=update, explore=True)
        d.add(o["hv"], o["n_front"], o["reward"])
    if update:
        d.add([[p for p in net.parameters()] for ag in eng.rl.agents for net in (ag.actor_model, ag.critic_model)])
    return d.engine(eng)


def design_game(**kw):
    """grid(8, symmetry="small"), 3 envs, max_front 50, pair_capacity 3, an episode of 3 game steps"""
    eng = engine(tm.TrussTopology.grid(8, symmetry="small"), 3, 3, game="test", max_front=50, pair_capacity=3, **kw)
    o = eng.design_episode(end_step=3)
    d = Digest()
    d.add(o["hv"], o["n_front"], o["R"], o["G_U"], o["final"])
    return d.engine(eng)


with contextlib.redirect_stdout(io.StringIO()):
    lines = [(f"{game.__name__:11s} {name:13s}", game(**kw)) for name, kw in COMBINATIONS.items() for game in (train_game, design_game)]
    if "--update" in flags:
        lines.append((f"{'train_game':11s} {'with updates':13s}", train_game(update=True)))
for what, digest in lines:
    print(f"{'emu' if EMU else 'hip'}  {what}  {digest}")
