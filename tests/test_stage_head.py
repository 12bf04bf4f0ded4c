"""Staging of the step kernels (phase 0: tables and input rows HBM -> LDS, band clear).  The HIP kernels issue the row loads of
the common fast path ahead of the phase schedule, behind one batch of kernel-argument loads (StepLane::stage_issue); the
generic path, the rollout kernels and the lane emulator stage inside phase_stage as before.  Results must not depend on
which of the two did the staging.

Every case runs through the lane emulator on the CPU and through the HIP library on the GPU: B = 5 (4 envs per workgroup:
the second workgroup has one live env and three clamped ones), 3 chained steps, each against the float64 oracle under
parity_common.compare_step's contract, the second with the caller's move ranges (mu_in / md_in); the analysis that precedes
them runs under TB_NO_DECODE with null action and coin pointers; one persistent rollout must equal the single steps bit for
bit.  On the GPU the exactly specified outputs (heights, sections, move ranges, tension flags, status) must also equal the
emulator's.

Topologies: the smallest trusses of the grid / benchmark families.  The fast path needs N % 4 == 0 and E % 4 == 0, and a
two-row truss of nx columns has N = 2 nx nodes: 4 columns give N = 8 and take the fast path without extra braces
(E = 16; one extra brace is all that 4 columns admit) and as the symmetric 'small' grid (coin used); 5 columns give
N = 10 and can only take the generic path, whatever the brace count (2 extra braces here, E = 23; the symmetric grid has
E = 21); the next fast size is 6 columns with 2 extra braces (N = 12, E = 28).  4 columns with one extra brace (E = 17)
take the generic path because of E alone.  Each runs with the kernel the topology would get (3 elements per lane, dense
band rows) and with TRUSS_EPL=5 (the padded rows of the metric configuration's kernel, the only one with the early issue).

What the CPU half covers: the emulator never calls stage_issue, so there phase_stage does the whole staging (stage_fast, the
generic path, the rollout's steps) -- the code every kernel without the early issue runs, the rollout kernels among them.
stage_issue and the pre_issued path of phase_stage are HIP-only (the step kernels of <16,8,1,5>) and are exercised by the
`gpu`-marked half alone (the single steps of the TRUSS_EPL=5 cases of the fast-path topologies)."""
import ctypes as C

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import synthetic
from oracle import truss_oracle as O
import parity_common as pc

B, STEPS = 5, 3
COIN = np.array([1, 0, 0, 1, 1], np.uint8)
KEYS = ("y", "sec", "point", "q0", "sr", "disp", "comp", "max_up", "max_down", "obj", "status")
EXACT = ("y", "sec", "comp", "max_up", "max_down", "status")        # compare_step asserts these bit for bit against the oracle

TOPOS = {   # name: (constructor, takes the fast path, symmetric)
    "c4": (lambda: synthetic.bench_topology(4, 0), True, False),
    "c4_sym": (lambda: tm.TrussTopology.grid(4, "small"), True, True),
    "c6_x2": (lambda: synthetic.bench_topology(6, 2), True, False),
    "c5_x2": (lambda: synthetic.bench_topology(5, 2), False, False),
    "c5_sym": (lambda: tm.TrussTopology.grid(5, "small"), False, True),
    "c4_x1": (lambda: synthetic.bench_topology(4, 1), False, False),
}
CASES = [(n, epl) for n in TOPOS for epl in (0, 5)]


def _hip():
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = tm.load()
    assert lib.backend == "hip"
    return lib


@pytest.fixture(scope="module", params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return pc.emu_lib() if request.param == "emu" else _hip()


class _Ref:
    """a topology's batch, actions and float64 oracle steps: computed once per module, shared by every test, never written"""

    def __init__(self, name):
        make, self.fast, self.sym = TOPOS[name]
        self.make = make
        topo = make()
        assert ((topo.N % 4 == 0 and topo.E % 4 == 0 and topo.N <= 64 and topo.E <= 128) == self.fast), (topo.N, topo.E)
        assert (topo.sym_nodes.shape[0] > 0) == self.sym
        seed = 500 + 7 * sorted(TOPOS).index(name)
        self.batch = b = synthetic.random_batch(topo, B, seed)
        self.ag, self.at = synthetic.random_actions(STEPS, B, topo.N, seed + 1)
        self.ot = ot = pc.oracle_topology(topo)
        load = pc.oracle_load(ot, b)
        self.int_obj = O.initial_objectives(ot, b["x"], b["y"], b["sec"], b["target"])
        self.steps, self.ranges = [], []
        y, sec = b["y"], b["sec"]
        for s in range(STEPS):
            mu = md = None
            if s == 1:       # the move ranges of the design the step starts from, as the step before left them (float32)
                mu, md = (np.asarray(self.steps[0][k], np.float32) for k in ("max_up", "max_down"))
            self.ranges.append((mu, md))
            o = O.env_step(ot, b["x"], y, sec, mu, md, self.ag[s], self.at[s], COIN.astype(np.float64), b["target"], load,
                           b["y_max"], b["d_min"], b["max_def"], b["is_roof"], self.int_obj)
            self.steps.append(o)
            y, sec = o["y"], o["sec"]


_refs = {}


def ref_of(name):
    if name not in _refs:
        _refs[name] = _Ref(name)
    return _refs[name]


def blob_units(lib, topo):
    """16-byte units per lane of the topology tables the kernel stages in front of the envs' LDS regions (an upper bound: the
    first env region begins behind them)"""
    info = np.zeros(16, np.int32)
    lib.check(lib.dll.truss_topo_lds_info(topo.native(lib), 0, info.ctypes.data_as(C.c_void_p), None, 0, None, 0), "truss_topo_lds_info")
    return -(-int(info[1]) // 1024)      # o_env0


def fresh_env(lib, r):
    """analysed env: the analysis is a TB_NO_DECODE launch without action rows and without a coin (null pointers)"""
    topo = r.make()
    env = pc.make_env(lib, topo, r.batch)
    env.analyze(set_normalisers=True)
    np.testing.assert_allclose(env.env_params[:, 5:7].cpu().numpy(), r.int_obj, rtol=0, atol=0)
    assert int(env.status.sum()) == 0
    return env, topo


def run_steps(lib, r):
    """the three single steps, each against the oracle; -> results per step"""
    env, topo = fresh_env(lib, r)
    if r.fast:
        assert blob_units(lib, topo) <= 3, "tables beyond the three units per lane of the early-issued path"
    dev = env.device
    coin = torch.tensor(COIN, device=dev)
    out = []
    for s in range(STEPS):
        mu, md = (None if v is None else torch.tensor(v, device=dev) for v in r.ranges[s])
        env.step(torch.tensor(r.ag[s], device=dev), torch.tensor(r.at[s], device=dev), coin, mu, md)
        res = {k: np.array(v) for k, v in env.results().items()}      # copies: on the CPU the results alias the env's buffers
        pc.compare_step(res, r.steps[s], r.ot)
        out.append(res)
    return out


@pytest.mark.parametrize("name,epl", CASES)
def test_steps_and_rollout(lib, monkeypatch, name, epl):
    if epl:
        monkeypatch.setenv("TRUSS_EPL", str(epl))
    r = ref_of(name)
    res = run_steps(lib, r)
    # the same three steps as one rollout call (the ranges passed in at step 1 are the ones the kernel computes itself)
    env, _ = fresh_env(lib, r)
    dev = env.device
    env.rollout(torch.tensor(r.ag, device=dev), torch.tensor(r.at, device=dev), STEPS, torch.tensor(COIN, device=dev))
    r2 = env.results()
    for k in KEYS:
        assert np.array_equal(res[-1][k], r2[k]), k
    if lib.backend == "hip":
        emu = pc.emu_lib()
        for a, b in zip(res, run_steps(emu, r)):
            for k in EXACT:
                assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["c4", "c5_x2"])
def test_null_optional_pointers(lib, monkeypatch, name):
    """No row is read through a pointer the launch does not use: a decoding step without a coin (NULL: the launch runs no mirror
    phase on a topology without mirror tables) gives the oracle's step.  (TB_NO_DECODE with a_geo = a_topo = coin = NULL is what
    every fresh_env of this file runs, on the topologies with mirror tables too.)"""
    monkeypatch.setenv("TRUSS_EPL", "5")
    r = ref_of(name)
    assert not r.sym
    env, _ = fresh_env(lib, r)
    dev = env.device
    nxt = env.cur ^ 1
    env._step_op(0, B, torch.tensor(r.ag[0], device=dev), torch.tensor(r.at[0], device=dev), None, None, None,
                 env.ybuf[env.cur], env.secbuf[env.cur], env.ybuf[nxt], env.secbuf[nxt])
    env.cur = nxt
    pc.compare_step(env.results(), r.steps[0], r.ot)
