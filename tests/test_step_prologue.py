"""The step's prologue and its element phase: the symmetry coin (staged with the input rows, kept in LDS across a
persistent rollout, not read at all where no symmetry table uses it), lanes whose element index is clamped, and move
ranges passed in by the caller.  Every case runs through the lane emulator on the CPU and through the HIP library on
the GPU, with the helpers and tolerances of parity_common."""
import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import synthetic
from oracle import truss_oracle as O
import parity_common as pc

B = 6                                            # one full 4-env wave and one partly filled: the env index is clamped
COIN = np.array([0, 1, 1, 0, 1, 0], np.uint8)
KEYS = ("y", "sec", "point", "q0", "sr", "disp", "comp", "max_up", "max_down", "obj", "status")


def _hip():
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = tm.load()
    assert lib.backend == "hip"
    return lib


@pytest.fixture(scope="module", params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return pc.emu_lib() if request.param == "emu" else _hip()


def _smallest_symmetric():
    """the smallest grid with both mirror tables: from 4 columns on, 'small' mirrors an interior bottom node too"""
    for nx in range(2, 9):
        topo = tm.TrussTopology.grid(nx, "small")
        if topo.sym_nodes.shape[0] > nx // 2 and topo.sym_elems.shape[0] > 0:
            return topo
    raise AssertionError("no symmetric grid found")


class _Case:
    """one topology's batch, actions and oracle inputs, computed once per module and left unchanged"""

    def __init__(self, topo, seed, n_steps=1):
        self.topo = topo
        self.batch = synthetic.random_batch(topo, B, seed)
        self.ag, self.at = synthetic.random_actions(n_steps, B, topo.N, seed + 1)
        self.ot = pc.oracle_topology(topo)
        self.load = pc.oracle_load(self.ot, self.batch)
        b = self.batch
        self.int_obj = O.initial_objectives(self.ot, b["x"], b["y"], b["sec"], b["target"])

    def env(self, lib):
        e = pc.make_env(lib, self.topo, self.batch)
        e.analyze(set_normalisers=True)
        return e

    def oracle(self, y, sec, s, coin, mu=None, md=None):
        b = self.batch
        return O.env_step(self.ot, b["x"], y, sec, mu, md, self.ag[s], self.at[s], np.asarray(coin, np.float64), b["target"],
                          self.load, b["y_max"], b["d_min"], b["max_def"], b["is_roof"], self.int_obj)

    def tensors(self, env, s):
        return torch.tensor(self.ag[s], device=env.device), torch.tensor(self.at[s], device=env.device)


@pytest.fixture(scope="module")
def sym_case():
    return _Case(_smallest_symmetric(), seed=41, n_steps=3)


@pytest.fixture(scope="module")
def bench_case():
    topo = synthetic.bench_topology(4, 0)       # the benchmark family at its smallest size
    assert topo.sym_nodes.shape[0] == 0 and topo.sym_elems.shape[0] == 0
    return _Case(topo, seed=43)


def test_coin_is_honoured(lib, sym_case):
    """heads envs and tails envs, in the full wave and in the partly filled one, each match the oracle"""
    c = sym_case
    env = c.env(lib)
    g, t = c.tensors(env, 0)
    env.step(g, t, torch.tensor(COIN, device=env.device))
    o = c.oracle(c.batch["y"], c.batch["sec"], 0, COIN)
    pc.compare_step(env.results(), o, c.ot)
    # the coin decides: the same step with every coin flipped gives another design in at least one env
    o2 = c.oracle(c.batch["y"], c.batch["sec"], 0, 1 - COIN)
    assert not np.array_equal(o["y"], o2["y"])


def test_coin_is_kept_across_persistent_rollout(lib, sym_case):
    """three chained steps in one launch (the coin is staged by the first step only) = three single steps, bit for bit"""
    c = sym_case
    e1, e2 = c.env(lib), c.env(lib)
    assert e2.persistent_rollout
    coin = torch.tensor(COIN, device=e1.device)
    y, sec = c.batch["y"], c.batch["sec"]
    for s in range(3):
        g, t = c.tensors(e1, s)
        e1.step(g, t, coin)
        o = c.oracle(y, sec, s, COIN)
        y, sec = o["y"], o["sec"]
    pc.compare_step(e1.results(), o, c.ot)
    e2.rollout(torch.tensor(c.ag, device=e2.device), torch.tensor(c.at, device=e2.device), 3, coin)
    r1, r2 = e1.results(), e2.results()
    for k in KEYS:
        assert np.array_equal(r1[k], r2[k]), k


def test_coin_is_ignored_without_symmetry(lib, bench_case):
    """no mirror table: an all-ones coin and an all-zeros coin give the same bits"""
    c = bench_case
    res = []
    for v in (0, 1):
        env = c.env(lib)
        g, t = c.tensors(env, 0)
        env.step(g, t, torch.full((B,), v, dtype=torch.uint8, device=env.device))
        res.append(env.results())
    for k in KEYS + ("disp_f64", "q0_f64", "energy", "reactions"):
        assert np.array_equal(res[0][k], res[1][k]), k
    pc.compare_step(res[1], c.oracle(c.batch["y"], c.batch["sec"], 0, np.zeros(B)), c.ot)


@pytest.mark.parametrize("n_extra,E", [(0, 76), (4, 80)])
def test_clamped_element_lanes(lib, n_extra, E):
    """E = 76 on 16 lanes x 5 elements: lanes 12..15 redo element 75 in their last slot -- the volume objective must not
    count it twice, member forces and stress ratios must be those of the oracle; E = 80 fills every slot"""
    topo = synthetic.bench_topology(16, n_extra)
    assert topo.E == E
    c = _Case(topo, seed=47 + n_extra)
    env = c.env(lib)
    info = topo.solver_info(lib)
    assert info["lanes_per_env"] == 16
    g, t = c.tensors(env, 0)
    env.step(g, t)
    o = c.oracle(c.batch["y"], c.batch["sec"], 0, np.zeros(B))
    r = env.results()
    pc.compare_step(r, o, c.ot)
    np.testing.assert_allclose(r["obj"][:, 0], o["obj"][:, 0], rtol=3e-7, atol=0)      # volume (float32 sum of float32 terms)


def test_move_ranges_passed_in(lib, bench_case, sym_case):
    """max_up_in / max_down_in given = the oracle with the same ranges = the ranges the kernel computes from the same heights"""
    for c in (bench_case, sym_case):
        e0 = c.env(lib)                               # analyze() leaves the move ranges of the initial design
        r0 = e0.results()
        mu, md = r0["max_up"].astype(np.float32), r0["max_down"].astype(np.float32)
        coin = torch.tensor(COIN, device=e0.device)
        g, t = c.tensors(e0, 0)
        e0.step(g, t, coin)
        e1 = c.env(lib)
        e1.step(g, t, coin, torch.tensor(mu, device=e1.device), torch.tensor(md, device=e1.device))
        ra, rb = e0.results(), e1.results()
        for k in KEYS + ("disp_f64", "q0_f64"):
            assert np.array_equal(ra[k], rb[k]), k
        pc.compare_step(rb, c.oracle(c.batch["y"], c.batch["sec"], 0, COIN, mu, md), c.ot)
