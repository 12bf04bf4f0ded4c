"""What truss_topo_create refuses, with which code and which text, and that a refusal leaves nothing behind.

Every input below reaches one failure exit of the topology builder (truss_host.h); inputs that are invalid in two ways
pin the order of the checks.  Nothing is launched for a refusal.  After each one a fresh grid(4) topology is built,
analysed and stepped once, and compared with the oracle (computed once per module).  Every case runs against the lane
emulator on the CPU and against the HIP library on the GPU."""
import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import synthetic
from oracle import truss_oracle as O
import parity_common as pc

PARALLEL = "two elements join the same pair of nodes (parallel members are not supported)"
NO_KERNEL = "no compiled kernel for half-bandwidth %d with %d elements (windows: 8, 16; up to 640 elements)"
B = 3


def _hip():
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = tm.load()
    assert lib.backend == "hip"
    return lib


@pytest.fixture(scope="module", params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return pc.emu_lib() if request.param == "emu" else _hip()


def grid4(parallel=False, restrained=False, bad_pair=False, bad_order=False, conn0=None):
    """TrussTopology.grid(4) (8 nodes, 16 elements) with the named defects"""
    g = tm.TrussTopology.grid(4)
    conn, res, pair, order = g.conn.copy(), g.res.copy(), g.pair.copy(), g.node_order.copy()
    if parallel:
        conn[1] = conn[0][::-1]
    if conn0 is not None:
        conn[0] = conn0
    if restrained:
        res[:] = 1
    if bad_pair:
        pair[0] = 0
    if bad_order:
        order = np.arange(g.N, dtype=np.int32)
        order[1] = 0
    return tm.TrussTopology(conn, res, g.top, pair, node_order=order)


def hub():
    """12 nodes: node 0 joins nine members, a chain runs through nodes 1..11; nodes 10 and 11 fully restrained"""
    conn = [(0, i) for i in range(1, 10)] + [(i, i + 1) for i in range(1, 11)]
    res = np.zeros((12, 2), np.uint8)
    res[10:] = 1
    return tm.TrussTopology(conn, res, np.zeros(12, np.uint8))


def lattice(n):
    """n x n square lattice (2 n (n - 1) members); node 0 pinned, node n - 1 on a y roller"""
    idx = np.arange(n * n).reshape(n, n)
    conn = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1)])
    res = np.zeros((n * n, 2), np.uint8)
    res[0] = 1
    res[n - 1, 1] = 1
    return tm.TrussTopology(conn, res, np.zeros(n * n, np.uint8))


def chain(n):
    """n nodes in a row; node 0 pinned, the last node on a y roller"""
    res = np.zeros((n, 2), np.uint8)
    res[0] = 1
    res[n - 1, 1] = 1
    return tm.TrussTopology([(i, i + 1) for i in range(n - 1)], res, np.zeros(n, np.uint8))


REFUSALS = {
    "parallel": (lambda: grid4(parallel=True), -2, PARALLEL),
    "conn_node_N": (lambda: grid4(conn0=[8, 1]), -1, "conn out of range"),
    "conn_same_node": (lambda: grid4(conn0=[1, 1]), -1, "conn out of range"),
    "no_free_dof": (lambda: grid4(restrained=True), -1, "no free DOF"),
    "pair_fixed_point": (lambda: grid4(bad_pair=True), -1, "pair[] must be an involution without fixed points"),
    "node_order": (lambda: grid4(bad_order=True), -1, "node_order is not a permutation"),
    "parallel_and_pair": (lambda: grid4(parallel=True, bad_pair=True), -2, PARALLEL),
    "parallel_and_no_free_dof": (lambda: grid4(parallel=True, restrained=True), -2, PARALLEL),
    "nine_members_at_a_node": (hub, -2, "a node joins more than 8 elements"),
    "lattice_10x10": (lambda: lattice(10), -2, NO_KERNEL % (21, 180)),
    "chain_700": (lambda: chain(700), -2, NO_KERNEL % (3, 699)),
}


class _Healthy:
    """grid(4): one batch, one set of actions and the oracle's step for them, computed once and left unchanged"""

    def __init__(self):
        topo = tm.TrussTopology.grid(4)
        self.batch = b = synthetic.random_batch(topo, B, 61)
        self.ag, self.at = synthetic.random_actions(1, B, topo.N, 62)
        self.ot = pc.oracle_topology(topo)
        load = pc.oracle_load(self.ot, b)
        int_obj = O.initial_objectives(self.ot, b["x"], b["y"], b["sec"], b["target"])
        self.step = O.env_step(self.ot, b["x"], b["y"], b["sec"], None, None, self.ag[0], self.at[0], np.zeros(B), b["target"],
                               load, b["y_max"], b["d_min"], b["max_def"], b["is_roof"], int_obj)

    def check(self, lib):
        """a fresh topology object (so truss_topo_create runs again): analysis, one step, against the oracle"""
        topo = tm.TrussTopology.grid(4)
        env = pc.make_env(lib, topo, self.batch)
        env.analyze(set_normalisers=True)
        env.step(torch.tensor(self.ag[0], device=env.device), torch.tensor(self.at[0], device=env.device))
        pc.compare_step(env.results(), self.step, self.ot)
        topo.close()


@pytest.fixture(scope="module")
def healthy():
    return _Healthy()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal(lib, healthy, name):
    build, code, message = REFUSALS[name]
    topo = build()
    with pytest.raises(tm.TrussError) as err:
        topo.native(lib)
    assert str(err.value) == "truss_topo_create failed (%d): %s" % (code, message)
    assert not topo._native
    healthy.check(lib)


def test_accepted_neighbour_of_the_lattice_refusal(lib):
    """the 6 x 6 lattice (36 nodes, 60 members) is inside the envelope that the 10 x 10 one leaves"""
    topo = lattice(6)
    nsc, tt, ndof = topo.dofs(lib)
    assert ndof == 2 * 36 - 3 and tt.shape == (60, 4)
    info = topo.solver_info(lib)
    assert sorted(info["perm"].tolist()) == list(range(ndof))
    assert info["half_bandwidth"] < 16
    topo.close()


def test_create_close_create(lib):
    """one topology object, created, closed and created again: the same DOF numbering and solver choice"""
    topo = tm.TrussTopology.grid(4)
    seen = []
    for _ in range(2):
        nsc, tt, ndof = topo.dofs(lib)
        info = topo.solver_info(lib)
        seen.append((nsc, tt, ndof, info))
        topo.close()
        assert not topo._native
    (nsc0, tt0, nd0, i0), (nsc1, tt1, nd1, i1) = seen
    assert nd0 == nd1 and np.array_equal(nsc0, nsc1) and np.array_equal(tt0, tt1)
    assert sorted(i0) == sorted(i1)
    for k in i0:
        assert np.array_equal(i0[k], i1[k]), k
