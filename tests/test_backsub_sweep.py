"""The column-sweep back substitution of the step kernel (truss_body.h: backsub_rows_adopt / backsub_step / backsub_share /
backsub_rebuild) at the shapes at which it can go wrong, not the workload's own.  Every case runs through the lane emulator on
the CPU and through the HIP library on the GPU, one or two wavefronts' worth of envs, analyze() only.

Criterion of every case: the float64 displacements and member forces (disp_f64, q0_f64) against oracle.fem_solve at the
contract's 1e-9, relative to the largest magnitude of the env's row, with status 0.

  * ndof < W: the three-bar truss (three pinned nodes, one free node: ndof = 2, the only block is partial and every cross-block
    term has to be zero), and a one-team truss whose ndof is no multiple of W (a partial top block above full blocks);
  * the two-team variants at every c = KA mod W, at the smallest grids that give each residue (derived below from the host's own
    report): the block switch inside the middle steps and the accumulators rebuilt after the hand-over to team B;
  * one topology per one-team variant, among them the W = 16 variant <16,16,1,5> and both RPL = 2 variants (two accumulators
    per lane);
  * EPB + 1 envs (EPB = 64 / G envs per wavefront): the partly filled last wavefront runs clamped duplicates;
  * ill-conditioned designs (the generator of test_step_status: sections as drawn, top nodes down to 1e-5 above their bottom
    nodes): the scaled residual  ||K d - P||inf / (||K||inf ||d||inf), in float64 on the host from the oracle's K, must not exceed
    4 x that of the per-row dot product this code replaced, on the same inputs.  The reordered sum has at most W terms: it can
    move the bound by a small constant, not by orders of magnitude.  The former code's values are recorded in PARENT_RESIDUAL
    (measured with the parent build: emulator here, HIP library on the MI355X; profiles/r15/README.md).
"""
import numpy as np
import pytest
import torch

import truss_mi355 as tm
from oracle import truss_oracle as O
import fem_reference as fr
import parity_common as pc
from test_solver_geometry import ONE_TEAM, TWO_TEAM, VARIANTS, _batch, element_range, force, vid
from test_step_status import ill_conditioned_batch

TIGHT = 1e-9


@pytest.fixture(scope="module", params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    if request.param == "emu":
        return pc.emu_lib()
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = tm.load()
    assert lib.backend == "hip"
    return lib


def row_rel(a, b):
    """per env: largest error of the row relative to the row's largest magnitude"""
    a = np.asarray(a, np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, np.float64).reshape(b.shape[0], -1)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-300)


def analyze_vs_oracle(lib, topo, batch):
    """analyze() of the batch; (results, the oracle's fem dict) after the module's criterion has been asserted"""
    ot = pc.oracle_topology(topo)
    fem = O.fem_solve(ot, batch["x"], batch["y"], batch["sec"], pc.oracle_load(ot, batch))
    env = pc.make_env(lib, topo, batch)
    env.analyze()
    r = env.results()
    assert not r["status"].any(), r["status"].tolist()
    ed, eq = row_rel(r["disp_f64"], fem["dnode"]), row_rel(r["q0_f64"], fem["q0"])
    print("[backsub] N=%d E=%d B=%d disp %.2e q0 %.2e" % (topo.N, topo.E, len(ed), ed.max(), eq.max()))
    assert ed.max() < TIGHT and eq.max() < TIGHT, (ed.tolist(), eq.tolist())
    return r, fem


def geometry(lib, topo, capfd, v):
    g = fr.solver_geometry(topo, lib, capfd)
    assert (g["G"], g["WL"], g["RPL"], g["EPL"]) == v, g
    return g


# ---- ndof < W and partial top blocks -----------------------------------------------------------------------------------------
def three_bar():
    """nodes 0, 1 (bottom) and 3 (top) pinned, node 2 (top) free, one bar from each pinned node to it: ndof = 2"""
    res = np.array([[1, 1], [1, 1], [0, 0], [1, 1]], np.uint8)
    return tm.TrussTopology(np.array([(0, 2), (1, 2), (3, 2)], np.int32), res, np.array([0, 0, 1, 1], np.uint8),
                            np.array([2, 3, 0, 1], np.int32))


@pytest.mark.parametrize("v", [None, (8, 8, 1, 5), (4, 4, 2, 20)], ids=lambda v: "host_choice" if v is None else vid(v))
def test_three_bar_truss(lib, capfd, monkeypatch, v):
    """the host's own choice for it (two teams with KA = 0: the middle block is the whole system) and two one-team variants"""
    if v is not None:
        force(monkeypatch, v)
    topo = three_bar()
    g = fr.solver_geometry(topo, lib, capfd)
    assert g["ndof"] == 2 and g["ndof"] < g["W"], g
    assert v is None or ((g["G"], g["WL"], g["RPL"]) == v[:3] and g["teams"] == 1), g
    batch = _batch(topo, 5, 11)
    batch["is_roof"][:] = 1.0                     # the free node is a top node: only the roof load reaches it
    analyze_vs_oracle(lib, topo, batch)
    topo.close()


@pytest.mark.parametrize("v", ONE_TEAM, ids=vid)
def test_one_team_partial_top_block(lib, capfd, monkeypatch, v):
    """every one-team variant (W = 8, 16, and 2 x 8, 2 x 4 with two rows per lane) at the smallest grid of its element range
    whose ndof is no multiple of W and spans more than one block; EPB + 1 envs: the second wavefront is partly filled"""
    force(monkeypatch, v)
    W = v[1] * v[2]
    lo, hi = element_range(v)
    topo = None
    for n in range(W + 1, 400):
        if n % W:
            try:
                topo = fr.grid_for(n, lo, hi)
                break
            except ValueError:
                continue
    assert topo is not None
    g = geometry(lib, topo, capfd, v)
    assert g["teams"] == 1 and g["ndof"] > W and g["ndof"] % W, g
    analyze_vs_oracle(lib, topo, _batch(topo, 64 // v[0] + 1, 20 + VARIANTS.index(v)))
    topo.close()


# ---- two teams: every c = KA mod W -------------------------------------------------------------------------------------------
def residue_topologies(v, lib, capfd):
    """{c: topology} for c = KA mod W of two-team variant v: supported grids of growing ndof inside the variant's element range
    until the host has reported every residue"""
    lo, hi = element_range(v)
    W = v[1] * v[2]
    found = {}
    for n in range(W + 1, 400):
        try:
            topo = fr.grid_for(n, lo, hi)
        except ValueError:
            continue
        g = geometry(lib, topo, capfd, v)
        assert g["teams"] == 2 and g["KA"] > 0, g
        if g["KA"] % W in found:
            topo.close()
            continue
        found[g["KA"] % W] = topo
        if len(found) == W:
            return found
    raise AssertionError("%s: residues %s only" % (vid(v), sorted(found)))


@pytest.mark.parametrize("v", TWO_TEAM, ids=vid)
def test_two_team_every_residue(lib, capfd, monkeypatch, v):
    force(monkeypatch, v)
    topos = residue_topologies(v, lib, capfd)
    assert sorted(topos) == list(range(v[1] * v[2]))
    for c, topo in sorted(topos.items()):
        analyze_vs_oracle(lib, topo, _batch(topo, 64 // v[0] + 1, 40 + c))       # EPB + 1 envs
        topo.close()


# ---- ill-conditioned designs: the residual against the per-row dot product's -------------------------------------------------
ILL_VARIANTS = [(16, 8, 1, 5), (16, 16, 1, 5), (16, 8, 2, 5), (4, 4, 2, 20)]
# largest scaled residual over the 9 envs with the parent's back substitution (per-row dot products, two partial sums), same
# inputs: backend -> variant -> value
PARENT_RESIDUAL = {
    "emu": {(16, 8, 1, 5): 1.7524e-16, (16, 16, 1, 5): 2.0909e-16, (16, 8, 2, 5): 1.3900e-16, (4, 4, 2, 20): 1.4669e-16},
    "hip": {(16, 8, 1, 5): 1.7524e-16, (16, 16, 1, 5): 2.0909e-16, (16, 8, 2, 5): 4.3084e-17, (4, 4, 2, 20): 1.2377e-16},
}
# the column sweeps, when this file was written: emu 8.60e-17, 1.12e-16, 1.39e-16, 9.32e-17; hip 8.60e-17, 1.12e-16, 6.95e-17, 9.32e-17


def scaled_residual(K, P, d):
    r = np.abs(np.einsum("bij,bj->bi", K, d) - P).max(axis=1)
    return r / (np.abs(K).sum(axis=2).max(axis=1) * np.abs(d).max(axis=1))


@pytest.mark.parametrize("v", ILL_VARIANTS, ids=vid)
def test_ill_conditioned_residual(lib, capfd, monkeypatch, v):
    from test_step_status import variant_topology
    topo = variant_topology(lib, capfd, monkeypatch, v)
    batch = ill_conditioned_batch(topo, 400 + VARIANTS.index(v))
    ot = pc.oracle_topology(topo)
    fem = O.fem_solve(ot, batch["x"], batch["y"], batch["sec"], pc.oracle_load(ot, batch))
    env = pc.make_env(lib, topo, batch)
    env.analyze()
    r = env.results()
    assert not r["status"].any(), r["status"].tolist()
    res = float(scaled_residual(fem["K"], fem["P"], fr.free_dofs(ot, r["disp_f64"])).max())
    parent = PARENT_RESIDUAL[lib.backend].get(v)
    print("[backsub residual] %s %s: %.3e (parent %s)" % (vid(v), lib.backend, res, parent))
    assert parent is not None, "no parent value recorded for this backend / variant"
    assert res <= 4 * parent, (res, parent)
