"""Float64 / long-double references of the FEM solve in truss_step_kernel, for the test suite.

The kernel's float64 results are judged by criteria that do not depend on the condition number of the stiffness matrix:

    backward error     ||K d - P||_inf / (||K||_inf ||d||_inf + ||P||_inf)                 (d: the kernel's disp_f64)
    equilibrium error  ||sum_e q0_e (c, s, -c, -s) - P||_inf over the free DOFs,   same denominator   (q0: the kernel's q0_f64)
    reaction error     ||sum_e q0_e (c, s, -c, -s) - r||_inf over the restrained DOFs, same denominator (r: the kernel's reactions)

with K and P from oracle.fem_solve and every residual evaluated in long double.  A backward-stable LDL^T in float64 stays within
a small multiple of u = 2^-53 whatever kappa(K) is; a pivot reciprocal, an element length or a reaction sum in float32 does not.
The forward error is checked against `refined_solution` within C * kappa_inf(K) * u.

`supported_grid` builds the test topologies: the reference's two-row grid with other supports, so that the number of free DOFs
(and with it the two-team split KA = (ndof - W + 1) / 2 of truss_host.h) takes every residue.  `solver_geometry` reads what the
host chose from its own TRUSS_VERBOSE line instead of repeating its formulas.
"""
from __future__ import annotations

import os
import re

import numpy as np

import truss_mi355 as tm

U64 = 2.0 ** -53
LD = np.longdouble


def supported_grid(nx, right_roller=False, extra_rollers=0, extra_pins=0, prune=0):
    """The reference grid truss (`TrussTopology.grid`) with other supports: the right pin made a roller (x free), plus
    `extra_rollers` interior bottom nodes restrained in y and `extra_pins` interior bottom nodes restrained in x and y (every
    other interior node first); at least one interior bottom node stays free, so that a bridge load has somewhere to go.  `prune` removes the last
    '/' braces (every bay keeps its '\\' brace: still stable).  The column-by-column node order keeps the half-bandwidth at most 7:
    ndof = 4 nx - 4 + right_roller - extra_rollers - 2 extra_pins at E = 5 nx - 4 - prune."""
    g = tm.TrussTopology.grid(nx)
    nfix = extra_rollers + extra_pins
    if nfix > nx - 3 or prune > nx - 1:
        raise ValueError(f"grid({nx}): {nfix} interior supports / {prune} pruned braces is too many")
    res = g.res.copy()
    if right_roller:
        res[nx - 1] = [0, 1]
    nodes = (list(range(1, nx - 1, 2)) + list(range(2, nx - 1, 2)))[:nfix]     # every other interior node first
    for i, v in enumerate(nodes):
        res[v] = [1, 1] if i < extra_pins else [0, 1]
    conn = g.conn[: g.E - prune] if prune else g.conn
    return tm.TrussTopology(conn, res, g.top, g.pair, node_order=g.node_order)


def grids_for(ndof, e_lo, e_hi, n_mult4=True):
    """Every `supported_grid` with exactly `ndof` free DOFs and e_lo < E <= e_hi (N a multiple of 4 with n_mult4: the fused
    observation writer and the persistent rollout need it): smaller grids first, then fewer pruned braces, then fewer extra
    supports."""
    for nx in range(4, 400):
        if n_mult4 and nx % 2:
            continue
        full = 5 * nx - 4
        for prune in range(max(0, full - e_hi), min(nx - 1, full - e_lo - 1) + 1):
            for nfix in range(0, nx - 2):
                for pins in range(0, nfix + 1):
                    for r in (1, 0):
                        if 4 * nx - 4 + r - (nfix - pins) - 2 * pins == ndof:
                            yield supported_grid(nx, bool(r), nfix - pins, pins, prune)
        if 2 * nx + 2 > ndof or full - (nx - 1) > e_hi:       # the fewest DOF / elements of this and every larger grid:
            return                                            # either one past its limit ends the search


def grid_for(ndof, e_lo, e_hi, n_mult4=True):
    """the first of grids_for()"""
    for t in grids_for(ndof, e_lo, e_hi, n_mult4):
        return t
    raise ValueError(f"no supported grid with {ndof} DOF and {e_lo} < E <= {e_hi}")


_GEOM = re.compile(r"\[truss_mi355\] N=(\d+) E=(\d+) ndof=(\d+) bw=(\d+) \| G=(\d+) WL=(\d+) RPL=(\d+) EPL=(\d+) "
                   r"teams=(\d+) KA=(\d+) mid=(\d+) \|.*fused observation writer (yes|no)")


def parse_geometry(text):
    """every `[truss_mi355] N= ...` line of truss_topo_create's TRUSS_VERBOSE output -> list of dicts"""
    keys = ("N", "E", "ndof", "bw", "G", "WL", "RPL", "EPL", "teams", "KA", "mid")
    out = []
    for m in _GEOM.finditer(text):
        d = dict(zip(keys, map(int, m.groups()[:11])))
        d["emit"] = m.group(12) == "yes"
        d["W"] = d["WL"] * d["RPL"]
        out.append(d)
    return out


def solver_geometry(topo, lib, capfd):
    """Create the native topology with TRUSS_VERBOSE=1 and return what the host printed about the solver it chose:
    N, E, ndof, bw, G, WL, RPL, EPL, teams, KA, mid, W, emit.  The TRUSS_LANES / TRUSS_WLANES / TRUSS_RPL overrides in force
    apply.  The handle stays cached in `topo`, so the env built next uses exactly this instance."""
    dev = None
    if lib.backend == "hip":
        import torch
        dev = torch.cuda.current_device()
    assert (lib.path, dev) not in topo._native, "solver_geometry() must create the native topology itself"
    capfd.readouterr()
    old = os.environ.get("TRUSS_VERBOSE")
    os.environ["TRUSS_VERBOSE"] = "1"
    try:
        topo.native(lib, dev)
    finally:
        if old is None:
            del os.environ["TRUSS_VERBOSE"]
        else:
            os.environ["TRUSS_VERBOSE"] = old
    _, err = capfd.readouterr()
    geo = parse_geometry(err)
    assert len(geo) == 1, err
    g = geo[0]
    assert (g["N"], g["E"]) == (topo.N, topo.E)
    return g


# ---- solver criteria ------------------------------------------------------------------------------------------------------
def free_dofs(otopo, disp):
    """[B, N, 2] nodal displacements -> [B, ndof] in the reference's DOF order (through nsc)"""
    flat = np.asarray(disp, np.float64).reshape(disp.shape[0], -1)
    d = np.zeros((flat.shape[0], otopo.ndof))
    free = otopo.nsc <= otopo.ndof
    d[:, otopo.nsc[free] - 1] = flat[:, free]
    return d


def error_scale(K, P, d):
    """||K||_inf ||d||_inf + ||P||_inf per env: the denominator of every solver criterion"""
    nK = np.abs(K).sum(axis=2).max(axis=1)
    return nK * np.abs(d).max(axis=1) + np.abs(P).max(axis=1)


def backward_error(K, P, d):
    """||K d - P||_inf / (||K||_inf ||d||_inf + ||P||_inf) per env, the residual in long double"""
    res = np.einsum("bij,bj->bi", K.astype(LD), d.astype(LD)) - P.astype(LD)
    return (np.abs(res).max(axis=1) / error_scale(K, P, d)).astype(np.float64)


def refined_solution(K, P, iters=3):
    """np.linalg.solve plus `iters` steps of iterative refinement with the residual in long double"""
    d = np.linalg.solve(K, P[:, :, None])[:, :, 0]
    Kl = K.astype(LD)
    for _ in range(iters):
        r = (P.astype(LD) - np.einsum("bij,bj->bi", Kl, d.astype(LD))).astype(np.float64)
        d = d + np.linalg.solve(K, r[:, :, None])[:, :, 0]
    return d


def cond_inf(K):
    return np.array([np.linalg.cond(k, np.inf) for k in K])


def forward_error(d, d_ref):
    return np.abs(d - d_ref).max(axis=1) / np.abs(d_ref).max(axis=1)


def member_end_forces(otopo, x, y, q0):
    """sum over the members of q0_e (c, s, -c, -s) at each of the 2N DOFs (reference numbering, 0-based), in long double;
    c, s from float32 heights as oracle.element_geometry"""
    xl = np.asarray(x, np.float64).astype(LD)
    yl = np.asarray(y, np.float32).astype(np.float64).astype(LD)
    a, b = otopo.conn[:, 0], otopo.conn[:, 1]
    dx, dy = xl[:, b] - xl[:, a], yl[:, b] - yl[:, a]
    L = np.sqrt(dx * dx + dy * dy)
    c, s = dx / L, dy / L
    q = np.asarray(q0, np.float64).astype(LD)
    f = np.stack([q * c, q * s, -q * c, -q * s], axis=-1)           # [B, E, 4]
    F = np.zeros((f.shape[0], 2 * otopo.N), LD)
    for j in range(4):
        np.add.at(F, (slice(None), otopo.ttnsc[:, j] - 1), f[:, :, j])
    return F


def equilibrium_error(otopo, x, y, q0, load, scale):
    """||sum of member end forces - applied load||_inf over the free DOFs / scale (error_scale), per env"""
    from oracle import truss_oracle as O
    F = member_end_forces(otopo, x, y, q0)[:, : otopo.ndof]
    P = O.load_vector(otopo, load).astype(LD)
    return (np.abs(F - P).max(axis=1) / scale).astype(np.float64)


def reaction_error(otopo, x, y, q0, reactions, scale):
    """||sum of member end forces - reactions||_inf over the restrained DOFs / scale, per env (reactions: the kernel's, in
    the reference's order of the restrained DOFs)"""
    nr = 2 * otopo.N - otopo.ndof
    F = member_end_forces(otopo, x, y, q0)[:, otopo.ndof:]
    r = np.asarray(reactions, np.float64)[:, :nr].astype(LD)
    return (np.abs(F - r).max(axis=1) / scale).astype(np.float64)


def reaction_balance(otopo, reactions, load, scale):
    """|sum rx + sum load_x| and |sum ry + sum load_y| / scale per env ([B, 2]): the reactions balance the applied load"""
    nr = 2 * otopo.N - otopo.ndof
    r = np.asarray(reactions, np.float64)[:, :nr].astype(LD)
    load = np.asarray(load, np.float64).astype(LD)
    flat_of = np.argsort(otopo.nsc - 1)                        # DOF id (0-based) -> node * 2 + axis
    axis = flat_of[np.arange(otopo.ndof, 2 * otopo.N)] % 2     # axis of every restrained DOF, in reaction order
    tot = [r[:, axis == ax].sum(axis=1) + load[:, :, ax].sum(axis=1) for ax in (0, 1)]
    return (np.abs(np.stack(tot, axis=1)) / scale[:, None]).astype(np.float64)
