"""Every solver instance of the step kernel against float64 / long-double references (tests/fem_reference.py).

truss_host.h splits the banded LDL^T of an env between two teams of lanes for every variant with G / WL >= 2 and RPL == 1:
KA = (ndof - W + 1) / 2 rows from each end, `mid` = ndof - 2 KA in the middle.  truss_body.h compiles a separate merge /
hand-over region for every c = KA mod W, and only the one matching the topology runs.  The one-team variants pad ndof to a
multiple of W.  The sweeps below build `supported_grid` topologies (other supports -> any ndof at a chosen element count) so that
every (c, mid) pair of every two-team variant and every ndof mod W residue of every one-team variant runs, in the plain step,
the fused-observation (EMIT) step and the persistent rollout.  Coverage is asserted from what the host reports about its own
choice (TRUSS_VERBOSE), not from a copy of its formulas.

Criteria per case (ragged batch, bridge and roof, load_x != 0 in about half the envs, two chained steps, outputs NaN-filled
before the checked step): strict compare_step against the oracle, backward error, equilibrium and reaction errors <= TAU,
reactions that balance the load, status 0, a second env bitwise equal, the persistent rollout bitwise equal to the steps.

Measured on the MI355X (pivot reciprocals by v_rcp_f64 + two Newton steps), largest over every variant, sweep case and env:
backward error 2.3e-16, equilibrium error 2.2e-16 (both at most 2.1 u), reaction error 2.6e-17, load balance 4.5e-16, and on the
80 / 128 / 256-node grids a forward error of at most 0.067 kappa_inf(K) u.  The emulator (exact 1 / d) stays below the same
values.  TAU = 16 u (1.8e-15) keeps a margin of 4x or more over every measured maximum; the float32 mutants below miss it by
1e5 or more.
"""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import synthetic
from oracle import truss_oracle as O
from conftest import ROOT
import fem_reference as fr
import parity_common as pc

TAU = 16 * fr.U64
NAN_FILLED = ("disp", "q0", "sr", "point", "energy", "reactions", "disp_f64", "q0_f64")
ROLLOUT_KEYS = ("y", "sec", "point", "q0", "sr", "disp", "comp", "max_up", "max_down", "obj", "status")


def _compiled(name):
    """(G, WL, RPL, EPL) list of a variant macro of truss_host.h (the full build, not the diagnostic one)"""
    txt = open(os.path.join(ROOT, "mop-truss-marl_amd", "csrc", "truss_host.h")).read()
    for m in re.finditer(r"#define %s\(X\)((?:[^\n]*\\\n)*[^\n]*)" % name, txt):
        v = [tuple(map(int, t)) for t in re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", m.group(1))]
        if v:
            return v
    raise AssertionError(f"{name} not found in truss_host.h")


VARIANTS = _compiled("TRUSS_VARIANTS")
ROLLOUT = set(_compiled("TRUSS_ROLLOUT_VARIANTS"))
EMIT = set(_compiled("TRUSS_EMIT_VARIANTS"))
TWO_TEAM = [v for v in VARIANTS if v[0] // v[1] >= 2 and v[2] == 1]
ONE_TEAM = [v for v in VARIANTS if v not in TWO_TEAM]
vid = lambda v: "G%d_WL%d_RPL%d_EPL%d" % v


def element_range(v):
    """(lo, hi]: the element counts for which the host picks variant v once its G / WL / RPL are forced"""
    G, WL, RPL, EPL = v
    smaller = [e for (g, wl, r, e) in VARIANTS if (g, wl, r) == (G, WL, RPL) and e < EPL]
    return (G * max(smaller) if smaller else 0), G * EPL


def force(monkeypatch, v):
    monkeypatch.setenv("TRUSS_LANES", str(v[0]))
    monkeypatch.setenv("TRUSS_WLANES", str(v[1]))
    monkeypatch.setenv("TRUSS_RPL", str(v[2]))


def sweep_topologies(v):
    """one supported grid per (KA mod 8, mid) pair (two teams: ndof = 2 KA + mid over 8 consecutive KA) or per ndof mod W
    (one team), all with N a multiple of 4, at the smallest sizes the element range of v allows"""
    lo, hi = element_range(v)
    W = v[1] * v[2]
    for start in range(W + 1, 400):
        if v in TWO_TEAM:
            if start % 2 == 0:                       # odd start: ndof = 2 KA + 7 for KA = (start - 7) / 2 ...
                continue
            window = range(start, start + 2 * W)
        else:
            window = range(start, start + W)
        try:
            return [fr.grid_for(n, lo, hi) for n in window]
        except ValueError:
            continue
    raise AssertionError(f"no sweep topologies for {v}")


def _batch(topo, B, seed):
    b = synthetic.random_batch(topo, B, seed)
    rng = np.random.default_rng(seed + 7)
    b["is_roof"] = (np.arange(B) % 2).astype(np.float64)
    b["load_x"] = np.where(rng.random(B) < 0.5, rng.uniform(-0.6, 0.6, B) * np.abs(b["load_y"]), 0.0)
    b["load_x"][0], b["load_x"][1 % B] = 0.0, 0.5 * abs(b["load_y"][1 % B])       # both kinds in every batch
    return b


def solver_errors(otopo, x, o, r, load):
    """backward / equilibrium / reaction / balance errors (per env) of native results r for oracle step o"""
    K, P = o["fem"]["K"], o["fem"]["P"]
    d = fr.free_dofs(otopo, r["disp_f64"])
    scale = fr.error_scale(K, P, d)
    return dict(backward=fr.backward_error(K, P, d),
                equilibrium=fr.equilibrium_error(otopo, x, o["y"], r["q0_f64"], load, scale),
                reaction=fr.reaction_error(otopo, x, o["y"], r["q0_f64"], r["reactions"], scale),
                balance=fr.reaction_balance(otopo, r["reactions"], load, scale).max(axis=1))


def assert_criteria(err, what):
    for k in ("backward", "equilibrium", "reaction", "balance"):
        assert float(err[k].max()) <= TAU, (what, k, float(err[k].max()))
    if "forward" in err:
        assert float(err["forward"].max()) <= 1.0, (what, "forward / (kappa u)", float(err["forward"].max()))


def check_case(lib, topo, B, seed, rollout):
    """two chained steps of a ragged batch vs the oracle and the float64 criteria; a second env must be bitwise equal; with
    rollout the persistent rollout of the same steps too.  Returns the criteria's maxima."""
    batch = _batch(topo, B, seed)
    ot = pc.oracle_topology(topo)
    load = pc.oracle_load(ot, batch)
    envs = [pc.make_env(lib, topo, batch) for _ in range(3 if rollout else 2)]
    for e in envs:
        e.analyze(set_normalisers=True)
    int_obj = O.initial_objectives(ot, batch["x"], batch["y"], batch["sec"], batch["target"])
    ag, at = synthetic.random_actions(2, B, topo.N, seed + 1)
    dev = envs[0].device
    G, T = torch.tensor(ag, device=dev), torch.tensor(at, device=dev)
    y, sec = batch["y"], batch["sec"]
    for s in range(2):
        if s == 1:
            for e in envs[:2]:
                for k in NAN_FILLED:
                    getattr(e, k).fill_(float("nan"))
        for e in envs[:2]:
            e.step(G[s], T[s])
        o = O.env_step(ot, batch["x"], y, sec, None, None, ag[s], at[s], np.zeros(B), batch["target"], load,
                       batch["y_max"], batch["d_min"], batch["max_def"], batch["is_roof"], int_obj)
        r = envs[0].results()
        pc.compare_step(r, o, ot)
        y, sec = o["y"], o["sec"]
    for k in NAN_FILLED:
        assert np.isfinite(r[k]).all(), k
    assert not r["status"].any()
    err = solver_errors(ot, batch["x"], o, r, load)
    assert_criteria(err, (topo.N, topo.E))
    r2 = envs[1].results()
    for k in r:
        assert np.array_equal(r[k], r2[k]), ("not deterministic", k)
    if rollout:
        e3 = envs[2]
        assert e3.persistent_rollout
        e3.rollout(G, T, 2)
        r3 = e3.results()
        for k in ROLLOUT_KEYS:
            assert np.array_equal(r[k], r3[k]), ("rollout", k)
    return {k: float(v.max()) for k, v in err.items()}


def run_sweep(lib, capfd, monkeypatch, v, B, report):
    """every topology of sweep_topologies(v) through check_case; the host's own report must show variant v and the full set of
    (KA mod 8, mid) pairs (two teams) / ndof mod W residues (one team)"""
    force(monkeypatch, v)
    W = v[1] * v[2]
    seen, worst = set(), {}
    for i, topo in enumerate(sweep_topologies(v)):
        g = fr.solver_geometry(topo, lib, capfd)
        assert (g["G"], g["WL"], g["RPL"], g["EPL"]) == v and g["bw"] < g["W"], g
        if v in TWO_TEAM:
            assert g["teams"] == 2 and g["KA"] > 0, g
            seen.add((g["KA"] % 8, g["mid"]))
        else:
            assert g["teams"] == 1, g
            seen.add(g["ndof"] % W)
        err = check_case(lib, topo, B, 100 + i, rollout=v in ROLLOUT)
        worst = {k: max(worst.get(k, 0.0), e) for k, e in err.items()}
        topo.close()
    if v in TWO_TEAM:
        assert seen == {(c, m) for c in range(8) for m in (7, 8)}, sorted(seen)
    else:
        assert seen == set(range(W)), sorted(seen)
    report(vid(v), worst)


def emit_topologies(v, lib, capfd):
    """as sweep_topologies for the fused observation writer: whether its tables fit the LDS depends on the layout, so each ndof
    takes the first supported grid for which the host reports the writer, and the window moves up until every ndof has one.
    Returns [(topology, host report)]."""
    lo, hi = element_range(v)
    W = v[1] * v[2]
    found = {}

    def emitting(n):
        if n not in found:
            found[n] = None
            for topo in itertools.islice(fr.grids_for(n, lo, hi), 40):
                g = fr.solver_geometry(topo, lib, capfd)
                if g["emit"]:
                    found[n] = (topo, g)
                    break
                topo.close()
        return found[n]

    for start in range(W + 1, 200):
        if v in TWO_TEAM and start % 2 == 0:
            continue
        window = range(start, start + (2 * W if v in TWO_TEAM else W))
        if all(emitting(n) for n in window):
            for n, tg in found.items():
                if tg and n not in window:
                    tg[0].close()
            return [found[n] for n in window]
    raise AssertionError(f"{vid(v)}: no window of supported grids gets the fused observation writer")


def run_emit_sweep(lib, capfd, monkeypatch, v, B):
    """every (KA mod 8, mid) pair / ndof mod W residue through run_obs_random(fused=True): the observation buffers start as
    NaN and the step's own launch fills them; against the oracle and the stand-alone observation kernel"""
    force(monkeypatch, v)
    W = v[1] * v[2]
    seen = set()
    for i, (topo, g) in enumerate(emit_topologies(v, lib, capfd)):
        assert (g["G"], g["WL"], g["RPL"], g["EPL"]) == v, g
        seen.add((g["KA"] % 8, g["mid"]) if v in TWO_TEAM else g["ndof"] % W)
        env = pc.run_obs_random(lib, 0, 0, B, seed=200 + i, fused=True, expect_one_launch=True, topo=topo)
        assert env.fused_obs
        topo.close()
    assert seen == ({(c, m) for c in range(8) for m in (7, 8)} if v in TWO_TEAM else set(range(W))), sorted(seen)


@pytest.fixture(scope="module")
def emu():
    return pc.emu_lib()


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lib = tm.load()
    assert lib.backend == "hip"
    return lib


@pytest.fixture(scope="module")
def report():
    """maxima of the criteria per variant, printed at the end of the module (pytest -s) for the record"""
    rows = {}
    yield lambda name, worst: rows.__setitem__(name, worst)
    for name, w in sorted(rows.items()):
        print("[solver criteria] %-22s " % name + " ".join("%s %.2e" % kv for kv in sorted(w.items())))


# ---- host-side checks ----------------------------------------------------------------------------------------------------
def test_variant_lists_and_split():
    """The sweeps are parametrized from the variant lists of truss_host.h, so a variant added there joins them; the parse found
    the lists and the two-team variants the kernel has today."""
    assert ROLLOUT <= set(VARIANTS) and EMIT <= set(VARIANTS)
    assert {(16, 8, 1, 3), (16, 8, 1, 5), (32, 8, 1, 3), (32, 8, 1, 10), (64, 8, 1, 10)} <= set(TWO_TEAM)


def test_no_two_team_wide_window(emu, capfd, monkeypatch):
    """No compiled variant reaches the guarded `nteams == 2 && W_ > 8` branch of truss_body.h: every variant is forced through
    the overrides and the host's report checked (and its team count matches the TWO_TEAM split the sweeps use).  If the list
    ever gains a two-team variant with a window wider than 8, this test fails and the merge sweep must grow with it."""
    for v in VARIANTS:
        force(monkeypatch, v)
        topo = sweep_topologies(v)[0]
        g = fr.solver_geometry(topo, emu, capfd)
        assert (g["G"], g["WL"], g["RPL"], g["EPL"]) == v, (v, g)
        assert g["teams"] == (2 if v in TWO_TEAM else 1), (v, g)
        assert not (g["teams"] == 2 and g["W"] > 8), (v, g)
        topo.close()


def test_supported_grid_dofs(emu):
    """ndof = 4 nx - 4 + roller - rollers - 2 pins, E = 5 nx - 4 - prune, half-bandwidth at most 7, same DOF numbering as the oracle"""
    for nx, r, k, p, prune in [(6, 1, 0, 0, 0), (8, 0, 3, 0, 2), (10, 1, 2, 3, 5), (12, 0, 0, 4, 0)]:
        t = fr.supported_grid(nx, bool(r), k, p, prune)
        nsc, tt, nd = t.dofs(emu)
        ot = pc.oracle_topology(t)
        assert nd == 4 * nx - 4 + r - k - 2 * p == ot.ndof and t.E == 5 * nx - 4 - prune
        assert np.array_equal(nsc, ot.nsc) and np.array_equal(tt, ot.ttnsc)
        assert t.solver_info(emu)["half_bandwidth"] <= 7
        t.close()


# ---- 1 + 4: merge sweep of the two-team variants (step, determinism, persistent rollout) ----------------------------------
@pytest.mark.parametrize("v", TWO_TEAM, ids=vid)
def test_merge_sweep_emulated(emu, capfd, monkeypatch, report, v):
    run_sweep(emu, capfd, monkeypatch, v, 5, report)


@pytest.mark.gpu
@pytest.mark.parametrize("v", TWO_TEAM, ids=vid)
def test_merge_sweep_hip(hip, capfd, monkeypatch, report, v):
    run_sweep(hip, capfd, monkeypatch, v, 23, report)


# ---- 2 (+ 4): padding sweep of the one-team variants -----------------------------------------------------------------------
@pytest.mark.parametrize("v", ONE_TEAM, ids=vid)
def test_padding_sweep_emulated(emu, capfd, monkeypatch, report, v):
    run_sweep(emu, capfd, monkeypatch, v, 3, report)


@pytest.mark.gpu
@pytest.mark.parametrize("v", ONE_TEAM, ids=vid)
def test_padding_sweep_hip(hip, capfd, monkeypatch, report, v):
    run_sweep(hip, capfd, monkeypatch, v, 23, report)


# ---- 3: fused observation over the sweep -----------------------------------------------------------------------------------
@pytest.mark.parametrize("v", sorted(EMIT), ids=vid)
def test_fused_observation_sweep_emulated(emu, capfd, monkeypatch, v):
    run_emit_sweep(emu, capfd, monkeypatch, v, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("v", sorted(EMIT), ids=vid)
def test_fused_observation_sweep_hip(hip, capfd, monkeypatch, v):
    run_emit_sweep(hip, capfd, monkeypatch, v, 23)


# ---- 5: large trusses by backward error ------------------------------------------------------------------------------------
def check_large(lib, num_x, B, tight):
    """the run of test_large_trusses (its inputs, its oracle comparison at `tight`), then the float64 criteria on the final
    design and the forward error against the refined solution in units of kappa_inf(K) u"""
    topo = tm.TrussTopology.grid(num_x)
    env = pc.run_random_rollout(lib, 0, 0, B, 2, seed=num_x, topo=topo, tight=tight)
    r = env.results()
    batch = synthetic.random_batch(topo, B, num_x)
    ot = pc.oracle_topology(topo)
    load = pc.oracle_load(ot, batch)
    fem = O.fem_solve(ot, batch["x"], r["y"], r["sec"], load)
    err = solver_errors(ot, batch["x"], dict(y=r["y"], fem=fem), r, load)
    K, P = fem["K"], fem["P"]
    err["forward"] = fr.forward_error(fr.free_dofs(ot, r["disp_f64"]), fr.refined_solution(K, P)) / (fr.cond_inf(K) * fr.U64)
    assert_criteria(err, num_x)
    return {k: float(v.max()) for k, v in err.items()}


@pytest.mark.parametrize("num_x,tight", [(40, 1e-9), (64, 1e-9), (128, 1e-7)])
def test_large_truss_criteria_emulated(emu, report, num_x, tight):
    """80 / 128 / 256 nodes (kappa_inf(K) up to ~3e9): the oracle comparison of test_large_trusses has to allow for the
    condition number, the backward, equilibrium and reaction errors do not; the forward error stays within kappa u"""
    report("grid(%d)" % num_x, check_large(emu, num_x, 2, tight))


@pytest.mark.gpu
@pytest.mark.parametrize("num_x,tight", [(40, 1e-9), (64, 1e-9), (128, 1e-7)])
def test_large_truss_criteria_hip(hip, report, num_x, tight):
    report("grid(%d)" % num_x, check_large(hip, num_x, 24, tight))


# ---- mutants: the criteria catch a float32 step in the solver --------------------------------------------------------------
# mutant -> (criterion it must break, whether the old oracle comparison -- compare_step at 1e-7 on 256 nodes, as
# test_large_trusses -- let it through)
MUTANTS = {1: ("backward", False), 2: ("backward", False), 3: ("reaction", False)}


def _mutant_run(lib, topo, B, seed, tight):
    """one step: (criteria per env, whether compare_step at `tight` passes)"""
    batch = _batch(topo, B, seed)
    ot = pc.oracle_topology(topo)
    load = pc.oracle_load(ot, batch)
    env = pc.make_env(lib, topo, batch)
    env.analyze(set_normalisers=True)
    int_obj = O.initial_objectives(ot, batch["x"], batch["y"], batch["sec"], batch["target"])
    ag, at = synthetic.random_actions(1, B, topo.N, seed + 1)
    env.step(torch.tensor(ag[0]), torch.tensor(at[0]))
    o = O.env_step(ot, batch["x"], batch["y"], batch["sec"], None, None, ag[0], at[0], np.zeros(B), batch["target"], load,
                   batch["y_max"], batch["d_min"], batch["max_def"], batch["is_roof"], int_obj)
    r = env.results()
    try:
        pc.compare_step(r, o, ot, tight=tight)
        passed = True
    except AssertionError:
        passed = False
    return solver_errors(ot, batch["x"], o, r, load), passed


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_break_their_criterion(mutant):
    """tests/emu built with TRUSS_EMU_MUTANTS: 1 pivot reciprocal in float32, 2 element 1/L in float32, 3 reactions summed in
    float32.  Each must exceed its criterion by >= 100 x on a supported grid with horizontal loads, where the unmutated build
    of the same library passes; at 256 nodes the old oracle tolerance is recorded in MUTANTS."""
    import ctypes
    crit, old_passes = MUTANTS[mutant]
    lib = tm.load(pc.build_emu(mutants=True))
    lib.dll.truss_emu_set_mutant.argtypes = [ctypes.c_int]
    topo = fr.supported_grid(10, True, 1, 1)
    big = tm.TrussTopology.grid(128)
    try:
        lib.dll.truss_emu_set_mutant(0)
        base, ok = _mutant_run(lib, topo, 5, 3, 1e-9)
        assert ok and float(base[crit].max()) <= TAU
        lib.dll.truss_emu_set_mutant(mutant)
        err, _ = _mutant_run(lib, topo, 5, 3, 1e-9)
        print("[mutant %d] %s error %.2e (unmutated %.2e)" % (mutant, crit, float(err[crit].max()), float(base[crit].max())))
        assert float(err[crit].max()) >= 100 * TAU, (crit, float(err[crit].max()))
        _, ok_old = _mutant_run(lib, big, 2, 128, 1e-7)
        assert ok_old == old_passes
    finally:
        lib.dll.truss_emu_set_mutant(0)
        topo.close()
        big.close()
