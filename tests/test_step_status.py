"""The step kernel at the edges of its input domain: flagged (not SPD) designs next to healthy ones, and ill-conditioned
designs that must not be flagged.  Every case runs through the lane emulator on the CPU and through the HIP library on the GPU,
on every compiled solver variant (TRUSS_VARIANTS of truss_host.h), at the smallest topology the variant accepts (the first of
test_solver_geometry.sweep_topologies: 8 to 44 nodes).

1. Flagged designs.  B = 2 EPB + 2 envs (EPB = 64 / G envs per wavefront), envs {0, 2 EPB - 1, 2 EPB} get one column collapsed
(top node on its bottom node: a zero-length member, NaN in K from that column's DOFs on), one run per column so that the first
bad pivot falls into team A's part, the middle block and team B's part.  Every wavefront that holds a bad env holds a healthy
one too (EPB >= 2; with G = 64 the isolation is between workgroups).  TRUSS_STATUS_NOT_SPD is raised on exactly the bad envs;
every output of every healthy env is bitwise what the all-healthy batch gives; one step from the collapsed design (the decode
lifts the top node to y_bottom + d_min) gives status 0 and the oracle's results: status describes the last step only.  The
persistent rollout and the fused observation writer run the same mixed batch.  The emulator mutants 4 (the flag folded over the
wavefront's 64 lanes instead of the env's G) and 5 (the fold returns 0) fail these checks.

What this does NOT prove: NaN spreads to every later pivot, so some lane of the env always sees a bad pivot and these inputs
cannot show that each lane's share of the pivot_check scan is needed.  An emulator mutant that kept only the flag of the env's
first lane was caught on 1 of the 10 variants.

2. Ill-conditioned designs.  B = 9: interior top nodes 1e-1 ... 1e-5 above their bottom nodes (a very short, very stiff
vertical member), spans scaled by 1, 1e-2, 1e2 and loads by 1, 1e-3, 1e3, every span scale with every load scale.
analyze() only (the decode would repair these designs); the reference is oracle.fem_solve plus fem_reference.refined_solution.
Asserted on the inputs: kappa_inf(K) <= 1e13 in every env (the refined reference is trustworthy), >= 1e10 in at least one env
of every variant.  Asserted on the results: status 0, every output finite, backward / equilibrium / reaction / balance errors
<= TAU (16 u, as test_solver_geometry), forward error <= 2 kappa_inf max(eta, u) with eta the env's own backward error
(||x - x^|| / ||x^|| <= kappa ||r|| / (||K|| ||x^||), and ||r|| / (||K|| ||x^||) <= 2 eta for the error_scale denominator),
a second env bitwise equal.

Measured in part 2, largest over the ten variants and their envs (per variant: pytest -s); the worst env of a variant has
kappa_inf(K) between 1.8e10 (G4_WL4_RPL2_EPL20) and 4.3e12 (G16_WL16_RPL1_EPL5):
  emulator (exact 1 / d):  backward 1.9e-16 (eta = 1.75 u), equilibrium 2.4e-16, reaction 9.3e-18, balance 1.5e-16,
                           forward error 0.87 kappa u = 0.37 of the asserted bound
  MI355X (v_rcp_f64 + two Newton steps):
                           backward 1.9e-16 (eta = 1.75 u), equilibrium 2.4e-16, reaction 2.6e-17, balance 1.4e-16,
                           forward error 0.87 kappa u = 0.30 of the asserted bound
The 30 GPU cases of the module take 2.5 s together.
"""
import ctypes

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import synthetic, _lib
from oracle import truss_oracle as O
import fem_reference as fr
import parity_common as pc
from test_solver_geometry import (EMIT, ROLLOUT, ROLLOUT_KEYS, TAU, VARIANTS, _batch, emit_topologies, force, solver_errors,
                                  sweep_topologies, vid)

RESULT_KEYS = ("y", "sec", "point", "obj", "q0", "sr", "disp", "comp", "max_up", "max_down", "disp_f64", "q0_f64", "energy",
               "reactions")
OBS_KEYS = ("x_n", "A_s", "A_n_ts", "A_n_cs", "nN_x_n", "nN_x_e")


def _hip():
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = tm.load()
    assert lib.backend == "hip"
    return lib


@pytest.fixture(scope="module", params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return pc.emu_lib() if request.param == "emu" else _hip()


@pytest.fixture(scope="module")
def report():
    """maxima of the part 2 criteria per variant, printed at the end of the module (pytest -s) for the record"""
    rows = {}
    yield lambda name, worst: rows.__setitem__(name, worst)
    for name, w in sorted(rows.items()):
        print("[ill-conditioned] %-26s " % name + " ".join("%s %.3g" % kv for kv in sorted(w.items())))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def columns(topo):
    """top node of every column, left to right (its bottom node is topo.pair[top])"""
    return [int(i) for i in np.flatnonzero(np.asarray(topo.top) == 1)]


# ---- 1. flagged designs ------------------------------------------------------------------------------------------------------
class Flagged:
    """the mixed batches of one variant on one topology: healthy batch, bad envs, actions, oracle inputs, and (per library) the
    all-healthy run every mixed run is compared with -- computed once and left unchanged"""

    def __init__(self, v, topo, seed):
        self.v, self.topo = v, topo
        self.EPB = 64 // v[0]
        self.B = 2 * self.EPB + 2
        self.bad = [0, 2 * self.EPB - 1, 2 * self.EPB]
        self.good = [b for b in range(self.B) if b not in self.bad]
        if self.EPB >= 2:                         # a bad set that fills a wavefront hides a broken fold
            for b in self.bad:
                wave = range(b // self.EPB * self.EPB, min((b // self.EPB + 1) * self.EPB, self.B))
                assert any(e in self.good for e in wave), (b, list(wave))
        assert self.B - 1 in self.good            # lanes past the batch redo the last env: it has to be a healthy one
        self.batch = _batch(topo, self.B, seed)
        self.ot = pc.oracle_topology(topo)
        self.load = pc.oracle_load(self.ot, self.batch)
        b = self.batch
        self.int_obj = O.initial_objectives(self.ot, b["x"], b["y"], b["sec"], b["target"])
        self.ag, self.at = synthetic.random_actions(2, self.B, topo.N, seed + 1)
        self.cols = columns(topo)
        self._healthy = {}

    def collapsed(self, c):
        """the healthy heights with column c's top node on its bottom node in the bad envs"""
        y = self.batch["y"].copy()
        top = self.cols[c]
        y[self.bad, top] = y[self.bad, self.topo.pair[top]]
        return y

    def env(self, lib, y=None):
        """an env with the healthy batch's normalisers whose last analysis is that of heights y (None: the healthy ones)"""
        e = pc.make_env(lib, self.topo, self.batch)
        e.analyze(set_normalisers=True)
        e.set_design(self.batch["y"] if y is None else y, self.batch["sec"])
        return e

    def healthy(self, lib):
        if lib.path not in self._healthy:
            e = self.env(lib)
            e.analyze()
            r = e.results()
            assert not r["status"].any()
            self._healthy[lib.path] = r
        return self._healthy[lib.path]

    def oracle(self, y, sec, s):
        b = self.batch
        return O.env_step(self.ot, b["x"], y, sec, None, None, self.ag[s], self.at[s], np.zeros(self.B), b["target"], self.load,
                          b["y_max"], b["d_min"], b["max_def"], b["is_roof"], self.int_obj)

    def actions(self, env):
        return torch.tensor(self.ag, device=env.device), torch.tensor(self.at, device=env.device)

    def expected_status(self):
        st = np.zeros(self.B, np.int32)
        st[self.bad] = 1
        return st


_TOPOS, _CHECKED, _CASES = {}, set(), {}


def variant_topology(lib, capfd, monkeypatch, v, emit=False):
    """the first topology of sweep_topologies(v) (emit: of emit_topologies), found once and shared by every test and library;
    its native topology is built under the variant's overrides and the host's own report must name variant v"""
    force(monkeypatch, v)
    if emit:
        if (lib.path, v) not in _TOPOS:
            found = emit_topologies(v, lib, capfd)
            for t, _ in found[1:]:
                t.close()
            topo, g = found[0]
            assert g["emit"] and (g["G"], g["WL"], g["RPL"], g["EPL"]) == v, g
            _TOPOS[(lib.path, v)] = topo
        return _TOPOS[(lib.path, v)]
    if v not in _TOPOS:
        topos = sweep_topologies(v)
        for t in topos[1:]:
            t.close()
        _TOPOS[v] = topos[0]
    if (lib.path, v) not in _CHECKED:
        g = fr.solver_geometry(_TOPOS[v], lib, capfd)
        assert (g["G"], g["WL"], g["RPL"], g["EPL"]) == v, g
        _CHECKED.add((lib.path, v))
    return _TOPOS[v]


def flagged_case(lib, capfd, monkeypatch, v, emit=False):
    """the Flagged case of (library, variant), created once"""
    topo = variant_topology(lib, capfd, monkeypatch, v, emit)
    key = (lib.path, v, emit)
    if key not in _CASES:
        _CASES[key] = Flagged(v, topo, seed=300 + VARIANTS.index(v))
    return _CASES[key]


def check_flag_and_isolation(lib, case, c):
    """column c collapsed in the bad envs: the flag on exactly those, the healthy envs bitwise as in the all-healthy batch.
    Returns the env (last analysis: the mixed batch) and the collapsed heights."""
    ref = case.healthy(lib)
    y = case.collapsed(c)
    env = case.env(lib, y)
    env.analyze()
    r = env.results()
    got = r["status"] & _lib.STATUS_NOT_SPD
    assert np.array_equal(got, case.expected_status()), ("status", c, got.tolist())
    assert not (r["status"] & ~_lib.STATUS_NOT_SPD).any(), ("status", c, r["status"].tolist())
    for k in RESULT_KEYS:
        assert same_bits(r[k][case.good], ref[k][case.good]), ("healthy envs changed", c, k)
    b = case.batch                                 # the flagged envs keep a valid design state: the next step starts from it
    mu, md = O.move_range(case.ot, y, b["y_max"], b["d_min"], b["is_roof"])
    for k, want in (("y", y), ("sec", b["sec"]), ("max_up", mu), ("max_down", md)):
        assert same_bits(r[k][case.bad], want[case.bad]), ("design state of the flagged envs", c, k)
    return env, y


def check_recovery(case, env, y, c):
    """one step from the collapsed design: the decode repairs it, status is 0 everywhere, the results are the oracle's"""
    g, t = case.actions(env)
    env.step(g[0], t[0])
    r = env.results()
    assert not r["status"].any(), ("status after the repairing step", c, r["status"].tolist())
    o = case.oracle(y, case.batch["sec"], 0)
    top = case.cols[c]
    gap = o["y"][case.bad, top] - o["y"][case.bad, case.topo.pair[top]]
    assert (gap >= np.float32(case.batch["d_min"][case.bad])).all(), gap       # the repair did happen
    pc.compare_step(r, o, case.ot)
    return o


def check_flagged(lib, case, cols=None):
    for c in range(len(case.cols)) if cols is None else cols:
        env, y = check_flag_and_isolation(lib, case, c)
        check_recovery(case, env, y, c)


@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_flagged_envs_status_isolation_recovery(lib, capfd, monkeypatch, v):
    case = flagged_case(lib, capfd, monkeypatch, v)
    assert len(case.cols) >= 4
    check_flagged(lib, case)


@pytest.mark.parametrize("v", sorted(ROLLOUT), ids=vid)
def test_flagged_envs_rollout(lib, capfd, monkeypatch, v):
    """two chained steps in one launch from the mixed batch = two step calls, bit for bit, status included (0 everywhere:
    the first step repairs the design)"""
    case = flagged_case(lib, capfd, monkeypatch, v)
    c = len(case.cols) // 2
    e1, y = check_flag_and_isolation(lib, case, c)
    e2, _ = check_flag_and_isolation(lib, case, c)
    assert e2.persistent_rollout
    g, t = case.actions(e1)
    o = None
    for s in range(2):
        e1.step(g[s], t[s])
        o = case.oracle(y if o is None else o["y"], case.batch["sec"] if o is None else o["sec"], s)
    e2.rollout(g, t, 2)
    r1, r2 = e1.results(), e2.results()
    pc.compare_step(r1, o, case.ot)
    assert not r2["status"].any()
    for k in ROLLOUT_KEYS:
        assert same_bits(r1[k], r2[k]), ("rollout", k)


@pytest.mark.parametrize("v", sorted(EMIT), ids=vid)
def test_flagged_envs_fused_observations(lib, capfd, monkeypatch, v):
    """the reset path with the observation tensors written by the step's own launch, on the mixed batch: the healthy envs'
    observations are bitwise those of the all-healthy batch, nothing times out; the flagged envs' tensors are unspecified"""
    case = flagged_case(lib, capfd, monkeypatch, v, emit=True)
    c = len(case.cols) // 2
    obs, st = [], []
    for y in (None, case.collapsed(c)):
        env = case.env(lib, y)
        assert env.fused_obs
        out = {k: torch.full_like(b, float("nan")) for k, b in env.obs_buffers().items()}
        env.analyze(obs=out)
        obs.append({k: t.cpu().numpy() for k, t in out.items()})
        st.append(env.results()["status"])
    assert not st[0].any()
    assert np.array_equal(st[1], case.expected_status()), ("status", st[1].tolist())     # no TRUSS_STATUS_OBS_TIMEOUT either
    for k in OBS_KEYS:
        assert np.isfinite(obs[0][k]).all(), ("not every element written", k)
        assert same_bits(obs[1][k][case.good], obs[0][k][case.good]), ("healthy envs' observations changed", k)


@pytest.mark.parametrize("mutant", [4, 5])
def test_status_fold_mutants_are_caught(capfd, monkeypatch, mutant):
    """tests/emu built with TRUSS_EMU_MUTANTS: 4 folds the bad-pivot flag over the wavefront's 64 lanes instead of the env's G,
    5 returns 0 from the fold.  The checks of test_flagged_envs_status_isolation_recovery fail on 5 for every variant and on 4
    for every variant with two or more envs per wavefront (with G = 64 mutant 4 is the plain fold); the unmutated build of the
    same library passes them."""
    lib = tm.load(pc.build_emu(mutants=True))
    lib.dll.truss_emu_set_mutant.argtypes = [ctypes.c_int]
    try:
        for v in VARIANTS:
            lib.dll.truss_emu_set_mutant(0)
            case = flagged_case(lib, capfd, monkeypatch, v)
            mid = [len(case.cols) // 2]
            check_flagged(lib, case, None if mutant == 4 else mid)      # the whole unmutated run once, a column the other time
            lib.dll.truss_emu_set_mutant(mutant)
            if mutant == 4 and case.EPB < 2:
                check_flagged(lib, case, mid)
                continue
            for c in (0, mid[0], len(case.cols) - 1):
                with pytest.raises(AssertionError, match="status"):
                    check_flagged(lib, case, [c])
    finally:
        lib.dll.truss_emu_set_mutant(0)


# ---- 2. ill-conditioned, unflagged designs -----------------------------------------------------------------------------------
KAPPA_MAX, KAPPA_REACHED = 1e13, 1e10
SPAN_SCALES = (1.0, 1e-2, 1e2)
LOAD_SCALES = (1.0, 1e-3, 1e3)
# env b: spans x SPAN_SCALES[b % 3], loads x LOAD_SCALES[b // 3] (every span scale meets every load scale), and the gap of the
# short vertical member (None: the env's heights stay as they are).  kappa grows with span / gap, and the small spans are
# ill-conditioned by themselves (members a hundred times higher than wide): the smallest gaps go with the small spans, the middle
# ones with the large spans, which puts kappa_inf(K) between 2e10 and 4.3e12 in the worst env of every variant; 1e-5 or 3e-5 with
# the large spans reaches 9e13.
GAPS = (1e-1, 1e-4, 1e-3, None, 1e-5, 3e-3, None, 3e-5, 1e-2)


def ill_conditioned_batch(topo, seed):
    batch = _batch(topo, 9, seed)
    cols = columns(topo)
    res = np.asarray(topo.res)
    free_cols = [t for t in cols[1:-1] if not res[topo.pair[t]].any()] or cols[1:-1]      # bottom node free where one is
    for b in range(9):
        s, l = SPAN_SCALES[b % 3], LOAD_SCALES[b // 3]
        batch["x"][b] = (batch["x"][b].astype(np.float64) * s).astype(np.float32)
        batch["max_def"][b] *= s
        batch["load_x"][b] *= l
        batch["load_y"][b] *= l
        if GAPS[b] is not None:
            top = free_cols[(7 * b) % len(free_cols)]
            batch["y"][b, top] = batch["y"][b, topo.pair[top]] + np.float32(GAPS[b])
    return batch


def check_ill_conditioned(lib, topo, seed):
    batch = ill_conditioned_batch(topo, seed)
    ot = pc.oracle_topology(topo)
    load = pc.oracle_load(ot, batch)
    fem = O.fem_solve(ot, batch["x"], batch["y"], batch["sec"], load)
    K, P = fem["K"], fem["P"]
    kappa = fr.cond_inf(K)
    assert (kappa <= KAPPA_MAX).all(), kappa
    assert kappa.max() >= KAPPA_REACHED, kappa
    envs = [pc.make_env(lib, topo, batch) for _ in range(2)]
    for e in envs:
        e.analyze()
    r, r2 = envs[0].results(), envs[1].results()
    err = solver_errors(ot, batch["x"], dict(y=batch["y"], fem=fem), r, load)
    d = fr.free_dofs(ot, r["disp_f64"])
    fwd = fr.forward_error(d, fr.refined_solution(K, P))
    eta = np.maximum(err["backward"], fr.U64)
    worst = {k: float(e.max()) for k, e in err.items()}
    worst.update(kappa=float(kappa.max()), fwd_over_kappa_u=float((fwd / (kappa * fr.U64)).max()),
                 fwd_over_bound=float((fwd / (2 * kappa * eta)).max()), eta_over_u=float(err["backward"].max() / fr.U64))
    print("[ill-conditioned] N=%d E=%d %s" % (topo.N, topo.E, " ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    assert not r["status"].any(), r["status"].tolist()
    for k, a in r.items():
        if a.dtype.kind == "f":
            assert np.isfinite(a).all(), k
    for k in ("backward", "equilibrium", "reaction", "balance"):
        assert worst[k] <= TAU, (k, worst[k])
    assert (fwd <= 2 * kappa * eta).all(), ("forward", (fwd / (2 * kappa * eta)).tolist())
    for k in r:
        assert same_bits(r[k], r2[k]), ("not deterministic", k)
    return worst


@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_ill_conditioned_designs(lib, capfd, monkeypatch, report, v):
    topo = variant_topology(lib, capfd, monkeypatch, v)
    report("%s %s" % (vid(v), lib.backend), check_ill_conditioned(lib, topo, 400 + VARIANTS.index(v)))
