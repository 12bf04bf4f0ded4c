"""Band rows of the step kernel: padded rows (row stride W + 2 doubles) of the 16-lane / 5-elements-per-lane kernels against the
float64 oracle, the persistent rollout against single steps, and invariants of the LDS layout read through truss_topo_lds_info.

Two-row trusses of 3 to 10 columns, each with two pins (KA = 2 nx - 6) and with a pin and a roller (KA = 2 nx - 5): every
KA mod 8 instantiation of the two-sided merge.  Trusses this small would get the 3-elements-per-lane kernel, whose rows are
dense; TRUSS_EPL=5 asks for the padded one.  TRUSS_LANES=8: the one-team path (dense rows)."""
import ctypes as C

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import synthetic
import parity_common as pc

INFO = ("lds_bytes", "o_env0", "env_stride", "envs", "W", "KS", "rowsA", "rowsB", "kb_b", "trash", "band_lo", "band_hi", "ev_lo",
        "ev_hi", "n_live", "n_offsets")
LDS_PER_CU = 160 * 1024
B, STEPS = 5, 3       # 4 envs per workgroup: the second workgroup is partly filled


def two_row(nx, roller):
    g = tm.TrussTopology.grid(nx)
    if not roller:
        return g
    res = np.array(g.res, np.uint8).reshape(-1, 2).copy()
    assert res[nx - 1].tolist() == [1, 1]
    res[nx - 1] = [0, 1]
    return tm.TrussTopology(g.conn, res, g.top, g.pair)


def lds_info(lib, topo, emit=0):
    h = topo.native(lib)
    info = np.zeros(len(INFO), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.check(lib.dll.truss_topo_lds_info(h, emit, vp(info), None, 0, None, 0), "truss_topo_lds_info")
    d = dict(zip(INFO, info.tolist()))
    live, offs = np.zeros(2 * d["n_live"], np.int32), np.zeros(d["n_offsets"], np.int32)
    lib.check(lib.dll.truss_topo_lds_info(h, emit, vp(info), vp(live), d["n_live"], vp(offs), d["n_offsets"]), "truss_topo_lds_info")
    d["live"], d["offsets"] = live.reshape(-1, 2).tolist(), offs
    return d


def steps_and_rollout(lib, topo, seed):
    """STEPS chained steps, each against the float64 oracle under parity_common.compare_step's full contract; then the same steps
    as one rollout call, which must give the last step's results bit for bit"""
    from oracle import truss_oracle as O
    batch = synthetic.random_batch(topo, B, seed)
    ag, at = synthetic.random_actions(STEPS, B, topo.N, seed + 1)
    coin = (np.random.default_rng(seed + 2).random(B) >= 0.5).astype(np.uint8)
    e1, e2 = pc.make_env(lib, topo, batch), pc.make_env(lib, topo, batch)
    e1.analyze(set_normalisers=True)
    e2.analyze(set_normalisers=True)
    dev = e1.device
    ot = pc.oracle_topology(topo)
    load = pc.oracle_load(ot, batch)
    int_obj = O.initial_objectives(ot, batch["x"], batch["y"], batch["sec"], batch["target"])
    y, sec = batch["y"], batch["sec"]
    for s in range(STEPS):
        e1.step(torch.tensor(ag[s], device=dev), torch.tensor(at[s], device=dev), torch.tensor(coin, device=dev))
        o = O.env_step(ot, batch["x"], y, sec, None, None, ag[s], at[s], coin.astype(np.float64), batch["target"], load,
                       batch["y_max"], batch["d_min"], batch["max_def"], batch["is_roof"], int_obj)
        pc.compare_step(e1.results(), o, ot)
        y, sec = o["y"], o["sec"]
    e2.rollout(torch.tensor(ag, device=dev), torch.tensor(at, device=dev), STEPS, torch.tensor(coin, device=dev))
    r1, r2 = e1.results(), e2.results()
    for k in ("y", "sec", "point", "q0", "sr", "disp", "comp", "max_up", "max_down", "status"):
        assert np.array_equal(r1[k], r2[k]), k


@pytest.fixture(scope="module")
def emu():
    return pc.emu_lib()


@pytest.mark.parametrize("roller", [False, True])
@pytest.mark.parametrize("nx", range(3, 11))
def test_padded_rows_emulated(emu, monkeypatch, nx, roller):
    monkeypatch.setenv("TRUSS_EPL", "5")
    topo = two_row(nx, roller)
    d = lds_info(emu, topo)
    assert (d["W"], d["KS"]) == (8, 10)
    assert (d["rowsA"] - 2 * d["W"]) % 8 == (2 * nx - 6 + roller) % 8      # rowsA = KA + 2 W
    steps_and_rollout(emu, topo, seed=100 + 2 * nx + roller)


@pytest.mark.parametrize("nx", [3, 6, 10])
def test_one_team_emulated(emu, monkeypatch, nx):
    monkeypatch.setenv("TRUSS_LANES", "8")
    topo = two_row(nx, False)
    assert topo.solver_info(emu)["lanes_per_env"] == 8
    d = lds_info(emu, topo)
    assert d["KS"] == d["W"] == 8 and d["rowsB"] == 0
    steps_and_rollout(emu, topo, seed=200 + nx)


def check_layout(d):
    offs = d["offsets"]
    W, KS = d["W"], d["KS"]
    assert offs.size and np.unique(offs).size == offs.size, "two table entries store to the same band entry"
    assert offs.min() >= 0 and offs.max() < d["trash"], "a table entry outside the band rows"
    assert d["band_lo"] + 8 * (d["trash"] + 1) <= d["band_hi"], "the trash slot lies outside the band region"
    # inside a row: never in the padding behind its W entries, nor in front of team B's rows
    a = offs[offs < d["rowsA"] * KS]
    b = offs[offs >= d["rowsA"] * KS]
    assert np.all(a % KS < W) and np.all(b >= d["kb_b"]) and np.all((b - d["kb_b"]) % KS < W)
    # row bases (ds_read_b128 / ds_write_b128 of whole rows) are 16-byte aligned in LDS
    assert (8 * KS) % 16 == 0 and (8 * d["kb_b"]) % 16 == 0
    assert d["band_lo"] % 16 == 0 and d["o_env0"] % 16 == 0 and d["env_stride"] % 16 == 0
    # the element values overlap nothing that is still read while they are live: the band, the rows and tables, the coin
    for lo, hi in d["live"] + [[d["band_lo"], d["band_hi"]]]:
        assert hi <= d["ev_lo"] or lo >= d["ev_hi"], (lo, hi, d["ev_lo"], d["ev_hi"])
        assert 0 <= lo < hi <= d["env_stride"]
    assert d["ev_hi"] <= d["env_stride"] - 4
    assert d["lds_bytes"] == d["o_env0"] + d["envs"] * d["env_stride"]


@pytest.mark.parametrize("emit", [0, 1])
@pytest.mark.parametrize("case", ["metric", "grid16", "grid5_epl5", "grid8", "grid8_lanes8", "grid32", "irregular"])
def test_layout_invariants(emu, monkeypatch, case, emit):
    if case == "grid5_epl5":
        monkeypatch.setenv("TRUSS_EPL", "5")
    if case == "grid8_lanes8":
        monkeypatch.setenv("TRUSS_LANES", "8")
    topo = {"metric": lambda: synthetic.bench_topology(16, 4), "grid16": lambda: tm.TrussTopology.grid(16),
            "grid5_epl5": lambda: two_row(5, True), "grid8": lambda: tm.TrussTopology.grid(8),
            "grid8_lanes8": lambda: tm.TrussTopology.grid(8), "grid32": lambda: tm.TrussTopology.grid(32),
            "irregular": lambda: pc.irregular_topology(3)}[case]()
    check_layout(lds_info(emu, topo, emit))


def test_metric_topology_keeps_four_workgroups_per_cu(emu):
    topo = synthetic.bench_topology(16, 4)
    plain, fused = lds_info(emu, topo, 0), lds_info(emu, topo, 1)
    assert (plain["KS"], fused["KS"]) == (10, 8)          # padded rows for the step and the rollout, dense for the EMIT kernel
    assert plain["lds_bytes"] <= LDS_PER_CU // 4 == 40960
    assert fused["lds_bytes"] == 40704                    # what the EMIT launch needed before the rows of the plain one were padded
    # team B 64 bytes (mod 128) behind team A, the next env 128 bytes (mod 256) behind this one
    assert (8 * plain["kb_b"]) % 128 == 64 and plain["env_stride"] % 256 == 128
    assert (8 * fused["kb_b"]) == 8 * fused["rowsA"] * 8 and fused["env_stride"] % 256 == 64


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [5, 8, 16])
def test_padded_rows_hip(monkeypatch, nx):
    lib = tm.load()
    assert lib.backend == "hip"
    monkeypatch.setenv("TRUSS_EPL", "5")
    for roller in (False, True):
        topo = two_row(nx, roller)
        assert lds_info(lib, topo)["KS"] == 10
        steps_and_rollout(lib, topo, seed=300 + 2 * nx + roller)
