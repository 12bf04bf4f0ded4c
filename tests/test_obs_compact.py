"""The compact layout of the node-graph adjacency observations (TRUSS_F_OBS_COMPACT / TRUSS_OBS_F_COMPACT): A_s, A_n_ts and A_n_cs
as [B, N, Kc] rows through the topology's neighbour table instead of [B, N, N].

The compact producer writes the values of the dense producer and nothing else, so the check is bitwise: for the same designs and
actions, compact == gather(dense, nbr) with +0 in the unused slots, from the step's own launch (fused writer or the observation
kernel queued behind it) and from truss_obs; x_n, nN_x_n, nN_x_e and every step result equal the dense run's.  On the CPU through the
lane emulator (the same lane program and host code), on the GPU through the HIP library."""
import os

import numpy as np
import pytest
import torch

import parity_common as pc
import truss_mi355 as tm
from truss_mi355 import _lib, ops, synthetic

POISON = -7.5          # buffers are pre-filled: what a launch leaves alone shows
ADJ = ("A_s", "A_n_ts", "A_n_cs")


def odd_truss():
    """5 nodes / 7 members (three triangles), no vertical pairs: analysis only, the observation kernel, N Kc = 25 (odd: the word path
    at a row offset that is no multiple of 4)"""
    conn = [(0, 1), (1, 2), (0, 3), (1, 3), (1, 4), (2, 4), (3, 4)]
    res = np.zeros((5, 2), np.uint8)
    res[0] = 1
    res[2, 1] = 1
    return tm.TrussTopology(np.array(conn, np.int32), res, np.array([0, 0, 0, 1, 1], np.uint8), pair=None)


def odd_batch(B, seed):
    rng = np.random.default_rng(seed)
    x = np.tile(np.array([0.0, 3.0, 6.0, 1.5, 4.5], np.float32), (B, 1))
    y = np.concatenate([np.zeros((B, 3)), np.round(rng.uniform(1.0, 4.0, (B, 2)), 2)], axis=1).astype(np.float32)
    return dict(x=x, y=y, sec=rng.integers(0, 5, (B, 7)).astype(np.int32), target=np.zeros((B, 5), np.float32) + y * 0.5,
                y_max=np.full(B, 5.0), d_min=np.full(B, 0.3), max_def=np.full(B, 0.006), load_x=np.zeros(B),
                load_y=-rng.uniform(5e3, 1.2e5, B), is_roof=np.zeros(B))


# name -> (topology, environment overrides at topology creation, lanes per env expected, fused writer expected, decode step)
CASES = {
    "emit 16x8x1x5": (lambda: synthetic.bench_topology(16, 4), {}, 16, True, True),             # 32 / 80, the metric topology
    "emit 16x8x1x3": (lambda: tm.TrussTopology.grid(8), {}, 16, True, True),                    # 16 / 36
    "emit 8x8x1x5": (lambda: tm.TrussTopology.grid(8), {"TRUSS_LANES": "8"}, 8, True, True),
    "N % 4 != 0": (lambda: tm.TrussTopology.grid(7), {}, 16, False, True),                      # 14 nodes: the observation kernel
    "odd N Kc": (odd_truss, {}, None, False, False),
    "64 nodes": (lambda: tm.TrussTopology.grid(32), {}, None, False, True),                     # row tiles, split launches
    "256 nodes": (lambda: tm.TrussTopology.grid(128), {}, None, False, True),
    "irregular": (lambda: pc.irregular_topology(3), {}, None, None, True),                      # rows of different degree
}


def _expand(c, nbr):
    """compact [B, N, Kc] -> dense [B, N, N] through the table"""
    B, N, _ = c.shape
    d = torch.zeros(B, N, N, dtype=c.dtype)
    ok = nbr >= 0
    rows = torch.arange(N)[:, None].expand_as(nbr)
    d[:, rows[ok], nbr[ok]] = c[:, ok]
    return d


def run_case(lib, name, monkeypatch, drop=None):
    """dense and compact runs of one case on `lib`: returns nothing, asserts everything"""
    make, envv, lanes, fused, decode = CASES[name]
    for k, v in envv.items():
        monkeypatch.setenv(k, v)
    topo = make()
    try:
        info = topo.solver_info(lib)
        if lanes is not None:
            assert info["lanes_per_env"] == lanes
        epb = 64 // info["lanes_per_env"]
        big = topo.N >= 64
        B = 2 if big else epb + 2                 # buffers of B envs ...
        n = 2 if big else epb + 1                 # ... n of them active: a full workgroup and a partial one, the rest untouched
        batch = odd_batch(B, 7) if not decode else synthetic.random_batch(topo, B, 7)
        ag, at = synthetic.random_actions(1, B, topo.N, 8)
        table = topo.neighbor_table()
        assert np.array_equal(topo.native_neighbors(lib), table) and table.dtype == np.int16          # the library's own table
        nbr = torch.tensor(table.astype(np.int64))
        assert len(set((table >= 0).sum(1).tolist())) > 1                                             # rows of different degree: padding
        out = {}
        for layout in ("dense", "compact"):
            env = pc.make_env(lib, topo, batch)
            dev = env.device
            assert env.obs_width(layout) == (topo.N if layout == "dense" else table.shape[1])
            if fused is not None:
                assert env.fused_obs == fused
            env.analyze(set_normalisers=True)
            got = {k: torch.full_like(v, POISON) for k, v in env.obs_buffers(layout).items()}
            if drop:
                got[drop] = None
            if decode:
                env.step(torch.tensor(ag[0][:n], device=dev), torch.tensor(at[0][:n], device=dev), n_active=n, obs=got, obs_layout=layout)
            else:
                env.analyze(n_active=n, obs=got, obs_layout=layout)
            alone = {k: torch.full_like(v, POISON) for k, v in env.obs_buffers(layout).items()}
            env.observe(alone, n_active=n, obs_layout=layout)                                     # truss_obs on the same results
            if dev.type == "cuda":
                torch.cuda.synchronize()
            assert int(env.status[:n].abs().sum()) == 0
            out[layout] = ({k: None if v is None else v.cpu() for k, v in got.items()}, {k: v.cpu() for k, v in alone.items()},
                           env.results())
        for which in (0, 1):
            d, c = out["dense"][which], out["compact"][which]
            for k in d:
                if d[k] is None:
                    assert c[k] is None
                    continue
                if k in ADJ:
                    want = d[k].gather(2, nbr.clamp(min=0).expand(d[k].shape[0], -1, -1)) * (nbr >= 0)
                    want[n:] = POISON                                                              # rows of inactive envs stay as they were
                    assert c[k].shape == (B, topo.N, table.shape[1]) and c[k].is_contiguous()
                    assert torch.equal(c[k], want), (name, k, which)
                    pad = c[k][:n][:, nbr < 0]
                    assert not torch.signbit(pad).any() and not (pad != 0).any()                   # +0.0, written
                    assert torch.equal(_expand(c[k][:n], nbr), d[k][:n])                           # nothing of the dense matrix is lost
                else:
                    assert torch.equal(c[k], d[k]), (name, k, which)
        rd, rc = out["dense"][2], out["compact"][2]
        for k in rd:
            assert np.array_equal(rd[k], rc[k], equal_nan=True), (name, k)
    finally:
        topo.close()


@pytest.fixture(scope="module")
def lib():
    return pc.emu_lib()


@pytest.mark.parametrize("name", list(CASES))
def test_compact_is_the_gather_of_dense_emulated(lib, name, monkeypatch):
    run_case(lib, name, monkeypatch)


def test_a_missing_tensor_emulated(lib, monkeypatch):
    """one of the three pointers NULL: the other two are written, in both producers"""
    run_case(lib, "emit 16x8x1x5", monkeypatch, drop="A_n_ts")
    run_case(lib, "N % 4 != 0", monkeypatch, drop="A_s")


@pytest.mark.parametrize("name", ["train0", "train_eval", "small_roof", "large_bridge", "large_roof"])
def test_compact_observation_golden_emulated(lib, name):
    """against the reference: the compact tensors of the replayed golden transitions, expanded to dense, within the tolerances of
    test_fused_observation_golden_emulated -- from the step's own launch (the analysis of the new design) and from truss_obs"""
    env = pc.run_golden_transitions(lib, name)
    f = np.load(os.path.join(pc.GOLDEN, name + ".npz"))
    nbr = torch.tensor(env.topo.neighbor_table().astype(np.int64))
    B = env.B
    fused = {k: torch.full_like(v, POISON) for k, v in env.obs_buffers("compact").items()}
    alone = {k: torch.full_like(v, POISON) for k, v in env.obs_buffers("compact").items()}
    env.observe(alone, obs_layout="compact")
    env.analyze(obs=fused, obs_layout="compact")
    for obs in (alone, fused):
        for k in ("x_n", "A_s", "A_n_ts", "A_n_cs", "nN_x_n"):
            a = _expand(obs[k], nbr) if k in ADJ else obs[k]
            np.testing.assert_allclose(a.numpy(), f["tr_out_" + k], rtol=1e-5, atol=5e-6, err_msg=k)
        xe, ref = obs["nN_x_e"].numpy(), f["tr_out_nN_x_e"]
        scale = np.maximum(np.abs(ref).max(axis=(0, 1), keepdims=True), 1.0)
        assert float((np.abs(xe - ref) / scale).max()) < 1e-5
    assert B == f["tr_in_node"].shape[0]


def test_refusals(lib):
    topo = synthetic.bench_topology(16, 4)
    B = 3
    env = pc.make_env(lib, topo, synthetic.random_batch(topo, B, 3))
    env.analyze(set_normalisers=True)
    Kc = env.obs_width("compact")
    assert Kc == topo.neighbor_table().shape[1] < topo.N and _lib.F_OBS_COMPACT == 0x8 and lib.has_obs_compact
    # the layout flag without TRUSS_F_EMIT_OBS
    with pytest.raises(tm.TrussError, match="TRUSS_F_OBS_COMPACT"):
        env._step_op(_lib.F_NO_DECODE | _lib.F_OBS_COMPACT, B, None, None, None, None, None, env.y, env.sec, env.y, env.sec)
    # a short buffer at the operators: N Kc floats per env are needed, never fewer
    short = dict(env.obs_buffers("compact"))
    short["A_n_cs"] = torch.zeros(B, topo.N, Kc - 1)
    with pytest.raises(tm.TrussError, match=rf"A_n_cs has {B * topo.N * (Kc - 1)} elements, needs {B * topo.N * Kc}"):
        env._step_op(_lib.F_NO_DECODE, B, None, None, None, None, None, env.y, env.sec, env.y, env.sec, obs=short, obs_layout="compact")
    with pytest.raises(tm.TrussError, match="A_n_cs has"):
        ops.call(env._ops.obs_flags, env._lib_id, env.h.value, 0, _lib.F_OBS_COMPACT, B, env.N, env.E, env.x, env.y, env.sec, env.max_up,
                 env.max_down, env.target, env.disp, env.q0, env.sr, env.comp, env.env_params, None, None, None, short["A_n_cs"], None, None)
    # a compact-sized buffer handed to a dense call is refused by the dense size check: no dense write into it
    with pytest.raises(tm.TrussError, match="A_s has"):
        env._step_op(_lib.F_NO_DECODE, B, None, None, None, None, None, env.y, env.sec, env.y, env.sec, obs=env.obs_buffers("compact"))
    # the Python side: shapes per layout, unknown layouts
    with pytest.raises(ValueError, match=r"obs\[A_s\]"):
        env.analyze(obs=env.obs_buffers("dense"), obs_layout="compact")
    with pytest.raises(ValueError, match=r"obs\[A_s\]"):
        env.observe(env.obs_buffers("compact"))
    with pytest.raises(ValueError, match="obs layout must be"):
        env.observe(obs_layout="csr")
    # truss_topo_neighbors: a short host buffer is refused, the width alone can be asked for
    import ctypes as C
    k, few = C.c_int32(), np.zeros(4, np.int16)
    assert lib.dll.truss_topo_neighbors(env.h, None, 0, C.byref(k)) == 0 and k.value == Kc
    assert lib.dll.truss_topo_neighbors(env.h, few.ctypes.data_as(C.c_void_p), 4, C.byref(k)) == -1
    topo.close()


def test_a_library_without_the_entry_is_refused(lib, monkeypatch):
    topo = tm.TrussTopology.grid(8)
    env = tm.BatchedTruss(topo, 2, lib=lib)
    monkeypatch.setattr(lib, "has_obs_compact", False)
    with pytest.raises(tm.TrussError, match="truss_topo_neighbors"):
        env.obs_buffers("compact")
    assert env.obs_buffers()["A_s"].shape == (2, 16, 16)          # the dense layout asks nothing of the library
    topo.close()


def test_operator_registration():
    ns = ops.namespace()
    for key in ("CPU", "CUDA", "Meta"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key("truss_mi355::obs_flags", key)
    assert "truss_topo_neighbors" not in ops.entries()          # no launch, no operator of its own
    assert "truss_topo_neighbors" in [n for n, _ in _lib._LATER_ENTRIES]


# ---- the same on the hardware ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_compact_is_the_gather_of_dense_hip(name, monkeypatch):
    """the HIP library: compact tensors from the fused launch where truss_topo_fused_obs is 1, from the observation kernel elsewhere,
    and from truss_obs; torch.equal to the gather of the dense run, status 0"""
    run_case(tm.load(), name, monkeypatch)


@pytest.mark.gpu
def test_a_missing_tensor_hip(monkeypatch):
    run_case(tm.load(), "emit 16x8x1x5", monkeypatch, drop="A_n_ts")
    run_case(tm.load(), "64 nodes", monkeypatch, drop="A_s")
