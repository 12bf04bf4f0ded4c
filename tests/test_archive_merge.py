"""The archive update of a game step as one launch (`truss_archive_merge`, csrc/truss_archive.h; reward.archive_merge,
BatchedMARL(archive_path="hip")).

References, never the code under test:
  (a) `_torch_block`: the archive block of BatchedMARL.game_step_all / _design_cull (candidate buffers, concatenation, one `truss_front`
      launch through reward.front_hv, gathers, clamp, accepted flags), lifted into this file, on the same device;
  (b) `_host_model`: utils.simple_cull_final + the Python restatement of the D3 truncation, per env, on the host.
Every output of the entry is a copy of an input value or a clamp of one, so the comparison with (a) is torch.equal on the rows, the
designs, the counts and the flags: no tolerance.  hv_front / metrics are sums: held to 1e-12 against truss_front's, the project's front
tolerance.  Generators are copies: nothing is imported from other test files."""
import contextlib
import ctypes
import io
import math

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import _lib, marl, ops, reward as RW, synthetic
import parity_common as pc
import utils as U
import master_DDPG_truss2D_MO as M
import truss2D_RL as RL

EMPTY = (0.0, 0.0, 2.0, 0.0)


# ---- generators ------------------------------------------------------------------------------------------------------------------
def _diag(rng, m, lo=0.05, hi=1.0):
    """m mutually non-dominated feasible rows on x + y = 1.05 (distinct x: every one of them is on the front of the set), in random
    order; continuous draws, so that no two crowding distances tie to within rounding"""
    t = rng.uniform(lo, hi, size=m)
    assert len(set(t)) == m and len(set(1.05 - t)) == m
    return np.stack([t, 1.05 - t, rng.uniform(0.2, 0.99, m), rng.uniform(0.2, 0.99, m)], axis=1)


def _case(seed, B, P, C, n_y, n_sec, extra_rows=3):
    """One batch: archives pts / n / y / sec, candidate arrays of R = B C + extra_rows rows and the slot table.  Env b plays scenario
    b % 12 (see below); its archive holds n[b] rows, the rows behind them are garbage (they are dead: nothing may depend on them)."""
    rng = np.random.default_rng(seed)
    R = B * C + extra_rows
    pts = rng.uniform(0.05, 1.15, size=(B, P, 4)); pts[:, :, 2:] = rng.uniform(0.2, 1.06, size=(B, P, 2))
    cand = rng.uniform(0.05, 1.15, size=(R, 4)); cand[:, 2:] = rng.uniform(0.2, 1.04, size=(R, 2))
    n = rng.integers(0, P + 1, size=B).astype(np.int32)
    n[:4] = (0, 1, P - 1, P)
    slot = np.arange(B * C, dtype=np.int32).reshape(B, C)
    for b in range(B):
        kind, rows = b % 12, slot[b].copy()
        if kind == 0:                                            # some slots empty, some candidates not ok
            slot[b, rng.random(C) < 0.3] = -1
            cand[rows[0::5], 2] = 1.01
            cand[rows[1::5], 3] = np.nan
            cand[rows[2::7], 2] = np.nan
        elif kind == 1:                                          # a candidate dominates the whole archive
            cand[rows[C // 2]] = (0.01, 0.01, 0.5, 0.5)
        elif kind == 2:                                          # all candidates dominated
            n[b] = max(n[b], 1)
            pts[b, 0] = (0.01, 0.01, 0.5, 0.5)
        elif kind == 3:                                          # objectives on a 1/20 grid: ties in obj1 and obj2
            pts[b, :, :2] = np.round(pts[b, :, :2] * 20) / 20
            cand[rows, :2] = np.round(cand[rows, :2] * 20) / 20
        elif kind == 4:                                          # a candidate identical to an archive row (a front row of the archive)
            n[b] = max(n[b], 2)
            pts[b, 1] = (0.02, 0.6, 0.7, 0.7)
            cand[rows[C - 1]] = pts[b, 1]
        elif kind == 5:                                          # two identical candidates
            cand[rows[0]] = (0.03, 0.03, 0.4, 0.6)
            cand[rows[C - 1]] = cand[rows[0]]
        elif kind == 6:                                          # objectives above 1 on the front (the clamp)
            n[b] = 0
            cand[rows, 0] += 0.6
            cand[rows[0]] = (1.3, 0.01, 0.5, 0.5)
            cand[rows[1]] = (0.01, 1.2, 0.5, 0.5)
        elif kind == 7:                                          # a long front: archive and candidates on one anti-diagonal
            n[b] = P
            d = _diag(rng, P + C)
            pts[b], cand[rows] = d[:P], d[P:]
        elif kind == 8:                                          # every slot empty
            slot[b] = -1
        elif kind == 9:                                          # nothing feasible at all
            n[b] = 0
            cand[rows, 2] = 1.5
    y = rng.standard_normal((B, P, n_y)).astype(np.float32)
    sec = rng.integers(0, 30, size=(B, P, n_sec)).astype(np.int32)
    cy = rng.standard_normal((R, n_y)).astype(np.float32)
    cs = rng.integers(30, 60, size=(R, n_sec)).astype(np.int32)
    return dict(pts=pts, n=n, y=y, sec=sec, cand=cand, cy=cy, cs=cs, slot=slot)


def _wide_case(seed, P, C, fronts):
    """len(fronts) envs of P + C rows whose front has exactly fronts[b] rows: that many rows of one anti-diagonal spread over the
    archive and the candidates, every other row dominated by one of them, infeasible or dead"""
    rng = np.random.default_rng(seed)
    B, n_y, n_sec = len(fronts), 12, 9
    c = _case(seed + 1, B, P, C, n_y, n_sec)
    c["slot"] = np.arange(B * C, dtype=np.int32).reshape(B, C)
    for b, m in enumerate(fronts):
        rows = np.empty((P + C, 4))
        d = _diag(rng, m)
        rows[:] = (1.1, 1.1, 0.5, 0.5)                           # dominated by every row of the diagonal
        rows[:, :2] += rng.uniform(0, 0.05, size=(P + C, 2))
        rows[rng.random(P + C) < 0.2, 3] = 1.2                   # ... or infeasible
        rows[rng.permutation(P + C)[:m]] = d
        if m == 0:
            rows[:, 2] = 1.5                                     # nothing feasible
        c["n"][b] = P
        c["pts"][b], c["cand"][c["slot"][b]] = rows[:P], rows[P:]
    return c


def _t(c, device):
    return {k: torch.tensor(v, device=device) for k, v in c.items()}


# ---- reference (a): the engine's torch block ----------------------------------------------------------------------------------------
def _torch_block(lib, t, max_front, max_out, slot=None):
    """BatchedMARL.game_step_all (archive update + the replay's accepted flags) / _design_cull on a table of slots: candidate buffers
    [B, C, .] filled by index put, the archive concatenated with them, one truss_front launch over all P + C rows, gathers."""
    wp, wn, wy, ws = t["pts"], t["n"], t["y"], t["sec"]
    slot = t["slot"] if slot is None else slot
    B, P, _ = wp.shape
    C, dev = slot.shape[1], wp.device
    points = t["cand"]
    ok = (points[:, 2:4] <= 1).all(dim=1)
    candP = torch.tensor(EMPTY, dtype=torch.float64, device=dev).expand(B, C, 4).clone()
    candY = torch.zeros((B, C, wy.shape[2]), dtype=torch.float32, device=dev)
    candS = torch.zeros((B, C, ws.shape[2]), dtype=torch.int32, device=dev)
    pmark = points.clone()
    pmark[:, 2] = torch.where(ok, pmark[:, 2], 2.0)
    eb, ec = torch.nonzero(slot >= 0, as_tuple=True)
    r = slot[eb, ec].long()
    candP[eb, ec] = pmark[r]
    candY[eb, ec] = t["cy"][r]
    candS[eb, ec] = t["cs"][r]
    okslot = torch.zeros((B, C), dtype=torch.bool, device=dev)
    okslot[eb, ec] = ok[r]
    arP = torch.arange(P, device=dev)
    origp = torch.cat([wp, candP], dim=1)
    allp = origp.clone()
    dead = arP[None, :] >= wn[:, None]
    allp[:, :P, 2] = torch.where(dead, 2.0, allp[:, :P, 2])                          # infeasible marker
    fr = RW.front_hv(allp, torch.full((B,), P + C, dtype=torch.int32, device=dev), None, max_front=max_front, lib=lib)
    fidx = fr["front_idx"][:, :max_out].long()
    take = fidx.clamp(min=0)
    ally = torch.cat([wy, candY], dim=1)
    alls = torch.cat([ws, candS], dim=1)
    rows = torch.arange(B, device=dev)[:, None]
    live = (fidx >= 0)[:, :, None]
    newp = torch.where(live, origp[rows, take], 0.0)
    newp[:, :, 0:2].clamp_(max=1.0)
    infront = torch.zeros((B, P + C), dtype=torch.bool, device=dev)
    infront.scatter_(1, take, live[:, :, 0])
    return dict(points=newp, y=torch.where(live, ally[rows, take], 0.0), sec=torch.where(live, alls[rows, take], 0),
                n=fr["n_front"].clamp(max=max_out), accepted=(infront[:, P:] & okslot).to(torch.uint8), front_idx=fr["front_idx"][:, :max_out],
                hv_front=fr["hv_front"], metrics=fr["metrics"], allp=allp)


# ---- reference (b): host model ---------------------------------------------------------------------------------------------------------
def _d3(rows, order, max_front):
    """D3: both ends + the max_front - 2 interior rows of largest crowding distance (ties: earlier position), in front order"""
    nf = len(order)
    if not max_front or nf <= max_front:
        return order
    f = [rows[k] for k in order]
    d = [math.sqrt((f[k][0] - f[k + 1][0]) ** 2 + (f[k][1] - f[k + 1][1]) ** 2) for k in range(nf - 1)]
    cr = [d[0]] + [d[k - 1] + d[k] for k in range(1, nf - 1)] + [d[-1]]
    keep = {0, nf - 1} | set(sorted(range(1, nf - 1), key=lambda k: -cr[k])[:max_front - 2])
    return [order[k] for k in range(nf) if k in keep]


def _host_front(rows):
    """input rows of the front in the kernel's order (obj1, obj2, first of identical rows), before truncation"""
    feas = [k for k, r in enumerate(rows) if not (r[2] > 1 or r[3] > 1)]
    if not feas:
        return []
    fr = U.simple_cull_final([list(rows[k]) for k in feas])[0]
    first = {}
    for k in feas:
        first.setdefault(tuple(rows[k]), k)
    return sorted((first[tuple(r)] for r in fr), key=lambda k: (rows[k][0], rows[k][1], k))


def _host_model(c, max_front, max_out):
    """the whole entry on the host: the rows the cull sees (dead rows, empty slots and not-ok candidates marked as the header says),
    the front, D3, and the outputs gathered from the sources"""
    B, P = c["pts"].shape[:2]
    C = c["slot"].shape[1]
    out = dict(points=np.zeros((B, max_out, 4)), y=np.zeros((B, max_out, c["y"].shape[2]), np.float32),
               sec=np.zeros((B, max_out, c["sec"].shape[2]), np.int32), n=np.zeros(B, np.int32), accepted=np.zeros((B, C), np.uint8),
               front_idx=np.full((B, max_out), -1, np.int32), full=[])
    for b in range(B):
        rows = [list(r) for r in c["pts"][b]]
        for i in range(P):
            if i >= c["n"][b]:
                rows[i][2] = 2.0
        for s in range(C):
            r = c["slot"][b, s]
            row = list(EMPTY) if r < 0 else list(c["cand"][r])
            if not (row[2] <= 1 and row[3] <= 1):
                row[2] = 2.0
            rows.append(row)
        full = _host_front(rows)
        order = _d3(rows, full, max_front)
        out["full"].append(len(full))
        out["n"][b] = len(order)
        for j, k in enumerate(order):
            out["front_idx"][b, j] = k
            out["points"][b, j] = (min(rows[k][0], 1.0), min(rows[k][1], 1.0), rows[k][2], rows[k][3])
            if k < P:
                out["y"][b, j], out["sec"][b, j] = c["y"][b, k], c["sec"][b, k]
            else:
                r = c["slot"][b, k - P]
                out["y"][b, j], out["sec"][b, j] = c["cy"][r], c["cs"][r]
                out["accepted"][b, k - P] = 1
    return out


# ---- running the entry, comparing ----------------------------------------------------------------------------------------------------
def _merge(lib, t, max_front, max_out=None, slot="table", **kw):
    slot_row = t["slot"] if isinstance(slot, str) else slot
    return RW.archive_merge(t["pts"], t["n"], t["y"], t["sec"], t["cand"], t["cy"], t["cs"], slot_row, n_slots=t["slot"].shape[1],
                            max_front=max_front, max_out=max_out, lib=lib, **kw)


EXACT = ("points", "y", "sec", "n", "accepted")


def _same_as_torch(got, ref, extras=False):
    for k in EXACT + (("front_idx",) if extras else ()):
        assert torch.equal(got[k], ref[k]), k
    if extras:
        torch.testing.assert_close(got["hv_front"], ref["hv_front"], rtol=0, atol=1e-12)
        torch.testing.assert_close(got["metrics"], ref["metrics"], rtol=0, atol=1e-12)


def _same_as_host(got, want):
    for k in EXACT + ("front_idx",):
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k], err_msg=k)


def _zeros_behind_the_front(got):
    for b, n in enumerate(got["n"].tolist()):
        for k in ("points", "y", "sec"):
            assert torch.all(got[k][b, n:] == 0) and not torch.any(torch.signbit(got[k][b, n:].double())), (k, b)


# (P, C) of the engine's train shapes, 64 rows exactly, odd / even widths, max_front (0: not truncated)
ONE_WAVE = {
    "20+42": dict(P=20, C=42, n_y=5, n_sec=7, max_front=20),
    "50+12": dict(P=50, C=12, n_y=16, n_sec=36, max_front=50),
    "19+45": dict(P=19, C=45, n_y=5, n_sec=7, max_front=19),
    "20+42 to 8": dict(P=20, C=42, n_y=16, n_sec=36, max_front=8),
    "19+45 whole": dict(P=19, C=45, n_y=16, n_sec=36, max_front=0),
}
_CACHE = {}


def _one_wave(name):
    """case, host model (b) -- computed once per case, shared, never modified"""
    if name not in _CACHE:
        s = ONE_WAVE[name]
        c = _case(100 + sorted(ONE_WAVE).index(name), 12, s["P"], s["C"], s["n_y"], s["n_sec"])
        mf = s["max_front"]
        _CACHE[name] = (c, _host_model(c, mf, mf if mf else s["P"] + s["C"]), mf)
    return _CACHE[name]


def _generator_does_what_it_says(name, c, want, mf):
    n = c["n"]
    assert {0, 1, c["pts"].shape[1] - 1, c["pts"].shape[1]} <= set(n.tolist())
    assert (c["slot"] < 0).any() and np.isnan(c["cand"]).any() and (c["cand"][:, 2] == 1.01).any()
    if mf:
        assert max(want["full"]) > mf, f"{name}: no front longer than max_front {mf}: truncation would not run"
        assert sum(f > mf for f in want["full"]) >= 1 and min(want["full"]) < mf
    assert want["accepted"][1].any() and want["n"][1] == 1           # the dominating candidate alone
    assert not want["accepted"][2].any()                              # all dominated
    assert want["accepted"][4][-1] == 0 and want["accepted"][5].sum() >= 1 and want["accepted"][5][-1] == 0   # the first copy survives
    assert (want["points"][6, :want["n"][6], :2] == 1.0).any()        # clamped objectives
    assert want["n"][9] == 0 and want["n"][8] <= n[8]


# ---- 8 (not GPU): the test's own references against each other; refusals without the entry -------------------------------------------
@pytest.mark.parametrize("name", sorted(ONE_WAVE))
def test_host_model_agrees_with_the_torch_block_on_the_emulator(name):
    """(b) against (a) run on the emulator's truss_front, on the one-wave cases' inputs: the references of the GPU tests hold each
    other here.  Also what the generator promises: truncation really runs, every listed situation occurs."""
    c, want, mf = _one_wave(name)
    _generator_does_what_it_says(name, c, want, mf)
    ref = _torch_block(pc.emu_lib(), _t(c, "cpu"), mf, want["points"].shape[1])
    _same_as_host(ref, want)


def test_archive_path_on_the_emulator(monkeypatch):
    lib = pc.emu_lib()
    assert not lib.has_archive and _lib.ARCHIVE_MAXROWS == 256
    c, _, mf = _one_wave("20+42")
    t = _t(c, "cpu")
    with pytest.raises(tm.TrussError, match="has no truss_archive_merge"):
        _merge(lib, t, mf)
    with pytest.raises(tm.TrussError, match="has no truss_archive_merge$"):      # the operator itself, handed a library without the entry
        o = [torch.zeros(12, 20, 4, dtype=torch.float64), torch.zeros(12, 20, 5), torch.zeros(12, 20, 7, dtype=torch.int32),
             torch.zeros(12, dtype=torch.int32)]
        ops.call(ops.namespace().archive_merge, ops.bind(lib), 0, 20, 42, t["pts"], t["n"], t["y"], t["sec"], t["slot"], t["cand"], t["cy"],
                 t["cs"], *o, None, None, None, None)
    monkeypatch.delenv("TRUSS_ARCHIVE", raising=False)
    with contextlib.redirect_stdout(io.StringIO()):
        assert _engine(lib, "cpu", None).archive_path == "torch"
        with pytest.raises(ValueError, match="no truss_archive_merge"):
            _engine(lib, "cpu", "hip")
        with pytest.raises(ValueError, match="archive_path must be"):
            _engine(lib, "cpu", "bogus")
        monkeypatch.setenv("TRUSS_ARCHIVE", "hip")
        with pytest.raises(ValueError, match="no truss_archive_merge"):
            _engine(lib, "cpu", None)
        assert _engine(lib, "cpu", "torch").archive_path == "torch"            # an explicit choice wins over the environment


def test_archive_operator_meta_registration():
    ns = ops.namespace()
    assert "truss_archive_merge" in ops.entries()
    B, P, C, R = 3, 20, 42, 130
    m = lambda *s, dt=torch.float64: torch.empty(*s, dtype=dt, device="meta")
    i32, f32 = torch.int32, torch.float32
    ins = [m(B, P, 4), m(B, dt=i32), m(B, P, 5, dt=f32), m(B, P, 7, dt=i32), m(B, C, dt=i32), m(R, 4), m(R, 5, dt=f32), m(R, 7, dt=i32)]
    outs = [m(B, P, 4), m(B, P, 5, dt=f32), m(B, P, 7, dt=i32), m(B, dt=i32)]
    ns.archive_merge(0, 0, 20, C, *ins, *outs, m(B, C, dt=torch.uint8), m(B, P, dt=i32), m(B), m(B, 5))
    ns.archive_merge(0, 0, 20, C, *ins[:4], None, *ins[5:], *outs, None, None, None, None)
    sch = str(ns.archive_merge.default._schema)
    for out in ("Tensor(a!) pts_out", "Tensor(d!) n_out", "Tensor(e!)? accepted", "Tensor(h!)? metrics", "Tensor? slot_row"):
        assert out in sch, out


# ---- 1: one-wave shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ONE_WAVE))
def test_one_wave_against_torch_block_and_host_model(name):
    lib = tm.load()
    c, want, mf = _one_wave(name)
    assert not mf or max(want["full"]) > mf                          # truncation is active in this case
    t = _t(c, "cuda")
    O = want["points"].shape[1]
    got = _merge(lib, t, mf, O, extras=True)
    _same_as_torch(got, _torch_block(lib, t, mf, O), extras=True)
    _same_as_host(got, want)
    _zeros_behind_the_front(got)
    assert torch.all(got["front_idx"][torch.arange(O, device="cuda")[None, :] >= got["n"][:, None]] == -1)


# ---- 2: wide shapes (the 256-thread instance) ----------------------------------------------------------------------------------------
WIDE = {
    "50+150 to 50": dict(P=50, C=150, fronts=(3, 63, 64, 65, 128, 131), max_front=50, max_out=50),
    "50+150 whole": dict(P=50, C=150, fronts=(1, 63, 64, 65, 127, 129), max_front=0, max_out=200),
    "64+192 to 64": dict(P=64, C=192, fronts=(60, 64, 65, 128, 129, 256), max_front=64, max_out=64),
    "64+192 whole": dict(P=64, C=192, fronts=(0, 64, 65, 128, 193, 256), max_front=0, max_out=256),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_against_torch_block(name):
    lib = tm.load()
    s = WIDE[name]
    c = _wide_case(300 + sorted(WIDE).index(name), s["P"], s["C"], s["fronts"])
    t = _t(c, "cuda")
    ref = _torch_block(lib, t, s["max_front"], s["max_out"])
    full = _torch_block(lib, t, 0, s["P"] + s["C"])["n"].tolist()
    assert full == list(s["fronts"])                                  # front sizes on both sides of 64 and 128: the cross-wave prefix
    got = _merge(lib, t, s["max_front"], s["max_out"], extras=True)
    _same_as_torch(got, ref, extras=True)
    _zeros_behind_the_front(got)
    if s["max_front"]:
        assert got["n"].tolist() == [min(f, s["max_front"]) for f in s["fronts"]]


# ---- 3: slot_row forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slot_row_forms_agree():
    """dense candidates (slot_row = None: slot c of env b is row b C + c), the same through a table onto shuffled candidate arrays, and
    empty slots as -1 against dense rows that hold the infeasible row: equal outputs; `accepted` follows the slots, not the rows"""
    lib = tm.load()
    B, P, C = 7, 20, 42
    c = _case(41, B, P, C, 8, 7, extra_rows=0)
    c["slot"] = np.arange(B * C, dtype=np.int32).reshape(B, C)
    t = _t(c, "cuda")
    dense = _merge(lib, t, 20, slot=None, extras=True)
    assert int(dense["accepted"].sum()) >= 1
    perm = torch.randperm(B * C, generator=torch.Generator().manual_seed(5)).to("cuda")
    shuf = dict(t)
    for k in ("cand", "cy", "cs"):
        shuf[k] = torch.empty_like(t[k])
        shuf[k][perm] = t[k]
    shuf["slot"] = perm[t["slot"].long()].int()
    table = _merge(lib, shuf, 20, extras=True)
    for k in EXACT + ("front_idx", "hv_front", "metrics"):
        assert torch.equal(dense[k], table[k]), k
    # empty slots: -1 in the table == the row [0, 0, 2, 0] with a zero design in the dense arrays
    empty = torch.rand((B, C), generator=torch.Generator().manual_seed(6)).to("cuda") < 0.4
    holes = dict(t)
    holes["slot"] = torch.where(empty, -1, t["slot"])
    filled = dict(t)
    rows = t["slot"][empty].long()
    filled["cand"], filled["cy"], filled["cs"] = t["cand"].clone(), t["cy"].clone(), t["cs"].clone()
    filled["cand"][rows] = torch.tensor(EMPTY, dtype=torch.float64, device="cuda")
    filled["cy"][rows] = 0
    filled["cs"][rows] = 0
    a, b = _merge(lib, holes, 20), _merge(lib, filled, 20, slot=None)
    for k in EXACT:
        assert torch.equal(a[k], b[k]), k
    assert not torch.any(a["accepted"].bool() & empty)
    _same_as_torch(a, _torch_block(lib, holes, 20, 20))


# ---- 4: bounds and reproducibility -------------------------------------------------------------------------------------------------
def _sentinel_outs(B, O, C, n_y, n_sec, pad, extras=True):
    S = 77
    dts = dict(points=((O, 4), torch.float64), y=((O, n_y), torch.float32), sec=((O, n_sec), torch.int32), n=((), torch.int32),
               accepted=((C,), torch.uint8))
    if extras:
        dts.update(front_idx=((O,), torch.int32), hv_front=((), torch.float64), metrics=((5,), torch.float64))
    bufs = {k: torch.full((B + 2 * pad,) + s, S, dtype=dt, device="cuda") for k, (s, dt) in dts.items()}
    return bufs, {k: v[pad:pad + B] for k, v in bufs.items()}, S


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["20+42", "19+45 whole", "wide"])
def test_outputs_stay_in_bounds_and_are_reproducible(name):
    lib = tm.load()
    if name == "wide":
        c, mf, O = _wide_case(77, 50, 150, (5, 64, 65, 129, 200, 30, 1)), 50, 53          # max_out above max_front: 3 rows of zeros at least
    else:
        c, _, mf = _one_wave(name)
        O = (mf or 64) + 3
    t = _t(c, "cuda")
    B, P = c["pts"].shape[:2]
    C, pad = c["slot"].shape[1], 2

    def run(tt, nb):
        bufs, views, S = _sentinel_outs(nb, O, C, c["y"].shape[2], c["sec"].shape[2], pad)
        assert all(v.is_contiguous() for v in views.values())
        got = RW.archive_merge(tt["pts"], tt["n"], tt["y"], tt["sec"], tt["cand"], tt["cy"], tt["cs"], tt["slot"], max_front=mf, max_out=O,
                               extras=True, out=views, lib=lib)
        torch.cuda.synchronize()
        for k, buf in bufs.items():
            assert got[k].data_ptr() == views[k].data_ptr()
            assert torch.all(buf[:pad] == S) and torch.all(buf[pad + nb:] == S), k
        return bufs, got

    (b1, g1), (b2, _) = run(t, B), run(t, B)
    for k in b1:
        assert torch.equal(b1[k], b2[k]), k
    _zeros_behind_the_front(g1)
    assert torch.all(g1["n"] <= (mf or P + C))
    rows = min(O, P + C)                                              # the torch block has no rows beyond P + C; the entry's are zeros (above)
    cut = {k: (v[:, :rows] if k in ("points", "y", "sec", "front_idx") else v) for k, v in g1.items()}
    _same_as_torch(cut, _torch_block(lib, t, mf, rows), extras=True)
    # the result of an env does not depend on the batch: 5 envs alone
    few = dict(t)
    for k in ("pts", "n", "y", "sec", "slot"):
        few[k] = t[k][:5].contiguous()
    _, g5 = run(few, 5)
    for k in g5:
        assert torch.equal(g5[k], g1[k][:5]), k


# ---- 5: argument checks ---------------------------------------------------------------------------------------------------------------
def _raw_args(lib, t, outs, mf, **over):
    P, C = t["pts"].shape[1], t["slot"].shape[1]
    a = _lib.ArchiveArgs()
    a.struct_size = ctypes.sizeof(_lib.ArchiveArgs)
    a.n_envs, a.max_points, a.n_slots, a.max_front, a.max_out = t["pts"].shape[0], P, C, mf, outs["points"].shape[1]
    a.n_y, a.n_sec, a.n_cand_rows = t["y"].shape[2], t["sec"].shape[2], t["cand"].shape[0]
    for f, k in (("pts_in", "pts"), ("n_in", "n"), ("y_in", "y"), ("sec_in", "sec"), ("slot_row", "slot"), ("cand_points", "cand"),
                 ("cand_y", "cy"), ("cand_sec", "cs")):
        setattr(a, f, t[k].data_ptr())
    for f, k in (("pts_out", "points"), ("y_out", "y"), ("sec_out", "sec"), ("n_out", "n"), ("accepted", "accepted")):
        setattr(a, f, outs[k].data_ptr())
    for f, v in over.items():
        setattr(a, f, v)
    return a


@pytest.mark.gpu
def test_argument_checks_refuse_and_write_nothing():
    lib = tm.load()
    c, _, mf = _one_wave("20+42")
    t = _t(c, "cuda")
    B, P, C, ny, ns = 12, 20, 42, 5, 7
    bufs, outs, S = _sentinel_outs(B, P, C, ny, ns, 1, extras=False)
    assert ctypes.sizeof(_lib.ArchiveArgs) == 8 + 10 * 4 + 16 * 8   # size_t, ten 32-bit words, sixteen pointers: truss_archive_args_t

    def raw(match, **over):
        rc = lib.dll.truss_archive_merge(ctypes.byref(_raw_args(lib, t, outs, mf, **over)), None)
        assert rc == -1
        with pytest.raises(tm.TrussError, match=match):
            lib.check(rc, "truss_archive_merge")

    raw("struct_size", struct_size=8)
    raw("n_envs < 0", n_envs=-1)
    raw("max_points", max_points=0)
    raw("n_slots", n_slots=-1)
    raw("256 rows", max_points=215)
    raw("max_front", max_front=1)
    raw("max_front", max_front=-2)
    raw("max_out", max_out=19)
    raw("max_out", max_front=0)                                       # untruncated needs P + C = 62 rows, the outputs have 20
    raw("n_y / n_sec", n_y=0)
    raw("n_y / n_sec", n_sec=0)
    raw("n_cand_rows", n_cand_rows=-1)
    raw("slot_row NULL needs", slot_row=None, n_cand_rows=B * C - 1)
    for f in ("pts_in", "n_in", "y_in", "sec_in", "cand_points", "cand_y", "cand_sec", "pts_out", "y_out", "sec_out", "n_out"):
        raw("NULL", **{f: None})
    raw("output y_out overlaps input y_in", y_out=t["y"].data_ptr())
    raw("output pts_out overlaps input pts_in", pts_out=t["pts"].data_ptr() + 32)
    raw("output n_out overlaps input slot_row", n_out=t["slot"].data_ptr() + 4 * B * C - 4 * B)
    raw("output accepted overlaps output sec_out", accepted=outs["sec"].data_ptr() + 4)
    # through the operator and the wrapper
    with pytest.raises(tm.TrussError, match="output y_out overlaps input y_in"):
        _merge(lib, t, mf, out=dict(y=t["y"]))
    with pytest.raises(ValueError, match="at most 256 rows"):
        RW.archive_merge(torch.zeros(2, 215, 4, dtype=torch.float64, device="cuda"), t["n"][:2], torch.zeros(2, 215, ny, device="cuda"),
                         torch.zeros(2, 215, ns, dtype=torch.int32, device="cuda"), t["cand"], t["cy"], t["cs"], t["slot"][:2], lib=lib)
    with pytest.raises(ValueError, match="needs n_slots"):
        RW.archive_merge(t["pts"], t["n"], t["y"], t["sec"], t["cand"], t["cy"], t["cs"], None, lib=lib)
    with pytest.raises(tm.TrussError, match="max_front must be 0"):
        _merge(lib, t, 1, P, out=outs)
    with pytest.raises(tm.TrussError, match="max_out is smaller"):
        _merge(lib, t, 0, P, out=outs)
    with pytest.raises(tm.TrussError, match="pts_in must be Double"):
        _merge(lib, dict(t, pts=t["pts"].float()), mf, out=outs)
    with pytest.raises(tm.TrussError, match="cand_y must be \\[R, n_y\\]"):
        _merge(lib, dict(t, cy=t["cy"][:, :4].contiguous()), mf, out=outs)
    with pytest.raises(tm.TrussError, match="slot_row must be contiguous"):
        _merge(lib, t, mf, slot=t["slot"].t().contiguous().t(), out=outs)
    with pytest.raises(tm.TrussError, match="y_out must be \\[B, max_out, n_y\\]"):
        _merge(lib, t, mf, out=dict(outs, y=torch.zeros(B, P + 1, ny, device="cuda")))
    torch.cuda.synchronize()
    for k, buf in bufs.items():
        assert torch.all(buf == S), k
    assert torch.equal(t["y"], torch.tensor(c["y"], device="cuda")) and torch.equal(t["pts"], torch.tensor(c["pts"], device="cuda"))
    # no envs: returns cleanly, empty tensors
    e = dict(t)
    for k in ("pts", "n", "y", "sec", "slot"):
        e[k] = t[k][:0].contiguous()
    got = _merge(lib, e, mf, extras=True)
    assert got["points"].shape == (0, P, 4) and got["y"].shape == (0, P, ny) and got["sec"].shape == (0, P, ns) and got["n"].shape == (0,)
    assert got["accepted"].shape == (0, C) and got["metrics"].shape == (0, 5)


# ---- 6: the engine, train game -------------------------------------------------------------------------------------------------------
def _agents(device, seed, hidden=16):
    torch.manual_seed(seed)
    return RL.MADDPG(M.lr, M.ep, M.epd, M.gamma, hidden, 8, 100, M.num_agents, M.num_action, M.mu, M.theta, M.sigma, device=device)


def _engine(lib, device, archive_path, rl=None, B=6, num_x=4, seed=3, **kw):
    topo = tm.TrussTopology.grid(num_x)
    eng = marl.BatchedMARL(topo, B, rl or _agents(device, seed), max_front=6, lib=lib, device=device, replay_capacity=256, batch_size=8,
                           seed=seed, tune_update_gemms=False, archive_path=archive_path, **kw)
    b = synthetic.random_batch(topo, B, seed)
    eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
    return eng


def _same_step(a, b):
    for k in ("hv", "n_front", "reward"):
        assert torch.equal(a[k], b[k]), k
    assert a["replay_added"] == b["replay_added"] and a["replay_size"] == b["replay_size"]


def _same_archive(ea, eb):
    for name in ("pts", "arch_y", "arch_sec", "n"):
        assert torch.equal(getattr(ea, name), getattr(eb, name)), name


@pytest.mark.gpu
@pytest.mark.parametrize("reward_path", ["torch", "hip"])
def test_engine_plays_the_same_train_game(reward_path):
    """8 nodes, B = 6, max_front = 6, three game steps without exploration; the two engines share one set of agents (nothing is
    updated) and differ in archive_path only.  Then three more steps with train=True, update=False: the replays hold the same rows.
    Both halves with either reward_path."""
    lib = tm.load()
    rl = _agents("cuda", 3)
    with contextlib.redirect_stdout(io.StringIO()):
        et, eh = (_engine(lib, "cuda", p, rl, reward_path=reward_path) for p in ("torch", "hip"))
        assert (et.archive_path, eh.archive_path) == ("torch", "hip")
        for _ in range(3):
            _same_step(et.game_step_all(train=False, explore=False), eh.game_step_all(train=False, explore=False))
            _same_archive(et, eh)
        assert int(eh.n.max()) >= 2
        for _ in range(3):
            _same_step(et.game_step_all(train=True, explore=False, update=False), eh.game_step_all(train=True, explore=False, update=False))
            _same_archive(et, eh)
    assert et.replay.size == eh.replay.size >= 1
    gt, gh = (torch.Generator(device="cuda").manual_seed(11) for _ in range(2))
    St, NSt, *rest_t = et.replay.sample(8, gt)
    Sh, NSh, *rest_h = eh.replay.sample(8, gh)
    for a, b in zip(rest_t, rest_h):
        assert torch.equal(a, b)
    for dt, dh in zip([St] + NSt, [Sh] + NSh):
        for k in dt:
            assert torch.equal(dt[k], dh[k]), k


@pytest.mark.gpu
def test_mixed_engine_forwards_archive_path():
    from truss_mi355 import pool
    lib = tm.load()
    mixes = []
    rl = _agents("cuda", 4)
    with contextlib.redirect_stdout(io.StringIO()):
        for path in ("torch", "hip"):
            classes = pool.grid_classes([4, 8], [6, 5])
            mix = marl.MixedMARL(classes, rl, bucket_envs=3, max_front=6, lib=lib, device="cuda", replay_capacity=128, batch_size=4, seed=2,
                                 tune_update_gemms=False, archive_path=path)
            per_class = []
            for k, e in enumerate(mix.engines):
                full = synthetic.random_batch(e.topo, classes[mix.class_ids[k]][1], 9 + k)
                per_class.append({key: v[mix.global_ids(k)] for key, v in full.items()})
            mix.reset(per_class)
            assert len(mix.engines) == 2 and all(e.archive_path == path for e in mix.engines)
            mixes.append(mix)
        for _ in range(2):
            ot, oh = (m.game_step_all(train=False, explore=False) for m in mixes)
            for a, b in zip(ot["per_class"], oh["per_class"]):
                _same_step(a, b)
            for ea, eb in zip(mixes[0].engines, mixes[1].engines):
                _same_archive(ea, eb)


# ---- 7: the engine, design game ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_engine_plays_the_same_design_game():
    lib = tm.load()
    topo = tm.TrussTopology.grid(4, "small")
    rl = _agents("cuda", 5)
    outs, engs = [], []
    with contextlib.redirect_stdout(io.StringIO()):
        for path in ("torch", "hip"):
            eng = marl.BatchedMARL(topo, 5, rl, lib=lib, device="cuda", seed=3, game="test", max_front=6, tune_update_gemms=False,
                                   archive_path=path)
            b = synthetic.random_batch(topo, 5, 3)
            eng.reset(b["x"], b["target"], b["y_max"], b["d_min"], b["max_def"], b["load_x"], b["load_y"], b["is_roof"], b["y"], b["sec"])
            outs.append(eng.design_episode(end_step=3, explore=False))
            engs.append(eng)
    ot, oh = outs
    assert engs[1].archive_path == "hip"
    for k in ("hv", "n_front", "R", "G_U"):
        assert torch.equal(ot[k], oh[k]), k
    assert set(ot["final"]) == set(oh["final"]) == {"points", "y", "sec", "n", "hv", "metrics"}
    for k in ot["final"]:
        assert ot["final"][k].shape == oh["final"][k].shape and ot["final"][k].dtype == oh["final"][k].dtype, k
        assert torch.equal(ot["final"][k], oh["final"][k]), k
    _same_archive(*engs)
    assert int(oh["final"]["n"].max()) >= 2
