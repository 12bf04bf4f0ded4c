"""`truss_front` above 64 rows (the 256-thread kernel, include/truss_mi355.h): ragged batches of up to 256 rows per env
against the drop-in utils.simple_cull_final / union_rectangles_fastest, the D3 truncation against a Python restatement,
and the HIP kernel against the serial CPU restatement (tests/emu) on the same inputs.  Sets of at most 64 rows in the same
batch shapes go through the 64-thread instance of the same kernel (max_points <= 64) and must give the same results as before."""
import math

import numpy as np
import pytest
import torch

import truss_mi355 as tm
from truss_mi355 import reward as RW
import parity_common as pc
import utils as U

SIZES = (1, 63, 64, 65, 129, 200, 256)


def _sets(seed, P=256):
    """B = 4 x len(SIZES) envs: per size a random cloud (small fronts), a cloud on a grid (ties in obj1 / obj2, exact duplicates)
    and two noisy anti-diagonals (long fronts, the second on a grid).  Infeasible rows (con > 1), points > 1 everywhere."""
    rng = np.random.default_rng(seed)
    sizes = [min(s, P) for s in SIZES for _ in range(4)]
    B = len(sizes)
    pts = np.zeros((B, P, 4))
    for b, s in enumerate(sizes):
        kind = b % 4
        p = rng.uniform(0.05, 1.15, size=(P, 4))
        p[:, 2:] = rng.uniform(0.2, 1.06, size=(P, 2))
        if kind >= 2:                                                    # along x + y = 1.1: most rows non-dominated
            t = rng.uniform(0.0, 1.15, size=P)
            p[:, 0], p[:, 1] = t, np.clip(1.1 - t + rng.normal(0.0, 0.01, size=P), 0.0, None)
        if kind in (1, 3):
            p[:, :2] = np.round(p[:, :2] * 40) / 40
            k = max(1, s // 8)                                           # exact duplicates of earlier rows
            src, dst = rng.integers(0, max(1, s // 2), size=k), rng.integers(s // 2, s, size=k) if s > 1 else [0]
            p[dst] = p[src]
        p[0, 2:] = 0.5                                                   # at least one feasible row
        pts[b] = p
    n = np.array(sizes, np.int32)
    ref = rng.uniform(0.85, 1.0, size=(B, 2))
    return pts, n, ref


def _run(lib, device, pts, n, ref, max_front):
    t = lambda a: torch.tensor(a, device=device)
    out = RW.front_hv(t(pts), t(n), t(ref), max_front=max_front, lib=lib)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_reference(out, pts, n, ref, min_long=4):
    """no truncation: front set and order, n_front, metrics and both HVs against the drop-in utils"""
    long_fronts = 0
    for b in range(len(n)):
        rows = [list(r) for r in pts[b, :n[b]]]
        fr, max_d, dis_d, p_cd, sum_d, std_cd = U.simple_cull_final(rows)
        nf = out["n_front"][b]
        assert nf == len(fr), b
        idx = out["front_idx"][b]
        assert np.all(idx[nf:] == -1) and np.all((idx[:nf] >= 0) & (idx[:nf] < n[b]))
        got = [tuple(pts[b, k]) for k in idx[:nf]]
        assert sorted(got) == sorted(tuple(r) for r in fr), b            # same set of rows
        assert [g[0] for g in got] == [r[0] for r in fr], b              # same obj1 order; tied obj1 rows compared as a set above
        keys = [(g[0], g[1], k) for g, k in zip(got, idx[:nf])]
        assert keys == sorted(keys), b                                   # the kernel's tie order: (obj2, input row)
        if len({g[0] for g in got}) == len(got):                         # the metrics depend on the order of tied rows
            np.testing.assert_allclose(out["metrics"][b], [max_d, dis_d, p_cd, sum_d, std_cd], rtol=0, atol=1e-12)
        hv = U.union_rectangles_fastest(fr, +1, -1, ref_point=list(ref[b]))
        hva = U.union_rectangles_fastest(rows, +1, -1, ref_point=list(ref[b]))
        assert abs(out["hv_front"][b] - hv) <= 1e-12 and abs(out["hv_all"][b] - hva) <= 1e-12, b
        long_fronts += nf > 64
    assert long_fronts >= min_long                                       # the cases exercise fronts longer than one wave


def _d3(pts_b, full_idx, max_front):
    """D3 restated: both ends + the max_front - 2 interior points of largest crowding distance (ties: earlier position),
    in front order"""
    f = [pts_b[k] for k in full_idx]
    nf = len(f)
    if nf <= max_front:
        return list(full_idx)
    d = [math.sqrt((f[k][0] - f[k + 1][0]) ** 2 + (f[k][1] - f[k + 1][1]) ** 2) for k in range(nf - 1)]
    cr = [d[0]] + [d[k - 1] + d[k] for k in range(1, nf - 1)] + [d[-1]]
    mid = sorted(range(1, nf - 1), key=lambda k: -cr[k])                 # stable: ties keep position order
    keep = {0, nf - 1} | set(mid[:max_front - 2])
    return [full_idx[k] for k in range(nf) if k in keep]


def _check_truncation(out_t, out_full, pts, n, max_front):
    cut = 0
    for b in range(len(n)):
        full = list(out_full["front_idx"][b, :out_full["n_front"][b]])
        want = _d3(pts[b], full, max_front)
        nt = out_t["n_front"][b]
        assert nt == len(want) == min(len(full), max_front), b
        assert list(out_t["front_idx"][b, :nt]) == want and np.all(out_t["front_idx"][b, nt:] == -1), b
        cut += len(full) > max_front
    assert cut >= 4


def _same(a, b, what):
    for k in ("front_idx", "n_front"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    for k in ("hv_front", "hv_all", "metrics"):
        np.testing.assert_allclose(a[k], b[k], rtol=0, atol=1e-12, err_msg=f"{what}: {k}")


def _check(lib, device, seed, P=256, min_long=4, max_fronts=(20, 50)):
    pts, n, ref = _sets(seed, P)
    full = _run(lib, device, pts, n, ref, 0)
    _check_reference(full, pts, n, ref, min_long)
    for mf in max_fronts:
        _check_truncation(_run(lib, device, pts, n, ref, mf), full, pts, n, mf)
    return pts, n, ref, full


# max_points strictly between 64 and 256: the 256-thread kernel with fewer rows than threads.  200 rows is what the design game
# culls; 65 rows put one row into the second wave, the smallest shape at which the prefix across waves can go wrong -- there
# _sets() makes no front longer than 64 (so no long-front cap) and only one or two longer than 50 (so truncation to 20 only).
BETWEEN = {200: dict(P=200), 65: dict(P=65, min_long=0, max_fronts=(20,))}


def test_front_wide_emulated():
    _check(pc.emu_lib(), "cpu", 5)


@pytest.mark.parametrize("P", sorted(BETWEEN))
@pytest.mark.parametrize("seed", [5, 6])
def test_front_between_emulated(seed, P):
    _check(pc.emu_lib(), "cpu", seed, **BETWEEN[P])


def test_front_limits_emulated():
    lib = pc.emu_lib()
    z = torch.zeros((2, 257, 4), dtype=torch.float64)
    with pytest.raises(Exception):
        RW.front_hv(z, torch.ones(2, dtype=torch.int32), None, 0, lib)
    out = RW.front_hv(torch.zeros((2, 256, 4), dtype=torch.float64), torch.tensor([0, 256], dtype=torch.int32), None, 0, lib)
    assert out["n_front"].tolist() == [0, 1] and out["hv_front"].tolist() == [0.0, 1.0]


def _check_hip(seed, **shape):
    pts, n, ref, full = _check(tm.load(), "cuda", seed, **shape)
    emu = pc.emu_lib()
    _same(full, _run(emu, "cpu", pts, n, ref, 0), "no truncation")
    for mf in shape.get("max_fronts", (20, 50)):
        _same(_run(tm.load(), "cuda", pts, n, ref, mf), _run(emu, "cpu", pts, n, ref, mf), f"max_front {mf}")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [5, 6])
def test_front_wide_hip(seed):
    _check_hip(seed)


@pytest.mark.gpu
@pytest.mark.parametrize("P", sorted(BETWEEN))
@pytest.mark.parametrize("seed", [5, 6])
def test_front_between_hip(seed, P):
    _check_hip(seed, **BETWEEN[P])


@pytest.mark.gpu
def test_front_narrow_unchanged_hip():
    """at most 64 rows: the 64-thread instance of the same kernel, bitwise the same as the emulator's decisions and within 1e-12 in the sums"""
    pts, n, ref = _sets(7, P=64)
    for mf in (0, 20):
        _same(_run(tm.load(), "cuda", pts, n, ref, mf), _run(pc.emu_lib(), "cpu", pts, n, ref, mf), f"64 rows, max_front {mf}")
