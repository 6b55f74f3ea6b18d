"""The uniform-entry segments of the dense z-sum (csrc/lzq_quad.h zsum_dispatch / zsum_uniform),
on the CPU.  tests/zsum_segments_host.cpp compiles the LZQ_HD functions of
csrc/lzq_exp2.h that the device code itself calls -- the segment predicates, the batch search, the
segment's table value and the uniform node -- and evaluates a 64-lane pass twice: with the
segmented dispatch, and with the single general loop (lzq::exp2_tab_scaled at every node).  The
two F must agree bit for bit in every lane, and the dispatch must take the path the regime names
(so that the uniform loop really is what the comparison exercises).

Lane sets are given as c2N = c2 * 8192 directly, so that a lane can sit exactly on a boundary of
the loop's own expression t = fma(c2N, g, M); the boundaries are found by bisection on that
expression (through the library), not from a formula.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import zsum_ref as Z
from conftest import PKG_NAME, ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
GRIDS = ((1200, 30.0), (13, 3.0))       # the default grid, and a runtime grid padded 13 -> 16
N = 8192.0
ZERO, FREE, SPLIT = 0, 1, 2             # plan[0] of zsum_segments_host.cpp
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


def load_lib():
    so = os.path.join(tempfile.mkdtemp(), "zsum_segments_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "zsum_segments_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.zseg_passes.argtypes = [ctypes.c_int, ctypes.c_int, DP, DP, ctypes.c_int, DP, ctypes.c_long, DP, IP]
    for f in (L.zseg_zero, L.zseg_clamped, L.zseg_dead):
        f.argtypes = [ctypes.c_double, ctypes.c_double]
    return L


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def run(L, g, c2, segmented, truncate):
    c2 = np.ascontiguousarray(np.asarray(c2, float).reshape(-1, 64))
    F = np.empty_like(c2)
    plan = np.empty((c2.shape[0], 3), np.int32)
    g4, om = np.ascontiguousarray(g.g4), np.ascontiguousarray(g.om)
    rc = L.zseg_passes(int(segmented), int(truncate), g4.ctypes.data_as(DP), om.ctypes.data_as(DP), g.nz,
                       c2.ctypes.data_as(DP), c2.shape[0], F.ctypes.data_as(DP), plan.ctypes.data_as(IP))
    assert rc == 0
    return F, plan


def both(L, g, c2, truncate):
    """(F, plan) of the segmented dispatch after checking it against the single general loop."""
    Fs, plan = run(L, g, c2, 1, truncate)
    Fg, pg = run(L, g, c2, 0, truncate)
    assert np.array_equal(Fs.view(np.int64), Fg.view(np.int64)), "segmented and general F differ"
    assert np.array_equal(plan[:, 2], pg[:, 2]) and np.all(plan[:, 2] % 8 == 0)
    return Fs, plan


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _dbl(i):
    return float(np.int64(i).view(np.float64))


def first_true(pred):
    """The negative double of smallest magnitude at which pred holds (pred monotone in |c2|)."""
    lo, hi = _bits(2.0 ** -300), _bits(2.0 ** 300)
    assert not pred(-_dbl(lo)) and pred(-_dbl(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(-_dbl(mid)):
            hi = mid
        else:
            lo = mid
    return -_dbl(hi)


def padded(g):
    nzp = (max(g.nz, 8) + 7) // 8 * 8
    return np.concatenate([g.g4, np.full(nzp - g.nz, g.g4[-1])])


def expected_k2(L, gp, c2, kend):
    """Brute force over the batch starts: the first at which every lane is clamped."""
    for k in range(0, kend, 8):
        if all(L.zseg_clamped(float(c), float(gp[k])) for c in c2):
            return k
    return kend


@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_zero_and_dead_regimes(lib, nz, z_max, truncate):
    g = Z.grid(nz, z_max)
    g_1, g_max = float(g.g4[1]), float(g.g4[-1])
    # the last c2 whose t at g_max is still M, and its neighbour beyond
    c_out = first_true(lambda c: not lib.zseg_zero(c, g_max))
    c_in = float(np.nextafter(c_out, 0.0))
    assert lib.zseg_zero(c_in, g_max) and not lib.zseg_zero(c_out, g_max)
    assert abs(c_in * g_max) <= 0.5 < abs(c_out * g_max) * (1 + 1e-15)
    c_dead = first_true(lambda c: bool(lib.zseg_dead(c, g_1)))
    below = -np.geomspace(abs(c_in) * 1e-30, abs(c_in), 64)
    F, plan = both(lib, g, below, truncate)                              # all below the zero boundary
    assert plan[0, 0] == ZERO and np.all(F > 0) and np.all(F == F[0])    # every node's 2^u factor is the same
    lanes = below.copy()
    lanes[17] = c_in                                                     # one lane ON the boundary
    assert both(lib, g, lanes, truncate)[1][0, 0] == ZERO
    lanes[17] = c_out                                                    # ... and one ulp beyond it
    assert both(lib, g, lanes, truncate)[1][0, 0] == FREE
    dead = -np.geomspace(abs(c_dead), abs(c_dead) * 1e6, 64)
    F, plan = both(lib, g, dead, truncate)                               # all dead
    assert plan[0, 0] == ZERO and np.all(F == 0.0) and not np.any(np.signbit(F))
    # dead plus one live lane: below the zero boundary, clamp-free beyond it, and the last live c2
    for live, path in ((c_in * 0.5, ZERO), (c_out * 100.0, FREE), (float(np.nextafter(c_dead, 0.0)), SPLIT)):
        lanes = dead.copy()
        lanes[40] = live
        F, plan = both(lib, g, lanes, truncate)
        assert plan[0, 0] == path and np.all(np.delete(F[0], 40) == 0.0)
        assert F[0, 40] > 0.0 or path == SPLIT      # the last live c2 sums to a subnormal or to 0


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_clamped_regimes(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    gp = padded(g)
    kend = gp.size
    g_1 = float(g.g4[1])
    rng = np.random.default_rng(5)
    seen = set()
    # the least negative lane clamps first at node kt; the other lanes are more negative (not dead)
    kts = {3, 5, 8, kend // 2 - 3, kend // 2, kend - 16, kend - 9, kend - 8, kend - 3, g.nz - 1}
    for kt in sorted(k for k in kts if k >= 3):      # node 1 cannot clamp in a live lane (the dead rule)
        c_lo = first_true(lambda c: bool(lib.zseg_clamped(c, float(gp[kt]))))
        lanes = c_lo * (1.0 + 3.0 * rng.random(64))
        lanes[rng.integers(64)] = c_lo
        assert not any(lib.zseg_dead(float(c), g_1) for c in lanes)
        F, plan = both(lib, g, lanes, 0)
        want = expected_k2(lib, gp, lanes, kend)
        assert plan[0].tolist() == [SPLIT, want, kend], (kt, plan[0], want)
        seen.add(want)
        # truncation ends the pass before any node clamps in every lane: the general loop alone
        Ft, pt = both(lib, g, lanes, 1)
        assert pt[0, 0] == SPLIT and pt[0, 1] == pt[0, 2] <= want
        assert np.array_equal(F.view(np.int64), Ft.view(np.int64))
        # a clamp-free lane among them: no uniform suffix
        lanes[3] = first_true(lambda c: not lib.zseg_zero(c, float(gp[-1]))) * 4.0
        assert both(lib, g, lanes, 0)[1][0].tolist() == [SPLIT, kend, kend]
    print(f"grid ({nz}, {z_max}): k2 values covered {sorted(seen)} of kend = {kend}")
    assert {8, kend - 8, kend} <= seen and (kend == 16 or any(8 < k < kend - 8 for k in seen))


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_random_lane_sets(lib, nz, z_max):
    """A few thousand passes of 64 consecutive y, at lane spacings from the workload's 0.012 up to
    mixed waves, over every regime; truncation on and off."""
    g = Z.grid(nz, z_max)
    rng = np.random.default_rng(11)
    n = 2000
    y0 = rng.uniform(-52.0, 40.0, n)
    dy = rng.choice([0.0, 98.0 / 7999.0, 0.1, 1.0], n)
    ys = y0[:, None] + dy[:, None] * np.arange(64)[None, :]
    ys[::7] = rng.permuted(ys[::7], axis=1)
    c2 = ((-(0.34 / 6.0) * np.exp(np.clip(ys, -50.0, 50.0))) * Z.LOG2E) * N
    for truncate in (0, 1):
        F, plan = both(lib, g, c2, truncate)
        paths = np.bincount(plan[:, 0], minlength=3)
        suffix = int(np.sum((plan[:, 0] == SPLIT) & (plan[:, 1] < plan[:, 2])))
        print(f"grid ({nz}, {z_max}) truncate {truncate}: zero / clamp-free / clamped passes {paths.tolist()}, "
              f"{suffix} with a uniform suffix")
        assert np.all(paths > 100) and (truncate or suffix > 30)
