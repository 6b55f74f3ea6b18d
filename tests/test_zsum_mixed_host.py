"""The clamped pass that holds dead lanes (csrc/lzq_quad.h zsum_dispatch's last branch and
zsum_uniform_lane, LZQ_PASS_LEAN; csrc/lzq_exp2.h seg_clamped_or_dead / seg_entry_lane), on the CPU.

A dead lane runs with c2e = +0.0: its t is M at every node, so it never passes seg_clamped and the
parent's search found no batch from which all 64 lanes are clamped -- the whole pass ran the clamped
general loop.  But the dead lane's clamped magic sum max(M, M + KMIN) is the constant M, so from the
first batch k2 at which every LIVE lane is clamped each lane reads one entry of its own at every node:
the new dispatch runs those nodes through the six-operation uniform node with the entry held per lane
(T''[0] for a dead lane, the entry of M + KMIN for the others).

tests/zsum_mixed_host.cpp evaluates a 64-lane pass with that dispatch (NEW), with the parent's (PARENT)
and with the single general loop (GENERAL) from the LZQ_HD functions the device code itself calls.  The
raw F before the dead lanes are zeroed must agree bit for bit between the three, and so must a checksum
over the bits of every node's value (F's rounding swallows a late node that is an ulp off; the checksum
does not).  k2 is checked against a brute-force scan of every node with the loop's own clamped sum.

Two deliberately broken dispatches (the per-lane entry taken from the clamp constant for dead lanes too;
the suffix started a batch early) must be told from the right one.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import test_zsum_dead_segment_host as HD
import zsum_ref as Z
from conftest import PKG_NAME, ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
GRIDS = ((1200, 30.0), (13, 3.0), (2400, 30.0))   # the default grid, a runtime grid padded 13 -> 16, a fine one
GENERAL, PARENT, NEW = -1, 0, 1                   # `mode` of zmixed_passes
ZERO, FREE, SPLIT, DEAD, MIXED = 0, 1, 2, 3, 4    # plan[0]
ENTRY_FROM_CLAMP, BATCH_EARLY = 1, 2              # `defect`
DP, IP, UP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)
bits = HD.bits
padded = HD.padded


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(tempfile.mkdtemp(), "zsum_mixed_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "zsum_mixed_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.zmixed_passes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, DP, DP, ctypes.c_int, DP, ctypes.c_long,
                                DP, DP, UP, IP]
    L.zmixed_tc.argtypes = [ctypes.c_double, DP, ctypes.c_int, DP]
    L.zmixed_tclamp.restype = ctypes.c_double
    L.zmixed_magic.restype = ctypes.c_double
    return L


@pytest.fixture(scope="module")
def dlib():
    return HD.load_lib()


def run(L, g, c2, mode, truncate, defect=0):
    """(raw F, F, checksum of the node values, plan = [path, k2, kend, dead lanes]) of the passes of 64 lanes in c2."""
    c2 = np.ascontiguousarray(np.asarray(c2, float).reshape(-1, 64))
    raw, F, V = np.empty_like(c2), np.empty_like(c2), np.empty(c2.shape, np.uint64)
    plan = np.empty((c2.shape[0], 4), np.int32)
    g4, om = np.ascontiguousarray(g.g4), np.ascontiguousarray(g.om)
    rc = L.zmixed_passes(int(mode), int(defect), int(truncate), g4.ctypes.data_as(DP), om.ctypes.data_as(DP), g.nz,
                         c2.ctypes.data_as(DP), c2.shape[0], raw.ctypes.data_as(DP), F.ctypes.data_as(DP),
                         V.ctypes.data_as(UP), plan.ctypes.data_as(IP))
    assert rc == 0
    return raw, F, V, plan


def same(a, b):
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
            and np.array_equal(a[2], b[2]))


def three(L, g, c2, truncate):
    """The new dispatch's result, after checking raw F, F and the node checksum against the parent's
    dispatch and the single general loop."""
    new = run(L, g, c2, NEW, truncate)
    for mode in (PARENT, GENERAL):
        got = run(L, g, c2, mode, truncate)
        assert np.array_equal(bits(new[0]), bits(got[0])), ("raw F differs from mode", mode)
        assert np.array_equal(bits(new[1]), bits(got[1])), ("F differs from mode", mode)
        assert np.array_equal(new[2], got[2]), ("node values differ from mode", mode)
        assert np.array_equal(new[3][:, 2:], got[3][:, 2:])       # kend and the dead lanes
    return new


def scan_k2(L, live, gp, kend):
    """Brute force over ALL executed nodes: the first batch start from which every LIVE lane's clamped magic
    sum is M + KMIN; kend if there is none.  Also checks that 'clamped' is monotone in k for every lane."""
    tclamp = L.zmixed_tclamp()
    ok = np.ones(kend, bool)
    for c in np.unique(live):
        v = np.empty(gp.size)
        assert L.zmixed_tc(float(c), gp.ctypes.data_as(DP), gp.size, v.ctypes.data_as(DP)) == 0
        f = v[:kend] == tclamp
        assert np.all(np.diff(f.astype(int)) >= 0), c
        ok &= f
    starts = np.flatnonzero(ok[::8]) * 8
    return int(starts[0]) if starts.size else kend


def clamped_lanes(dlib, g, n, deep=False):
    """n live lanes that clamp inside the pass: from just beyond the clamp-free boundary (which clamps at the
    last nodes only) to the last live c2N; deep: the 10% next to the dead threshold, which clamp early."""
    _, c_free, c_live, _ = HD.thresholds(dlib, g)
    return -np.geomspace(abs(c_live) * 0.9 if deep else abs(c_free) * 1.001, abs(c_live), n)


def mixed_wave(dlib, g, where, deep=False):
    """64 lanes: dead at the boolean mask `where`, clamped elsewhere."""
    c_dead = HD.thresholds(dlib, g)[3]
    lanes = np.empty(64)
    lanes[where] = HD.dead_lanes(c_dead)[:int(where.sum())]
    lanes[~where] = clamped_lanes(dlib, g, int((~where).sum()), deep)
    return lanes


def masks():
    """d = 1, 32, 63 dead lanes (spread over the wave), and a single dead lane at 0 / 31 / 63."""
    out = {}
    for d in (1, 32, 63):
        m = np.zeros(64, bool)
        m[np.linspace(5, 58, d).round().astype(int) if d < 63 else np.arange(64) != 40] = True
        assert m.sum() == d
        out[f"d{d}"] = m
    for lane in (0, 31, 63):
        m = np.zeros(64, bool)
        m[lane] = True
        out[f"lane{lane}"] = m
    return out


@pytest.mark.parametrize("deep", [False, True])
@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("mix", list(masks()))
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_mixed_pass_has_the_general_loops_bits(lib, dlib, nz, z_max, mix, truncate, deep):
    g = Z.grid(nz, z_max)
    where = masks()[mix]
    lanes = mixed_wave(dlib, g, where, deep)
    raw, F, V, plan = three(lib, g, lanes, truncate)
    path, k2, kend, ndead = plan[0].tolist()
    assert path == MIXED and ndead == int(where.sum())
    assert np.all(F[0, where] == 0.0) and not np.any(np.signbit(F[0, where]))
    assert np.array_equal(bits(F[0, ~where]), bits(raw[0, ~where]))
    # what the zeroing hides: a dead lane summed omega'_k T''[0] (A^2 + beta) over the executed nodes
    assert np.all(raw[0, where] > 0.0) and len(set(bits(raw[0, where]).tolist())) == 1
    # k2: brute force over the live lanes alone; the parent's search over all 64 finds no batch
    assert kend % 8 == 0 and k2 % 8 == 0
    assert k2 == scan_k2(lib, lanes[~where], padded(g), kend)
    parent = run(lib, g, lanes, PARENT, truncate)[3][0].tolist()
    assert parent[0] == SPLIT and parent[1] == kend
    if deep and not truncate:
        assert k2 < kend                                          # the suffix is not empty on a dense pass
    print(f"({nz}, {z_max}) {mix} truncate={truncate}: k2 = {k2} of {kend}")


@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_controls_keep_their_plan(lib, dlib, nz, z_max, truncate):
    """An all-clamped and an all-dead wave keep their old plan; dead lanes among zero or clamp-free lanes are
    a zero pass (a dead lane is a zero lane, and small), never the new branch."""
    g = Z.grid(nz, z_max)
    c_zero, c_free, c_live, c_dead = HD.thresholds(dlib, g)
    clamped = clamped_lanes(dlib, g, 64)
    new, par = three(lib, g, clamped, truncate), run(lib, g, clamped, PARENT, truncate)
    assert new[3][0].tolist() == par[3][0].tolist() and new[3][0, 0] == SPLIT and new[3][0, 3] == 0
    assert new[3][0, 1] == scan_k2(lib, clamped, padded(g), int(new[3][0, 2]))
    dead = HD.dead_lanes(c_dead)
    new, par = three(lib, g, dead, truncate), run(lib, g, dead, PARENT, truncate)
    assert new[3][0].tolist() == par[3][0].tolist() and new[3][0, 0] == DEAD and new[3][0, 3] == 64
    # dead plus clamp-free cannot reach the last branch: every lane is `small`, so the pass is clamp-free
    # (or zero), and the plan never claims the mixed path for it
    for live, path in ((-np.geomspace(abs(c_zero) * 4.0, abs(c_free), 32), FREE),
                       (-np.geomspace(abs(c_zero) * 1e-30, abs(c_zero), 32), ZERO)):
        for first in (0, 1):
            lanes = HD.dead_lanes(c_dead)
            lanes[first::2] = live
            new = three(lib, g, lanes, truncate)
            assert new[3][0, 0] == path and new[3][0, 3] == 32


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_broken_dispatches_are_told_apart(lib, dlib, nz, z_max):
    g = Z.grid(nz, z_max)
    where = masks()["d32"]
    lanes = mixed_wave(dlib, g, where, deep=True)
    good = run(lib, g, lanes, NEW, 0)
    assert same(good, run(lib, g, lanes, GENERAL, 0))
    k2, kend = int(good[3][0, 1]), int(good[3][0, 2])
    assert 0 < k2 < kend
    # the clamp constant's entry for the dead lanes too: their node values are wrong from k2 on (raw F and
    # the checksum see it; the zeroing hides it from F), the live lanes are untouched
    bad = run(lib, g, lanes, NEW, 0, defect=ENTRY_FROM_CLAMP)
    assert not np.any(bad[2][0, where] == good[2][0, where])
    assert not np.any(bits(bad[0][0, where]) == bits(good[0][0, where]))
    assert np.array_equal(bad[2][0, ~where], good[2][0, ~where])
    assert np.array_equal(bits(bad[1]), bits(good[1]))
    # the suffix a batch early: the live lane that clamps last still reads other entries in that batch
    bad = run(lib, g, lanes, NEW, 0, defect=BATCH_EARLY)
    assert not np.array_equal(bad[2][0, ~where], good[2][0, ~where])
    assert np.array_equal(bad[2][0, where], good[2][0, where])   # a dead lane's entry is T''[0] throughout


def test_c2_mixed_pass(lib):
    """The C2 workload on the default grid: one pass of 125 mixes dead and clamped lanes (pass 93)."""
    import test_zsum_group_host as HG
    g = Z.grid(1200, 30.0)
    c2 = HG.c2_points()
    new = three(lib, g, c2, 0)
    plan = new[3]
    mixed = np.flatnonzero(plan[:, 0] == MIXED)
    assert mixed.tolist() == [93]
    k2, kend, ndead = plan[93, 1:].tolist()
    assert kend == 1200 and 0 < ndead < 64
    print(f"C2 pass 93: {ndead} dead lanes, k2 = {k2}: {kend - k2} of 1200 nodes take the six-operation node")
