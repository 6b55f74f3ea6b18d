"""The frozen tails of the dense z-sum (csrc/lzq_quad.h zsum_held / zsum_frozen_t, LZQ_FROZEN_SEG;
csrc/lzq_exp2.h seg_frozen_s / seg_frozen_t), on the CPU.

gamma4 saturates, so a lane's rounded s = fma(c2N, g, A) (zero passes) or t = fma(c2N, g, M)
(clamp-free passes) stops changing before the pass ends.  From the first 8-node batch k3 at whose
first node every lane of the wave holds the value it has at the last executed node, the device
forms what depends on that value once per lane and runs the rest of the node: F's accumulate alone
(frozen s), or s, q, v and the accumulate (frozen t).  tests/zsum_frozen_host.cpp compiles the LZQ_HD
functions of csrc/lzq_exp2.h that the device code itself calls and evaluates a 64-lane pass with
that dispatch (FROZEN = 2), with its frozen-s part alone (1), with the parent's dispatch (0) and
with the single general loop (lzq::exp2_tab_scaled at every node, -1).  F must agree bit for bit
between all of them, and so must a checksum over the bits of every node's value: at the saturated
end of the (., 30) grids omega' is ~1e-10 of the sum, so F's rounding swallows a node value that is
an ulp off, and the checksum does not.

k3 is checked against a brute-force scan of all nodes with the loop's own s and t
(zfrozen_values).  Lanes are given as c2N = c2 * 8192 directly.

The deliberately broken dispatches (the tail's constants formed at the grid's last node instead of
the last executed one; k3 rounded down; the tail started a batch early) must be told from the right
one.  The last tests pin what the device build must keep: registers and occupancy of every kernel
that takes zsum_dispatch, and that -DLZQ_FROZEN_SEG=0 is the parent's machine code (profiles/round10/
parent_pmc_summary.json), so the ablation's "parent" library can be built from this tree.
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import zsum_ref as Z
from conftest import PKG_NAME, ROOT, pkg

HERE = os.path.dirname(os.path.abspath(__file__))
GRIDS = ((1200, 30.0), (13, 3.0), (2400, 30.0))   # the default grid, a runtime grid padded 13 -> 16, a fine one
GENERAL, PARENT, FROZEN_S, FROZEN = -1, 0, 1, 2   # `frozen` of zfrozen_passes
ZERO, FREE, SPLIT, DEAD = 0, 1, 2, 3              # plan[0]
S, T = 0, 1                                       # `kind` of zfrozen_values
DP, IP, UP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)
N = 8192.0


def load_lib():
    so = os.path.join(tempfile.mkdtemp(), "zsum_frozen_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "zsum_frozen_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.zfrozen_passes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, DP, DP, ctypes.c_int, DP, ctypes.c_long,
                                 DP, UP, IP]
    L.zfrozen_values.argtypes = [ctypes.c_int, ctypes.c_double, DP, ctypes.c_int, DP]
    for f in (L.zfrozen_zero, L.zfrozen_dead, L.zfrozen_small):
        f.argtypes = [ctypes.c_double, ctypes.c_double]
    return L


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def run(L, g, c2, frozen, truncate, defect=0):
    """(F, checksum of the node values, plan = [path, k2, kend, k3]) of the passes of 64 lanes in c2."""
    c2 = np.ascontiguousarray(np.asarray(c2, float).reshape(-1, 64))
    F, V = np.empty_like(c2), np.empty(c2.shape, np.uint64)
    plan = np.empty((c2.shape[0], 4), np.int32)
    g4, om = np.ascontiguousarray(g.g4), np.ascontiguousarray(g.om)
    rc = L.zfrozen_passes(int(frozen), int(defect), int(truncate), g4.ctypes.data_as(DP), om.ctypes.data_as(DP), g.nz,
                          c2.ctypes.data_as(DP), c2.shape[0], F.ctypes.data_as(DP), V.ctypes.data_as(UP),
                          plan.ctypes.data_as(IP))
    assert rc == 0
    return F, V, plan


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def all_modes(L, g, c2, truncate):
    """(F, V, plan) of the full dispatch, after checking F and the node checksum against the frozen-s
    dispatch, the parent's dispatch and the single general loop."""
    ref = run(L, g, c2, FROZEN, truncate)
    for mode in (FROZEN_S, PARENT, GENERAL):
        got = run(L, g, c2, mode, truncate)
        assert np.array_equal(bits(ref[0]), bits(got[0])), ("F differs from mode", mode)
        assert np.array_equal(ref[1], got[1]), ("node values differ from mode", mode)
        assert np.array_equal(ref[2][:, 2], got[2][:, 2]) and np.all(ref[2][:, 2] % 8 == 0)
        if mode != GENERAL:                                       # the paths are the parent's; only k3 is new
            assert np.array_equal(ref[2][:, :2], got[2][:, :2])
        if mode == PARENT:
            assert np.array_equal(got[2][:, 3], got[2][:, 2])     # no tails
        if mode == FROZEN_S:                                      # the same tails on zero passes, none elsewhere
            z = ref[2][:, 0] == ZERO
            assert np.array_equal(got[2][z, 3], ref[2][z, 3]) and np.array_equal(got[2][~z, 3], got[2][~z, 2])
    return ref


def padded(g):
    nzp = (max(g.nz, 8) + 7) // 8 * 8
    return np.concatenate([g.g4, np.full(nzp - g.nz, g.g4[-1])])


def values(L, kind, c, gp):
    v = np.empty(gp.size)
    assert L.zfrozen_values(kind, float(c), gp.ctypes.data_as(DP), gp.size, v.ctypes.data_as(DP)) == 0
    return v


def scan(L, kind, lanes, gp, kend):
    """Brute force over ALL nodes: (k3, first frozen node) of a wave -- the first batch start, and the
    first node, from which every lane holds its value of node kend - 1; also checks that 'frozen' is
    monotone in k for every lane (what the device's binary search relies on)."""
    frozen = np.ones(kend, bool)
    for c in np.unique(lanes):
        v = values(L, kind, c, gp)[:kend]
        f = v == v[kend - 1]
        assert np.all(np.diff(f.astype(int)) >= 0), c          # false ... false true ... true
        frozen &= f
    first = int(np.argmax(frozen))                               # frozen[kend - 1] is True
    starts = np.flatnonzero(frozen[::8]) * 8
    return (int(starts[0]) if starts.size else kend), first


def lane_k3(L, kind, c, gp, kend):
    return scan(L, kind, [c], gp, kend)[0]


def c_zero_max(L, g):
    """The zero lane of largest |c2N| (seg_zero's own threshold, by bisection on the bits)."""
    g_max = float(g.g4[-1])
    lo, hi = np.float64(1e-30).view(np.int64), np.float64(1e30).view(np.int64)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if L.zfrozen_zero(-float(np.int64(mid).view(np.float64)), g_max):
            lo = mid
        else:
            hi = mid
    return -float(np.int64(lo).view(np.float64))


def zero_tail_lanes(g):
    """64 zero lanes whose s freezes inside the pass: |c2N| g_max from 1e-9 to 1e-4."""
    return -np.geomspace(1e-9, 1e-4, 64) / float(g.g4[-1])


def free_tail_lanes(g):
    """64 clamp-free lanes whose t freezes inside the pass: |c2N| g_max from 2 to 2000 octave/8192 units."""
    return -np.geomspace(2.0, 2000.0, 64) / float(g.g4[-1])


def tail_wave(L, kind, g, gp):
    """(lanes, k3, first frozen node) of a wave with a tail.  On the (., 30) grids the first frozen node
    lies inside a batch.  The 16-node grid has two batches, and no such wave: a value that changes before
    node 7 (g = 0.60) changes again before g_max = 2.12, the rounding boundaries being equally spaced in
    g; its wave changes once, between nodes 7 and 8, so the first frozen node is 8 = k3."""
    if g.nz == 13:
        unit = 2.0 ** -39 if kind == S else 1.0                  # ulp(A), or t's integer step
        lanes = -np.geomspace(1.25, 1.45, 64) * unit / float(g.g4[-1])
        k3, first = scan(L, kind, lanes, gp, gp.size)
        assert (k3, first) == (8, 8)
        return lanes, k3, first
    return off_boundary(L, kind, zero_tail_lanes(g) if kind == S else free_tail_lanes(g), gp, gp.size)


def off_boundary(L, kind, lanes, gp, kend):
    """The wave scaled (by up to a few percent) until its first frozen node is NOT a batch start, so that
    rounding k3 down differs from rounding it up."""
    for i in range(200):
        w = lanes * (1.0 + 0.003 * i)
        k3, first = scan(L, kind, w, gp, kend)
        if first % 8 != 0 and 8 <= k3 < kend:
            return w, k3, first
    raise AssertionError("no wave with its first frozen node inside a batch")


@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_whole_frozen_zero_pass(lib, nz, z_max, truncate):
    """|c2N| g_max far below half an ulp of A, c2N = +-0 and tiny positive c2N among the lanes: s = A at
    every node, k3 = 0, and the whole pass is the accumulate alone."""
    g = Z.grid(nz, z_max)
    gp = padded(g)
    lanes = -np.geomspace(1e-300, 1e-14, 64) / float(g.g4[-1])
    lanes[[3, 17]] = 0.0, -0.0
    lanes[[5, 40, 63]] = 5e-324, 1e-300, 1e-20                   # positive: s = A from above
    F, V, plan = all_modes(lib, g, lanes, truncate)
    assert plan[0].tolist() == [ZERO, 0, gp.size, 0]
    assert scan(lib, S, lanes, gp, gp.size)[0] == 0
    assert len(set(bits(F[0]).tolist())) == 1 and F[0, 0] > 0.0  # one v for every lane and node


@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_zero_pass_with_a_tail(lib, nz, z_max, truncate):
    g = Z.grid(nz, z_max)
    gp = padded(g)
    lanes, k3, first = tail_wave(lib, S, g, gp)
    F, V, plan = all_modes(lib, g, lanes, truncate)
    assert plan[0].tolist() == [ZERO, 0, gp.size, k3] and 0 < k3 < gp.size
    assert k3 == (first + 7) // 8 * 8                            # rounded UP to the batch


@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_clamp_free_pass_with_a_tail(lib, nz, z_max, truncate):
    g = Z.grid(nz, z_max)
    gp = padded(g)
    lanes, k3, first = tail_wave(lib, T, g, gp)
    F, V, plan = all_modes(lib, g, lanes, truncate)
    assert plan[0].tolist() == [FREE, gp.size, gp.size, k3] and 0 < k3 < gp.size
    assert k3 == (first + 7) // 8 * 8
    assert run(lib, g, lanes, FROZEN_S, truncate)[2][0, 3] == gp.size   # part 1 alone takes no tail here


def later_lane(L, kind, base, gp, kend):
    """A lane of larger |c2N| than `base` whose own k3 is exactly one batch later than base's."""
    K = lane_k3(L, kind, base, gp, kend)
    assert K + 8 < kend
    for f in np.geomspace(1.0, 64.0, 4000)[1:]:
        if lane_k3(L, kind, base * f, gp, kend) == K + 8:
            return base * f, K
    raise AssertionError("no lane freezing exactly one batch later")


@pytest.mark.parametrize("lane", [0, 31, 63])
@pytest.mark.parametrize("kind", [S, T], ids=["frozen_s", "frozen_t"])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_one_late_lane_moves_k3_by_its_batch(lib, nz, z_max, kind, lane):
    g = Z.grid(nz, z_max)
    gp = padded(g)
    g_max = float(g.g4[-1])
    if nz == 13 and kind == S:
        # two batches: the rest of the wave whole-frozen (k3 = 0), the late lane frozen from node 8 (tail_wave)
        rest, late, K = -1e-14 / g_max, -1.35 * 2.0 ** -39 / g_max, 0
    elif nz == 13:
        # a wave is clamp-free (not zero) only with a lane whose t leaves M, and that happens after node 0: the
        # rest freezes at node 8 (t = M - 1 for |u| in [0.6, 1.48]), the late lane only inside the last batch
        rest, late, K = -0.6 / float(g.g4[8]), -0.6 / float(g.g4[9]), 8
    else:
        rest = (-1e-6 if kind == S else -50.0) / g_max
        late, K = later_lane(lib, kind, rest, gp, gp.size)
    assert lane_k3(lib, kind, rest, gp, gp.size) == K and lane_k3(lib, kind, late, gp, gp.size) == K + 8
    lanes = np.full(64, rest)
    _, _, plan0 = all_modes(lib, g, lanes, 0)
    assert plan0[0, 3] == K and plan0[0, 0] == (ZERO if kind == S else FREE)
    lanes[lane] = late
    _, _, plan = all_modes(lib, g, lanes, 0)
    assert plan[0, 3] == K + 8 and plan[0, 0] == plan0[0, 0]
    assert scan(lib, kind, lanes, gp, gp.size)[0] == K + 8


def moving_t_lane(L, g, gp):
    """A clamp-free lane whose t changes between the last batch start and the last node."""
    kend, g_last = gp.size, float(gp[-1])
    for n in (10 ** 6, 10 ** 5, 10 ** 4, 3000, 300, 30, 3):
        c = -(n + 0.5) * (1.0 + 1e-12) / g_last                  # u_last just beyond a rounding boundary
        v = values(L, T, c, gp)
        if v[kend - 8] != v[kend - 1] and L.zfrozen_small(c, float(g.g4[-1])):
            return c
    raise AssertionError("no clamp-free lane whose t moves to the last node")


@pytest.mark.parametrize("lane", [0, 31, 63])
@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_one_lane_that_never_freezes_keeps_the_old_paths(lib, nz, z_max, truncate, lane):
    g = Z.grid(nz, z_max)
    gp = padded(g)
    # zero pass: the lane at the zero boundary moves s by dozens of ulps inside the last batch
    lanes = zero_tail_lanes(g)
    lanes[lane] = c_zero_max(lib, g)
    v = values(lib, S, lanes[lane], gp)
    assert v[gp.size - 8] != v[-1]
    F, V, plan = all_modes(lib, g, lanes, truncate)
    assert plan[0].tolist() == [ZERO, 0, gp.size, gp.size]       # no tail
    assert same((F, V), run(lib, g, lanes, PARENT, truncate)[:2])
    # clamp-free pass
    lanes = free_tail_lanes(g)
    lanes[lane] = moving_t_lane(lib, g, gp)
    F, V, plan = all_modes(lib, g, lanes, truncate)
    assert plan[0, 0] == FREE and plan[0, 3] == plan[0, 2]       # no tail (kend may be truncated)


@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_dead_lanes_mixed_in(lib, nz, z_max, truncate):
    """Dead lanes run with c2e = +0.0: s = A and t = M at every node, frozen from node 0, so they never
    delay a tail, and they are zeroed as before."""
    g = Z.grid(nz, z_max)
    gp = padded(g)
    dead = -np.geomspace(1.0, 1e6, 64) * (N * 1077.0 / float(g.g4[1]))
    assert all(lib.zfrozen_dead(float(c), float(g.g4[1])) for c in dead)
    for kind, path in ((S, ZERO), (T, FREE)):
        live = tail_wave(lib, kind, g, gp)[0]
        for first in (0, 1):
            lanes = dead.copy()
            lanes[first::2] = live[first::2]
            F, V, plan = all_modes(lib, g, lanes, truncate)
            is_dead = np.arange(64) % 2 != first
            assert plan[0, 0] == path
            assert plan[0, 3] == scan(lib, kind, lanes[~is_dead], gp, int(plan[0, 2]))[0] < plan[0, 2]
            assert np.all(F[0, is_dead] == 0.0) and not np.any(np.signbit(F[0, is_dead]))
            assert np.all(F[0, ~is_dead] > 0.0)
            ref = run(lib, g, np.where(is_dead, 0.0, lanes), FROZEN, truncate)[0]   # c2 = +0.0 lanes, not zeroed
            assert np.array_equal(bits(F[0, ~is_dead]), bits(ref[0, ~is_dead]))


def truncated_tail_lane(L, g, gp):
    """A clamp-free lane that truncation cuts inside the saturated stretch, with a frozen-t tail before
    the cut and a different t at the grid's last node: (c2N, kend)."""
    nzp = gp.size
    for ks in range(int(0.70 * g.nz), int(0.95 * g.nz)):
        c = -(1080.0 * N) / float(gp[ks])                        # thr = g[ks]: executed up to ks, rounded up
        kend = (ks + 1 + 7) // 8 * 8
        if kend >= nzp or not (gp[ks + 1] > gp[ks]):
            continue
        v = values(L, T, c, gp)
        if v[kend - 8] == v[kend - 1] and v[nzp - 1] != v[kend - 1]:
            return c, kend
    raise AssertionError("no truncated clamp-free lane with a tail")


@pytest.mark.parametrize("nz,z_max", [G for G in GRIDS if G[1] == 30.0])
def test_truncated_tail_takes_its_value_at_the_last_executed_node(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    gp = padded(g)
    c, kend = truncated_tail_lane(lib, g, gp)
    lanes = np.full(64, c)
    F, V, plan = all_modes(lib, g, lanes, 1)
    assert plan[0, 0] == FREE and plan[0, 2] == kend < gp.size and plan[0, 3] < kend
    assert plan[0, 3] == scan(lib, T, lanes, gp, kend)[0]
    assert np.array_equal(bits(F), bits(run(lib, g, lanes, FROZEN, 0)[0]))   # and truncation is exact
    # defect 1: the entry and w formed from t at node nzp - 1 -- another table entry, other node values
    Fd, Vd, pd = run(lib, g, lanes, FROZEN, 1, defect=1)
    assert np.array_equal(pd, plan) and not np.array_equal(Vd, V)
    # untruncated the two nodes are one and the defect is none
    assert same(run(lib, g, lanes, FROZEN, 0, defect=1)[:2], run(lib, g, lanes, FROZEN, 0)[:2])


@pytest.mark.parametrize("defect", [2, 3], ids=["k3_rounded_down", "tail_one_batch_early"])
@pytest.mark.parametrize("kind", [S, T], ids=["frozen_s", "frozen_t"])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_broken_tail_starts_are_told_apart(lib, nz, z_max, kind, defect):
    g = Z.grid(nz, z_max)
    gp = padded(g)
    lanes, k3, first = tail_wave(lib, kind, g, gp)
    F, V, plan = all_modes(lib, g, lanes, 0)
    Fd, Vd, pd = run(lib, g, lanes, FROZEN, 0, defect=defect)
    assert plan[0, 3] == k3
    if defect == 2 and first % 8 == 0:                           # (the 16-node grid: nothing to round)
        assert pd[0, 3] == k3 and same((Fd, Vd), (F, V))
        return
    assert pd[0, 3] == k3 - 8                                    # both defects start the tail in the batch before
    assert not np.array_equal(Vd, V)                             # a lane that still moves gets its last value early
    if nz == 13 and kind == T:                                   # omega' is not small on this grid: F itself moves
        assert not np.array_equal(bits(Fd), bits(F))


def c2_workload():
    """c2N of the C2 workload's y-grid (every point has the same), padded to whole passes."""
    B, Tp, I_p = 100.0, 100.0, 0.34                              # yields_config_equal_mass.json (C2's base)
    y_of = lambda T: 0.5 * B * ((Tp / T) ** 2 - 1.0)
    ys = np.linspace(max(y_of(5.0 * Tp), -80.0), min(y_of(1e-3 * Tp), 50.0), 8000)
    c2 = ((-(I_p / 6.0) * np.exp(np.clip(ys, -50.0, 50.0))) * Z.LOG2E) * N
    return np.concatenate([c2, np.full(-len(c2) % 64, c2[-1])])


def test_each_new_path_is_taken_on_the_default_grid(lib):
    """The plan of the C2 workload on the (1200, 30) grid: whole-frozen zero passes, zero passes with a
    tail and clamp-free passes with a tail all occur, and every pass agrees with the general loop."""
    g = Z.grid(1200, 30.0)
    F, V, plan = all_modes(lib, g, c2_workload(), 0)
    path, kend, k3 = plan[:, 0], plan[:, 2], plan[:, 3]
    assert np.all(kend == 1200)
    whole = (path == ZERO) & (k3 == 0)
    ztail = (path == ZERO) & (k3 > 0) & (k3 < kend)
    ttail = (path == FREE) & (k3 < kend)
    assert whole.sum() >= 1 and ztail.sum() >= 1 and ttail.sum() >= 1
    assert np.all(k3[(path == SPLIT) | (path == DEAD)] == 1200)   # no tail on the other paths
    print(f"C2 plan: {int(whole.sum())} whole-frozen zero passes, {int(ztail.sum())} zero passes with a tail "
          f"({int((kend - k3)[ztail].sum())} nodes), {int(ttail.sum())} clamp-free passes with a tail "
          f"({int((kend - k3)[ttail].sum())} nodes)")


def _kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    return kr


def test_zsum_kernels_keep_registers_and_occupancy():
    """tools/kernel_resources.py: every yields_*, window and A/V quadrature kernel within 64 VGPRs, without
    scratch or spilled VGPRs, at the 8 waves/SIMD of its __launch_bounds__; the ODE A/V table kernels keep
    their 28 bytes."""
    kr = _kernel_resources()
    rows = [r for src in ("lzq_kernels.hip", "lzq_aov.hip", "lzq_window.hip") for r in kr.resources(src, [])]
    quad = [r for r in rows if any(k in r["kernel"] for k in ("yields_", "aov_kernel", "ztable_kernel"))
            and "ode_aov_table" not in r["kernel"]]
    assert len([r for r in quad if "yields_grid_kernel" in r["kernel"]]) >= 2 and len(quad) >= 20
    for r in quad:
        assert int(r["VGPRs"]) <= 64, r
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r
        assert int(r["Occupancy [waves/SIMD]"]) == 8, r
    ode = [r for r in rows if "ode_aov_table" in r["kernel"] and "ILi1E" in r["kernel"]]
    assert len(ode) == 2
    for r in ode:
        assert int(r["ScratchSize [bytes/lane]"]) == 28 and int(r["Occupancy [waves/SIMD]"]) == 8, r


def test_frozen_seg_off_is_the_parent_machine_code(tmp_path):
    """-DLZQ_FROZEN_SEG=0 compiles the headline kernels to the ISA the parent's profile was taken on."""
    b, codeobj = pkg("build"), pkg("codeobj")
    out = str(tmp_path / "lzq_kernels_off.so")
    subprocess.run([b.hipcc(), *b.FLAGS, "-DLZQ_FROZEN_SEG=0", "-I", b.INCLUDE, os.path.join(b.CSRC, "lzq_kernels.hip"),
                    "-o", out], check=True)
    got = codeobj.kernel_isa_sha256(out)
    assert got is not None, "llvm-objdump (ROCm) is needed to disassemble the code object"
    with open(os.path.join(ROOT, "profiles", "round10", "parent_pmc_summary.json")) as f:
        want = json.load(f)["kernel_isa_sha256"]
    assert want == "e7732af65ea5d00347bd39e4ce6be341e9c1edd9beb71a7de72b3608d6b8aac5"   # the parent's, pinned
    assert got == want
