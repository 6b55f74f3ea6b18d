"""The all-dead passes of the dense z-sum with the node's value formed once (csrc/lzq_quad.h zsum_dead,
LZQ_DEAD_SEG; csrc/lzq_exp2.h seg_node_dead), on the CPU.

A pass whose 64 lanes are all dead runs with c2e = +0.0 in every lane, so s = fma(+0 * g, A) = A at
every node, and q = fma(A, A, beta) and v = T''[0] * q are one number for the whole pass: the device
forms them once and runs F's accumulate alone at every node.  tests/zsum_dead_segment_host.cpp compiles
the LZQ_HD functions of csrc/lzq_exp2.h that the device code itself calls and evaluates a 64-lane pass
three ways: with the dispatch whose all-dead path runs seg_node_dead (mode DEADSEG), with the dispatch
of -DLZQ_DEAD_SEG=0, where those passes take the four-operation zero node (mode ZEROSEG), and with
the single general loop (lzq::exp2_tab_scaled at every node, mode GENERAL).

A dead lane's F is overwritten with +0 whatever the loop summed, so the F of an all-dead pass cannot
tell a right loop from a wrong one: the harness also returns the raw sums from before the zeroing,
and those must agree bit for bit between the three.  One ulp on the live side of the dead threshold a
lane takes the whole pass off the dead path, and its raw sum is not the dead loop's -- the comparison
can fail.

Lanes are given as c2N = c2 * 8192 directly, so that a lane can sit exactly on a threshold of the
library's own predicates; the thresholds are found by bisection on them.

The last two tests pin what the device build must keep: the headline kernels' registers and
occupancy, and that -DLZQ_DEAD_SEG=0 is the parent's machine code (profiles/round9/
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
GRIDS = ((1200, 30.0), (13, 3.0))       # the default grid, and a runtime grid padded 13 -> 16
GENERAL, DEADSEG, ZEROSEG = 0, 1, 2     # mode of zdead_passes
ZERO, FREE, SPLIT, DEAD = 0, 1, 2, 3    # plan[0] of zsum_dead_segment_host.cpp
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


def load_lib():
    so = os.path.join(tempfile.mkdtemp(), "zsum_dead_segment_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "zsum_dead_segment_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.zdead_passes.argtypes = [ctypes.c_int, ctypes.c_int, DP, DP, ctypes.c_int, DP, ctypes.c_long, DP, DP, IP]
    L.zdead_nodes.argtypes = [ctypes.c_double, DP, ctypes.c_int, DP]
    for f in (L.zdead_zero, L.zdead_dead, L.zdead_small):
        f.argtypes = [ctypes.c_double, ctypes.c_double]
    return L


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def run(L, g, c2, mode, truncate):
    """(F, raw sums before the dead lanes are zeroed, plan) of the passes of 64 lanes in c2."""
    c2 = np.ascontiguousarray(np.asarray(c2, float).reshape(-1, 64))
    F, raw = np.empty_like(c2), np.empty_like(c2)
    plan = np.empty((c2.shape[0], 3), np.int32)
    g4, om = np.ascontiguousarray(g.g4), np.ascontiguousarray(g.om)
    rc = L.zdead_passes(int(mode), int(truncate), g4.ctypes.data_as(DP), om.ctypes.data_as(DP), g.nz,
                        c2.ctypes.data_as(DP), c2.shape[0], F.ctypes.data_as(DP), raw.ctypes.data_as(DP),
                        plan.ctypes.data_as(IP))
    assert rc == 0
    return F, raw, plan


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def three(L, g, c2, truncate):
    """(F, raw, plan) of the dispatch with the dead loop, after checking F AND the raw sums against
    the dispatch without it and against the single general loop."""
    Fd, rd, plan = run(L, g, c2, DEADSEG, truncate)
    for mode in (ZEROSEG, GENERAL):
        Fm, rm, pm = run(L, g, c2, mode, truncate)
        assert np.array_equal(bits(Fd), bits(Fm)), ("F differs from mode", mode)
        assert np.array_equal(bits(rd), bits(rm)), ("raw sums differ from mode", mode)
        assert np.array_equal(plan[:, 2], pm[:, 2]) and np.all(plan[:, 2] % 8 == 0)
        if mode == ZEROSEG:      # without the dead loop an all-dead pass is a zero pass, and nothing else moves
            assert np.array_equal(np.where(plan[:, 0] == DEAD, ZERO, plan[:, 0]), pm[:, 0])
    return Fd, rd, plan


def nodes(L, c2N, g4):
    """(seg_node_dead, seg_node_zero, seg_node, exp2_tab_scaled) of one lane at every node, as int64 bits."""
    g4 = np.ascontiguousarray(g4, dtype=np.float64)
    v = np.empty((4, g4.size))
    assert L.zdead_nodes(float(c2N), g4.ctypes.data_as(DP), g4.size, v.ctypes.data_as(DP)) == 0
    return v.view(np.int64)


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


def thresholds(L, g):
    """(c_zero, c_free, c_live, c_dead): the last c2N of a zero lane, the last of a clamp-free lane, the
    last live c2N, and its neighbour one ulp beyond, the first dead one."""
    g_1, g_max = float(g.g4[1]), float(g.g4[-1])
    c_zero = float(np.nextafter(first_true(lambda c: not L.zdead_zero(c, g_max)), 0.0))
    c_free = float(np.nextafter(first_true(lambda c: not L.zdead_small(c, g_max)), 0.0))
    c_dead = first_true(lambda c: bool(L.zdead_dead(c, g_1)))
    c_live = float(np.nextafter(c_dead, 0.0))
    assert L.zdead_dead(c_dead, g_1) and not L.zdead_dead(c_live, g_1)
    assert abs(c_zero) < abs(c_free) < abs(c_live) < abs(c_dead)
    return c_zero, c_free, c_live, c_dead


def dead_lanes(c_dead):
    return -np.geomspace(abs(c_dead), abs(c_dead) * 1e6, 64)      # from the threshold itself up to 1e6 x it


@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_all_dead_pass_runs_the_dead_loop(lib, nz, z_max, truncate):
    g = Z.grid(nz, z_max)
    c_dead = thresholds(lib, g)[3]
    kend = 8 if truncate else padded(g).size                      # truncated: thr = 0, the first batch alone
    F, raw, plan = three(lib, g, dead_lanes(c_dead), truncate)
    assert plan[0].tolist() == [DEAD, 0, kend]
    assert np.all(F == 0.0) and not np.any(np.signbit(F))        # +0, no sign bit
    # what the zeroing hides: every lane summed omega'_k T''[0] (A^2 + beta) over the executed nodes, the
    # sum a live wave of c2 = +0.0 lanes (a zero pass, nothing zeroed) gets from the four-operation node
    assert np.all(raw > 0.0) and len(set(bits(raw[0]).tolist())) == 1
    if not truncate:                                              # (truncated, a c2 = 0 lane runs every node)
        F0, raw0, plan0 = three(lib, g, np.zeros(64), truncate)
        assert plan0[0, 0] == ZERO and np.array_equal(bits(F0), bits(raw0)) and np.array_equal(bits(F0), bits(raw))


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_the_four_nodes_agree_node_by_node(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    gp = padded(g)
    v = nodes(lib, 0.0, gp)                                       # c2 = +0.0, what the dispatch hands a dead lane
    assert all(np.array_equal(v[0], v[i]) for i in (1, 2, 3))
    assert len(set(v[0].tolist())) == 1                           # one number for the whole pass
    # -0.0 and the smallest subnormal: c2 * g is -0 or far below half an ulp of A, so s = A here too and
    # the equality happens to hold (checked, not assumed).  The dispatch never passes either as "dead":
    # its c2e is the literal +0.0.
    for c in (-0.0, 5e-324):
        w = nodes(lib, c, gp)
        assert all(np.array_equal(v[0], w[i]) for i in (1, 2, 3)), c
    # a live zero lane at the zero boundary moves s by up to 1/2: the dead node is NOT its node (the
    # comparison above can fail), while the other three still agree with each other
    c_zero = thresholds(lib, g)[0]
    w = nodes(lib, c_zero, gp)
    assert w[0, g.nz - 1] != w[1, g.nz - 1] and w[0, -1] != w[3, -1]
    assert np.array_equal(w[1], w[2]) and np.array_equal(w[1], w[3])


@pytest.mark.parametrize("lane", [0, 31, 63])
@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_one_live_lane_takes_the_pass_off_the_dead_path(lib, nz, z_max, truncate, lane):
    g = Z.grid(nz, z_max)
    _, _, c_live, c_dead = thresholds(lib, g)
    _, raw_dead, _ = run(lib, g, dead_lanes(c_dead), DEADSEG, truncate)
    lanes = dead_lanes(c_dead)
    lanes[lane] = c_live                                          # one ulp on the live side of the threshold
    F, raw, plan = three(lib, g, lanes, truncate)                 # (three: that lane's F has the general loop's bits)
    assert plan[0, 0] == SPLIT                                    # a clamped pass, not the dead path
    others = np.arange(64) != lane
    assert np.all(F[0, others] == 0.0) and not np.any(np.signbit(F[0, others]))
    assert _bits(F[0, lane]) == _bits(raw[0, lane])               # live: not zeroed
    # its sum is the underflowing sum of a clamped lane, not the dead loop's omega' T''[0] (A^2 + beta) sum
    assert _bits(raw[0, lane]) != _bits(raw_dead[0, lane]) and raw[0, lane] < raw_dead[0, lane]


@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_mixed_waves_are_not_planned_dead(lib, nz, z_max, truncate):
    g = Z.grid(nz, z_max)
    c_zero, c_free, c_live, c_dead = thresholds(lib, g)
    live = {ZERO: -np.geomspace(abs(c_zero) * 1e-30, abs(c_zero), 32),
            FREE: -np.geomspace(abs(c_zero) * 4.0, abs(c_free), 32),
            SPLIT: -np.geomspace(abs(c_free) * 1.001, abs(c_live), 32)}
    for path, c in live.items():
        for first in (0, 1):                                      # dead lanes odd, then even
            lanes = dead_lanes(c_dead)
            lanes[first::2] = c
            F, raw, plan = three(lib, g, lanes, truncate)
            assert plan[0, 0] == path, (path, first)
            dead = np.arange(64) % 2 != first
            assert np.all(F[0, dead] == 0.0) and not np.any(np.signbit(F[0, dead]))
            assert np.array_equal(bits(F[0, ~dead]), bits(raw[0, ~dead]))
            if path != SPLIT:                                     # (a lane near the dead threshold sums to 0)
                assert np.all(F[0, ~dead] > 0.0)


def test_headline_kernels_keep_registers_and_occupancy():
    """tools/kernel_resources.py on lzq_kernels.hip: every yields_grid_kernel instantiation within 64
    VGPRs, without scratch or spilled VGPRs, at the 8 waves/SIMD of its __launch_bounds__."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    rows = [r for r in kr.resources("lzq_kernels.hip", []) if "yields_grid_kernel" in r["kernel"]]
    assert len(rows) >= 2
    for r in rows:
        assert int(r["VGPRs"]) <= 64, r
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r
        assert int(r["Occupancy [waves/SIMD]"]) == 8, r


def test_dead_seg_off_is_the_parent_machine_code(tmp_path):
    """-DLZQ_DEAD_SEG=0 compiles the headline kernels to the ISA the parent's profile was taken on."""
    b, codeobj = pkg("build"), pkg("codeobj")
    out = str(tmp_path / "lzq_kernels_off.so")
    subprocess.run([b.hipcc(), *b.FLAGS, "-DLZQ_DEAD_SEG=0", "-I", b.INCLUDE, os.path.join(b.CSRC, "lzq_kernels.hip"),
                    "-o", out], check=True)
    got = codeobj.kernel_isa_sha256(out)
    assert got is not None, "llvm-objdump (ROCm) is needed to disassemble the code object"
    with open(os.path.join(ROOT, "profiles", "round9", "parent_pmc_summary.json")) as f:
        assert got == json.load(f)["kernel_isa_sha256"]
