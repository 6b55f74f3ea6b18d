"""Grouped passes of the dense z-sum (csrc/lzq_quad.h yb_group / yb_group_run, LZQ_GROUP_SEG;
csrc/lzq_exp2.h seg_group_slot / seg_group_kind), on the CPU.

Runs of consecutive passes of yb_wave that are F's accumulate alone from node 0 -- all 64 lanes dead
(zsum_dead), or a zero pass whose every lane's s is frozen from the first node (zsum_held with k3 = 0)
-- are swept through z together, four or two at a time: each lane carries that many independent F
chains, each in node order from 0, and the passes are integrated in ascending pass order.
tests/zsum_group_host.cpp models one point (one 64-lane wavefront over n y-nodes) with the device's own
LZQ_HD predicates: the cue `grp`, the sizes tried, the chains, the zeroing of dead lanes and the
y-loop's acc = fma(w_j, F_j, acc).  It is compared with the per-pass dispatch of
tests/zsum_frozen_host.cpp (LZQ_GROUP_SEG = 0), bit for bit, on F, on the checksum over every node's
value and on acc, for LZQ_GROUP_SEG = 2 and 4.

Two deliberately broken loops (the group test taken on slot 0 only; the passes of a group integrated in
descending order) must be told from the right one.  The last test pins that -DLZQ_GROUP_SEG=0 is the
parent's machine code (profiles/round11/parent_pmc_summary.json), so the ablation's baseline library
can be built from this tree.
"""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import test_zsum_frozen_host as HF
import zsum_ref as Z
from conftest import PKG_NAME, ROOT, pkg

HERE = os.path.dirname(os.path.abspath(__file__))
GRIDS = HF.GRIDS                                  # (1200, 30), (13, 3) padded to 16, (2400, 30)
ZERO, FREE, SPLIT, DEAD = HF.ZERO, HF.FREE, HF.SPLIT, HF.DEAD
DP, IP, UP = HF.DP, HF.IP, HF.UP
N = 8192.0
GRP_DEAD, GRP_WHOLE = 1, 2                        # kGrpDead, kGrpWhole
SLOT_0_ONLY, DESCENDING = 1, 2                    # `defect` of zgroup_point
bits = HF.bits


def load_lib():
    so = os.path.join(tempfile.mkdtemp(), "zsum_group_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "zsum_group_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.zgroup_point.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, DP, DP, ctypes.c_int, DP, DP, ctypes.c_long,
                               DP, UP, DP, IP]
    L.zgroup_slot.argtypes = [ctypes.c_double] * 4
    return L


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def weights(n, seed=7):
    return np.random.default_rng(seed).uniform(0.5, 1.5, n)


def run(L, g, c2, gmax, truncate=0, defect=0, wy=None):
    """(F, node-value checksum, acc, plan) of one point with y-nodes c2; plan rows = [group size, path,
    classification made at this base, k3]."""
    c2 = np.ascontiguousarray(np.asarray(c2, float).ravel())
    n = c2.size
    wy = np.ascontiguousarray(weights(n) if wy is None else wy)
    npass = (n + 63) // 64
    F, V = np.zeros((npass, 64)), np.zeros((npass, 64), np.uint64)
    acc, plan = np.zeros(64), np.zeros((npass, 4), np.int32)
    g4, om = np.ascontiguousarray(g.g4), np.ascontiguousarray(g.om)
    rc = L.zgroup_point(int(gmax), int(defect), int(truncate), g4.ctypes.data_as(DP), om.ctypes.data_as(DP), g.nz,
                        c2.ctypes.data_as(DP), wy.ctypes.data_as(DP), n, F.ctypes.data_as(DP), V.ctypes.data_as(UP),
                        acc.ctypes.data_as(DP), plan.ctypes.data_as(IP))
    assert rc == 0
    return F, V, acc, plan


def same(a, b):
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
            and np.array_equal(bits(a[2]), bits(b[2])))


def grouped(L, g, c2, truncate=0):
    """{gmax: plan} for gmax = 2, 4, after checking F, the node checksum and acc against the per-pass loop."""
    ref = run(L, g, c2, 0, truncate)
    assert np.all(ref[3][:, 0] == 1) and np.all(ref[3][:, 2] == 0)
    plans = {}
    for gmax in (2, 4):
        got = run(L, g, c2, gmax, truncate)
        assert np.array_equal(bits(ref[0]), bits(got[0])), ("F differs", gmax)
        assert np.array_equal(ref[1], got[1]), ("node values differ", gmax)
        assert np.array_equal(bits(ref[2]), bits(got[2])), ("acc differs", gmax)
        plans[gmax] = got[3]
    return plans, ref


def dead_lanes(g, n=64):
    return -np.geomspace(1.0, 1e6, n) * (N * 1077.0 / float(g.g4[1]))


def whole_lanes(g, n=64):
    """Live lanes with s = A at every node: |c2N| g_max far below half an ulp of A; +-0 and tiny positive among them."""
    c = -np.geomspace(1e-300, 1e-14, n) / float(g.g4[-1])
    c[3::64], c[17::64] = 0.0, -0.0
    c[5::64], c[40::64] = 5e-324, 1e-20
    return c


def general_lanes(g, n=64):
    """Clamp-free lanes, no zero pass: |c2N| g_max from 2 to 2000."""
    return -np.geomspace(2.0, 2000.0, n) / float(g.g4[-1])


def slot_class(L, g, c):
    gp = HF.padded(g)
    return L.zgroup_slot(float(c), float(gp[0]), float(gp[1]), float(gp[-1]))


def whole_boundary(L, g):
    """(c_in, c_out): the whole-frozen lane of largest |c2N| and its neighbour one ulp beyond, which is not."""
    lo, hi = np.float64(1e-30).view(np.int64), np.float64(1.0).view(np.int64)   # (a lane of large |c2N| is dead)
    assert slot_class(L, g, -1e-30) == GRP_WHOLE and slot_class(L, g, -1.0) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if slot_class(L, g, -float(np.int64(mid).view(np.float64))) & GRP_WHOLE:
            lo = mid
        else:
            hi = mid
    return -float(np.int64(lo).view(np.float64)), -float(np.int64(hi).view(np.float64))


def sizes(plan):
    return plan[:, 0].tolist()


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_all_dead_groups(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    c2 = dead_lanes(g, 64 * 9)
    assert all(slot_class(lib, g, c) == GRP_DEAD | GRP_WHOLE for c in c2[::37])
    plans, ref = grouped(lib, g, c2)
    assert sizes(plans[4]) == [4] * 8 + [1] and sizes(plans[2]) == [2] * 8 + [1]
    assert np.all(plans[4][:, 1] == DEAD) and np.all(plans[2][:, 1] == DEAD)
    assert np.all(ref[0] == 0.0) and not np.any(np.signbit(ref[0])) and np.all(ref[2] == 0.0)


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_whole_frozen_groups(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    c2 = whole_lanes(g, 64 * 9)
    plans, ref = grouped(lib, g, c2)
    assert sizes(plans[4]) == [4] * 8 + [1] and sizes(plans[2]) == [2] * 8 + [1]
    assert np.all(plans[4][:, 1] == ZERO) and np.all(plans[4][:, 3] == 0)   # held from node 0
    assert np.all(ref[3][:, 1] == ZERO) and np.all(ref[3][:, 3] == 0)       # as the single pass: k3 = 0
    assert np.all(ref[0] > 0.0) and np.all(ref[2] > 0.0)


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_group_mixing_dead_and_frozen_passes(lib, nz, z_max):
    """A dead pass next to a frozen one, and dead lanes inside frozen passes: the group is the held one (a
    dead lane passes the whole test with c2e = +0), the dead lanes' F is the exact zero."""
    g = Z.grid(nz, z_max)
    c2 = whole_lanes(g, 64 * 8).reshape(8, 64)
    d = dead_lanes(g)
    c2[1], c2[6] = d, d                       # whole passes of dead lanes
    c2[2, ::3], c2[4, 1::2] = d[::3], d[1::2]  # dead lanes among live ones
    plans, ref = grouped(lib, g, c2)
    assert sizes(plans[4]) == [4] * 8 and np.all(plans[4][:, 1] == ZERO)
    assert sizes(plans[2]) == [2] * 8 and np.all(plans[2][:, 1] == ZERO)
    assert ref[3][1, 1] == DEAD and ref[3][6, 1] == DEAD          # the single passes take zsum_dead
    F = ref[0]
    assert np.all(F[1] == 0.0) and np.all(F[2, ::3] == 0.0) and np.all(F[4, 1::2] == 0.0) and np.all(F[0] > 0.0)
    assert not np.any(np.signbit(F))


@pytest.mark.parametrize("lane", [0, 31, 63])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_one_lane_an_ulp_off_drops_the_group(lib, nz, z_max, lane):
    g = Z.grid(nz, z_max)
    c_in, c_out = whole_boundary(lib, g)
    base = whole_lanes(g, 64 * 4).reshape(4, 64)
    # at the boundary itself the four passes group
    c2 = base.copy()
    c2[3, lane] = c_in
    plans, _ = grouped(lib, g, c2)
    assert sizes(plans[4]) == [4] * 4 and sizes(plans[2]) == [2] * 4
    # an ulp beyond it in the LAST slot: the group of four drops to its first half, the rest run singly
    c2[3, lane] = c_out
    plans, ref = grouped(lib, g, c2)
    assert sizes(plans[4]) == [2, 2, 1, 1] and sizes(plans[2]) == [2, 2, 1, 1]
    assert plans[4][2, 2] == 1 and plans[4][3, 2] == 0           # the pair (2, 3) was tried and refused
    assert not (ref[3][3, 1] == ZERO and ref[3][3, 3] == 0)       # that pass alone is no accumulate-only pass
    # in the second slot: singles throughout
    c2 = base.copy()
    c2[1, lane] = c_out
    plans, _ = grouped(lib, g, c2)
    assert sizes(plans[4]) == [1, 1, 1, 1] and sizes(plans[2]) == [1, 1, 1, 1]


@pytest.mark.parametrize("n,want4,want2", [
    (64 * 6 + 16, [4, 4, 4, 4, 2, 2, 1], [2, 2, 2, 2, 2, 2, 1]),
    (64 * 5 + 16, [4, 4, 4, 4, 1, 1], [2, 2, 2, 2, 1, 1]),
    (64 * 7, [4, 4, 4, 4, 2, 2, 1], [2, 2, 2, 2, 2, 2, 1]),
    (64 * 3 + 63, [2, 2, 1, 1], [2, 2, 1, 1]),
    (64 + 1, [1, 1], [1, 1]),
    (40, [1], [1]),
])
@pytest.mark.parametrize("kind", ["dead", "whole"])
def test_short_ends_and_partial_last_pass(lib, kind, n, want4, want2):
    """Only full passes are grouped; a y-count that leaves fewer than G passes takes the smaller group or singles."""
    g = Z.grid(1200, 30.0)
    c2 = dead_lanes(g, n) if kind == "dead" else whole_lanes(g, n)
    plans, _ = grouped(lib, g, c2)
    assert sizes(plans[4]) == want4 and sizes(plans[2]) == want2


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_no_group_is_tried_after_a_pass_that_is_not_accumulate_only(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    c2 = whole_lanes(g, 64 * 8).reshape(8, 64)
    c2[1] = general_lanes(g)
    plans, ref = grouped(lib, g, c2)
    assert ref[3][1, 1] == FREE
    p = plans[4]
    assert sizes(p) == [1, 1, 1, 4, 4, 4, 4, 1]
    assert p[:, 2].tolist() == [1, 1, 0, 1, 0, 0, 0, 0]           # pass 2 follows the general pass: no attempt
    p = plans[2]
    assert sizes(p) == [1, 1, 1, 2, 2, 2, 2, 1]
    assert p[:, 2].tolist() == [1, 1, 0, 1, 0, 1, 0, 0]


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_truncated_passes_are_never_grouped(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    c2 = np.concatenate([whole_lanes(g, 64 * 4), dead_lanes(g, 64 * 4)])
    plans, ref = grouped(lib, g, c2, truncate=1)
    for gmax in (2, 4):
        assert np.all(plans[gmax][:, 0] == 1) and np.all(plans[gmax][:, 2] == 0)
    dense = run(lib, g, c2, 4, 0)
    assert sizes(dense[3]) == [4] * 8
    assert np.array_equal(bits(dense[0]), bits(ref[0])) and np.array_equal(bits(dense[2]), bits(ref[2]))


def c2_points():
    """c2N of the C2 workload's 8000 y-nodes (every point has the same)."""
    B, Tp, I_p = 100.0, 100.0, 0.34                              # yields_config_equal_mass.json (C2's base)
    y_of = lambda T: 0.5 * B * ((Tp / T) ** 2 - 1.0)
    ys = np.linspace(max(y_of(5.0 * Tp), -80.0), min(y_of(1e-3 * Tp), 50.0), 8000)
    return ((-(I_p / 6.0) * np.exp(np.clip(ys, -50.0, 50.0))) * Z.LOG2E) * N


def group_counts(plan):
    """{(size, path): number of groups} of the grouped passes of a plan."""
    out = {}
    p = 0
    while p < len(plan):
        s = int(plan[p, 0])
        if s > 1:
            out[(s, int(plan[p, 1]))] = out.get((s, int(plan[p, 1])), 0) + 1
        p += s
    return out


def test_c2_plan(lib):
    """The C2 workload on the default grid: 14 frozen and 30 dead passes of 125 are grouped."""
    g = Z.grid(1200, 30.0)
    plans, ref = grouped(lib, g, c2_points())
    p4 = plans[4]
    assert len(p4) == 125
    assert group_counts(p4) == {(4, ZERO): 3, (2, ZERO): 1, (4, DEAD): 7, (2, DEAD): 1}
    assert int((p4[:, 0] > 1).sum()) == 44
    assert group_counts(plans[2]) == {(2, ZERO): 7, (2, DEAD): 15}
    refused = int(((p4[:, 0] == 1) & (p4[:, 2] == 1)).sum())
    assert refused == 2                                           # passes 14 and 15: classifications that come to nothing
    print(f"C2 plan: {int((p4[:, 0] > 1).sum())} of 125 passes grouped "
          f"({44 * 1200 / 150000:.1%} of the nodes), {refused} refused classifications per point")


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_broken_loops_are_told_apart(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    # the group test on slot 0 only: a general pass behind a whole one is swept as if it were frozen
    c2 = whole_lanes(g, 64 * 4).reshape(4, 64)
    c2[1] = general_lanes(g)
    good, bad = run(lib, g, c2, 4), run(lib, g, c2, 4, defect=SLOT_0_ONLY)
    assert same(good, run(lib, g, c2, 0))
    assert sizes(bad[3]) == [4] * 4 and sizes(good[3]) == [1, 1, 1, 1]
    assert not np.array_equal(bad[1][1], good[1][1]) and not np.array_equal(bits(bad[0][1]), bits(good[0][1]))
    assert np.array_equal(bad[1][0], good[1][0])
    # the passes of a group integrated last to first: every F is right, acc is not
    c2 = whole_lanes(g, 64 * 8).reshape(8, 64)
    c2[5] = dead_lanes(g)
    good, bad = run(lib, g, c2, 4), run(lib, g, c2, 4, defect=DESCENDING)
    assert same(good, run(lib, g, c2, 0))
    assert np.array_equal(bits(bad[0]), bits(good[0])) and np.array_equal(bad[1], good[1])
    assert not np.array_equal(bits(bad[2]), bits(good[2]))
    assert np.allclose(bad[2], good[2], rtol=1e-14, atol=0.0)     # the same sum, rounded in another order


def test_group_seg_off_is_the_parent_machine_code(tmp_path):
    """-DLZQ_GROUP_SEG=0 compiles the headline kernels to the ISA the parent's profile was taken on."""
    b, codeobj = pkg("build"), pkg("codeobj")
    out = str(tmp_path / "lzq_kernels_off.so")
    subprocess.run([b.hipcc(), *b.FLAGS, "-DLZQ_GROUP_SEG=0", "-I", b.INCLUDE, os.path.join(b.CSRC, "lzq_kernels.hip"),
                    "-o", out], check=True)
    got = codeobj.kernel_isa_sha256(out)
    assert got is not None, "llvm-objdump (ROCm) is needed to disassemble the code object"
    with open(os.path.join(ROOT, "profiles", "round11", "parent_pmc_summary.json")) as f:
        want = json.load(f)["kernel_isa_sha256"]
    assert want == "3d2c7709c642aa385d51339897b20f5b10d7ae62ed91b158b518e6118b4a8385"   # the parent's, pinned
    assert got == want
