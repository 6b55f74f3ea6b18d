"""The zero stretch of the dense z-sum without its range reduction (csrc/lzq_quad.h
zsum_uniform<YB, true>, LZQ_ZERO_SEG; csrc/lzq_exp2.h seg_node_zero), on the CPU.

On a pass whose 64 lanes all have t = fma(c2N, g_max, M) = M the device forms s = fma(c2N, g, A) at
every node instead of recomputing t (= M) and w = (M + A) - t (= A).  tests/zsum_zero_segment_host.cpp
compiles the LZQ_HD functions of csrc/lzq_exp2.h that the device code itself calls and evaluates a
64-lane pass twice: with the dispatch whose zero path runs seg_node_zero, and with the single general
loop (lzq::exp2_tab_scaled at every node).  The two F must agree bit for bit in every lane, and so
must the three nodes (seg_node_zero, seg_node, exp2_tab_scaled) node by node; one ulp beyond the
boundary the dispatch must leave the zero path, and there the shortened node does differ from the
general one -- the comparison can fail.

Lanes are given as c2N = c2 * 8192 directly, so that a lane can sit exactly on the boundary of the
loop's own expression; the boundary is found by bisection on the library's own seg_zero.

The last two tests pin what the device build must keep: the headline kernels' registers and
occupancy, and that -DLZQ_ZERO_SEG=0 is the parent's machine code (profiles/round8/
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
ZERO, FREE, SPLIT = 0, 1, 2             # plan[0] of zsum_zero_segment_host.cpp
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(tempfile.mkdtemp(), "zsum_zero_segment_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "zsum_zero_segment_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.zzero_passes.argtypes = [ctypes.c_int, ctypes.c_int, DP, DP, ctypes.c_int, DP, ctypes.c_long, DP, IP]
    L.zzero_nodes.argtypes = [ctypes.c_double, DP, ctypes.c_int, DP]
    for f in (L.zzero_zero, L.zzero_dead):
        f.argtypes = [ctypes.c_double, ctypes.c_double]
    return L


def run(L, g, c2, segmented, truncate):
    c2 = np.ascontiguousarray(np.asarray(c2, float).reshape(-1, 64))
    F = np.empty_like(c2)
    plan = np.empty((c2.shape[0], 3), np.int32)
    g4, om = np.ascontiguousarray(g.g4), np.ascontiguousarray(g.om)
    rc = L.zzero_passes(int(segmented), int(truncate), g4.ctypes.data_as(DP), om.ctypes.data_as(DP), g.nz,
                        c2.ctypes.data_as(DP), c2.shape[0], F.ctypes.data_as(DP), plan.ctypes.data_as(IP))
    assert rc == 0
    return F, plan


def both(L, g, c2, truncate):
    """(F, plan) of the dispatch after checking it against the single general loop."""
    Fs, plan = run(L, g, c2, 1, truncate)
    Fg, pg = run(L, g, c2, 0, truncate)
    assert np.array_equal(Fs.view(np.int64), Fg.view(np.int64)), "zero-segment and general F differ"
    assert np.array_equal(plan[:, 2], pg[:, 2]) and np.all(plan[:, 2] % 8 == 0)
    return Fs, plan


def nodes(L, c2N, g4):
    """(seg_node_zero, seg_node, exp2_tab_scaled) of one lane at every node, as int64 bits."""
    g4 = np.ascontiguousarray(g4, dtype=np.float64)
    v = np.empty((3, g4.size))
    assert L.zzero_nodes(float(c2N), g4.ctypes.data_as(DP), g4.size, v.ctypes.data_as(DP)) == 0
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


def boundary(L, g):
    """(c_in, c_out): the last c2N whose t at g_max is still M (the tie |c2N| g_max = 1/2, which rounds
    to the even M), and its neighbour one ulp beyond."""
    g_max = float(g.g4[-1])
    c_out = first_true(lambda c: not L.zzero_zero(c, g_max))
    c_in = float(np.nextafter(c_out, 0.0))
    assert L.zzero_zero(c_in, g_max) and not L.zzero_zero(c_out, g_max)
    assert abs(c_in * g_max) <= 0.5 < abs(c_out * g_max) * (1 + 1e-15)
    return c_in, c_out


@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_zero_passes_equal_the_general_loop(lib, nz, z_max, truncate):
    g = Z.grid(nz, z_max)
    g_1 = float(g.g4[1])
    kend = padded(g).size
    c_in, c_out = boundary(lib, g)
    c_dead = first_true(lambda c: bool(lib.zzero_dead(c, g_1)))
    below = -np.geomspace(abs(c_in) * 1e-30, abs(c_in) * (1 - 1e-9), 64)
    F, plan = both(lib, g, below, truncate)                              # 64 lanes spread below the boundary
    assert plan[0].tolist() == [ZERO, 0, kend] and np.all(F > 0)
    lanes = below.copy()
    lanes[17] = c_in                                                     # one lane exactly ON the boundary
    F, plan = both(lib, g, lanes, truncate)
    assert plan[0, 0] == ZERO and F[0, 17] > 0
    lanes[17] = c_out                                                    # ... and one ulp beyond it: not the zero path
    assert both(lib, g, lanes, truncate)[1][0, 0] == FREE
    dead = -np.geomspace(abs(c_dead), abs(c_dead) * 1e6, 64)
    F, plan = both(lib, g, dead, truncate)                               # all dead: c2e = 0, F zeroed, +0
    assert plan[0, 0] == ZERO and np.all(F == 0.0) and not np.any(np.signbit(F))
    mixed = dead.copy()                                                  # dead and small lanes in one wave
    mixed[0::2] = below[0::2]
    mixed[40] = c_in
    F, plan = both(lib, g, mixed, truncate)
    assert plan[0, 0] == ZERO and np.all(F[0, 1::2] == 0.0) and not np.any(np.signbit(F[0, 1::2]))
    assert np.all(F[0, 0::2] > 0.0)
    signed = below.copy()                                                # c2 = +-0 and tiny positive c2
    signed[[0, 1, 2, 3, 4]] = [0.0, -0.0, 5e-324, 1e-300, abs(c_in) * 1e-3]
    F, plan = both(lib, g, signed, truncate)
    assert plan[0].tolist() == [ZERO, 0, kend] and np.all(F > 0)
    assert _bits(F[0, 0]) == _bits(F[0, 1]) == _bits(F[0, 2]) == _bits(F[0, 3])   # u = 0 at every node


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_the_three_nodes_agree_node_by_node(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    gp = padded(g)
    c_in, c_out = boundary(lib, g)
    lanes = list(-np.geomspace(abs(c_in) * 1e-30, abs(c_in) * (1 - 1e-9), 64))
    lanes += [c_in, 0.0, -0.0, 5e-324, 1e-300, abs(c_in) * 1e-3]
    for c in lanes:
        v = nodes(lib, c, gp)
        assert np.array_equal(v[0], v[1]) and np.array_equal(v[0], v[2]), c
    # one ulp beyond the boundary the shortened node is NOT the general node: at g_max the general
    # node has t = M - 1, reads the entry below and forms s = u + 1 + A; the shortened one keeps
    # T''[0] and s = u + A.  (The comparison above can fail.)
    v = nodes(lib, c_out, gp)
    assert v[0, -1] != v[2, -1] and v[0, g.nz - 1] != v[2, g.nz - 1]
    assert np.array_equal(v[1, :2], v[2, :2]) and np.array_equal(v[0, :2], v[2, :2])   # t = M still at the first nodes


def test_headline_kernels_keep_registers_and_occupancy():
    """tools/kernel_resources.py on lzq_kernels.hip: every yields_grid_kernel instantiation within 64
    VGPRs, without scratch, at the 8 waves/SIMD of its __launch_bounds__."""
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


def test_zero_seg_off_is_the_parent_machine_code(tmp_path):
    """-DLZQ_ZERO_SEG=0 compiles the headline kernels to the ISA the parent's profile was taken on."""
    b, codeobj = pkg("build"), pkg("codeobj")
    out = str(tmp_path / "lzq_kernels_off.so")
    subprocess.run([b.hipcc(), *b.FLAGS, "-DLZQ_ZERO_SEG=0", "-I", b.INCLUDE, os.path.join(b.CSRC, "lzq_kernels.hip"),
                    "-o", out], check=True)
    got = codeobj.kernel_isa_sha256(out)
    assert got is not None, "llvm-objdump (ROCm) is needed to disassemble the code object"
    with open(os.path.join(ROOT, "profiles", "round8", "parent_pmc_summary.json")) as f:
        assert got == json.load(f)["kernel_isa_sha256"]
