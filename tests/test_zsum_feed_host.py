"""The packed omega' array of a z grid's device image and the accumulate-only loops that read it
(csrc/lzq_exp2.h zimage_doubles / zimage_pack / zimage_omega; csrc/lzq_quad.h acc_omega in zsum_dead and
zsum_held, single and grouped; LZQ_ACC_FEED), on the CPU.

F = fma(omega'_k, v, F) with a value that is fixed per lane is priced by the 64-byte lines of the z table
its scalar loads touch.  Out of the interleaved {g4, omega'} nodes an 8-node batch is two lines, half of
each unused; the image therefore carries the weights once more as contiguous doubles behind its nzp nodes,
one line per batch, and the loops that need omega' alone read them there.  Nothing else moves: the same
operands in the same order.

tests/zsum_feed_host.cpp builds the image with the library's own zimage_pack and models one point (one
64-lane wavefront over n y-nodes, grouped passes included) reading the weights where the device reads them.
It is compared with tests/zsum_group_host.cpp's pass loop on the nodes' own weights, bit for bit, on F, on the
checksum over every node's value, on a checksum over every weight read, and on the y-loop's acc.

Two deliberately broken feeds (the array looked for behind the unpadded node count; a held tail reading the
array from its start) must be told from the right one.  The last test pins that -DLZQ_ACC_FEED=0 is the
parent's machine code (profiles/round13/parent_pmc_summary.json), so the ablation's baseline library can be
built from this tree.
"""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import test_zsum_frozen_host as HF
import test_zsum_group_host as HG
import zsum_ref as Z
from conftest import PKG_NAME, ROOT, pkg

HERE = os.path.dirname(os.path.abspath(__file__))
GRIDS = HF.GRIDS                                  # (1200, 30), (13, 3) padded to 16, (2400, 30)
ZERO, FREE, SPLIT, DEAD = HF.ZERO, HF.FREE, HF.SPLIT, HF.DEAD
DP, IP, UP = HF.DP, HF.IP, HF.UP
BEHIND_NZ, TAIL_FROM_START = 1, 2                 # `defect` of zfeed_point
bits = HF.bits


def load_lib():
    so = os.path.join(tempfile.mkdtemp(), "zsum_feed_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "zsum_feed_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.zgroup_point.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, DP, DP, ctypes.c_int, DP, DP, ctypes.c_long,
                               DP, UP, DP, IP]
    L.zgroup_slot.argtypes = [ctypes.c_double] * 4
    L.zfrozen_values.argtypes = [ctypes.c_int, ctypes.c_double, DP, ctypes.c_int, DP]   # (HF's lane builders)
    L.zfeed_image.argtypes = [DP, DP, ctypes.c_int, DP]
    L.zfeed_point.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, DP, DP, ctypes.c_int, DP, DP,
                              ctypes.c_long, DP, UP, DP, IP, UP, IP]
    return L


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def run(L, g, c2, feed, gmax=4, truncate=0, defect=0, wy=None):
    """(F, node-value checksum, acc, plan, weight checksum, fed nodes per pass) of one point with y-nodes c2."""
    c2 = np.ascontiguousarray(np.asarray(c2, float).ravel())
    n = c2.size
    wy = np.ascontiguousarray(HG.weights(n) if wy is None else wy)
    npass = (n + 63) // 64
    F, V, W = np.zeros((npass, 64)), np.zeros((npass, 64), np.uint64), np.zeros((npass, 64), np.uint64)
    acc, plan, fed = np.zeros(64), np.zeros((npass, 4), np.int32), np.zeros(npass, np.int32)
    g4, om = np.ascontiguousarray(g.g4), np.ascontiguousarray(g.om)
    rc = L.zfeed_point(int(feed), int(defect), int(gmax), int(truncate), g4.ctypes.data_as(DP), om.ctypes.data_as(DP),
                       g.nz, c2.ctypes.data_as(DP), wy.ctypes.data_as(DP), n, F.ctypes.data_as(DP),
                       V.ctypes.data_as(UP), acc.ctypes.data_as(DP), plan.ctypes.data_as(IP), W.ctypes.data_as(UP),
                       fed.ctypes.data_as(IP))
    assert rc == 0
    return F, V, acc, plan, W, fed


def same(a, b):
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
            and np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(a[4], b[4]))


def fed_point(L, g, c2, truncate=0, wy=None):
    """The point with the packed feed, after checking it against the pass loop of zsum_group_host.cpp and against
    the per-pass dispatch, on the nodes' own weights: F, node values, weights read and acc, bit for bit."""
    got = run(L, g, c2, 1, 4, truncate, wy=wy)
    for gmax in (4, 2, 0):
        own = run(L, g, c2, 0, gmax, truncate, wy=wy)
        ref = HG.run(L, g, c2, gmax, truncate, wy=wy)
        assert np.array_equal(bits(own[0]), bits(ref[0])) and np.array_equal(bits(own[2]), bits(ref[2]))
        assert np.array_equal(bits(got[0]), bits(ref[0])), ("F differs", gmax)
        assert np.array_equal(got[1], ref[1]), ("node values differ", gmax)
        assert np.array_equal(bits(got[2]), bits(ref[2])), ("acc differs", gmax)
        fed = run(L, g, c2, 1, gmax, truncate, wy=wy)
        assert same(fed, own) and np.array_equal(fed[5], own[5]), ("weights read differ", gmax)
    return got


def mixed_point(g, L):
    """Ten passes of every kind: whole-frozen and dead runs (grouped), zero passes with a tail, a clamp-free and a
    clamped pass, dead lanes among live ones."""
    gp = HF.padded(g)
    tail = HF.tail_wave(L, HF.S, g, gp)[0]
    c2 = np.concatenate([HG.whole_lanes(g, 64 * 2), tail, tail * 1.01, HG.general_lanes(g),
                         HG.dead_lanes(g, 64 * 4), tail[::-1]]).reshape(10, 64)
    c2[7, ::3] = tail[::3]                          # live lanes in a dead pass: the pass is a zero pass with a tail
    c2[3, 5::7] = HG.dead_lanes(g)[5::7]            # dead lanes in a zero pass
    return c2


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_packed_array_is_the_nodes_own_weights(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    nzp = (max(nz, 8) + 7) // 8 * 8
    assert lib.zfeed_image_doubles(nz) == 3 * nzp
    img = np.full(3 * nzp, np.nan)
    g4, om = np.ascontiguousarray(g.g4), np.ascontiguousarray(g.om)
    assert lib.zfeed_image(g4.ctypes.data_as(DP), om.ctypes.data_as(DP), nz, img.ctypes.data_as(DP)) == 0
    nodes, packed = img[:2 * nzp].reshape(nzp, 2), img[2 * nzp:]
    assert np.array_equal(bits(packed), bits(nodes[:, 1]))                     # ZNode::omega, bit for bit
    assert np.array_equal(bits(packed[:nz]), bits(np.ldexp(g.om, -512)))
    assert np.array_equal(bits(packed[nz:]), np.zeros(nzp - nz, np.int64))     # padding: +0
    assert np.array_equal(nodes[:nz, 0], g.g4) and np.all(nodes[nz:, 0] == g.g4[-1])
    assert (packed.ctypes.data - img.ctypes.data) % 64 == 0                    # whole 64-byte lines behind the nodes


@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_every_kind_of_pass_reads_the_same_weights(lib, nz, z_max, truncate):
    g = Z.grid(nz, z_max)
    F, V, acc, plan, W, fed = fed_point(lib, g, mixed_point(g, lib), truncate)
    nzp = (max(nz, 8) + 7) // 8 * 8
    path, size, k3 = plan[:, 1], plan[:, 0], plan[:, 3]
    assert set(path.tolist()) >= {ZERO, DEAD, FREE}
    acc_only = (path == ZERO) | (path == DEAD)
    assert np.all(fed[~acc_only] == 0) and np.all(W[~acc_only] == 0)
    if truncate:
        assert np.all(size == 1)                                              # truncation is never grouped
        assert np.any((fed > 0) & (fed < nzp))
    else:
        assert np.any(size > 1) and np.all(fed[size > 1] == nzp)              # a group's chains: every node
        tails = (path == ZERO) & (size == 1) & (k3 > 0)
        assert tails.sum() >= 2 and np.array_equal(fed[tails], nzp - k3[tails])  # a tail: from its own k3
        assert np.all(fed[(path == DEAD)] == nzp)
    assert np.all(fed % 8 == 0)


@pytest.mark.parametrize("n", [64 * 6 + 16, 64 * 3 + 63, 64 + 1, 40])
@pytest.mark.parametrize("kind", ["dead", "whole", "tail"])
def test_short_ends_and_partial_last_pass(lib, kind, n):
    g = Z.grid(1200, 30.0)
    if kind == "tail":
        c2 = np.resize(HF.zero_tail_lanes(g), n)
    else:
        c2 = HG.dead_lanes(g, n) if kind == "dead" else HG.whole_lanes(g, n)
    got = fed_point(lib, g, c2)
    assert np.all(got[5] > 0)


def test_c2_plan_takes_the_packed_feed(lib):
    """The C2 workload on the default grid: 42.8% of the point's nodes read the packed array -- the grouped
    sweeps, the two whole passes outside a group and the held tails -- and the z-table lines a point's scalar
    loads touch fall by the lines those batches no longer read."""
    g = Z.grid(1200, 30.0)
    F, V, acc, plan, W, fed = fed_point(lib, g, HG.c2_points())
    size, path, k3 = plan[:, 0], plan[:, 1], plan[:, 3]
    assert len(plan) == 125 and int((size > 1).sum()) == 44
    nodes = 125 * 1200
    share = fed.sum() / nodes
    tails = (size == 1) & (path == ZERO) & (k3 > 0) & (fed > 0)
    single_whole = (size == 1) & (fed == 1200)
    assert int(fed[size > 1].sum()) == 44 * 1200 and int(single_whole.sum()) == 2
    assert int(fed[tails].sum()) == 9008                                      # the frozen-s tails
    assert abs(share - 0.428) < 0.0005
    print(f"C2 plan: {int(fed.sum())} of {nodes} nodes ({share:.1%}) read the packed array: "
          f"{int(fed[size > 1].sum())} in groups, {int(fed[single_whole].sum())} in whole single passes, "
          f"{int(fed[tails].sum())} in {int(tails.sum())} held tails")


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_broken_feeds_are_told_apart(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    c2 = mixed_point(g, lib)
    good = run(lib, g, c2, 1)
    assert same(good, run(lib, g, c2, 0))
    # the array looked for behind the nz real nodes: right where nz needs no padding, wrong where it does
    bad = run(lib, g, c2, 1, defect=BEHIND_NZ)
    if nz % 8 == 0:
        assert same(bad, good)
    else:
        assert not np.array_equal(bad[4], good[4]) and not np.array_equal(bits(bad[0]), bits(good[0]))
        assert not np.array_equal(bits(bad[2]), bits(good[2]))
    # a held tail reading the array from its start: the whole passes are right, the tails are not
    bad = run(lib, g, c2, 1, defect=TAIL_FROM_START)
    tails = (good[3][:, 1] == ZERO) & (good[3][:, 0] == 1) & (good[3][:, 3] > 0) & (good[5] > 0)
    assert tails.any()
    assert np.array_equal(bits(bad[0][~tails]), bits(good[0][~tails])) and np.array_equal(bad[4][~tails], good[4][~tails])
    live = good[0][tails] != 0.0
    assert np.all(bad[4][tails] != good[4][tails]) and np.all(bits(bad[0][tails])[live] != bits(good[0][tails])[live])
    assert not np.array_equal(bits(bad[2]), bits(good[2]))


def test_acc_feed_off_is_the_parent_machine_code(tmp_path):
    """-DLZQ_ACC_FEED=0 compiles the headline kernels to the ISA the parent's profile was taken on."""
    b, codeobj = pkg("build"), pkg("codeobj")
    out = str(tmp_path / "lzq_kernels_off.so")
    subprocess.run([b.hipcc(), *b.FLAGS, "-DLZQ_ACC_FEED=0", "-I", b.INCLUDE, os.path.join(b.CSRC, "lzq_kernels.hip"),
                    "-o", out], check=True)
    got = codeobj.kernel_isa_sha256(out)
    assert got is not None, "llvm-objdump (ROCm) is needed to disassemble the code object"
    with open(os.path.join(ROOT, "profiles", "round13", "parent_pmc_summary.json")) as f:
        want = json.load(f)["kernel_isa_sha256"]
    assert want == "d04ac70d49c44207a31bab33a9adfc3db3d8248e970fd3266f27309c423b1be4"   # the parent's, pinned
    assert got == want
