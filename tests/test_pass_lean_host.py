"""The lean per-pass work of the dense y-loop (csrc/lzq_quad.h LZQ_PASS_LEAN, csrc/lzq_ynode.h), on the CPU.

A pass of yb_wave that touches neither end of the y-grid forms y_j and its trapezoid weight without the
end-of-grid selects of the general forms (j == n - 1 ? y_hi, j > 0, j + 1 < n, j < n, min(j, n - 1)): the
same convert, multiply, add and subtract.  tests/pass_lean_host.cpp compiles the header's functions, which
the device code calls: for every pass of n = 2000 (a partial last pass), 2048, 2112 (full passes) and 8000
(the headline), the interior forms are compared bit for bit with the general forms on every node of every
pass the gate lets through, and both with numpy.linspace and the weights the reference forms from
numpy.diff.  The gate must refuse the first pass, the last one and a partial one -- and exactly the passes
on which the two forms differ or the interior form would read past the grid.

The last test pins that -DLZQ_PASS_LEAN=0 is the parent's machine code
(profiles/round12/parent_pmc_summary.json), so the ablation's baseline library can be built from this tree.
"""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT, pkg

HERE = os.path.dirname(os.path.abspath(__file__))
DP = ctypes.POINTER(ctypes.c_double)
NS = (2000, 2048, 2112, 8000)
# y-ranges: the C2 workload's (y_lo = -48, y_hi clipped to 50), one reaching below -50, a short one around 0
RANGES = ((-48.0, 50.0), (-80.0, 37.3), (-0.3, 0.7))


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(tempfile.mkdtemp(), "pass_lean_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "pass_lean_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.ylean_pass.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, DP, DP, DP, DP]
    L.ylean_gate.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return L


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def one_pass(L, y_lo, y_hi, n, base):
    a = [np.empty(64) for _ in range(4)]
    gate = L.ylean_pass(y_lo, y_hi, n, base, *[x.ctypes.data_as(DP) for x in a])
    return gate, a


def reference(y_lo, y_hi, n):
    """numpy.linspace and the trapezoid weights of fpy:267, (d_{j-1} + d_j)/2 with d = diff(ys), 0 beyond an end."""
    ys = np.linspace(y_lo, y_hi, n)
    d = np.diff(ys)
    dl, dr = np.concatenate([[0.0], d]), np.concatenate([d, [0.0]])
    return ys, 0.5 * (dl + dr)


@pytest.mark.parametrize("y_lo,y_hi", RANGES)
@pytest.mark.parametrize("n", NS)
def test_interior_forms_are_the_general_forms_on_every_interior_pass(lib, n, y_lo, y_hi):
    ys, ws = reference(y_lo, y_hi, n)
    npass = (n + 63) // 64
    gates = []
    for p in range(npass):
        base = 64 * p
        gate, (yg, wg, yi, wi) = one_pass(lib, y_lo, y_hi, n, base)
        gates.append(gate)
        m = min(64, n - base)
        # the general forms are numpy's on every node of the grid; tail lanes repeat the last node with weight 0
        assert np.array_equal(bits(yg[:m]), bits(ys[base:base + m])), (p, "y_node is not numpy.linspace")
        assert np.array_equal(bits(wg[:m]), bits(ws[base:base + m])), (p, "y_weight is not the reference's")
        assert np.all(wg[m:] == 0.0) and np.all(bits(yg[m:]) == bits(ys[-1:]))
        if gate:
            assert m == 64
            assert np.array_equal(bits(yi), bits(yg)), (p, "interior y differs")
            assert np.array_equal(bits(wi), bits(wg)), (p, "interior weight differs")
    # the gate refuses the first pass, the last pass (full or partial) and nothing it need not
    assert gates[0] == 0 and gates[-1] == 0
    want = [int(64 * p >= 64 and 64 * p + 64 + 1 < n) for p in range(npass)]
    assert gates == want
    assert sum(gates) == npass - 2 - int(n % 64 == 1)            # (n = 64 k + 1: the pass before the 1-node tail too)
    print(f"n = {n}, [{y_lo}, {y_hi}]: {sum(gates)} of {npass} passes interior")


@pytest.mark.parametrize("n", NS)
def test_refused_passes_are_the_ones_the_interior_forms_get_wrong(lib, n):
    """On the first pass the interior weight has a left difference node 0 does not have; on the last, node
    n - 1 is y_hi itself, not (n - 1) * step + y_lo (they differ by rounding on this range), and the partial
    pass has lanes past the grid."""
    y_lo, y_hi = -48.0, 50.0
    gate, (yg, wg, yi, wi) = one_pass(lib, y_lo, y_hi, n, 0)
    assert gate == 0 and bits(wi[0]) != bits(wg[0]) and np.array_equal(bits(wi[1:]), bits(wg[1:]))
    base = (n - 1) // 64 * 64
    gate, (yg, wg, yi, wi) = one_pass(lib, y_lo, y_hi, n, base)
    last = n - 1 - base
    assert gate == 0
    assert bits(wi[last]) != bits(wg[last])                       # no right difference at the last node
    if last < 63:
        assert not np.array_equal(bits(yi[last + 1:]), bits(yg[last + 1:]))   # tail lanes
    # a full pass whose right neighbour is the last node: j + 1 = n - 1 must read y_hi
    if n % 64 == 0:
        assert lib.ylean_gate(y_lo, y_hi, n, n - 64, 64) == 0
        assert lib.ylean_gate(y_lo, y_hi, n + 1, n - 64, 64) == 0  # j + 1 = n - 1 of an (n + 1)-node grid
        assert lib.ylean_gate(y_lo, y_hi, n + 2, n - 64, 64) == 1


def test_gate_of_groups_and_of_a_degenerate_step(lib):
    y_lo, y_hi, n = -48.0, 50.0, 8000
    # a group of four passes is interior when all four are
    for base in range(0, n - 256, 64):
        want = all(lib.ylean_gate(y_lo, y_hi, n, base + 64 * b, 64) for b in range(4))
        assert lib.ylean_gate(y_lo, y_hi, n, base, 256) == int(want), base
    assert lib.ylean_gate(y_lo, y_hi, n, 0, 256) == 0 and lib.ylean_gate(y_lo, y_hi, n, 64, 256) == 1
    # (n = 125 * 64: the group that ends at the last node is refused, the one a pass before it is not)
    assert lib.ylean_gate(y_lo, y_hi, n, n - 64 * 4, 256) == 0 and lib.ylean_gate(y_lo, y_hi, n, n - 64 * 5, 256) == 1
    # numpy's step == 0 branch (delta / (n - 1) underflows): the general form divides instead, no pass is interior
    assert lib.ylean_gate(0.0, 5e-324, n, 640, 64) == 0
    gate, (yg, wg, yi, wi) = one_pass(lib, 0.0, 5e-324, n, 6400)
    ys, _ = reference(0.0, 5e-324, n)
    assert gate == 0 and np.array_equal(bits(yg), bits(ys[6400:6464])) and not np.array_equal(bits(yi), bits(yg))


def test_pass_lean_off_is_the_parent_machine_code(tmp_path):
    """-DLZQ_PASS_LEAN=0 compiles the headline kernels to the ISA the parent's profile was taken on."""
    b, codeobj = pkg("build"), pkg("codeobj")
    out = str(tmp_path / "lzq_kernels_off.so")
    subprocess.run([b.hipcc(), *b.FLAGS, "-DLZQ_PASS_LEAN=0", "-I", b.INCLUDE, os.path.join(b.CSRC, "lzq_kernels.hip"),
                    "-o", out], check=True)
    got = codeobj.kernel_isa_sha256(out)
    assert got is not None, "llvm-objdump (ROCm) is needed to disassemble the code object"
    with open(os.path.join(ROOT, "profiles", "round12", "parent_pmc_summary.json")) as f:
        want = json.load(f)["kernel_isa_sha256"]
    assert want == "01973681b2799811ac89c894b1acaf318f6689c18ebf2c15259790c0b7b5d5bc"   # the parent's, pinned
    assert got == want
