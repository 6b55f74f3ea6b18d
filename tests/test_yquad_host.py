"""The reference of the Y_B y-quadrature (tests/yquad_ref.py) on the CPU: what tests/test_gpu_yquad.py
relies on, shown without a GPU.

(1) the mp y-quadrature, fed F_j formed in numpy from fpy:154-164, reproduces Y_B of the reference
    program itself (tests/golden/golden_points.json, n_y = 8000) within the sum tolerance;
(2) the y-node restatement is numpy.linspace and the compiled csrc/lzq_ynode.h, bit for bit, at every
    n_y of the GPU tests;
(3) a plain numpy FP64 model of the loop passes every case at node and sum level, so the reference and
    its tolerance admit correct arithmetic;
(4) six seeded defects of that model are rejected, each at the level that can see it;
(5) the node-probe window of the GPU test is exactly 1 at its own node and exactly 0 at every other;
(6) the case list reaches the regimes it is there for and holds no undecidable node.
"""
import ctypes
import os
import re
import subprocess
import tempfile
import time

import mpmath as mp
import numpy as np
import pytest

import yquad_ref as Y
from conftest import PKG_NAME, ROOT, full_cfg, golden, pkg

HERE = os.path.dirname(os.path.abspath(__file__))
DP = ctypes.POINTER(ctypes.c_double)
SIGMAS = (9.0, 0.3)

_cache = {}


def case_ref(case, n_y=Y.NY):
    """(config, y-grid, host F, Nodes) of a case, computed once and shared by the tests."""
    key = (case, n_y)
    if key not in _cache:
        c = Y.cfg_of(case)
        grid = Y.ygrid(c, n_y)
        F = Y.host_F(c, grid[3])
        _cache[key] = (c, grid, F, Y.nodes_ref(c, grid[3], F))
    return _cache[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------
# (1) the anchor to the reference program
# ---------------------------------------------------------------------------------------------
def fpy_F(c, ys):
    """fpy:154-164 in numpy doubles on the default z grid."""
    z = np.linspace(0.0, 30.0, 1200)
    ez = np.exp(-z)
    g4 = 6.0 - ez * (z ** 3 + 3.0 * z ** 2 + 6.0 * z + 6.0)
    trap = getattr(np, "trapezoid", None) or np.trapz
    out = np.empty(ys.size)
    for a in range(0, ys.size, 1000):
        expy = np.exp(np.clip(ys[a:a + 1000], -50.0, 50.0))
        out[a:a + 1000] = trap(z ** 2 * np.exp(-z) * np.exp(-(c["I_p"] / 6.0) * expy[:, None] * g4), z, axis=1)
    return out


def test_reference_reproduces_the_golden_yields():
    pts = golden("golden_points.json")["points"]
    picked = [0, 4, 5] + [i for i, p in enumerate(pts) if p["config"]["m_chi_GeV"] >= 3000.0
                          and p["final"]["Y_B"] > 0.0][:1]       # one non-relativistic config
    assert len(picked) == 4
    t0 = time.time()
    for i in picked:
        c = full_cfg(pts[i]["config"])
        _, _, _, ys = Y.ygrid(c, 8000)
        nd = Y.nodes_ref(c, ys, fpy_F(c, ys))
        assert not nd.undecided
        ref = Y.sum_ref(nd, Y.win_gauss(nd, c["source_shape_sigma_y"]))
        rel, ratio, bad = Y.compare_sum(pts[i]["final"]["Y_B"], ref)
        print(f"golden point {i} (m = {c['m_chi_GeV']}, {int((~nd.relativistic).sum())} non-relativistic nodes): "
              f"rel err {rel:.3e}, err/tol {ratio:.3f}")
        assert bad is None, (i, bad)
    print(f"anchor: {time.time() - t0:.1f} s")


# ---------------------------------------------------------------------------------------------
# (2) the y-nodes and the restated constants
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ylib():
    so = os.path.join(tempfile.mkdtemp(), "pass_lean_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "pass_lean_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.ylean_pass.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, DP, DP, DP, DP]
    return L


@pytest.mark.parametrize("n_y", (Y.NY,) + Y.NYS_MORE)
def test_ynodes_are_linspace_and_the_header(ylib, n_y):
    for case in Y.CASES:
        y_lo, y_hi, step, ys = Y.ygrid(Y.cfg_of(case), n_y)
        assert ys.size == n_y and np.array_equal(bits(ys), bits(np.linspace(y_lo, y_hi, n_y))), case
        d = np.diff(ys)
        ws = 0.5 * (np.concatenate([[0.0], d]) + np.concatenate([d, [0.0]]))
        for base in range(0, n_y, 64):
            a = [np.empty(64) for _ in range(4)]
            ylib.ylean_pass(y_lo, y_hi, n_y, base, *[x.ctypes.data_as(DP) for x in a])
            m = min(64, n_y - base)
            assert np.array_equal(bits(a[0][:m]), bits(ys[base:base + m])), (case, base)
            assert np.array_equal(bits(a[1][:m]), bits(ws[base:base + m])), (case, base)
        # the probe window's exact zeros: q >= 0.75 step 1e6 at every other node, and exp_sc clamps q^2/2 >= 1100 to 0
        assert 0.5 * (0.75 * step * 1e6) ** 2 > 1e6, (case, step)


def test_constants_are_the_headers():
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "lzq_physics.h")).read()

    def const(name):
        return eval(re.search(rf"constexpr double {name} = ([^;]+);", src).group(1))
    ph = pkg("physics_host")
    assert (const("kZeta3"), const("kS0M3"), const("kGeVToKg"), const("kMProtonKg")) == \
        (Y.ZETA3, Y.S0_M3, Y.GEV_TO_KG, Y.M_PROTON_KG)
    assert (const("kPi"), const("kMplGeV")) == (ph.PI, ph.M_PL_GEV)


# ---------------------------------------------------------------------------------------------
# (6) the cases
# ---------------------------------------------------------------------------------------------
def test_cases_reach_their_regimes_and_hold_no_undecidable_node():
    nearest = min(case_ref(case)[3].nearest_branch for case in Y.CASES)
    for case in Y.CASES:
        nd = case_ref(case)[3]
        assert not nd.undecided, (case, nd.undecided[:4])
        for s in SIGMAS:
            assert not Y.win_gauss(nd, s).undecided
    for case in Y.MULTI_NY:
        for n_y in Y.NYS_MORE:
            nd = case_ref(case, n_y)[3]
            assert not nd.undecided, (case, n_y, nd.undecided[:4])
            nearest = min(nearest, nd.nearest_branch)
    print(f"nearest node to T = m/3 over all cases: {nearest:.2e} (relative)")
    assert nearest > Y.UNDECIDED

    def of(case):
        c, (y_lo, y_hi, step, ys), F, nd = case_ref(case)
        return c, y_lo, y_hi, ys, F, nd, np.array(nd.zero)

    c, y_lo, y_hi, ys, F, nd, zero = of("shipped")
    assert (y_lo, y_hi) == (-48.0, 50.0) and nd.relativistic.all()
    c, y_lo, y_hi, ys, F, nd, zero = of("clips")
    assert (y_lo, y_hi) == (-80.0, 50.0) and (ys < -50.0).sum() > 100 and (F == 0.0).sum() > 100 and F[0] > 0.0
    assert ys[-1] == 50.0 and not (ys > 50.0).any()             # the `live` rule's edge: y = 50 is live
    c, y_lo, y_hi, ys, F, nd, zero = of("heavy")
    assert not nd.relativistic.any() and nd.X.min() < 6.1 and nd.X.max() > 42.0
    c, y_lo, y_hi, ys, F, nd, zero = of("branch")
    flips = np.nonzero(np.diff(nd.relativistic.astype(int)))[0]
    assert flips.size == 1 and (flips[0] + 1) % 64 not in (0,), "both branches inside one wavefront"
    assert nd.relativistic[flips[0] // 64 * 64:flips[0] // 64 * 64 + 64].sum() not in (0, 64)
    c, y_lo, y_hi, ys, F, nd, zero = of("underflow")
    with mp.workdps(Y.DPS):
        e = [mp.exp(-mp.mpf(x)) for x in nd.X]
        normal = sum(v >= mp.ldexp(1, -1022) for v in e)
        sub = sum(mp.ldexp(1, -1075) <= v < mp.ldexp(1, -1022) for v in e)
        gone = sum(v < mp.ldexp(1, -1075) for v in e)
    assert normal > 64 and sub >= 4 and gone > 64, (normal, sub, gone)
    assert nd.X.min() < 121.0 and nd.X.max() > 848.0
    c, y_lo, y_hi, ys, F, nd, zero = of("dead source")
    assert zero.all()
    c, y_lo, y_hi, ys, F, nd, zero = of("small denom")
    assert not nd.relativistic.any() and nd.denom.min() < 1.2e-3
    c, y_lo, y_hi, ys, F, nd, zero = of("denom floor")
    assert nd.denom[0] == 1e-12 and nd.denom[1] > 1e-4
    c, y_lo, y_hi, ys, F, nd, zero = of("low B")
    assert nd.denom.max() > 100.0 and 0 < nd.relativistic.sum() < nd.n
    c, y_lo, y_hi, ys, F, nd, zero = of("narrow")
    assert abs((ys[1] - ys[0]) - 0.01) < 1e-3 and F[-1] > 0.0
    # the cap of the module docstring, on the amplification-free nodes of every case
    for case in Y.CASES:
        nd = case_ref(case)[3]
        free = nd.relativistic & (nd.denom >= 0.5) & (np.abs(nd.ys) <= 50.0)
        assert max([nd.rel0[j] for j in np.nonzero(free)[0]], default=0.0) <= Y.CAP_U * Y.U


# ---------------------------------------------------------------------------------------------
# (3) the clean model
# ---------------------------------------------------------------------------------------------
def windows(nd):
    return [("W = 1", None, Y.win_one(nd))] + [(f"sigma_y = {s}", s, Y.win_gauss(nd, s)) for s in SIGMAS]


@pytest.mark.parametrize("case", list(Y.CASES))
def test_clean_model_inside_tolerance(case):
    c, grid, F, nd = case_ref(case)
    for name, sigma, win in windows(nd):
        terms, yb = Y.model(c, grid[3], F, sigma)
        worst, ratio, bad = Y.compare_nodes(terms, nd, win)
        ref = Y.sum_ref(nd, win)
        rel, sratio, sbad = Y.compare_sum(yb, ref)
        print(f"{case} [{name}]: nodes worst rel err {worst:.3e}, err/tol {ratio:.3f}; sum rel err {rel:.3e}, "
              f"err/tol {sratio:.3f}")
        assert not bad, (case, name, bad[:4])
        assert sbad is None, (case, name, sbad)
        assert ratio < 1.0 and sratio < 1.0


@pytest.mark.parametrize("case", Y.MULTI_NY)
def test_clean_model_at_the_other_node_counts(case):
    for n_y in Y.NYS_MORE:
        c, grid, F, nd = case_ref(case, n_y)
        win = Y.win_one(nd)
        terms, yb = Y.model(c, grid[3], F)
        worst, ratio, bad = Y.compare_nodes(terms, nd, win)
        rel, sratio, sbad = Y.compare_sum(yb, Y.sum_ref(nd, win))
        print(f"{case} n_y = {n_y}: nodes err/tol {ratio:.3f}; sum rel err {rel:.3e}, err/tol {sratio:.3f}")
        assert not bad and sbad is None and ratio < 1.0 and sratio < 1.0


# ---------------------------------------------------------------------------------------------
# (4) the seeded defects
# ---------------------------------------------------------------------------------------------
# defect -> (case, level, sigma): the level that can see it
SEEN = {"a": ("shipped", "node", None), "b": ("narrow", "sum", None), "c": ("clips", "node", 9.0),
        "d": ("heavy", "node", 9.0), "e": ("heavy", "node", 9.0), "f": ("shipped", "sum", None)}


@pytest.mark.parametrize("defect", sorted(Y.DEFECTS))
def test_defect_rejected(defect):
    case, level, sigma = SEEN[defect]
    c, grid, F, nd = case_ref(case)
    win = Y.win_one(nd) if sigma is None else Y.win_gauss(nd, sigma)
    terms, yb = Y.model(c, grid[3], F, sigma, defect=defect)
    _, ratio, bad = Y.compare_nodes(terms, nd, win)
    _, sratio, sbad = Y.compare_sum(yb, Y.sum_ref(nd, win))
    print(f"defect ({defect}) {Y.DEFECTS[defect]} on '{case}': {len(bad)} of {nd.n} nodes rejected "
          f"(worst err/tol {ratio:.3g}), sum err/tol {sratio:.3g}")
    if level == "node":
        assert bad, f"defect ({defect}) survives at node level"
    else:
        assert sbad is not None, f"defect ({defect}) survives in the sum"
    if defect in ("d", "e"):
        assert all(not nd.relativistic[b[0]] for b in bad) or defect == "e"
    if defect == "c":
        # only per node: under the default window the clipped nodes carry nothing of the sum
        assert all(nd.ys[b[0]] < -50.0 for b in bad) and sbad is None
    if defect in ("b", "f"):
        assert not bad                      # the terms are right: only the sum can see it


# ---------------------------------------------------------------------------------------------
# (5) the node probe's window
# ---------------------------------------------------------------------------------------------
def probe_block(y0, step):
    return {"kind": "plateau", "y0": float(y0), "half_width": step / 4.0, "sigma_lo": 1e-6, "sigma_hi": 1e-6}


@pytest.mark.parametrize("case", list(Y.CASES))
def test_probe_window_is_one_node(case):
    W = pkg("window")
    _, _, step, ys = Y.ygrid(Y.cfg_of(case))
    want = np.zeros(ys.size)
    for j in range(ys.size):
        blk = W.to_window(probe_block(ys[j], step))
        if j == 0:
            W.check(blk)
        _, got = W.eval_host(blk, ys)
        want[j] = 1.0
        assert np.array_equal(bits(got), bits(want)), (case, j)
        want[j] = 0.0
