"""The z-sum F(c) = sum_k omega_k 2^(c2 gamma4_k) of the A/V kernels, on the CPU: a one-lane host
restatement of lzq::zsum_dispatch (tests/zsum_host.cpp, built on the LZQ_HD functions of
csrc/lzq_exp2.h) against the mpmath reference and the derived tolerance of tests/zsum_ref.py, on
the y sets, grids and variants of tests/test_gpu_zsum.py.  Three things are shown without a GPU:

(a) correct arithmetic stays inside the tolerance, i.e. the reference alone admits it;
(b) the same comparison on the same y sets rejects eight deliberate defects of the model, i.e. a
    kernel that were wrong in one of these ways would fail tests/test_gpu_zsum.py;
(c) in the model, the exact-underflow truncation is bit-identical to the dense sum, and the
    clamp-free instantiation gives the bits of the clamped one for a lane that never clamps.

The model's c2 is ((-(I_p/6) * exp(yh)) * log2(e)) * N with numpy's exp (<= 1 ulp, as the
device's exp_sc): bit-identity of device F with this model is not claimed (zsum_ref.K_C covers it).
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import zsum_ref as Z
from conftest import BASE_CFG, PKG_NAME, ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
I_P = BASE_CFG["I_p"]
VCODE = {"table": 1, "poly11": 0}


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(tempfile.mkdtemp(), "zsum_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "zsum_host.cpp"), "-o", so], check=True)
    L = ctypes.CDLL(so)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    L.zsum_model.argtypes = [ctypes.c_int] * 5 + [dp, dp, ctypes.c_int, dp, ctypes.c_long, dp, ip]
    L.zsum_tab_index.argtypes = [ctypes.c_double, ctypes.c_double]
    L.zsum_consts.argtypes = [dp]
    L.zsum_consts.restype = None
    return L


def model_c2(variant, ys):
    """c2 of the kernels' y loop (lzq_quad.h yb_wave / aov_kernel), numpy's exp for exp_sc."""
    ey = np.exp(np.clip(np.asarray(ys, float), -50.0, 50.0))
    return ((-(I_P / 6.0) * ey) * Z.LOG2E) * (8192.0 if variant == "table" else 1.0)


def model(L, g, variant, ys, mutant=0, mut_index=0, truncate=0, force_clamp=0):
    c2 = np.ascontiguousarray(model_c2(variant, ys))
    F = np.empty_like(c2)
    kend = np.empty(c2.size, np.int32)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    g4, om = np.ascontiguousarray(g.g4), np.ascontiguousarray(g.om)
    rc = L.zsum_model(VCODE[variant], mutant, mut_index, truncate, force_clamp, g4.ctypes.data_as(dp),
                      om.ctypes.data_as(dp), g.nz, c2.ctypes.data_as(dp), c2.size, F.ctypes.data_as(dp),
                      kend.ctypes.data_as(ip))
    assert rc == 0, f"zsum_model: {rc}"
    F[np.asarray(ys, float) > 50.0] = 0.0   # fpy:159, applied by the kernels after the sum
    return F, kend


def case(nz, z_max):
    g = Z.grid(nz, z_max)
    ys = Z.y_set(g, I_P, Z.density_of(nz))
    refs = Z.refs_for(g, I_P, ys)
    items = [(r.F, r, 1 if y <= 50.0 else None) for r, y in zip(refs, ys)]
    return g, ys, refs, items, Z.accumulation(refs)


def test_constants_match_header(lib):
    """The numbers zsum_ref.py restates are the header's."""
    c = (ctypes.c_double * 7)()
    lib.zsum_consts(c)
    assert c[0] == Z.LOG2E and c[1] == 8192.0 and c[2] == -Z.CLAMP_OCT and c[3] == 1.0 and c[5] == Z.DEAD_OCT
    assert [lib.zsum_padded_nodes(n) for n in (2, 5, 8, 13, 1200, 2401)] == [8, 8, 8, 16, 1200, 2408]


@pytest.mark.parametrize("nz,z_max", Z.GRIDS)
def test_model_inside_tolerance(lib, nz, z_max):
    """(a), with (c): dense, truncated and forced-clamp runs of the faithful model."""
    g, ys, refs, items, acc = case(nz, z_max)
    print(f"grid ({nz}, {z_max}): {len(ys)} y, y_clamp/y_sat/y_dead = "
          + "/".join(f"{b:.3f}" for b in g.boundaries(I_P)) + f", measured accumulation error {acc:.2e}")
    for variant in Z.VARIANTS:
        F, kend = model(lib, g, variant, ys)
        worst, ratio, bad = Z.compare(F, items, variant, acc)
        print(f"  {variant}: worst rel err {worst:.3e}, worst err/tol {ratio:.3f}")
        assert not bad, (variant, bad[:4])
        Ft, kt = model(lib, g, variant, ys, truncate=1)
        assert np.array_equal(F.view(np.int64), Ft.view(np.int64)), "truncated sum differs from the dense one"
        assert np.all(kt <= kend) and np.all(kt % 8 == 0)
        assert kt.min() < kend.min() or kend.min() == 8, "the y set never truncates"
        Fc, _ = model(lib, g, variant, ys, force_clamp=1)
        assert np.array_equal(F.view(np.int64), Fc.view(np.int64)), "clamp-free and clamped bits differ"


@pytest.mark.parametrize("nz,z_max", [(1200, 30.0), (13, 3.0)])
def test_model_on_ftable_and_knot_sets(lib, nz, z_max):
    """(a) and (c) on the other two y sets of tests/test_gpu_zsum.py: the compared nodes of the F
    table's y-grid (-80 .. 50), truncation bit-identical over all its 2000 nodes, and the ODE
    tables' knots (default grid)."""
    from conftest import full_cfg
    g = Z.grid(nz, z_max)
    _, _, _, ygrid = Z.ft_ygrid({**full_cfg(BASE_CFG), **Z.FT_WINDOW})
    sets = {"F table": [float(y) for y in ygrid[Z.ft_pick(g, I_P, ygrid)]]}
    if nz == 1200:
        sets["ODE knots"] = [float(y) for y in Z.ode_knot_y({**full_cfg(BASE_CFG), **Z.ODE_WINDOW})[2]]
    for name, ys in sets.items():
        refs = Z.refs_for(g, I_P, ys)
        acc = Z.accumulation(refs)
        for variant in Z.VARIANTS:
            F, _ = model(lib, g, variant, ys)
            worst, ratio, bad = Z.compare(F, Z.f_items(refs), variant, acc)
            print(f"{name} ({nz}, {z_max}) {variant}: {len(ys)} y, accumulation {acc:.2e}, worst rel err {worst:.3e}, "
                  f"worst err/tol {ratio:.3f}")
            assert not bad, (name, variant, bad[:4])
    for variant in Z.VARIANTS:
        F, kend = model(lib, g, variant, ygrid)
        Ft, kt = model(lib, g, variant, ygrid, truncate=1)
        assert np.array_equal(F.view(np.int64), Ft.view(np.int64))
        assert len(set(kt.tolist())) > (8 if nz == 1200 else 1)   # the passes end at many different nodes


def table_mutant_index(lib, g, ys, refs, acc):
    """Mutant 1's table index: the entry read by the node with the largest share of F relative to
    the tolerance there, over the tested y (it must carry more than 1e-3 of F)."""
    import mpmath as mp
    c2 = model_c2("table", ys)
    best = (0.0, None, 0.0)
    with mp.workdps(Z.DPS):
        for y, r, c in zip(ys, refs, c2):
            if y > 50.0 or r.F < mp.ldexp(1, -900):
                continue
            cm = Z.c_of_y(I_P, y)
            k = max(range(1, g.nz), key=lambda k: g.om_mp[k] * mp.exp(cm * g.g4_mp[k]))
            share = float(g.om_mp[k] * mp.exp(cm * g.g4_mp[k]) / r.F)
            score = share / Z.tol("table", r.S, acc, prefactor=False)
            if score > best[0]:
                best = (score, lib.zsum_tab_index(float(c), float(g.g4[k])), share)
    assert best[2] > 1e-3
    return best[1]


MUTANTS = {1: "table entry wrong by 2^-40", 2: "kSqBeta off by 1e-9", 3: "dead threshold at 1000 octaves",
           # 4: the constant 1506 raised to 1570 octaves (T'' * 2^(e+512) leaves the normal range and the
           # exponent insert wraps).  Lowered to 1442 it would clamp more nodes, each still far below
           # 2^-1074 after the accumulate's rounding: the same bits, no defect (lzq_exp2.h's argument)
           4: "clamp constant raised by 64 octaves", 5: "last real node dropped",
           6: "padding nodes carry the last omega", 7: "kend rounded down", 8: "poly11 conversion does not saturate"}
# the grid on which each mutant is shown: the default one, a padded one for the padding mutant
MUTANT_GRID = {m: (13, 3.0) if m == 6 else (1200, 30.0) for m in MUTANTS}
MUTANT_VARIANTS = {1: ("table",), 2: ("table",), 4: ("table",), 8: ("poly11",)}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_rejected(lib, mutant):
    """(b): the comparison of test_model_inside_tolerance, same y set and tolerance, rejects the
    defect in every variant it applies to."""
    g, ys, refs, items, acc = case(*MUTANT_GRID[mutant])
    for variant in MUTANT_VARIANTS.get(mutant, Z.VARIANTS):
        idx = table_mutant_index(lib, g, ys, refs, acc) if mutant == 1 else 0
        F, _ = model(lib, g, variant, ys, mutant=mutant, mut_index=idx, truncate=1 if mutant == 7 else 0)
        worst, ratio, bad = Z.compare(F, items, variant, acc)
        print(f"mutant {mutant} ({MUTANTS[mutant]}), {variant}: {len(bad)} of {len(ys)} y rejected, "
              f"worst err/tol {ratio:.3g}")
        assert bad, f"mutant {mutant} ({MUTANTS[mutant]}) survives on {variant}"
