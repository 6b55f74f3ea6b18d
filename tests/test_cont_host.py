"""The continuum z rule (csrc/lzq_cont.h) on the CPU: its node table, gamma4, the
rule's own error against the true z-integral, and the host build of A/V_cont against the fixture
tests/golden/golden_cont.json (the reference's formula with the z-integral by mpmath.quad; nothing
in it comes from the library).  tests/test_gpu_cont.py holds the device side.

The tolerance is zsum_ref.tol's, derived there; the one new term is the rule error, which this file
measures (test_rule_error) and bounds by the table exponential's own minimax bound, so that the rule
is never the dominant error of a device result.
"""
import math

import mpmath as mp
import numpy as np
import pytest

import zsum_ref as Z
from conftest import BASE_CFG, full_cfg, golden, pkg

Z_MAX = 30.0
KERNEL_FIELDS = ("I_p", "beta_over_H", "T_p_GeV", "v_w", "g_star")
RULE_BOUND = Z.TAB_VARIANTS[Z.DEFAULT_TAB]     # 1.73e-14


class ContGrid:
    """zsum_ref.Grid's duck type on the continuum tables (what f_ref / ref_at / av_ref read)."""

    def __init__(self, z_max):
        self.nz, self.z_max = -1, z_max
        self.z, self.g4, self.om = pkg("_native").cont_tables(z_max)
        with mp.workdps(Z.DPS):
            self.g4_mp = [mp.mpf(float(x)) for x in self.g4]
            self.om_mp = [mp.mpf(float(x)) for x in self.om]
        self.cache = {}


_grids = {}


def cont_grid(z_max=Z_MAX):
    if z_max not in _grids:
        _grids[z_max] = ContGrid(z_max)
    return _grids[z_max]


def gamma4_mp(z):
    """gamma(4, z) at the working precision without the cancellation of fpy:156."""
    if z < 1:
        s, t, j = mp.mpf(0), mp.mpf(1), 0
        while True:
            a = t / (j + 4)
            s += a
            if abs(a) < mp.ldexp(1, -mp.mp.prec - 8) * abs(s):
                return z ** 4 * s
            j += 1
            t = -t * z / j
    return 6 - mp.exp(-z) * (((z + 3) * z + 6) * z + 6)


def F_true(I_p, y, z_max):
    """int_0^z_max z^2 e^-z exp(c gamma4(z)) dz by mpmath.quad (inside a workdps context), the break
    points following the integrand's cut-off z_c = (4/a)^(1/4)."""
    yh = min(max(mp.mpf(y), mp.mpf(-50)), mp.mpf(50))
    a = (mp.mpf(I_p) / 6) * mp.exp(yh)
    zm, zc = mp.mpf(z_max), (4 / a) ** mp.mpf("0.25")
    sc = mp.mpf(1)    # mp.quad stops on an absolute error: the integrand is scaled to an integral of O(1)
    if zc >= zm / 8:
        pts = [0, zm / 32, zm / 16, zm / 8, zm / 4, zm / 2, zm]
    else:
        sc = zc ** 3
        zu = min(zm, 2 * (4 * 2600 / a) ** mp.mpf("0.25"))
        pts = [0] + [zc * f for f in (0.25, 0.5, 0.75, 1, 1.25, 1.5, 2, 2.5, 3, 4, 6, 8) if zc * f < zu] + [zu]
        if zu < zm:
            pts += [t for t in (2 * zu, 4 * zu, 8 * zu, 16 * zu) if t < zm] + [zm]
    val, err = mp.quad(lambda z: z * z * mp.exp(-z - a * gamma4_mp(z)) / sc, pts, error=True, method="gauss-legendre")
    assert err <= mp.mpf(10) ** -22 * val, (y, val, err)
    return val * sc


_rule = {}


def rule_error(n=201):
    """(worst, where): the worst relative error of the 60-digit sum over the table's own doubles
    against the true integral, n y over [-50, 50] for each of two I_p (measured once per n; the GPU
    tests take a coarser ladder, whose worst can only be smaller)."""
    if n not in _rule:
        g = cont_grid()
        worst, at = 0.0, None
        for I_p in (0.05, 1.0):
            for y in np.linspace(-50.0, 50.0, n):
                r = Z.ref_at(g, I_p, float(y))
                with mp.workdps(30):
                    t = F_true(I_p, float(y), Z_MAX)
                    e = float(abs(r.F - t) / t)
                if e > worst:
                    worst, at = e, (I_p, float(y))
        _rule[n] = (worst, at)
    return _rule[n]


def test_table_shape():
    nat = pkg("_native")
    z, g4, om = nat.cont_tables(Z_MAX)
    assert z.size == g4.size == om.size == 520            # 26 panels x 20 Gauss-Legendre points
    assert z[0] > 0.0 and z[-1] < Z_MAX and np.all(np.diff(z) > 0.0)
    assert np.all(om > 0.0) and np.all(np.diff(g4) >= 0.0) and g4[0] > 0.0 and g4[-1] < 6.0
    again = nat.cont_tables(Z_MAX)
    assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip((z, g4, om), again))
    # the device image scales omega by 2^-512 (lzq_exp2.h kOmegaBias): every weight stays a normal double
    assert om.min() * 2.0 ** -512 >= 2.0 ** -1022
    # the dead-lane rule of zsum_dispatch (c2N gamma4 of the first node <= -1077 N octaves) is out of
    # reach of any y <= 50 at I_p <= 6: no lane is ever dead on this table
    assert Z.LOG2E * math.exp(50.0) * g4[0] < Z.DEAD_OCT
    z3, _, _ = nat.cont_tables(3.0)
    assert z3.size == 460 and z3[-1] < 3.0                # 23 panels: the edge 3 * 2^-22 is the first below 1e-6
    # the weights integrate z^2 e^-z: gamma(3, z_max)
    with mp.workdps(30):
        assert abs(sum(mp.mpf(float(x)) for x in om) / mp.gammainc(3, 0, Z_MAX) - 1) < 1e-15


def test_gamma4_accuracy():
    """gamma4_k against mpmath's gamma(4, z_k) of the node's own double: <= 4 ulp (the error enters F
    amplified by S, like an error of c: zsum_ref.K_C counts 7 u for c)."""
    g = cont_grid()
    worst = 0.0
    with mp.workdps(50):
        for zk, gk in zip(g.z, g.g4):
            t = mp.gammainc(4, 0, mp.mpf(float(zk)))
            worst = max(worst, float(abs(mp.mpf(float(gk)) - t) / mp.mpf(math.ulp(float(gk)))))
    print(f"continuum gamma4: worst error {worst:.3f} ulp over {g.z.size} nodes")
    assert worst <= 4.0


def test_rule_error():
    """The rule is never the dominant error: below the table exponential's minimax bound (measured
    1.70e-16, at (I_p, y) = (1.0, 41.5))."""
    worst, at = rule_error()
    print(f"continuum rule error: worst {worst:.3e} at (I_p, y) = {at}, bound {RULE_BOUND:.3e}")
    assert worst < RULE_BOUND


def fixture_items(fx, g):
    """compare()'s rows with the fixture's A/V as the value (Ref and scale from the table's own sum)."""
    kernel = {**full_cfg(BASE_CFG), **fx["kernel"]}
    rows = Z.av_ref(kernel, fx["y"], g)
    with mp.workdps(Z.DPS):
        return [(mp.mpf(s), r, sc) for s, (_, r, sc) in zip(fx["A_over_V_str"], rows)]


def test_host_aov_vs_fixture():
    """lzq_aov_cont_host (libm exp: the poly11 row of zsum_ref.tol, <= 1 ulp) against the fixture, the
    rule error on top; exact +0 for y > 50.  Negative control: the reference grid's own A/V at the same
    y fails the same comparison, at a y where it is 0 and the integral is not."""
    fx = golden("golden_cont.json")["aov"]
    assert fx["z_max"] == Z_MAX and {k: BASE_CFG[k] for k in KERNEL_FIELDS} == fx["kernel"]
    g = cont_grid()
    items = fixture_items(fx, g)
    acc = Z.accumulation([r for _, r, _ in items])
    extra = [rule_error()[0]] * len(items)
    got = pkg("_native").aov_cont_host(fx["kernel"], fx["y"], Z_MAX)
    worst, ratio, bad = Z.compare(got, items, "poly11", acc, extra_rel=extra)
    print(f"host A/V_cont vs fixture: {len(items)} y, accumulation {acc:.2e}, worst rel err {worst:.3e}, "
          f"worst err/tol {ratio:.3f}")
    assert not bad, bad[:4]
    zeros = [(x, math.copysign(1.0, x)) for x, y in zip(got, fx["y"]) if y > 50.0]
    assert len(zeros) == 2 and all(z == (0.0, 1.0) for z in zeros)
    assert got[fx["y"].index(-60.0)] == got[fx["y"].index(-50.0)] > 0.0          # the -50 clip
    # the fixture's doubles are its strings rounded
    assert all(float(s) == v for s, v in zip(fx["A_over_V_str"], fx["A_over_V"]))
    _, _, bad_grid = Z.compare(fx["A_over_V_grid"], items, "poly11", acc, extra_rel=extra)
    flagged = {b[0] for b in bad_grid}
    dark = [y for y, gv, v in zip(fx["y"], fx["A_over_V_grid"], fx["A_over_V"]) if gv == 0.0 and v > 0.0]
    assert len(dark) >= 8 and all(27.0 < y <= 50.0 for y in dark) and set(dark) <= flagged


def test_refusals():
    nat = pkg("_native")
    for bad in (0.0, -1.0, math.inf, math.nan, 1e-60):
        with pytest.raises(nat.LzqError) as e:
            nat.cont_tables(bad)
        assert e.value.code == -1, e.value                                      # LZQ_EINVAL
        with pytest.raises(nat.LzqError):
            nat.aov_cont_host({k: BASE_CFG[k] for k in KERNEL_FIELDS}, [0.0], bad)
    for bad in (0.0, -3.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            nat.cont_z_max(bad)
    with pytest.raises(nat.LzqError):   # every linspace entry point keeps refusing nz < 0
        nat.ztables(-1, Z_MAX)
