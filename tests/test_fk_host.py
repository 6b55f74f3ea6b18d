"""The momentum-averaged LZ probability P-bar on the CPU: the library's host build (lzq_fk_pbar_host,
csrc/lzq_fk.h fk_pbar with libm) against mpmath, its exact results, its refusals, and the class grouping
of fk.py.  No GPU.

The references on the box are mpmath.quad at 40 digits, committed as tests/golden/fk_pbar_box.json
(tools/fk_rule_error.py writes it; eight of them are recomputed here).  Gate: 1e-11 relative, the
project's parity gate for yields (tests/test_gpu_parity.py); measured worst: 3.6e-14 (the print below;
profiles/fk/rule_error.json has the same number).
"""
import math

import mpmath as mp
import numpy as np
import pytest

import fk_ref as R
from conftest import golden, pkg

GATE = 1e-11
TWO_PI = 2.0 * math.pi


def host(block, mu, g, stats=0):
    """P-bar from the host build at g = 2 pi delta_0."""
    return pkg("fk").pbar_host(block, mu, np.asarray(g, dtype=np.float64) / TWO_PI, stats)


def rel(got, ref):
    with mp.workdps(40):
        return float(abs(mp.mpf(float(got)) - ref) / ref)


def test_box_against_mpmath():
    g = golden("fk_pbar_box.json")
    cases = g["cases"]
    # the box: 5 mu x 5 g x (p = 0, and p in {1, 2, 3.5} x 2 v_ref) x 2 statistics
    assert len(cases) == 5 * 5 * (1 + 3 * 2) * 2
    assert {c["mu"] for c in cases} == {0, 0.3, 3, 42, 849} and {c["v_ref"] for c in cases} == {0.1, 1.0}
    assert {c["g"] for c in cases} == {1e-9, 1e-3, 0.1, 1, 10} and {c["p"] for c in cases} == {0, 1, 2, 3.5}
    worst, wc = 0.0, None
    with mp.workdps(g["dps"]):
        for c in cases:
            got = host({"p": c["p"], "v_ref": c["v_ref"]}, c["mu"], c["g"], c["stats"])[0]
            e = rel(got, mp.mpf(c["pbar"]))
            if e > worst:
                worst, wc = e, c
    print(f"P-bar host build vs mpmath.quad on {len(cases)} cases: worst relative error {worst:.3e} at {wc}")
    assert worst <= GATE, (worst, wc)


def test_golden_references_are_mpmath_quad():
    """Eight of the committed references, spread over the box, recomputed."""
    cases = golden("fk_pbar_box.json")["cases"]
    with mp.workdps(40):
        for c in cases[3::len(cases) // 8][:8]:
            ref = R.pbar_quad(c["mu"], c["g"], c["p"], c["v_ref"], c["stats"])
            assert abs(mp.mpf(c["pbar"]) - ref) / ref < mp.mpf(10) ** -25, c


@pytest.mark.parametrize("stats", [0, 1])
def test_p0_is_the_closed_form(stats):
    gs = np.concatenate([np.logspace(-12, 1, 27), [20.0, 37.5, 50.0]])
    worst = 0.0
    for mu in (0.0, 0.3, 3.0, 42.0, 849.0):
        got = host({"p": 0.0}, mu, gs, stats)
        with mp.workdps(40):
            for g, x in zip(gs, got):
                worst = max(worst, rel(x, -mp.expm1(-mp.mpf(float(g)))))
    print(f"p = 0 vs -expm1(-g), stats {stats}: worst relative error {worst:.3e}")
    assert worst <= GATE


@pytest.mark.parametrize("stats", [0, 1])
def test_massless_limit(stats):
    """mu = 0: v = 1 at every t, so P-bar = -expm1(-g v_ref^p)."""
    worst = 0.0
    for p, v_ref in ((1.0, 0.5), (2.0, 0.1), (3.5, 0.7), (8.0, 1.0)):
        gs = np.logspace(-9, 1.5, 12)
        got = host({"p": p, "v_ref": v_ref}, 0.0, gs, stats)
        with mp.workdps(40):
            for g, x in zip(gs, got):
                worst = max(worst, rel(x, -mp.expm1(-mp.mpf(float(g)) * mp.mpf(v_ref) ** mp.mpf(p))))
    print(f"mu = 0 vs -expm1(-g v_ref^p), stats {stats}: worst relative error {worst:.3e}")
    assert worst <= GATE


@pytest.mark.parametrize("stats", [0, 1])
@pytest.mark.parametrize("block", [{"p": 0.0}, {"p": 1.0, "v_ref": 0.1}, {"p": 3.5, "v_ref": 1.0}, {"p": 8.0, "v_ref": 0.5}])
def test_exact_ends(block, stats):
    mus = np.array([0.0, 3.0, 849.0])
    one = pkg("fk").pbar_host(block, mus, np.inf, stats)
    nul = pkg("fk").pbar_host(block, mus, 0.0, stats)
    assert np.array_equal(one.view(np.int64), np.ones(3).view(np.int64))
    assert np.array_equal(nul.view(np.int64), np.zeros(3).view(np.int64))        # +0, not -0


def test_large_mu_anchor():
    """The kinematics, not the rule: at large mu and p = 2, F = v_ref^2 mu / (2 t) (1 + O(t/mu)) under
    the Maxwell-Boltzmann weight t e^-t, so P-bar -> 1 - 2 c K_2(2 sqrt c), c = g v_ref^2 mu / 2.  The
    anchor is only correct to O(1/mu); the tolerance is mpmath.quad's own distance to it, twice."""
    mu, v_ref = 1e4, 0.3
    with mp.workdps(40):
        for g in (1e-5, 1e-3, 0.1):
            c = mp.mpf(g) * mp.mpf(v_ref) ** 2 * mu / 2
            anchor = 1 - 2 * c * mp.besselk(2, 2 * mp.sqrt(c))
            for stats in (0, 1):
                exact = R.pbar_quad(mu, g, 2.0, v_ref, stats)
                tol = 2 * abs(exact - anchor)
                got = host({"p": 2.0, "v_ref": v_ref}, mu, g, stats)[0]
                print(f"anchor g = {g}, stats {stats}: P-bar = {got!r}, anchor {float(anchor)!r}, "
                      f"|quad - anchor| / anchor = {float(abs(exact - anchor) / anchor):.3e}")
                assert abs(mp.mpf(float(got)) - anchor) <= tol
                assert rel(got, exact) <= GATE


REFUSED = [({"kind": 1}, None, "kind"), ({"p": float("nan")}, None, "p ="), ({"p": -0.5}, None, "p ="),
           ({"p": 8.5}, None, "p ="), ({"v_ref": float("nan")}, None, "v_ref"), ({"v_ref": 0.0}, None, "v_ref"),
           ({"v_ref": -1.0}, None, "v_ref"), ({"v_ref": 1.0 + 2 ** -52}, None, "v_ref"),
           ({"p": 1.0}, float("nan"), "delta0"), ({"p": 1.0}, -1e-300, "delta0")]


@pytest.mark.parametrize("block,delta,word", REFUSED)
def test_refusals(block, delta, word):
    fk, nat = pkg("fk"), pkg("_native")
    rec = fk.to_fk(block)
    with pytest.raises(nat.LzqError) as ei:
        fk.check(rec, None if delta is None else [delta])
    assert ei.value.code == -1 and word in str(ei.value)
    with pytest.raises(nat.LzqError) as ei:
        fk.pbar_host(rec, 1.0, 0.1 if delta is None else delta)
    assert ei.value.code == -1 and word in str(ei.value)
    # the accepted neighbours
    fk.check(fk.to_fk({"p": 8.0, "v_ref": 1.0}), [0.0])
    fk.check(fk.to_fk({"p": 0.0, "v_ref": 5e-324}), [math.inf])
    with pytest.raises(nat.LzqError) as ei:
        fk.pbar_host({"p": 1.0}, -1.0, 0.1)
    assert "mu" in str(ei.value)
    with pytest.raises(ValueError):
        fk.to_fk({"kind": "tabulated"})
    with pytest.raises(ValueError):
        fk.to_fk({"q": 1.0})


def test_class_grouping():
    fk, cfgm = pkg("fk"), pkg("config")
    from conftest import BASE_CFG, full_cfg
    base = cfgm.to_point(full_cfg(BASE_CFG))
    n = 12
    pts = np.repeat(base, n)
    delta = np.full(n, 0.02)
    fks = fk.to_fks({"p": 1.0, "v_ref": 0.5}, n)
    # members of the key, one change each (points 1..9); fields outside it (10, 11) do not split
    pts["T_p_GeV"][1] = 101.0
    pts["beta_over_H"][2] = 99.0
    pts["T_min_over_Tp"][3] = 0.002
    pts["T_max_over_Tp"][4] = 4.0
    pts["m_chi_GeV"][5] = 1.0
    pts["stats"][6] = 1
    delta[7] = np.nextafter(0.02, 1.0)
    fks["p"][8] = 2.0
    fks["v_ref"][9] = 0.25
    pts["source_shape_sigma_y"][10] = 3.0
    pts["P_chi_to_B"][11] = 0.5
    rep, cls = fk.class_groups(pts, delta, fks)
    assert rep.dtype == np.int64 and cls.dtype == np.int32
    assert rep.size == 10 and cls[0] == cls[10] == cls[11]
    assert len({int(c) for c in cls[:10]}) == 10
    assert all(cls[int(r)] == k for k, r in enumerate(rep)) and set(rep.tolist()) == set(range(10))
    # delta_0 from P: the inverse of the closed form, 0 and +inf at the ends
    d = fk.delta_from_P(np.array([0.0, 0.14925839040304145, 1.0]))
    assert d[0] == 0.0 and math.isinf(d[2]) and abs(-math.expm1(-TWO_PI * d[1]) - 0.14925839040304145) < 1e-16
    assert np.array_equal(fk.point_delta(pts[:2]), fk.delta_from_P(pts["P_chi_to_B"][:2]))


def test_counted_tolerance_against_the_rule():
    """The host build against the rule's own sums in long double, within the counted tolerance of
    fk_ref.pbar_tol: the count the GPU tests assert is not vacuous on the CPU either."""
    worst = 0.0
    for stats in (0, 1):
        for p, v_ref in ((0.0, 1.0), (1.0, 1.0), (3.5, 0.1)):
            for mu in (0.0, 0.3, 3.0, 849.0):
                for g in (1e-9, 0.1, 10.0):
                    got = host({"p": p, "v_ref": v_ref}, mu, g, stats)[0]
                    ref = R.pbar_rule_ld(mu, g, p, v_ref, stats)[()]
                    tol = R.pbar_tol(mu, g, p, v_ref, stats)
                    assert tol < 1e-12
                    q = float(abs(np.longdouble(got) - ref) / ref) / tol
                    worst = max(worst, q)
    print(f"host build vs the rule in long double: worst error / counted tolerance {worst:.3f}")
    assert worst < 1.0
