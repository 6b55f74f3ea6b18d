"""Wash-out and source depletion on the y-grid quadrature, on the CPU (csrc/lzq_wash.h through the
library's host entry points; tests/wash_ref.py): what tests/test_gpu_wash.py relies on, shown without a GPU.

(1) lzq_wash_factor_host against mpmath within the counted tolerance, its exact ends and its refusals;
(2) the numpy restatement of the definition reproduces the reference program's own rtol-1e-12 Radau solves
    (tests/golden/golden_ode.json `tight`) on every sigma_v = 0 case, Y_B and Y_chi, and the two window
    refusals give the fast path's exact 0.0;
(3) four seeded defects of the restatement are rejected by that comparison;
(4) lzq_solve_check_host_wash: every new refusal, and lzq_solve_check_host's list without a base block.
"""
import ctypes
import json
import math

import numpy as np
import pytest

import wash_ref as WR
import yquad_ref as Y
from conftest import BASE_CFG, full_cfg, golden, pkg

GAMMAS = (0.0, 1e-12, 0.3, 5.0, 50.0, 800.0)
# (name, config overrides, y): T(y) / T_lo of the case
RATIOS = {
    "1": (dict(T_min_over_Tp=1.0), 0.0),
    "1 + 2^-52": (dict(T_min_over_Tp=1.0 - 2.0 ** -53), 0.0),
    "1.6 / 0.6": (dict(T_max_over_Tp=1.6, T_min_over_Tp=0.6), "y_lo"),
    "5000": (dict(T_max_over_Tp=5.0, T_min_over_Tp=1e-3), "y_lo"),
    "1e30 / 1e-30 (the clamp)": (dict(T_p_GeV=1e30, T_min_over_Tp=0.0), 0.0),
}
# The worst relative distance between the restatement and `tight` over the golden cases, Y_B and Y_chi,
# as test_restatement_against_golden measured it (printed there); the assertion is 3 x it: a distance
# between two discretisations (8000 trapezoid nodes in y against the 800-knot spline of A/V in T) that
# moves with the window, not a rounding count.  It moves by four orders with main()'s window [0.001, 5] T_p
# (case 21), whose knots are 0.625 GeV apart where A/V changes over 1 GeV: a Gauss-Legendre quadrature of
# the reference's own spline reproduces that case's `tight` to 8e-14, so the distance is the spline's.
# (test_wide_window_distance_is_the_splines below repeats that check.)  That case therefore has its own
# measurement, and the windows of at most 2 T_p keep theirs.
MEASURED_DISTANCE = 1.09e-8          # windows up to [0.4, 2.0] T_p: cases 0-4, 12-18
MEASURED_DISTANCE_WIDE = 1.65e-4     # main()'s window [0.001, 5] T_p: case 21


def measured_for(c):
    return MEASURED_DISTANCE_WIDE if c["T_max_over_Tp"] - c["T_min_over_Tp"] > 2.0 else MEASURED_DISTANCE


def bound_for(c):
    return 3.0 * measured_for(c)


def point_of(c):
    return pkg("config").to_point(c)


def case_y(c, y):
    return Y.ygrid(c, 2000)[0] if y == "y_lo" else float(y)


@pytest.mark.parametrize("ratio", list(RATIOS))
def test_factor_against_mp(ratio):
    W = pkg("wash")
    over, y = RATIOS[ratio]
    c = full_cfg({**BASE_CFG, **over})
    y = case_y(c, y)
    T, T_lo = float(WR.T_of_y(c, [y])[0]), WR.T_lo_of(c)
    if ratio == "1":
        assert T / T_lo == 1.0
    if ratio == "1 + 2^-52":
        assert T / T_lo == 1.0 + 2.0 ** -52
    if ratio.startswith("1e30"):
        assert T_lo == 1e-30 and T == 1e30
    worst = 0.0
    for g in GAMMAS:
        got = W.factor_host(point_of(c), {"Gamma_wash_over_H": g}, [y])[0]
        bad = WR.check_factor(got, g, T, T_lo)
        assert bad is None, (ratio, bad)
        w, L = WR.omega_mp(g, T, T_lo)
        if g > 0 and float(w) > 2.0 ** -1000:
            worst = max(worst, abs(got - float(w)) / float(w) / WR.count(g, L))
        if ratio == "1":
            assert got == 1.0                      # log 1 = 0 and exp(-0) = 1 exactly
    print(f"omega [T/T_lo = {ratio}]: worst error / count {worst:.3f}")
    # the clamp case leaves the double range: exactly +0 from Gamma = 50 on, the subnormal band between
    if ratio.startswith("1e30"):
        for g in (50.0, 800.0):
            z = W.factor_host(point_of(c), {"Gamma_wash_over_H": g}, [y])[0]
            assert z == 0.0 and math.copysign(1.0, z) > 0
        g_sub = 740.0 / math.log(1e60)             # omega ~ e^-740: a subnormal
        z = W.factor_host(point_of(c), {"Gamma_wash_over_H": g_sub}, [y])[0]
        assert 0.0 < z < 2.0 ** -1022 and WR.check_factor(z, g_sub, T, T_lo) is None


def test_factor_identities_and_refusals():
    W, nat = pkg("wash"), pkg("_native")
    c = full_cfg(BASE_CFG)
    ys = Y.ygrid(c, 2000)[3][::97]
    for g in (0.0, -1.0, -0.0):
        out = W.factor_host(point_of(c), {"Gamma_wash_over_H": g, "deplete_DM_from_source": True}, ys)
        assert np.all(out == 1.0)
    for block, field, code in (({"Gamma_wash_over_H": math.nan}, "Gamma_wash_over_H", -1),
                               ({"sigma_v_chi_GeV_m2": math.nan}, "sigma_v_chi_GeV_m2", -1),
                               ({"sigma_v_chi_GeV_m2": 1e-20}, "sigma_v_chi_GeV_m2", -3)):
        with pytest.raises(ValueError, match=field):
            W.check(W.to_wash(block))
        with pytest.raises(nat.LzqError, match=field) as e:
            W.factor_host(point_of(c), block, ys)
        assert e.value.code == code                # LZQ_EINVAL for a NaN, LZQ_EUNSUPPORTED for sigma_v > 0
    # sigma_v <= 0 is 0 after the max of fpy:279
    W.check(W.to_wash({"sigma_v_chi_GeV_m2": -1e-12, "Gamma_wash_over_H": -1.0}))
    with pytest.raises(ValueError, match="unknown field"):
        W.to_wash({"Gamma": 1.0})


# ---------------------------------------------------------------------------------------------
# (2), (3) the restatement against the reference program's tight solves
# ---------------------------------------------------------------------------------------------
def golden_cases():
    """(index, config, tight or None) of every golden case whose sigma_v is 0 after the max."""
    out = []
    for i, p in enumerate(golden("golden_ode.json")["points"]):
        c = full_cfg(p["config"])
        if max(c["sigma_v_chi_GeV_m2"], 0.0) == 0.0:
            out.append((i, c, p.get("tight")))
    return out


_terms = {}


def distances(defect=None):
    """[(index, field, relative distance, its bound)] of the restatement from `tight`, plus -- the golden file has
    no sigma_v = 0 case with depletion AND Gamma > 0 -- the depleting case 3 at Gamma = 5, whose Y_chi is
    case 3's own: fpy:283 reads neither Y_B nor Gamma."""
    rows = []
    for i, c, tight in golden_cases():
        if tight is None:
            continue
        YB, Ychi, _terms[i] = WR.restate(c, defect=defect, terms=_terms.get(i))
        rows.append((i, "Y_B", abs(YB - tight["Y_B"]) / abs(tight["Y_B"]), bound_for(c)))
        rows.append((i, "Y_chi", abs(Ychi - tight["Y_chi"]) / abs(tight["Y_chi"]), bound_for(c)))
        if c["deplete_DM_from_source"] and c["Gamma_wash_over_H"] == 0.0 and c["incident_flux_scale"] < 1e-6:
            _, Ychi5, _ = WR.restate(dict(c, Gamma_wash_over_H=5.0), defect=defect, terms=_terms[i])
            rows.append((i, "Y_chi at Gamma = 5", abs(Ychi5 - tight["Y_chi"]) / abs(tight["Y_chi"]), bound_for(c)))
    return rows


def test_restatement_against_golden():
    cases = golden_cases()
    assert len([1 for _, _, t in cases if t is not None]) == 13
    rows = distances()
    for i, field, d, b in rows:
        print(f"golden case {i:2d} {field:18s} distance {d:.3e} (bound {b:.3e})")
        assert d <= b, (i, field)
    for meas in (MEASURED_DISTANCE, MEASURED_DISTANCE_WIDE):
        worst = max(d for _, _, d, b in rows if b == 3.0 * meas)
        print(f"worst distance {worst:.3e} (measured constant {meas:.3e})")
        assert 0.9 * meas <= worst <= 1.1 * meas   # the constant is the measurement, not a loose cap
    # a negative Y_chi is the reference's answer too (flux = 1e-3): nothing is clamped
    neg = [c for _, c, t in cases if t is not None and t["Y_chi"] < 0]
    assert len(neg) == 1 and neg[0]["incident_flux_scale"] == 1e-3 and WR.restate(neg[0])[1] < 0
    # the zero-width and the inverted window: the fast path's exact 0.0
    refused = [c for _, c, t in cases if t is None]
    assert len(refused) == 2
    for c in refused:
        YB, Ychi, _ = WR.restate(c)
        assert YB == 0.0 and math.copysign(1.0, YB) > 0 and Ychi == c["Y_chi_init"]


def spline_quadrature(c):
    """Y_B of the reference's own linear system with ITS discretisation of A/V -- CubicSpline through
    max(A/V, 0) at linspace(T_lo, T_hi, 800) (fpy:208-212), A/V restated from the library's host z tables
    -- integrated in T by 16 x 20-point Gauss-Legendre per knot interval: Y_B = int S_B / (s H T)
    (T_lo / T)^Gamma dT, the closed form of fpy:285 for sigma_v = 0."""
    from scipy.interpolate import CubicSpline
    ph = pkg("physics_host")
    Tp, B = c["T_p_GeV"], c["beta_over_H"]
    T_lo, T_hi = c["T_min_over_Tp"] * Tp, c["T_max_over_Tp"] * Tp
    Ts = np.linspace(T_lo, T_hi, 800)
    yk = np.array([ph.y_of_T(T, Tp, B) for T in Ts])
    pref0 = (c["I_p"] / 2.0) * ((B * ph.H_std(Tp, c["g_star"])) / max(c["v_w"], 1e-12))
    Av = np.where(yk > 50.0, 0.0, pref0 * np.exp(np.clip(yk, -50.0, 50.0)) * Y.host_F(c, yk, 1200, 30.0))
    sp = CubicSpline(Ts, np.maximum(Av, 0.0), extrapolate=True)
    xg, wg = np.polynomial.legendre.leggauss(20)
    G = max(c["Gamma_wash_over_H"], 0.0)
    edges = np.concatenate([np.linspace(a, b, 17)[:-1] for a, b in zip(Ts[:-1], Ts[1:])] + [Ts[-1:]])
    h = 0.5 * np.diff(edges)[:, None]
    T = h * xg[None, :] + 0.5 * (edges[:-1] + edges[1:])[:, None]
    y = (Tp * Tp / (T * T) - 1.0) * B / 2.0
    win = np.exp(-0.5 * (y / max(c["source_shape_sigma_y"], 1e-6)) ** 2)
    m, g = c["m_chi_GeV"], c["g_chi"]
    with np.errstate(under="ignore"):                      # fpy:90-120, both branches (fermion)
        n_eq = np.where(T > m / 3.0, g * (3.0 * Y.ZETA3 / (4.0 * math.pi ** 2)) * T ** 3,
                        g * (m / (2.0 * math.pi)) ** 1.5 * T ** 1.5 * np.exp(-m / T))
        vbar = np.where(T > m / 3.0, 1.0, np.sqrt(8.0 * T / (math.pi * m)))
    J = c["incident_flux_scale"] * 0.25 * n_eq * vbar
    s = (2.0 * math.pi ** 2 / 45.0) * c["g_star_s"] * T ** 3
    H = 1.66 * math.sqrt(c["g_star"]) * T * T / ph.M_PL_GEV
    f = c["P_chi_to_B"] * J * sp(T) * win / (s * H * T) * (T_lo / T) ** G
    return float(np.sum(h * wg[None, :] * f))


def test_wide_window_distance_is_the_splines():
    """Case 21 (main()'s window, Gamma = 1) lies 1.65e-4 from the y-grid restatement.  Integrating the
    reference's own 800-knot spline of A/V by a converged quadrature reproduces its `tight` Y_B to a few
    1e-13 (and case 17's and case 0's likewise), so `tight` is converged FOR THE SPLINE and the distance is
    between the spline (knots 0.625 GeV apart where A/V changes over ~1 GeV) and the y-grid."""
    pts = golden("golden_ode.json")["points"]
    for i in (21, 17, 0):
        c, tight = full_cfg(pts[i]["config"]), pts[i]["tight"]["Y_B"]
        got = spline_quadrature(c)
        d_spline, d_grid = abs(got - tight) / tight, abs(WR.restate(c, terms=_terms.get(i))[0] - tight) / tight
        print(f"golden case {i}: spline quadrature {d_spline:.2e} from `tight`, y-grid restatement {d_grid:.2e}")
        assert d_spline <= 1e-12
        assert d_grid >= 100.0 * d_spline


@pytest.mark.parametrize("defect", list(WR.DEFECTS))
def test_seeded_defects_fail(defect):
    rows = distances(defect)
    failed = [(i, field, d) for i, field, d, b in rows if not d <= b]
    print(f"defect {defect} ({WR.DEFECTS[defect]}): {len(failed)} of {len(rows)} comparisons fail, e.g. {failed[:2]}")
    assert failed


# ---------------------------------------------------------------------------------------------
# (4) the solve's host-side refusals
# ---------------------------------------------------------------------------------------------
def solve_rc(field, axes=(), lo=0.0, hi=1.0, wash=None, window=False, **kw):
    nat, S, W = pkg("_native"), pkg("solve"), pkg("wash")
    L = nat.load()
    sv = S.to_ctypes(dict({"field": field, "lo": lo, "hi": hi}, **kw))
    arr = (nat.LzqAxis * max(1, len(axes)))()
    for a, name in enumerate(axes):
        arr[a].field, arr[a].n, arr[a].values = W.field_code(name), 1, None
    win = nat.LzqWindow() if window else None
    ob = W.to_ctypes(W.to_wash(wash)) if wash is not None else None
    rc = L.lzq_solve_check_host_wash(ctypes.byref(sv), ctypes.byref(win) if window else None,
                                     ctypes.byref(ob) if ob is not None else None, arr, len(axes))
    return rc, (L.lzq_last_error() or b"").decode()


def test_solve_check_wash_twin():
    dep = {"deplete_DM_from_source": True}
    assert solve_rc("Gamma_wash_over_H", wash=dep)[0] == 0
    assert solve_rc("Gamma_wash_over_H", axes=("delta_LZ", "deplete_DM_from_source", "I_p"), wash=dep)[0] == 0
    # the new refusals
    rc, msg = solve_rc("Gamma_wash_over_H", axes=("delta_LZ", "Gamma_wash_over_H"), wash=dep)
    assert rc == -1 and "axis 1 writes the solve field" in msg
    rc, msg = solve_rc("Gamma_wash_over_H", lo=-0.5, wash=dep)
    assert rc == -1 and "lo = -0.5 < 0" in msg
    rc, msg = solve_rc("Gamma_wash_over_H", wash={"sigma_v_chi_GeV_m2": 1e-20})
    assert rc == -3 and "sigma_v_chi_GeV_m2" in msg
    rc, msg = solve_rc("P_chi_to_B", wash={"sigma_v_chi_GeV_m2": 1e-20})
    assert rc == -3 and "sigma_v_chi_GeV_m2" in msg
    rc, msg = solve_rc("Gamma_wash_over_H", wash={"Gamma_wash_over_H": math.nan})
    assert rc == -1 and "Gamma_wash_over_H is NaN" in msg
    rc, msg = solve_rc("deplete_DM_from_source", wash=dep)
    assert rc == -1 and "not a solve field" in msg
    # the generic ones hold for the new field
    assert "lo < hi" in solve_rc("Gamma_wash_over_H", lo=1.0, hi=1.0, wash=dep)[1]
    assert "xtol" in solve_rc("Gamma_wash_over_H", wash=dep, xtol=1.0)[1]
    assert "must be finite" in solve_rc("Gamma_wash_over_H", hi=math.inf, wash=dep)[1]
    # every field allowed today stays allowed next to wash axes, every refusal of today stays one
    assert solve_rc("P_chi_to_B", axes=("Gamma_wash_over_H", "deplete_DM_from_source"), wash=dep)[0] == 0
    assert solve_rc("window_sigma", axes=("Gamma_wash_over_H",), wash=dep, window=True)[0] == 0
    assert "changes the z-sum tables" in solve_rc("I_p", axes=("Gamma_wash_over_H",), wash=dep)[1]
    assert "writes the solve field" in solve_rc("P_chi_to_B", axes=("Gamma_wash_over_H", "P_chi_to_B"), wash=dep)[1]
    # without a base block: lzq_solve_check_host, whose allowed list is unchanged
    rc, msg = solve_rc("Gamma_wash_over_H")
    assert rc == -1 and "unknown solve field 96" in msg
    assert solve_rc("P_chi_to_B")[0] == 0
    # (lzq_solve_check_host reads an axis only to see whether it writes the solve field: an axis field it
    # does not know is the launch's to refuse, tests/test_gpu_wash.py test_wash_axis_refused_elsewhere)
    assert solve_rc("P_chi_to_B", axes=("Gamma_wash_over_H",))[0] == 0
    S = pkg("solve")
    with pytest.raises(ValueError, match="needs the wash-out quadrature"):
        S.check({"field": "Gamma_wash_over_H", "lo": 0.0, "hi": 1.0}, [])
    S.check({"field": "Gamma_wash_over_H", "lo": 0.0, "hi": 1.0}, ["delta_LZ"], wash=dep)
    with pytest.raises(ValueError, match="lo = -1 < 0"):
        S.check({"field": "Gamma_wash_over_H", "lo": -1.0, "hi": 1.0}, [], wash=dep)


# ---------------------------------------------------------------------------------------------
# (5) the sweep spec's "wash_rule"
# ---------------------------------------------------------------------------------------------
AXES = [{"field": "delta_LZ", "values": [0.02, 0.05, 0.1]}, {"field": "Gamma_wash_over_H", "values": [0.0, 0.5, 2.0]}]
DEPLETING = {"deplete_DM_from_source": True}


def test_wash_rule_spec_section():
    sw = pkg("sweep")
    plain = sw.spec_from_json({"name": "s", "axes": AXES, "base": DEPLETING})
    spec = sw.spec_from_json({"name": "s", "axes": AXES, "base": DEPLETING, "wash_rule": "quadrature"})
    # absent: today's ODE routing and today's checkpoint key (the section is not written)
    assert plain.wash_rule == "ode" and "wash_rule" not in plain.to_json() and sw.is_ode_spec(plain)
    assert not sw.uses_wash(plain)
    assert spec.to_json()["wash_rule"] == "quadrature" and not sw.is_ode_spec(spec) and sw.uses_wash(spec)
    assert sw.spec_from_json(json.loads(json.dumps(spec.to_json()))).to_json() == spec.to_json()
    assert sw.spec_key(plain) != sw.spec_key(spec)
    assert sw.wash_block(spec) == {"sigma_v_chi_GeV_m2": 0.0, "Gamma_wash_over_H": 0.0, "deplete_DM_from_source": True}
    # window, solve and the continuum rule are then allowed; without the rule they stay refused
    more = {"window": {"kind": "plateau", "half_width": 3.0}, "z_rule": "continuum",
            "solve": {"field": "Gamma_wash_over_H", "lo": 0.0, "hi": 5.0}}
    full = sw.spec_from_json({"name": "s", "axes": AXES[:1], "base": DEPLETING, "wash_rule": "quadrature", **more})
    assert full.solve["field"] == "Gamma_wash_over_H" and full.continuum and sw.uses_wash(full)
    for k, v in more.items():
        with pytest.raises(ValueError):
            sw.spec_from_json({"name": "s", "axes": AXES[:1], "base": DEPLETING, k: v})
    # a spec without wash-out or depletion keeps its routes under the rule
    assert not sw.uses_wash(sw.spec_from_json({"name": "s", "axes": AXES[:1], "wash_rule": "quadrature"}))
    # the CLI form of the solve
    assert pkg("solve").parse_cli("Gamma_wash_over_H:0:5:DM_over_B=5.357")["field"] == "Gamma_wash_over_H"


@pytest.mark.parametrize("extra,msg", [
    ({"base": {"sigma_v_chi_GeV_m2": 1e-20}}, "sigma_v_chi_GeV_m2 != 0"),
    ({"base": {"sigma_v_chi_GeV_m2": -1e-20}}, "sigma_v_chi_GeV_m2 != 0"),
    ({"axes": AXES + [{"field": "sigma_v_chi_GeV_m2", "values": [0.0, 1e-30]}]}, "sigma_v_chi_GeV_m2 axis"),
    ({"axes": AXES + [{"field": "sigma_v_chi_GeV_m2", "values": [0.0]}]}, "drop it"),
    ({"axes": [{"field": "Gamma_wash_over_H", "values": [0.0, float("nan")]}]}, "Gamma_wash_over_H is NaN"),
    ({"fk": {"kind": "power", "p": 1.0}}, "momentum kernel together with wash-out"),
    ({"wash_rule": "spline"}, "wash_rule must be"),
    ({"solve": {"field": "Gamma_wash_over_H", "lo": 0.0, "hi": 5.0}}, "writes the solve field"),
    ({"axes": AXES[:1], "solve": {"field": "Gamma_wash_over_H", "lo": -1.0, "hi": 5.0}}, "lo = -1 < 0"),
])
def test_wash_rule_refusals_say_why(extra, msg):
    sw = pkg("sweep")
    d = dict({"name": "s", "axes": AXES, "base": DEPLETING, "wash_rule": "quadrature"}, **extra)
    with pytest.raises(ValueError, match=msg):
        sw.spec_from_json(d)
