"""The per-point root solve, host side (no GPU).

tests/solve_host.cpp compiles the stepping rule of csrc/lzq_solve.h -- the LZQ_HD functions the GPU
kernel itself calls, -ffp-contract=off -- and drives it through a callback exactly as the kernel
does.  Checked here: known roots of analytic functions, the bracket's sign invariant and the halving
of its width evaluation by evaluation, the evaluation bound, every end state (roots at the ends, no
bracket, non-finite values, max_evals, xtol = 0), the rule on the CPU oracle against the reference's
own roots (tests/golden/golden_solve.json, made by scipy's brentq on the reference), the refusals of
lzq_solve_check_host with their messages, and the solve spec's mapping / CLI forms.
"""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT, full_cfg, golden, pkg

HERE = os.path.dirname(os.path.abspath(__file__))
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
FIELD_FN = ctypes.CFUNCTYPE(ctypes.c_double, ctypes.c_double)
OK, MAX_EVALS, NO_BRACKET, NAN = 0, 1, 2, 3
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(tempfile.mkdtemp(), "solve_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "solve_host.cpp"), "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.solve_run.argtypes = [FIELD_FN, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                            DP, DP, IP, IP]
    return L


class Run:
    def __init__(self, L, fn, lo, hi, target=0.0, xtol=1e-12, max_evals=64):
        res, trace = np.full(6, np.nan), np.full((256, 6), np.nan)
        masks, slot = np.zeros(256, np.int32), ctypes.c_int(-2)
        self.calls = []

        def field(x):
            self.calls.append(x)
            return float(fn(x))

        n = L.solve_run(FIELD_FN(field), lo, hi, target, xtol, max_evals, res.ctypes.data_as(DP),
                        trace.ctypes.data_as(DP), masks.ctypes.data_as(IP), ctypes.byref(slot))
        self.n, self.trace, self.masks, self.slot = n, trace[:n], masks[:n], slot.value
        self.x, self.x_lo, self.x_hi, self.residual = res[:4]
        self.evals, self.status = int(res[4]), int(res[5])
        self.lo, self.hi, self.target, self.fn = lo, hi, target, fn
        assert self.evals == n == len(self.calls)

    def check_invariants(self):
        """What must hold for every solve that found a bracket."""
        t = self.trace
        assert self.status in (OK, MAX_EVALS)
        assert self.x_lo <= self.x <= self.x_hi and self.lo <= self.x_lo and self.x_hi <= self.hi
        # the evaluations are what the trace says, and the trace's f is field(x) - target
        assert np.array_equal(t[:, 0], np.array(self.calls))
        for x, f in t[:, :2]:
            assert f == self.fn(x) - self.target
        # from the second evaluation on: the ends carry f of opposite strict signs (or an exact zero
        # closed the bracket), the bracket is nested, each x was strictly inside the one before
        for k in range(1, self.n):
            a, b, fa, fb = t[k, 2:6]
            if a == b:
                assert fa == 0.0 == fb and k == self.n - 1
                continue
            assert a < b and fa * fb < 0.0 and (fa < 0.0) != (fb < 0.0), k
            if k >= 2:
                pa, pb = t[k - 1, 2:4]
                assert pa <= a and b <= pb and pa < t[k, 0] < pb, k
        # the width at least halves over any three evaluations after the first two (the midpoint's
        # own rounding: one ulp of the larger end)
        w = t[1:, 3] - t[1:, 2]
        for k in range(len(w) - 3):
            slack = 4 * EPS * max(abs(t[k + 1, 2]), abs(t[k + 1, 3]))
            assert w[k + 3] <= 0.5 * w[k] + slack, (k, w[k], w[k + 3])
        # x is the end with the smaller |f| (ties: the lower), the residual is f evaluated there
        a, b, fa, fb = t[-1, 2:6]
        assert (self.x_lo, self.x_hi) == (a, b)
        upper = abs(fb) < abs(fa)
        assert self.x == (b if upper else a) and self.residual == (fb if upper else fa)
        assert self.residual == self.fn(self.x) - self.target
        assert self.slot == (1 if upper else 0)
        # the record slot of x was written by the evaluation AT x (the last one that wrote that slot)
        last = max(k for k in range(self.n) if self.masks[k] & (1 << self.slot))
        assert t[last, 0] == self.x

    def check_converged(self, xtol):
        assert self.status == OK
        a, b = self.x_lo, self.x_hi
        adjacent = a == b or np.nextafter(a, b) == b
        assert (b - a) <= xtol * max(abs(a), abs(b)) or adjacent


ANALYTIC = [
    # (name, f, lo, hi, root)
    ("linear_inc", lambda x: 3.0 * x - 2.0, -1.0, 5.0, 2.0 / 3.0),
    ("linear_dec", lambda x: 7.0 - 2.0 * x, 0.0, 10.0, 3.5),
    ("cubic", lambda x: (x - 1.0) * (x * x + x + 2.0), -3.0, 4.0, 1.0),
    ("cubic_flat", lambda x: (x - 0.5) ** 3, -2.0, 3.0, 0.5),
    ("exp_dec", lambda x: math.exp(-x) - 0.2, 0.0, 30.0, -math.log(0.2)),
    ("exp_inc", lambda x: 0.2 - math.exp(-x), 0.0, 30.0, -math.log(0.2)),
    ("recip_dec", lambda x: 1.0 / x - 4.0, 1e-3, 1e3, 0.25),
    ("recip_inc", lambda x: 4.0 - 1.0 / x, 1e-3, 1e3, 0.25),
    ("log_wide", lambda x: math.log(x) - 3.0, 1e-6, 1e9, math.exp(3.0)),
]


@pytest.mark.parametrize("name,f,lo,hi,root", ANALYTIC, ids=[c[0] for c in ANALYTIC])
def test_analytic_roots(lib, name, f, lo, hi, root):
    for xtol in (1e-6, 1e-12):
        r = Run(lib, f, lo, hi, xtol=xtol)
        r.check_invariants()
        r.check_converged(xtol)
        # the bracket holds the true root up to f's own rounding near it, and is xtol wide
        tol = xtol * max(abs(r.x_lo), abs(r.x_hi)) + (1e-5 if name == "cubic_flat" else 64 * EPS * abs(root))
        assert abs(r.x - root) <= tol, (name, r.x, root)
        bound = 2 + 3 * math.ceil(math.log2((hi - lo) / (xtol * abs(r.x)))) + 3
        assert r.evals <= min(bound, 64)


def test_target_is_subtracted_once(lib):
    r = Run(lib, lambda x: x * x, 0.0, 10.0, target=2.0)
    r.check_invariants()
    assert abs(r.x - math.sqrt(2.0)) <= 2e-12


def test_step_function_closes_to_adjacent_doubles(lib):
    s = 0.3141592653589793
    r = Run(lib, lambda x: -1.0 if x < s else 2.0, 0.0, 1.0, xtol=0.0, max_evals=256)
    r.check_invariants()
    assert r.status == OK and np.nextafter(r.x_lo, 1.0) == r.x_hi
    assert r.x_lo < s <= r.x_hi and r.x == r.x_lo and r.residual == -1.0
    # bisection-like: about three evaluations per halving at worst
    assert r.evals <= 2 + 3 * 62


def test_steep_exponential_stays_within_the_halving_bound(lib):
    f = lambda x: math.exp(50.0 * x) - 1e10  # noqa: E731
    xtol = 1e-12
    r = Run(lib, f, 0.0, 1.0, xtol=xtol, max_evals=256)
    r.check_invariants()
    r.check_converged(xtol)
    root = math.log(1e10) / 50.0
    assert abs(r.x - root) <= 2 * xtol
    assert r.evals <= 2 + 3 * math.ceil(math.log2((1.0 - 0.0) / (xtol * abs(r.x))))


def test_root_exactly_at_an_end(lib):
    r = Run(lib, lambda x: x - 2.0, 2.0, 5.0)
    assert (r.status, r.evals, r.x, r.x_lo, r.x_hi, r.residual, r.slot) == (OK, 1, 2.0, 2.0, 2.0, 0.0, 0)
    assert r.masks[0] == 3
    r = Run(lib, lambda x: x - 5.0, 2.0, 5.0)
    assert (r.status, r.evals, r.x, r.x_lo, r.x_hi, r.residual) == (OK, 2, 5.0, 5.0, 5.0, 0.0)
    assert r.masks[1] & (1 << r.slot)


def test_exact_zero_inside_closes_the_bracket(lib):
    r = Run(lib, lambda x: x - 3.0, 1.0, 5.0)   # the first secant point of a straight line
    assert r.status == OK and r.x == 3.0 == r.x_lo == r.x_hi and r.residual == 0.0 and r.evals == 3
    assert r.masks[2] == 3


def test_no_bracket_is_detected_after_two(lib):
    for f in (lambda x: x * x + 1.0, lambda x: -1.0 - x):
        r = Run(lib, f, 1.0, 5.0)
        assert (r.status, r.evals, r.slot) == (NO_BRACKET, 2, -1)
        assert math.isnan(r.x) and math.isnan(r.residual) and (r.x_lo, r.x_hi) == (1.0, 5.0)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_values(lib, bad):
    r = Run(lib, lambda x: bad if x == 1.0 else x - 3.5, 1.0, 5.0)       # at lo: one evaluation
    assert (r.status, r.evals, r.slot) == (NAN, 1, -1) and math.isnan(r.x) and (r.x_lo, r.x_hi) == (1.0, 5.0)
    r = Run(lib, lambda x: bad if x == 5.0 else x - 3.5, 1.0, 5.0)       # at hi: two
    assert (r.status, r.evals) == (NAN, 2) and math.isnan(r.x) and math.isnan(r.residual)
    r = Run(lib, lambda x: x ** 3 - 20.0 if x in (1.0, 5.0) else bad, 1.0, 5.0)   # inside
    assert (r.status, r.evals) == (NAN, 3) and math.isnan(r.x) and (r.x_lo, r.x_hi) == (1.0, 5.0)


def test_max_evals_keeps_a_valid_bracket(lib):
    f = lambda x: math.exp(-x) - 0.2  # noqa: E731
    for m, want in ((2, 2), (3, 3), (1, 2), (-5, 2), (7, 7)):
        r = Run(lib, f, 0.0, 30.0, max_evals=m)
        assert (r.status, r.evals) == (MAX_EVALS, want)
        r.check_invariants()
        assert r.x_lo < -math.log(0.2) < r.x_hi
    assert lib.solve_clamp(1000) == 256 and lib.solve_clamp(0) == 2 and lib.solve_clamp(64) == 64
    r = Run(lib, lambda x: -1.0 if x < 0.7 else 1.0, 0.0, 1.0, xtol=0.0, max_evals=100000)
    assert r.evals <= 256


def test_xtol_zero_runs_to_adjacent_doubles(lib):
    r = Run(lib, lambda x: math.exp(-x) - 0.2, 0.0, 30.0, xtol=0.0, max_evals=256)
    r.check_invariants()
    assert r.status == OK and (r.x_lo == r.x_hi or np.nextafter(r.x_lo, np.inf) == r.x_hi)


def test_result_is_a_pure_function_of_its_inputs(lib):
    f = lambda x: 1.0 / x - 4.0  # noqa: E731
    a, b = Run(lib, f, 1e-3, 1e3), Run(lib, f, 1e-3, 1e3)
    assert a.trace.tobytes() == b.trace.tobytes() and (a.x, a.evals) == (b.x, b.evals)


# ---- the rule on the CPU oracle against the reference's roots -----------------------------------
def _cases():
    return golden("golden_solve.json")["cases"]


def root_tolerance(case, xtol):
    """|x/x_ref - 1| <= xtol + 1e-11/|S|: the suite's guard band on yields against the reference is
    1e-11, and a relative error eps in the field moves the root by eps/|S|."""
    return xtol + 1e-11 / abs(case["log_slope"])


def oracle_field(O, cfg, case, tf):
    """The oracle's target field at the case's n_y: Y_B from its quadrature at that n_y, the rest from
    its fast path (whose Y_chi and rho_DM do not depend on n_y; rho_B / Y_B is a constant)."""
    p = O.point_yields(cfg, nz=case["nz"], z_max=case["z_max"])
    T_p = cfg["T_p_GeV"]
    yb = O.yb_quadrature(cfg, cfg["T_min_over_Tp"] * T_p, cfg["T_max_over_Tp"] * T_p, n_y=case["n_y"], nz=case["nz"],
                         z_max=case["z_max"])
    if tf == "Y_B":
        return yb
    assert tf == "DM_over_B"
    return p["rho_DM_kg_m3"] / (yb * (p["rho_B_kg_m3"] / p["Y_B"]))


@pytest.mark.parametrize("case", [c for c in _cases() if c["window"] is None], ids=lambda c: c["name"])
def test_rule_on_the_oracle_lands_on_the_reference_root(lib, case):
    from oracle import oracle as O
    sv = case["solve"]
    cfg = full_cfg(case["config"])
    tf = sv["target"]["field"]
    r = Run(lib, lambda x: oracle_field(O, dict(cfg, **{sv["field"]: x}), case, tf),
            sv["lo"], sv["hi"], target=sv["target"]["value"], xtol=1e-12)
    r.check_invariants()
    r.check_converged(1e-12)
    print(f"{case['name']}: x = {r.x!r} x_ref = {case['x_ref']!r} err = {abs(r.x / case['x_ref'] - 1.0):.3e} "
          f"evals = {r.evals}")
    assert abs(r.x / case["x_ref"] - 1.0) <= root_tolerance(case, 1e-12), (r.x, case["x_ref"])
    assert r.evals <= 64


def test_fixtures_cover_what_they_should():
    cs = _cases()
    assert len(cs) >= 12 and all(abs(c["log_slope"]) >= 0.1 for c in cs)
    assert {(c["nz"], c["z_max"]) for c in cs} == {(1200, 30.0), (13, 3.0)}
    fields = {c["solve"]["field"] for c in cs}
    assert {"P_chi_to_B", "source_shape_sigma_y", "m_chi_GeV", "v_w", "incident_flux_scale", "Y_chi_init",
            "window_half_width", "window_y0", "window_sigma_lo", "window_scale"} <= fields
    assert any(c["solve"]["target"]["field"] == "Y_B" for c in cs)
    assert any(c["config"]["regime"] == "thermal" for c in cs)
    # at x_ref the reference's field is the target (brentq's rtol of 4 eps times the slope), except where
    # the sign change is a jump: the suppressed m_chi case, whose T > m/3 branch switches node by node
    for c in cs:
        if c["continuous"]:
            assert abs(c["value_at_x_ref"] / c["solve"]["target"]["value"] - 1.0) <= 64 * EPS * max(1.0, abs(c["log_slope"]))
    assert sum(c["continuous"] for c in cs) >= 12


# ---- lzq_solve_check_host: every refusal, with its message -----------------------------------------
GOOD = {"field": "source_shape_sigma_y", "lo": 1.0, "hi": 50.0}
REFUSALS = [
    # (solve overrides, axis names, window?, part of the message)
    ({"field": "I_p"}, [], False, "changes the z-sum tables"),
    ({"field": "beta_over_H"}, [], False, "changes the z-sum tables"),
    ({"field": "T_p_GeV"}, [], False, "changes the z-sum tables"),
    ({"field": "T_min_over_Tp"}, [], False, "changes the z-sum tables"),
    ({"field": "T_max_over_Tp"}, [], False, "changes the z-sum tables"),
    ({"field": "window_table"}, [], True, "window table index"),
    ({"field": "window_half_width"}, [], False, "needs a window"),
    ({"field": "source_shape_sigma_y"}, ["m_chi_GeV"], True, "not read when the point has a window block"),
    ({}, ["m_chi_GeV", "source_shape_sigma_y"], False, "axis 1 writes the solve field"),
    ({"field": "window_sigma"}, ["window_sigma_lo"], True, "axis 0 writes the solve field"),
    ({"field": "window_sigma_hi"}, ["v_w", "window_sigma"], True, "axis 1 writes the solve field"),
    ({"field": "P_chi_to_B"}, ["delta_LZ"], False, "an LZ axis writes P"),
    ({"field": "delta_LZ"}, ["m_mix", "dprime"], False, "write delta_LZ"),
    ({"field": "m_mix"}, [], False, "needs a dprime axis"),
    ({"field": "dprime"}, ["v_w"], False, "needs an m_mix axis"),
    ({"lo": 5.0, "hi": 5.0}, [], False, "lo < hi"),
    ({"lo": 9.0, "hi": 5.0}, [], False, "lo < hi"),
    ({"lo": float("nan")}, [], False, "must be finite"),
    ({"hi": float("inf")}, [], False, "must be finite"),
    ({"xtol": 1.0}, [], False, "xtol"),
    ({"xtol": -1e-3}, [], False, "xtol"),
    ({"xtol": float("nan")}, [], False, "xtol"),
    ({"target": {"field": "DM_over_B", "value": float("nan")}}, [], False, "target"),
]


@pytest.mark.parametrize("over,axes,window,msg", REFUSALS)
def test_check_host_refusals(over, axes, window, msg):
    V = pkg("solve")
    with pytest.raises(ValueError, match=msg):
        V.check(dict(GOOD, **over), axes, {"kind": "plateau"} if window else None)


def test_check_host_accepts_every_allowed_field():
    V, N = pkg("solve"), pkg("_native")
    for f in ("m_chi_GeV", "g_chi", "v_w", "g_star", "g_star_s", "P_chi_to_B", "source_shape_sigma_y",
              "incident_flux_scale", "Y_chi_init", "n_chi_at_Tp_GeV3", "delta_LZ"):
        V.check(dict(GOOD, field=f), ["I_p", "T_p_GeV"], None)
    V.check(dict(GOOD, field="m_mix"), ["dprime"], None)
    V.check(dict(GOOD, field="dprime"), ["m_mix", "I_p"], None)
    for f in N.WINDOW_FIELD:
        if f != "window_table":
            V.check(dict(GOOD, field=f), ["m_chi_GeV", "window_table"], {"kind": "gauss"})
    V.check(dict(GOOD, field="window_sigma_lo"), ["window_sigma_hi", "window_y0"], {"kind": "plateau"})
    # the raw entry point: a target field outside the record, no solve at all
    L = N.load()
    s = V.to_ctypes(GOOD)
    s.target_field = 6
    assert L.lzq_solve_check_host(ctypes.byref(s), None, None, 0) == -1 and b"target field" in L.lzq_last_error()
    assert L.lzq_solve_check_host(None, None, None, 0) == -1


def test_entry_point_refuses_a_P_override_with_a_P_or_LZ_solve():
    """lzq_sweep_grid_solve's own check of d_P (before any HIP call): section 2's last refusal, which
    lzq_solve_check_host cannot make (it does not see d_P)."""
    V, N, C = pkg("solve"), pkg("_native"), pkg("config")
    L = N.load()
    base = C.to_ctypes_point(C.to_point(full_cfg({})))
    ax = (N.LzqAxis * 2)()
    ax[0].field, ax[0].n, ax[0].values = N.FIELD["m_chi_GeV"], 3, 8
    ax[1].field, ax[1].n, ax[1].values = N.FIELD["dprime"], 2, 8
    for field, n_axes in (("P_chi_to_B", 1), ("delta_LZ", 1), ("m_mix", 2)):
        sv = V.to_ctypes({"field": field, "lo": 0.01, "hi": 1.0})
        rc = L.lzq_sweep_grid_solve(ctypes.byref(base), None, ax, n_axes, ctypes.byref(sv), 0, 1, 2000, 13, 3.0, 8, 8,
                                    1 << 20, None, 8, 8, None)
        assert rc == -1 and b"per-point P override (d_P) together with a solve for P or an LZ field" in L.lzq_last_error()
    # the same call's other host-side refusals come first or after, each with its message
    sv = V.to_ctypes({"field": "I_p", "lo": 0.1, "hi": 1.0})
    assert L.lzq_sweep_grid_solve(ctypes.byref(base), None, ax, 1, ctypes.byref(sv), 0, 1, 2000, 13, 3.0, None, 8,
                                  1 << 20, None, 8, 8, None) == -1 and b"z-sum tables" in L.lzq_last_error()
    sv = V.to_ctypes({"field": "v_w", "lo": 0.1, "hi": 1.0})
    assert L.lzq_sweep_grid_solve(ctypes.byref(base), None, ax, 1, ctypes.byref(sv), 2, 5, 2000, 13, 3.0, None, 8,
                                  1 << 20, None, 8, 8, None) == -1 and b"outside grid" in L.lzq_last_error()
    assert L.lzq_sweep_grid_solve(ctypes.byref(base), None, ax, 1, ctypes.byref(sv), 0, 1, 2000, 13, 3.0, None, 8,
                                  16, None, 8, 8, None) == -1 and b"workspace" in L.lzq_last_error()


def test_solve_spec_forms():
    V = pkg("solve")
    s = V.normalize(GOOD)
    assert s == {"field": "source_shape_sigma_y", "lo": 1.0, "hi": 50.0, "target": {"field": "DM_over_B", "value": 5.357},
                 "xtol": 1e-12, "max_evals": 64}
    assert V.normalize(s) == s                                            # idempotent: the JSON round trip
    import json
    assert V.normalize(json.loads(json.dumps(s))) == s
    assert V.parse_cli("source_shape_sigma_y:1:50") == s
    t = V.parse_cli("m_chi_GeV:100:1e3:Y_B=2e-11")
    assert t["target"] == {"field": "Y_B", "value": 2e-11} and (t["lo"], t["hi"]) == (100.0, 1000.0)
    assert V.normalize(dict(GOOD, max_evals=1000))["max_evals"] == 256
    assert V.normalize(dict(GOOD, max_evals=0))["max_evals"] == 2
    for bad in ("sigma", "a:b:c", "m_chi_GeV:1", "m_chi_GeV:1:2:Y_B", "m_chi_GeV:1:2:Y_B=", "nope:1:2",
                "m_chi_GeV:1:2:nope=3"):
        with pytest.raises(ValueError):
            V.parse_cli(bad)
    for bad in ({"field": "m_chi_GeV"}, dict(GOOD, extra=1), dict(GOOD, target={"field": "nope"}),
                dict(GOOD, target={"field": "Y_B", "value": 1.0, "sigma": 2.0}), dict(GOOD, max_evals=2.5)):
        with pytest.raises(ValueError):
            V.normalize(bad)
    c = V.to_ctypes(dict(GOOD, target={"field": "Y_B", "value": 1e-10}))
    assert (c.field, c.target_field, c.lo, c.hi, c.target, c.xtol, c.max_evals) == (9, 0, 1.0, 50.0, 1e-10, 1e-12, 64)


def test_summary_block():
    V = pkg("solve")
    nan = float("nan")
    res = np.array([[2.0, 1.9, 2.1, 1e-15, 17, 0], [4.0, 3.9, 4.1, -1e-3, 3, 1], [nan, 1.0, 50.0, nan, 2, 2],
                    [nan, 1.0, 50.0, nan, 1, 3], [9.0, 9.0, 9.0, 0.0, 5, 0]])
    s = V.summary(GOOD, res)
    assert s["status"] == {"ok": 2, "max_evals": 1, "no_bracket": 1, "nan": 1, "bad_table": 0}
    assert s["x"] == {"min": 2.0, "median": 4.0, "max": 9.0} and s["evals"] == {"mean": 5.6, "max": 17}
    assert s["field"] == "source_shape_sigma_y" and s["target"] == {"field": "DM_over_B", "value": 5.357}
    assert V.summary(GOOD, res[2:4])["x"] is None


def test_kernels_resources_are_reported():
    """tools/kernel_resources.py on lzq_solve.hip: both instantiations at the 8 waves/SIMD of their
    __launch_bounds__ (DESIGN §4.12 records the registers and the scratch)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    rows = [r for r in kr.resources("lzq_solve.hip", []) if "grid_solve_kernel" in r["kernel"]]
    assert len(rows) == 2
    for r in rows:
        assert int(r["Occupancy [waves/SIMD]"]) == 8, r
        assert 2 * int(r["LDS Size [bytes/block]"]) <= 160 * 1024, r
