#!/usr/bin/env python3
"""Golden fixtures for the per-point root solve (include/lzq.h lzq_sweep_grid_solve), made by running
the REFERENCE itself with no change to its code: each root is found with scipy.optimize.brentq
(rtol 4 eps) on the reference's own yields as a function of the solve parameter.

Cases without a window run the reference's fast path as main() does (fpy:361-417: its
integrate_YB_by_quadrature, then the densities from its own functions and constants); window cases use
the recipe of make_golden_window.py (source_shape_sigma_y = 1e300 and bs.aov wrapped to return
A/V(y) W(y)).  Per case: the configuration, window and solve spec, x_ref, the reference's value of the
target field at x_ref (equal to the target unless the sign change is a jump of the field: "continuous"),
and the logarithmic slope S = dln field / dln x by central difference (a relative
error eps in the field moves the root by eps/|S|, which is the tolerance the tests use).

Writes tests/golden/golden_solve.json.  Runs only where the reference is (it never travels to the GPU
box).

    python tests/golden/make_golden_solve.py     # ~2 min
"""
from __future__ import annotations

import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _base_cfg, _fpy  # noqa: E402
from make_golden_window import WindowedKernel, win  # noqa: E402

POINT_FIELDS = ("m_chi_GeV", "g_chi", "v_w", "g_star", "g_star_s", "P_chi_to_B", "source_shape_sigma_y",
                "incident_flux_scale", "Y_chi_init", "n_chi_at_Tp_GeV3")
WINDOW_FIELDS = {"window_y0": ("y0",), "window_half_width": ("half_width",), "window_sigma_lo": ("sigma_lo",),
                 "window_sigma_hi": ("sigma_hi",), "window_sigma": ("sigma_lo", "sigma_hi"), "window_scale": ("scale",)}
PLANCK = {"field": "DM_over_B", "value": 5.357}
TABLES = {"bump": {"u": [-40.0, -10.0, 0.0, 5.0, 20.0, 45.0], "W": [[0.0, 0.3, 1.0, 0.8, 0.2, 0.0]]}}


def reference_fields(fpy, c, w, tabs, n_y, nz, z_max):
    """The `final` block of the reference's fast path (fpy:372-384, 413-417) for config c, with the
    window w (None: the reference's own Gaussian)."""
    d = fpy.default_config()
    d.update(c)
    if w is not None:
        d["source_shape_sigma_y"] = 1e300
    cfg = fpy.Config(**d)
    assert (not cfg.deplete_DM_from_source) and cfg.sigma_v_chi_GeV_m2 == 0.0 and cfg.Gamma_wash_over_H == 0.0
    bs = fpy.BoltzmannSystem(cfg, float(cfg.P_chi_to_B))
    aov = fpy.AoverVKernel(cfg.I_p, cfg.beta_over_H, cfg.T_p_GeV, cfg.v_w, cfg.g_star, z_max=z_max, nz=nz)
    bs.aov = aov if w is None else WindowedKernel(aov, w, tabs)
    T_p = cfg.T_p_GeV
    T_hi, T_lo = cfg.T_max_over_Tp * T_p, cfg.T_min_over_Tp * T_p
    YB = bs.integrate_YB_by_quadrature(T_lo, T_hi, n_y=n_y)
    if cfg.regime.lower().startswith("therm"):
        Ychi = fpy.n_chi_eq(T_hi, cfg.m_chi_GeV, cfg.g_chi, cfg.chi_stats) / fpy.s_entropy(T_hi, cfg.g_star_s)
    elif cfg.Y_chi_init is not None:
        Ychi = float(cfg.Y_chi_init)
    elif cfg.n_chi_at_Tp_GeV3 is not None:
        Ychi = float(cfg.n_chi_at_Tp_GeV3) / max(fpy.s_entropy(T_p, cfg.g_star_s), 1e-300)
    else:
        Ychi = 1.0e-12
    rhoB = YB * fpy.S0_M3 * fpy.M_PROTON_KG
    rhoDM = Ychi * fpy.S0_M3 * (cfg.m_chi_GeV * fpy.GEV_TO_KG)
    return {"Y_B": YB, "Y_chi": Ychi, "rho_B_kg_m3": rhoB, "rho_DM_kg_m3": rhoDM,
            "DM_over_B": rhoDM / max(rhoB, 1e-300)}


def with_x(c, w, field, x):
    """(config, window) with the solve field set to x."""
    if field in POINT_FIELDS:
        return dict(c, **{field: x}), w
    return c, dict(w, **{k: x for k in WINDOW_FIELDS[field]})


def cases():
    base = _base_cfg()
    Z, Zs = (1200, 30.0), (13, 3.0)
    plateau = win("plateau", y0=-5.0, half_width=3.0, sigma_lo=4.0, sigma_hi=6.0)
    out = [
        # (name, config, window, tables, field, lo, hi, target, n_y, (nz, z_max))
        ("P_shipped_8000", base, None, None, "P_chi_to_B", 0.01, 1.0, PLANCK, 8000, Z),
        ("P", base, None, None, "P_chi_to_B", 0.01, 1.0, PLANCK, 2000, Zs),
        ("sigma_y", base, None, None, "source_shape_sigma_y", 1.0, 50.0, PLANCK, 2000, Z),
        ("sigma_y_small_grid", base, None, None, "source_shape_sigma_y", 1.0, 50.0, None, 2000, Zs),
        ("m_chi_linear", base, None, None, "m_chi_GeV", 0.1, 1000.0, PLANCK, 2000, Z),
        ("v_w", base, None, None, "v_w", 0.01, 1.0, PLANCK, 2000, Z),
        ("flux", base, None, None, "incident_flux_scale", 1e-10, 1e-8, None, 2000, Zs),
        ("Y_chi_init", base, None, None, "Y_chi_init", 1e-11, 1e-8, None, 2000, Zs),
        ("m_chi_suppressed", base, None, None, "m_chi_GeV", 100.0, 1000.0, {"field": "Y_B", "value": 2e-11}, 2000, Z),
        ("thermal", dict(base, regime="thermal"), None, None, "P_chi_to_B", 1e-6, 1.0, None, 2000, Zs),
        ("plateau_half_width", base, plateau, None, "window_half_width", 0.0, 40.0, None, 2000, Zs),
        ("plateau_y0", base, win("plateau", y0=0.0, half_width=2.0, sigma_lo=5.0, sigma_hi=5.0), None, "window_y0",
         8.0, 45.0, None, 2000, Zs),
        ("two_sided_sigma_lo", base, win("plateau", y0=8.0, sigma_lo=5.0, sigma_hi=3.0), None, "window_sigma_lo", 0.5,
         60.0, None, 2000, Zs),
        ("table_scale", base, win("table", table=0), "bump", "window_scale", 0.2, 5.0, None, 2000, Z),
    ]
    return out


def main():
    import numpy as np
    from scipy.optimize import brentq
    fpy = _fpy()
    rows = []
    for name, c, w, t, field, lo, hi, target, n_y, (nz, z_max) in cases():
        tabs = TABLES[t] if t else None

        def value(x, tf):
            cc, ww = with_x(c, w, field, float(x))
            return reference_fields(fpy, cc, ww, tabs, n_y, nz, z_max)[tf]

        if target is None:   # a case without a preset target: the geometric mean of the end values
            tf = "DM_over_B"
            a, b = value(lo, tf), value(hi, tf)
            target = {"field": tf, "value": float(math.sqrt(a * b))}
        tf, tv = target["field"], target["value"]
        flo, fhi = value(lo, tf) - tv, value(hi, tf) - tv
        assert flo * fhi < 0.0, (name, flo, fhi)
        x_ref = brentq(lambda x: value(x, tf) - tv, lo, hi, xtol=1e-300, rtol=4 * np.finfo(float).eps,
                       maxiter=200)
        v_ref = value(x_ref, tf)
        h = 1e-4
        S = (math.log(value(x_ref * (1 + h), tf)) - math.log(value(x_ref * (1 - h), tf))) / \
            (math.log1p(h) - math.log1p(-h))
        assert abs(S) >= 0.1, (name, S)
        rows.append({"name": name, "config": c, "window": w, "tables": t, "n_y": n_y, "nz": nz, "z_max": z_max,
                     "solve": {"field": field, "lo": lo, "hi": hi, "target": target}, "x_ref": x_ref,
                     "value_at_x_ref": v_ref, "log_slope": S,
                     # False: brentq closed on a jump of the field, not on a root (the T > m/3 branch of
                     # fpy:90-120 switches node by node as m_chi moves): the sign change is there all the same
                     "continuous": abs(v_ref / tv - 1.0) <= 1e-9})
        print(f"{name:22s} x_ref = {x_ref!r:24} value = {v_ref!r:24} S = {S:+.4f}")
    out = {"generator": "tests/golden/make_golden_solve.py (scipy.optimize.brentq, rtol 4 eps, on the reference's fast "
                        "path fpy:361-417; window cases by make_golden_window.py's recipe)",
           "numpy": np.__version__, "tables": TABLES, "cases": rows}
    path = os.path.join(HERE, "golden_solve.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, len(rows), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
