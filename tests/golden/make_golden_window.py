#!/usr/bin/env python3
"""Golden fixtures for the source activity window W(y) (include/lzq.h lzq_window; PAPER §10 step
4), made by running the REFERENCE itself with no change to its code:

* `cfg.source_shape_sigma_y = 1e300`: (y/sigma)^2 underflows to 0, so the reference's own window
  (fpy:262) is exactly 1.0 at every node;
* `bs.aov` (a public attribute, fpy:197) is replaced by a wrapper whose `A_over_V_y(y)` returns
  `inner.A_over_V_y(y) * W(y)`, so fpy:261-265 integrates P J A/V W / (s H T) |dT/dy|.

W(y) is written here in plain Python from the definition in include/lzq.h (no library call, no
np.interp).  With W the Gaussian of sigma = 9 the recipe reproduces the unmodified reference on the
shipped config to 1e-15 relative (asserted below; not to the bit: the wrapper multiplies A/V by W
before P J, the reference after, fpy:264).  Writes tests/golden/golden_window.json:
(config, window, n_y, nz, z_max) -> Y_B.

Runs only in the build container (the reference never travels to the GPU box).

    python tests/golden/make_golden_window.py     # ~20 s
"""
from __future__ import annotations

import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _base_cfg, _fpy, random_points  # noqa: E402

NEUTRAL = {"y0": 0.0, "half_width": 0.0, "sigma_lo": 1.0, "sigma_hi": 1.0, "scale": 1.0, "table": 0}
Y_B_FLOOR = 1e-250                    # a kept case is exactly 0 or at least this


def win(kind, **kw):
    return dict(NEUTRAL, kind=kind, **kw)


def window_value(w, tabs, y):
    """W(y) of include/lzq.h, one IEEE operation per step."""
    y = float(y)
    if w["kind"] == "table":
        u, W = tabs["u"], tabs["W"][w["table"]]
        v = (y - w["y0"]) / w["scale"]
        if v < u[0]:
            return W[0]
        if v >= u[-1]:
            return W[-1]
        lo, hi = 0, len(u) - 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if u[mid] <= v:
                lo = mid
            else:
                hi = mid
        return W[lo] + (v - u[lo]) * ((W[lo + 1] - W[lo]) / (u[lo + 1] - u[lo]))
    if w["kind"] == "gauss":
        q = y * (1.0 / max(w["sigma_hi"], 1e-6))
    else:
        u = y - w["y0"]
        d = max(abs(u) - w["half_width"], 0.0)
        q = d * (1.0 / max(w["sigma_lo"] if u < 0.0 else w["sigma_hi"], 1e-6))
    return math.exp(-0.5 * (q * q))


class WindowedKernel:
    """bs.aov's stand-in: the reference's own kernel times W(y)."""

    def __init__(self, inner, w, tabs):
        self.inner, self.w, self.tabs = inner, w, tabs

    def A_over_V_y(self, y):
        return self.inner.A_over_V_y(y) * window_value(self.w, self.tabs, y)


def reference_Y_B(fpy, c, w, tabs, n_y, nz, z_max):
    d = fpy.default_config()
    d.update(c)
    d["source_shape_sigma_y"] = 1e300
    cfg = fpy.Config(**d)
    bs = fpy.BoltzmannSystem(cfg, float(cfg.P_chi_to_B))
    bs.aov = WindowedKernel(fpy.AoverVKernel(cfg.I_p, cfg.beta_over_H, cfg.T_p_GeV, cfg.v_w, cfg.g_star, z_max=z_max,
                                             nz=nz), w, tabs)
    return bs.integrate_YB_by_quadrature(cfg.T_min_over_Tp * cfg.T_p_GeV, cfg.T_max_over_Tp * cfg.T_p_GeV, n_y=n_y)


def table_sets(fpy, base):
    """Named (u, W rows) sets; every row of a set shares its knots."""
    import numpy as np
    sets = {"two": {"u": [-10.0, 20.0], "W": [[1.0, 0.25], [0.0, 1.0]]},
            "ends0": {"u": [-20.0, -5.0, 0.0, 10.0, 30.0], "W": [[0.0, 0.5, 1.0, 0.7, 0.0]]}}
    # 1024 non-uniform knots over [-60, 55]: a bump, and a switch-on with an exponential tail
    u = [-60.0 + 115.0 * (i / 1023.0) ** 1.5 for i in range(1024)]
    sets["k1024"] = {"u": u, "W": [[math.exp(-0.5 * ((x - 3.0) / 7.0) ** 2) for x in u],
                                   [math.exp(-max(x, 0.0) / 12.0) / (1.0 + math.exp(-(x + 5.0) / 2.0)) for x in u]]}
    # a knot exactly on a y-node of the shipped config's n_y = 2000 grid (fpy:234-247)
    y_lo = max(fpy.y_of_T(base["T_max_over_Tp"] * base["T_p_GeV"], base["T_p_GeV"], base["beta_over_H"]), -80.0)
    y_hi = min(fpy.y_of_T(base["T_min_over_Tp"] * base["T_p_GeV"], base["T_p_GeV"], base["beta_over_H"]), 50.0)
    ys = np.linspace(y_lo, y_hi, 2000)
    sets["node"] = {"u": [-30.0, float(ys[700]), float(ys[1100]), 40.0], "W": [[0.1, 1.0, 0.4, 0.05]]}
    return sets


def cases(fpy):
    base = _base_cfg()
    sets = table_sets(fpy, base)
    D = (2000, 1200, 30.0)
    on_base = [
        (win("gauss", sigma_hi=9.0), None),
        (win("gauss", sigma_hi=2.5), None),
        (win("plateau", y0=5.0, sigma_lo=6.0, sigma_hi=6.0), None),                      # a shifted Gaussian
        (win("plateau", y0=-10.0, half_width=4.0, sigma_lo=3.0, sigma_hi=12.0), None),   # flat top, two shoulders
        (win("plateau", half_width=200.0), None),                                        # W = 1 on the whole range
        (win("plateau", y0=2.0, half_width=10.0, sigma_lo=1e-3, sigma_hi=1e-3), None),   # a top-hat: the shoulder
        (win("plateau", y0=70.0, sigma_lo=15.0, sigma_hi=15.0), None),                   # falls between two y-nodes
        (win("plateau", y0=70.0, half_width=1.0, sigma_lo=1e-3, sigma_hi=1e-3), None),   # y0 above the range: 0
        (win("plateau", y0=-60.0, half_width=20.0, sigma_lo=1.0, sigma_hi=5.0), None),   # y0 below the range
        (win("plateau", sigma_lo=4.0, sigma_hi=20.0), None),                             # a two-sided Gaussian
        (win("table", table=0), "two"),
        (win("table", table=1), "two"),
        (win("table", table=0), "k1024"),
        (win("table", table=1), "k1024"),
        (win("table", table=0, y0=5.0, scale=3.0), "k1024"),                             # shifted and stretched
        (win("table"), "node"),
        (win("table"), "ends0"),
        (win("table", y0=200.0), "ends0"),                                               # below the first knot: 0
        (win("table", y0=-3.0, scale=0.25), "ends0"),
    ]
    out = [(base, w, t, *D) for w, t in on_base]
    for i in (0, 3, 5, 12, 16):                                                          # the (13, 3) z grid
        out.append((base, on_base[i][0], on_base[i][1], 2000, 13, 3.0))
    for i in (0, 4, 13):                                                                 # n_y = 8000
        out.append((base, on_base[i][0], on_base[i][1], 8000, 1200, 30.0))
    # seeded configs on both sides of the T = m/3 branch of fpy:90-120: relativistic everywhere,
    # non-relativistic everywhere, the branch inside the y range, then make_golden.py's generator
    seeded = [dict(base, m_chi_GeV=50.0), dict(base, m_chi_GeV=3000.0), dict(base, m_chi_GeV=300.0)]
    seeded += random_points(5, seed=77)
    for c in seeded:
        out.append((c, win("gauss", sigma_hi=float(c["source_shape_sigma_y"])), None, *D))
        out.append((c, on_base[3][0], None, *D))
        out.append((c, on_base[13][0], "k1024", *D))
    return sets, out


def main():
    import numpy as np
    fpy = _fpy()
    sets, cs = cases(fpy)
    rows = []
    for c, w, t, n_y, nz, z_max in cs:
        yb = reference_Y_B(fpy, c, w, sets[t] if t else None, n_y, nz, z_max)
        if yb == 0.0 or abs(yb) >= Y_B_FLOOR:   # keep only cases on which a relative error means something
            rows.append({"config": c, "window": w, "tables": t, "n_y": n_y, "nz": nz, "z_max": z_max, "Y_B": yb})
        else:
            print("dropped (|Y_B| below the floor):", w, yb)
    assert all(r["Y_B"] == 0.0 or (math.isfinite(r["Y_B"]) and abs(r["Y_B"]) >= Y_B_FLOOR) for r in rows)
    assert len(rows) >= 45, len(rows)
    assert any(r["Y_B"] == 0.0 for r in rows)
    shipped = [r for r in rows if r["config"] == _base_cfg() and r["window"] == win("gauss", sigma_hi=9.0) and
               (r["n_y"], r["nz"], r["z_max"]) == (8000, 1200, 30.0)]
    d = fpy.default_config()
    d.update(_base_cfg())
    cfg = fpy.Config(**d)
    own = fpy.BoltzmannSystem(cfg, float(cfg.P_chi_to_B)).integrate_YB_by_quadrature(
        cfg.T_min_over_Tp * cfg.T_p_GeV, cfg.T_max_over_Tp * cfg.T_p_GeV, n_y=8000)
    assert len(shipped) == 1 and abs(shipped[0]["Y_B"] - own) <= 1e-15 * own, (shipped, own)
    out = {"generator": "tests/golden/make_golden_window.py (reference fpy:231-267 with source_shape_sigma_y = 1e300 "
                        "and bs.aov wrapped to return A/V(y) W(y))",
           "numpy": np.__version__, "tables": sets, "cases": rows}
    path = os.path.join(HERE, "golden_window.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, len(rows), "cases,", os.path.getsize(path), "bytes")
    for r in rows:
        print(r["window"]["kind"], r["tables"], r["n_y"], r["nz"], r["Y_B"])


if __name__ == "__main__":
    main()
