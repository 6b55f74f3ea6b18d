#!/usr/bin/env python3
"""Golden fixture of the continuum A/V (csrc/lzq_cont.h), made by running the
REFERENCE itself with no change to its code: `bs.aov` (a public attribute, fpy:197) is replaced by
a kernel whose `A_over_V_y(y)` is the definition

    A/V_cont(y) = 0                                          for y > 50
                = pref0 e^yh F(c),  yh = clip(y, +-50),  c = -(I_p/6) e^yh,
      F(c)      = int_0^z_max z^2 e^-z exp(c gamma(4, z)) dz

with the z-integral evaluated by mpmath.quad at 40 digits (gamma(4, z) from its series below z = 1
and its closed form above, both at the working precision) and the product rounded once to a double.
pref0, the clip and the y > 50 zero are the reference's (fpy:158-165).  Nothing here comes from the
library.  Writes tests/golden/golden_cont.json:

* "aov": A/V_cont of the shipped kernel at ~40 y (30 digits as a string, and the double), next to the
  reference grid's own A_over_V_y at the same y;
* "cases": (config, window, n_y, z_max) -> Y_B of fpy:231-267 on the continuum A/V.

Runs only in the build container (the reference never travels to the GPU box).

    python tests/golden/make_golden_cont.py     # ~3 min on 8 cores
"""
from __future__ import annotations

import json
import math
import multiprocessing
import os
import sys

import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _base_cfg, _fpy  # noqa: E402
from make_golden_window import win, window_value  # noqa: E402

DPS = 40
N_Y = 2000
Y_B_FLOOR = 1e-250                    # a kept case is exactly 0 or at least this
PROTOTYPE_SHIPPED_NY8000 = 1.80507532e-10   # the issue's prototype (n_y = 8000): a sanity band, not a gate


def gamma4(z):
    """gamma(4, z) at the working precision, without the cancellation of fpy:156 at small z."""
    if z < 1:
        s, t, j = mp.mpf(0), mp.mpf(1), 0          # t = (-z)^j / j!
        while True:
            a = t / (j + 4)
            s += a
            if abs(a) < mp.ldexp(1, -mp.mp.prec - 8) * abs(s):
                break
            j += 1
            t = -t * z / j
        return z ** 4 * s
    return 6 - mp.exp(-z) * (((z + 3) * z + 6) * z + 6)


def F_cont(I_p, y, z_max):
    """The z-integral at y (inside a workdps context); the break points follow the cut-off of
    exp(-a gamma4), z_c = (4/a)^(1/4), and the range ends where the integrand is below e^-2600."""
    yh = min(max(mp.mpf(y), mp.mpf(-50)), mp.mpf(50))
    a = (mp.mpf(I_p) / 6) * mp.exp(yh)
    zm = mp.mpf(z_max)
    zc = (4 / a) ** mp.mpf("0.25")
    if zc >= zm / 8:
        pts = [0, zm / 32, zm / 16, zm / 8, zm / 4, zm / 2, zm]
    else:
        zu = min(zm, 2 * (4 * 2600 / a) ** mp.mpf("0.25"))
        pts = [0] + [zc * f for f in (0.25, 0.5, 0.75, 1, 1.25, 1.5, 2, 2.5, 3, 4, 6, 8) if zc * f < zu] + [zu]
        if zu < zm:                                   # (for a ~ 1 the tail beyond the cut-off still counts)
            pts += [t for t in (2 * zu, 4 * zu, 8 * zu, 16 * zu) if t < zm] + [zm]
    val, err = mp.quad(lambda z: z * z * mp.exp(-z - a * gamma4(z)), pts, error=True)
    assert err <= mp.mpf(10) ** -30 * val, (y, val, err)
    return val


def aov_cont(k, y, z_max):
    """A/V_cont(y) of the kernel k = (I_p, beta_over_H, T_p, v_w, g_star) as an mp number."""
    if y > 50.0:
        return mp.mpf(0)
    I_p, B, Tp, v_w, g_star = (mp.mpf(float(x)) for x in k)
    v_w = max(v_w, mp.mpf(1e-12))
    H_p = mp.mpf(1.66) * mp.sqrt(g_star) * Tp * Tp / mp.mpf(MPL_GEV)    # fpy:85
    yh = min(max(mp.mpf(y), mp.mpf(-50)), mp.mpf(50))
    return (I_p / 2) * (B * H_p / v_w) * mp.exp(yh) * F_cont(float(k[0]), y, z_max)


MPL_GEV = None   # fpy.MPL_GEV (set in main and in the workers)


def _work(args):
    k, z_max, mpl, ys = args
    global MPL_GEV
    MPL_GEV = mpl
    with mp.workdps(DPS):
        return [mp.nstr(aov_cont(k, y, z_max), 32) for y in ys]


def aov_many(pool, k, z_max, ys):
    ys = [float(y) for y in ys]
    chunks = [ys[i:i + 25] for i in range(0, len(ys), 25)]
    out = []
    for part in pool.map(_work, [(k, z_max, MPL_GEV, c) for c in chunks]):
        out += part
    return out


class ContinuumKernel:
    """bs.aov's stand-in: A/V_cont, precomputed at the y-nodes the quadrature will ask for."""

    def __init__(self, table, w=None):
        self.table, self.w = table, w

    def A_over_V_y(self, y):
        v = self.table[float(y)]
        return v * window_value(self.w, None, y) if self.w is not None else v


def y_nodes(fpy, cfg, n_y):
    """The y-grid of fpy:234-247 (None when the window is empty)."""
    import numpy as np
    y_lo = max(fpy.y_of_T(cfg.T_max_over_Tp * cfg.T_p_GeV, cfg.T_p_GeV, cfg.beta_over_H), -80.0)
    y_hi = min(fpy.y_of_T(cfg.T_min_over_Tp * cfg.T_p_GeV, cfg.T_p_GeV, cfg.beta_over_H), 50.0)
    if y_hi <= y_lo:
        return None
    return np.linspace(y_lo, y_hi, max(int(n_y), 2000))


def reference_Y_B(fpy, pool, c, w, n_y, z_max):
    d = fpy.default_config()
    d.update(c)
    if w is not None:
        d["source_shape_sigma_y"] = 1e300     # the reference's own window is exactly 1 (make_golden_window.py)
    cfg = fpy.Config(**d)
    bs = fpy.BoltzmannSystem(cfg, float(cfg.P_chi_to_B))
    ys = y_nodes(fpy, cfg, n_y)
    table = {}
    if ys is not None:
        k = (cfg.I_p, cfg.beta_over_H, cfg.T_p_GeV, cfg.v_w, cfg.g_star)
        table = {float(y): float(v) for y, v in zip(ys, aov_many(pool, k, z_max, ys))}
    bs.aov = ContinuumKernel(table, w)
    return bs.integrate_YB_by_quadrature(cfg.T_min_over_Tp * cfg.T_p_GeV, cfg.T_max_over_Tp * cfg.T_p_GeV, n_y=n_y)


def cases():
    base = _base_cfg()
    return [("shipped", base, None, 30.0),
            ("I_p=0.05", dict(base, I_p=0.05), None, 30.0),
            ("I_p=1.0", dict(base, I_p=1.0), None, 30.0),
            ("m_chi=3000", dict(base, m_chi_GeV=3000.0), None, 30.0),
            ("beta_over_H=200", dict(base, beta_over_H=200.0), None, 30.0),
            ("empty window", dict(base, T_min_over_Tp=2.0, T_max_over_Tp=1.5), None, 30.0),
            ("z_max=3", base, None, 3.0),
            ("plateau", base, win("plateau", y0=-10.0, half_width=4.0, sigma_lo=3.0, sigma_hi=12.0), 30.0)]


def aov_ys():
    ys = [float(y) for y in range(-50, 51, 5)]                        # the ladder
    ys += [27.5, 30.0, 33.0, 36.0, 39.0, 42.0, 44.0, 46.0, 47.5, 48.5, 49.0, 49.5, 49.9]   # the grid gives 0 here
    ys += [-7.3, 0.7, 3.1, 11.9, 19.3]
    ys += [math.nextafter(50.0, math.inf), 60.0, -60.0]               # (50.0 is on the ladder)
    return ys


def main():
    import numpy as np
    global MPL_GEV
    fpy = _fpy()
    MPL_GEV = fpy.MPL_GEV
    base = _base_cfg()
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        d = fpy.default_config()
        d.update(base)
        cfg = fpy.Config(**d)
        k = (cfg.I_p, cfg.beta_over_H, cfg.T_p_GeV, cfg.v_w, cfg.g_star)
        grid = fpy.AoverVKernel(*k)
        ys = aov_ys()
        vals = aov_many(pool, k, 30.0, ys)
        aov = {"kernel": dict(zip(("I_p", "beta_over_H", "T_p_GeV", "v_w", "g_star"), map(float, k))), "z_max": 30.0,
               "y": ys, "A_over_V": [float(v) for v in vals], "A_over_V_str": vals,
               "A_over_V_grid": [grid.A_over_V_y(y) for y in ys]}
        # the break points and the precision do not matter: a few y again at 60 digits, the range halved
        with mp.workdps(60):
            for y in (-50.0, -7.3, 11.9, 30.0, 49.9):
                yh = mp.mpf(y)
                a = (mp.mpf(float(k[0])) / 6) * mp.exp(yh)
                pts = [0] + [mp.mpf(30) * mp.mpf(2) ** -j for j in range(40, -1, -1)]
                chk = mp.quad(lambda z: z * z * mp.exp(-z - a * gamma4(z)), pts)
                own = F_cont(float(k[0]), y, 30.0)
                assert abs(chk - own) <= mp.mpf(10) ** -28 * own, (y, chk, own)
        rows = []
        for name, c, w, z_max in cases():
            yb = reference_Y_B(fpy, pool, c, w, N_Y, z_max)
            print(name, yb, flush=True)
            if yb == 0.0 or abs(yb) >= Y_B_FLOOR:
                rows.append({"name": name, "config": c, "window": w, "n_y": N_Y, "z_max": z_max, "Y_B": yb})
            else:
                print("dropped (|Y_B| below the floor):", name, yb)
    assert len(rows) >= 8 and any(r["Y_B"] == 0.0 for r in rows), rows
    shipped = rows[0]["Y_B"]
    # sanity band (the prototype ran n_y = 8000; the y-quadrature's own step error is far below 1e-6)
    assert abs(shipped / PROTOTYPE_SHIPPED_NY8000 - 1.0) < 1e-6, shipped
    pos = [i for i, (g, v) in enumerate(zip(aov["A_over_V_grid"], aov["A_over_V"])) if g == 0.0 and v > 0.0]
    assert len(pos) >= 8, pos   # the reference grid's A/V is 0 where the integral is not
    out = {"generator": "tests/golden/make_golden_cont.py (reference fpy:231-267 with bs.aov replaced by the converged "
                        "z-integral, mpmath.quad at 40 digits)",
           "numpy": np.__version__, "mpmath": mp.__version__, "aov": aov, "cases": rows}
    path = os.path.join(HERE, "golden_cont.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, len(rows), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
