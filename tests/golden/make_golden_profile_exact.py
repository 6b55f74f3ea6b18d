#!/usr/bin/env python3
"""Golden vectors for the bounce-profile propagation (csrc/lzq_profile.hip) on CURVED profiles: the
exact conversion probability through cubic-spline profiles, by the power-series solution of
tests/profile_exact.py (mpmath, 40 digits), for the kernel's own start state and projection.  The
53 Weber fixtures (make_golden_weber.py) have piecewise-linear Delta and constant m; these meet the
cubic terms of the Magnus polynomials, the m', m'' terms of the dressed edge states and the step
rule on curved intervals with an answer that shares nothing with the scheme.

    python tests/golden/make_golden_profile_exact.py   # writes tests/golden/golden_profile_exact.json

Shapes store their knots, samples and the 8-double interval rows (scipy CubicSpline, not-a-knot) as
hex floats: the GPU is handed exactly the rows the reference solved.  Each case records
  point     - (y_B, y_chi, lambda_tr_eff, v_w);
  P         - the exact probability (40 digits) on Delta = y_B phi - y_chi Phi, m = lambda phi formed
              from the rows without rounding;
  e_ref     - |restatement - P| at 4 and 16 steps per radian (tests/profile_ref.py
              propagate_profile on the CPU): the scheme's truncation error at that step count, which
              kernel and restatement share;
  steps     - Magnus steps of the restatement at 4 and 16 steps per radian;
  dP_spline - what a spline-coefficient error at the suite's bound (1e-11 of a row's largest
              coefficient, tests/test_gpu_profile.py test_splines_match_scipy) does to P: the largest
              |change| of the restatement's P (4 steps per radian) over 4 draws in which EVERY
              coefficient of every row moves by the full bound with a random sign.

Cases (each <= ~3000 steps at 16 steps per radian):
  wiggly    - wiggly(24, seed 0 / 1, span 4) x the four coupling sets of
              test_propagation_matches_restatement;
  cut_wall  - a tanh wall cut at +-1.5 w: phi', Phi' large at both ends (the m', m'' edge terms);
  four_knot - the 4-knot minimum on a short window;
  six_knot  - 6 knots over +-3 w: the crossing interval is strongly cubic;
  ratio50   - knot spacings alternating 1 : 50 at a fast wall: one-step intervals, and a step rule
              whose end sample comes from the next interval;
  slow_wall / fast_wall - v_w = 0.05 / 0.95;
  tiny_delta / big_delta - delta_LZ ~ 1e-6 / ~ 5;
  lambda_zero - no mixing: P = 0.
"""
import json
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import profile_cases as C   # noqa: E402
import profile_exact as X   # noqa: E402
import profile_ref as R     # noqa: E402

SPLINE_BOUND = 1e-11


def wall(x, w=1.0, v=1.0, V=1.3):
    return x, 0.5 * v * (1.0 - np.tanh(x / w)), 0.5 * V * (1.0 + np.tanh(x / w))


def shapes():
    s = {f"wiggly{k}": C.wiggly(24, k, span=4.0) for k in range(2)}
    s["cut_wall"] = wall(np.linspace(-1.5, 1.5, 13))
    s["four_knot"] = wall(np.linspace(-0.4, 0.4, 4))
    s["six_knot"] = wall(np.linspace(-3.0, 3.0, 6))
    s["ratio50"] = wall(-2.0 + np.concatenate([[0.0], np.cumsum(np.tile([0.01, 0.5], 8))[:-1]]))
    s["wall16"] = wall(np.linspace(-2.0, 2.0, 16))
    return s


def cases():
    out = [(f"wiggly{k}_{i}", f"wiggly{k}", c[:4]) for k in range(2) for i, c in enumerate(C.COUPLINGS)]
    out += [("cut_wall", "cut_wall", (1.0, 1.0, 0.3, 0.3)),
            ("four_knot", "four_knot", (1.0, 1.0, 0.2, 0.3)),
            ("six_knot", "six_knot", (1.3, 0.8, 0.1, 0.3)),
            ("ratio50", "ratio50", (1.0, 1.0, 0.3, 0.5)),
            ("slow_wall", "wall16", (1.0, 1.0, 0.1, 0.05)),
            ("fast_wall", "wall16", (1.0, 1.0, 0.1, 0.95)),
            ("tiny_delta", "wall16", (1.0, 1.0, 1.5e-3, 0.3)),
            ("big_delta", "wall16", (1.0, 1.0, 3.3, 0.3)),
            ("lambda_zero", "wall16", (1.0, 1.0, 0.0, 0.3))]
    return out


def steps(x, c8, pt, spr):
    return sum(R.interval_steps(x, c8[:, :4], c8[:, 4:], j, *pt, spr) for j in range(len(x) - 1))


def hexes(a):
    return [float(v).hex() for v in np.asarray(a).ravel()]


def main():
    out = {"dps": X.DPS, "generator": "tests/golden/make_golden_profile_exact.py",
           "spline_bound": SPLINE_BOUND, "shapes": {}, "cases": []}
    sh = shapes()
    rows = {}
    for name, (x, phi, Phi) in sh.items():
        rows[name] = C.rows8(x, phi, Phi)
        out["shapes"][name] = {"knots": hexes(x), "phi": hexes(phi), "Phi": hexes(Phi), "coef": hexes(rows[name])}
    rng = np.random.default_rng(0)
    for name, shape, pt in cases():
        x, c8 = sh[shape][0], rows[shape]
        P = X.propagate_exact(x, *X.dm_rows(c8, *pt[:3]), pt[3])
        rec = {"name": name, "shape": shape, "point": list(pt), "P": mpmath.nstr(P, X.DPS), "e_ref": {}, "steps": {}}
        for spr in (4, 16):
            Pr = R.propagate_profile(x, c8[:, :4], c8[:, 4:], *pt, spr=float(spr))
            rec["e_ref"][str(spr)] = float(abs(Pr - P))
            rec["steps"][str(spr)] = steps(x, c8, pt, float(spr))
            if spr == 4:
                P4 = Pr
        scale = np.repeat(np.stack([np.abs(c8[:, :4]).max(axis=1), np.abs(c8[:, 4:]).max(axis=1)], axis=1), 4, axis=1)
        worst = 0.0
        for _ in range(4):
            cp = c8 + SPLINE_BOUND * scale * rng.choice([-1.0, 1.0], c8.shape)
            worst = max(worst, abs(R.propagate_profile(x, cp[:, :4], cp[:, 4:], *pt, spr=4.0) - P4))
        rec["dP_spline"] = float(worst)
        out["cases"].append(rec)
        print(name, rec["P"][:18], rec["e_ref"], rec["steps"], rec["dP_spline"], flush=True)
    with open(os.path.join(HERE, "golden_profile_exact.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
