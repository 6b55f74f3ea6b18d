"""Profiles shared by the exact-reference tests of the bounce-profile path (TEST INFRASTRUCTURE):
tests/test_gpu_profile_exact.py, tests/test_profile_exact_host.py and
tests/golden/make_golden_profile_exact.py build their inputs here, so host and GPU tests see the
same rows."""
from fractions import Fraction

import numpy as np

import profile_ref as R

COUPLINGS = [(1.0, 1.1, 0.2, 0.3, 0), (0.8, 1.5, 0.05, 0.6, 1), (1.6, 0.9, 0.4, 0.2, 0), (1.2, 1.2, 1.0, 0.9, 1)]
KNOT_COUNTS = (6, 7, 16, 29)
PER_COUNT = 512


def wiggly(n, seed, span=6.0):
    """tests/test_gpu_profile.py wiggly: tanh walls plus a smooth bump train, non-uniform knots."""
    rng = np.random.default_rng(seed)
    x = np.linspace(-span, span, n)
    x[1:-1] += rng.uniform(-0.3, 0.3, n - 2) * (x[1] - x[0])
    phi = 0.5 * (1.0 - np.tanh(x)) + 0.3
    Phi = 0.5 * (1.0 + np.tanh(x - 0.5)) + 0.6 * np.sin(2.3 * x + rng.uniform(0, 6))
    return x, phi, Phi


def rows8(x, phi, Phi):
    """The 8-double interval rows (phi c0..c3, Phi c0..c3) of scipy's not-a-knot splines."""
    return np.ascontiguousarray(np.concatenate([R.spline_coefs(x, phi), R.spline_coefs(x, Phi)], axis=1))


def rows_D(coef8, yB, ychi):
    """Delta rows as the kernel's interval_coefs forms them (no contraction): y_B phi_k - y_chi Phi_k."""
    return yB * coef8[:, :4] - ychi * coef8[:, 4:]


def knot_zero_profile(rng, n):
    """A tanh wall whose Delta vanishes on interior knot k to rounding: Phi is shifted so that
    y_B phi[k] - y_chi Phi[k] ~ 0.  Draw order: w, (y_B, y_chi), k."""
    x = np.linspace(-3, 3, n)
    w = rng.uniform(0.5, 2)
    yB, ychi = rng.uniform(0.5, 2, 2)
    k = int(rng.integers(1, n - 1))
    phi = 0.5 * (1 - np.tanh(x / w)) + 0.1
    Phi = 0.5 * (1 + np.tanh((x - 0.3) / w)) + 0.05
    Phi = Phi + (yB * phi[k] / ychi - Phi[k])
    return x, phi, Phi, float(yB), float(ychi), k


def knot_zero_seeded(count=3000):
    """The seeded set of the pre-fix defect: default_rng(1), n = integers(6, 30) drawn first."""
    rng = np.random.default_rng(1)
    for _ in range(count):
        yield knot_zero_profile(rng, int(rng.integers(6, 30)))


def knot_zero_batches():
    """The GPU batches: default_rng(1), KNOT_COUNTS x PER_COUNT shapes, one point each."""
    rng = np.random.default_rng(1)
    return {n: [knot_zero_profile(rng, n) for _ in range(PER_COUNT)] for n in KNOT_COUNTS}


def end_signs(x, coef8, yB, ychi):
    """Signs of Delta at the two ends (exact on the rows): (first row at 0, last row at L)."""
    D = [[Fraction(yB) * Fraction(float(r[k])) - Fraction(ychi) * Fraction(float(r[4 + k])) for k in range(4)]
         for r in (coef8[0], coef8[-1])]
    L = Fraction(float(x[-1])) - Fraction(float(x[-2]))
    a, b = D[0][0], sum(c * L ** k for k, c in enumerate(D[1]))
    return (a > 0) - (a < 0), (b > 0) - (b < 0)


def step_angles2(x, c8, yB, ychi, lam, vw, spr):
    """|n|^2 of every Magnus step the restatement takes (what the kernel's cos_sinc_step branches on)."""
    cD, cM = R.dm_coefs(c8[:, :4], c8[:, 4:], yB, ychi, lam)
    out = []
    for j in range(len(x) - 1):
        S = R.interval_steps(x, c8[:, :4], c8[:, 4:], j, yB, ychi, lam, vw, spr)
        h = (x[j + 1] - x[j]) / S
        for i in range(S):
            a = [(R.pp_eval(cM[j], (i + g) * h), R.pp_eval(cD[j], (i + g) * h)) for g in R.GL3]
            out.append(sum(v * v for v in R.magnus6_vector(a[0], a[1], a[2], h / vw)))
    return np.array(out)


# ---- hand-built rows: y_B = 0, y_chi = -1, lambda = 1, so Delta is the Phi row and m the phi row,
# exactly.  Every coefficient is dyadic; m = 1.  (name, knots, Delta rows, expected [(xi, Delta')])
_T23 = 2.0 ** -23
HAND = [
    ("knot zero, sign change", [0, 1, 2, 3], [[-1, 1, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0]], [(1.0, 1.0)]),
    ("knot zero, no sign change", [0, 1, 2, 3], [[1, -2, 1, 0], [0, 0, 1, 0], [1, 2, 1, 0]], []),
    ("zeros on both end knots", [0, 1, 2, 3], [[0, 3, -1, 0], [2, 1, -1, 0], [2, -1, -1, 0]], []),
    ("zeros on both end knots, one crossing between", [0, 1, 2, 3],
     [[0, -4.5, 4.5, -1], [-1, 1.5, 1.5, -1], [1, 1.5, -1.5, -1]], [(1.5, 2.25)]),
    ("zero interval between + and -", [0, 1, 2, 3], [[1, -1, 0, 0], [0, 0, 0, 0], [0, -1, 0, 0]], [(1.0, -1.0)]),
    ("zero interval between + and +", [0, 1, 2, 3], [[1, -1, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0]], []),
    ("tangent double root", [0, 2, 4, 6], [[2, -3, 0, 1], [4, 0, 0, 0], [4, 0, 0, 0]], []),
    ("three simple roots", [0, 4, 8, 12], [[-6, 11, -6, 1], [6, 0, 0, 0], [6, 0, 0, 0]],
     [(1.0, 2.0), (2.0, -1.0), (3.0, 2.0)]),
    ("two roots 1.2e-7 L apart", [0, 1, 2, 3],
     [[0.25 + _T23 / 2, -(1 + _T23), 1, 0], [0.25 - _T23 / 2, 0, 0, 0], [0.25 - _T23 / 2, 0, 0, 0]],
     [(0.5, -_T23), (0.5 + _T23, _T23)]),
    ("quadratic, two roots", [0, 4, 8, 12], [[3, -4, 1, 0], [3, 0, 0, 0], [3, 0, 0, 0]], [(1.0, -2.0), (3.0, 2.0)]),
    ("linear", [0, 1, 2, 3], [[-1.5, 1, 0, 0], [-0.5, 1, 0, 0], [0.5, 1, 0, 0]], [(1.5, 1.0)]),
    ("knots near 1e6, spacing 2^-10", [1e6 + k / 1024 for k in range(4)],
     [[-1.25, 1024, 0, 0], [-0.25, 1024, 0, 0], [0.75, 1024, 0, 0]], [(1e6 + 1 / 1024 + 1 / 4096, 1024.0)]),
]
TRIPLE = ("triple root", [0, 2, 4, 6], [[-1, 3, -3, 1], [1, 0, 0, 0], [1, 0, 0, 0]])   # (t - 1)^3: by residual
HAND_VW = 0.5   # delta_LZ = m^2 / (2 v_w |Delta'|) = 1 / |Delta'|


def hand_rows8(rows):
    """8-double rows with phi = 1 (m = 1) and Phi = the given Delta rows."""
    d = np.asarray(rows, float)
    return np.ascontiguousarray(np.concatenate([np.tile([1.0, 0.0, 0.0, 0.0], (len(d), 1)), d], axis=1))
