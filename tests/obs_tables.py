"""What the observable tests share (tests/test_obs_host.py, tests/test_gpu_obs.py): axis
shorthands, the special values, and a synthetic table of yield records with them salted in."""
import numpy as np

INF, NAN = float("inf"), float("nan")
TERM = {"field": "Y_B", "target": 1.0, "sigma": 0.5}
DOWN = lambda x: float(np.nextafter(x, -np.inf))


def lin(field, lo, hi, bins):
    return {"field": field, "lo": lo, "hi": hi, "bins": bins}


def log(field, lo, hi, per_octave):
    return {"field": field, "lo": lo, "hi": hi, "per_octave": per_octave}


# range ends, the values just below them, octave edges, a value whose linear product rounds up to
# the bin count (0.9 of 9 bins), zeros of both signs, a subnormal, the smallest normal, non-finite
SPECIALS = [0.0, -0.0, 5e-324, 2.2250738585072014e-308, NAN, INF, -INF, 1e300, -1e300, 0.01, 1000.0, DOWN(1000.0),
            DOWN(0.01), 1.0, 2.0, DOWN(2.0), 10.0, DOWN(10.0), 2e-10, DOWN(2e-10), 1e-10, 0.9, DOWN(0.9)]

# 133 + 200 cells, 20,000 cells (more than a block keeps: straight to global memory), 2-D log x linear
SALTED_OBS = ([log("DM_over_B", 0.01, 1000.0, 8)], [lin("Y_chi", 0.0, 2e-10, 200)],
              [lin("Y_chi", 0.0, 2e-10, 200), lin("DM_over_B", 0.0, 10.0, 100)],
              [log("rho_B_kg_m3", 1e-12, 1e3, 2), lin("P_used", -1.0, 0.9, 9)])


def salted_table(n=20_000, seed=3):
    """Rows drawn over many decades (both signs), with the special values salted into every column
    but the first, whose chi2 under TERM is uniform in [0, 150) with NaN, inf and overflow planted."""
    rng = np.random.default_rng(seed)
    t = 10.0 ** rng.uniform(-14.0, 4.0, (n, 6)) * np.where(rng.random((n, 6)) < 0.1, -1.0, 1.0)
    t[:, 0] = 1.0 + 0.5 * np.sqrt(rng.uniform(0.0, 150.0, n))
    t[:, 1] = rng.uniform(0.0, 2.2e-10, n)                              # a linear axis's range and a little more
    t[::3, 4] = rng.uniform(-1.0, 11.0, t[::3].shape[0])                # and the other's
    k = min(40, n // (2 * len(SPECIALS)))
    for j in range(1, 6):
        at = rng.choice(n, k * len(SPECIALS), replace=False)
        t[at, j] = np.tile(SPECIALS, k)
    bad = rng.choice(n, n // 25, replace=False)
    t[bad[0::3], 0], t[bad[1::3], 0], t[bad[2::3], 0] = NAN, INF, 1e300
    return t
