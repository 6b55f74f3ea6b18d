"""High-precision reference of the A/V z-sum (TEST INFRASTRUCTURE; mpmath, 60 digits):

    F(c)   = sum_k omega_k e^(c gamma4_k),  c = -(I_p/6) e^yh,  yh = clamp(y, -50, 50)   fpy:161-164
    A/V(y) = (I_p/2)(beta/v_w) e^yh F(c)  for y <= 50, else 0                             fpy:158-165

and the tolerance with which the kernels (csrc/lzq_quad.h zsum / zsum_dispatch, the exponential
of csrc/lzq_exp2.h) are compared with it.  The tables z, gamma4, omega are the doubles the
library builds on the host (_native.ztables, lzq_ztables: no GPU) and sums on the device; they are
taken as exact numbers, so the comparison measures the kernel's exponential and accumulation and
not the cancellation inside gamma4 (fpy:156).

The tolerance is derived, not tuned.  Relative part, in units of u = 2^-53:

    exponential   table: the minimax bound of the default table form, TAB_VARIANTS[DEFAULT_TAB] of
                  tests/test_exp2_host.py (1.73e-14); poly11: 1 ulp = 2 u
    c2            K_C * S * u.  S(c) = sum omega |c gamma4| e^(c gamma4) / F is the factor by which
                  a relative error of c becomes one of F.  K_C = 7 counts the roundings between y
                  and c2N: exp_sc <= 1 ulp (2), the quotient I_p/6 (1), its product with e^y (1),
                  the rounding of the constant log2(e) (1), the product with it (1), and the one
                  rounding of the argument reduction (1); the scaling by N = 2^13 is exact
    prefactor     K_P * u, K_P = 12: H_std's sqrt and four products/quotients (5), beta = B H_p (1),
                  beta / v_w (1), the product with I_p/2 (1), exp_sc (2), pref0 * e^y (1) and the
                  product with F (1).  Absent (0) where F itself is compared
    accumulation  4 * acc, acc MEASURED against this reference (not the worst case nz * u, which at
                  nz = 1200 is 1.3e-13 and would swallow the exponential's bound): the relative
                  error of a plain left-to-right FP64 sum of the correctly rounded terms (numpy, no
                  project code) against the mpmath sum, worst over the same y set on the same grid;
                  the factor 4 covers the random-walk spread between summation orders and the
                  kernel's own per-term roundings (table entry, polynomial, product)

Absolute part, for results in the subnormal range: every accumulate of a term above 2^-1074
rounds on the subnormal grid, so scale * m * 2^-1074 with m the number of such nodes and scale the
prefactor pref0 e^yh (1 for F), plus one subnormal ulp 2^-1074 for the rounding of the product
with the prefactor.  Where the reference F is below half the smallest subnormal, 2^-1075, every
term is, each accumulate rounds to the sum it started from, and the kernel must return exactly 0.
"""
import math

import mpmath as mp
import numpy as np

from conftest import pkg
from test_exp2_host import DEFAULT_TAB, TAB_VARIANTS

DPS = 60
U = 2.0 ** -53
K_C = 7
K_P = 12
ACC_MARGIN = 4
LOG2E = float.fromhex("0x1.71547652b82fep0")   # lzq::kLog2E (csrc/lzq_exp2.h), the double the kernels multiply by
CLAMP_OCT, SAT_OCT, DEAD_OCT = 1506.0, 2.0 ** 31, 1077.0   # lzq_exp2.h kTabKMin, int32, lzq_quad.h dead rule
VARIANTS = ("table", "poly11")
# (nz, z_max) of the GPU tests: the default grid, two padded ones (13 -> 16, 5 -> 8), two fine ones
GRIDS = ((1200, 30.0), (13, 3.0), (5, 7.5), (2400, 30.0), (12000, 30.0))


def exp_term(variant):
    return TAB_VARIANTS[DEFAULT_TAB] if variant == "table" else 2 * U


class Grid:
    """The host tables of one (nz, z_max) and what the tests derive from them."""

    def __init__(self, nz, z_max):
        self.nz, self.z_max = nz, z_max
        self.z, self.g4, self.om = pkg("_native").ztables(nz, z_max)
        with mp.workdps(DPS):
            self.g4_mp = [mp.mpf(float(x)) for x in self.g4]
            self.om_mp = [mp.mpf(float(x)) for x in self.om]
        self.cache = {}

    def boundaries(self, I_p):
        """y of the regime changes of the shipped kernel on this grid: clamp onset, saturation of
        poly11's integer conversion, the dead-lane threshold."""
        k = LOG2E * (I_p / 6.0)
        return (math.log(CLAMP_OCT / (k * self.g4[-1])), math.log(SAT_OCT / (k * self.g4[-1])),
                math.log(DEAD_OCT / (k * self.g4[1])))


_grids = {}


def grid(nz, z_max):
    key = (int(nz), float(z_max))
    if key not in _grids:
        _grids[key] = Grid(*key)
    return _grids[key]


class Ref:
    __slots__ = ("y", "F", "S", "m", "plain")


def c_of_y(I_p, y):
    """c = -(I_p/6) e^yh as an mp number (inside a workdps context)."""
    yh = min(max(mp.mpf(y), mp.mpf(-50)), mp.mpf(50))
    return -(mp.mpf(float(I_p)) / 6) * mp.exp(yh)


def f_ref(c, g):
    """(F, S, m, plain) of the grid g at the mp number c <= 0: the sum, its sensitivity to c, the
    number of nodes whose term exceeds 2^-1074, and the left-to-right FP64 sum of the correctly
    rounded terms (the accumulation measurement).  Terms with c gamma4 < -1200 ln 2 are exact zeros
    at every tolerance here; gamma4 is non-decreasing (lzq_ztables refuses other grids), so the
    loop stops at the first."""
    cut = -1200 * mp.log(2)
    tiny = mp.ldexp(1, -1074)
    F = W = mp.mpf(0)
    m = 0
    plain = 0.0
    for gk, wk in zip(g.g4_mp, g.om_mp):
        x = c * gk
        if x < cut:
            break
        t = wk * mp.exp(x)
        F += t
        W -= t * x
        m += t > tiny
        plain += float(t)
    return F, (W / F if F > 0 else mp.mpf(0)), m, plain


def ref_at(g, I_p, y):
    """The reference of F at one y (cached per grid: the variants and tests share it)."""
    key = (float(I_p), y if isinstance(y, float) else mp.nstr(y, 50))   # y: a double, or an mp number
    r = g.cache.get(key)
    if r is None:
        with mp.workdps(DPS):
            r = Ref()
            r.y = float(y)
            r.F, S, r.m, r.plain = f_ref(c_of_y(I_p, y), g)
            r.S = float(S)
        g.cache[key] = r
    return r


def refs_for(g, I_p, ys):
    return [ref_at(g, I_p, y) for y in ys]


def accumulation(refs):
    """Measured accumulation error of the y set: worst relative error of the plain FP64 sum against
    the mp sum, over the results in the normal range."""
    worst = 0.0
    with mp.workdps(DPS):
        for r in refs:
            if r.F > mp.ldexp(1, -1000):
                worst = max(worst, float(abs(mp.mpf(r.plain) - r.F) / r.F))
    return worst


def kernel_constants(kernel):
    """(pref0, I_p) of AoverVKernel(I_p, beta_over_H, T_p, v_w, g_star) as mp numbers, fpy:146-151
    and fpy:162 with the constants of csrc/lzq_physics.h / physics_host.py from their doubles."""
    ph = pkg("physics_host")
    I_p, B, Tp, g_star = (mp.mpf(float(kernel[k])) for k in ("I_p", "beta_over_H", "T_p_GeV", "g_star"))
    v_w = max(mp.mpf(float(kernel["v_w"])), mp.mpf(1e-12))
    H_p = mp.mpf(1.66) * mp.sqrt(g_star) * Tp * Tp / mp.mpf(ph.M_PL_GEV)
    return (I_p / 2) * (B * H_p / v_w), I_p


def av_ref(kernel, ys, g):
    """[(A/V as mp, Ref, scale = pref0 e^yh as mp)] at every y; A/V = 0 and scale = None for y > 50."""
    out = []
    with mp.workdps(DPS):
        pref0, _ = kernel_constants(kernel)
        for y in ys:
            r = ref_at(g, kernel["I_p"], y)
            if y > 50.0:
                out.append((mp.mpf(0), r, None))
                continue
            yh = min(max(mp.mpf(y), mp.mpf(-50)), mp.mpf(50))
            sc = pref0 * mp.exp(yh)
            out.append((sc * r.F, r, sc))
    return out


def tol(variant, S, acc, prefactor=True, extra_rel=0.0):
    """The relative tolerance (module docstring)."""
    return exp_term(variant) + K_C * S * U + (K_P * U if prefactor else 0.0) + ACC_MARGIN * acc + extra_rel


def compare(got, items, variant, acc, extra_rel=None):
    """got[i] against items[i] = (value, Ref, scale) (av_ref's rows; scale = 1 and value = Ref.F where F
    itself is compared, prefactor absent).  Returns (worst relative error over the normal-range
    results, worst error / tolerance, list of failures); a failure is (y, got, reference, tolerance
    or a reason)."""
    worst = ratio = 0.0
    bad = []
    with mp.workdps(DPS):
        half = mp.ldexp(1, -1075)
        for i, (x, (val, r, sc)) in enumerate(zip(got, items)):
            x = float(x)
            if sc is None or r.F < half:            # y > 50, or every term below half a subnormal
                if x != 0.0 or math.copysign(1.0, x) < 0:
                    bad.append((r.y, x, 0.0, "must be exactly +0"))
                continue
            if not math.isfinite(x):
                bad.append((r.y, x, float(val), "not finite"))
                ratio = math.inf
                continue
            pre = sc != 1
            rel = tol(variant, r.S, acc, prefactor=pre, extra_rel=0.0 if extra_rel is None else extra_rel[i])
            t = rel * val + sc * r.m * mp.ldexp(1, -1074) + (mp.ldexp(1, -1074) if pre else 0)
            e = abs(mp.mpf(x) - val)
            q = float(e / t)
            ratio = max(ratio, q)
            if val > mp.ldexp(1, -1000):
                worst = max(worst, float(e / val))
            if q > 1.0:
                bad.append((r.y, x, float(val), float(t / val)))
    return worst, ratio, bad


def f_items(refs):
    """compare()'s rows for F itself."""
    return [(r.F, r, 1) for r in refs]


def y_set(g, I_p, density=1):
    """The y values of the A/V comparison on grid g (module order, NOT sorted: 64 consecutive
    values share a wavefront in aov_kernel, so the waves are of mixed composition).  density
    thins the sets on the fine grids so that the reference keeps to its time."""
    y_clamp, y_sat, y_dead = g.boundaries(I_p)
    d = max(1, int(density))
    sub = [y_dead + math.log(o / DEAD_OCT) for o in np.linspace(1000.0, 1076.5, max(4, 12 // d))]
    ys = [-60.0, -50.0, math.nextafter(-50.0, -math.inf), math.nextafter(-50.0, math.inf)]
    ys += list(np.arange(-50.0, 8.01, 2.0 * d))                                    # coarse ladder
    ys += list(np.linspace(y_clamp - 0.5, y_clamp + 0.5, 32 // d))
    ys += list(np.linspace(y_sat - 0.25, y_sat + 0.25, 16 // d))
    ys += list(np.linspace(y_dead - 2.0, y_dead + 0.2, 64 // d))
    ys += [math.nextafter(y_dead, -math.inf), y_dead, math.nextafter(y_dead, math.inf)]
    ys += sub                                                                       # A/V subnormal
    ys += [50.0, math.nextafter(50.0, math.inf), 60.0]
    return [float(y) for y in ys]


def density_of(nz):
    return 1 if nz <= 1200 else (2 if nz <= 2400 else 4)


# ---------------------------------------------------------------------------------------------
# the y sets of the F-table and ODE-knot tests (shared by the GPU tests and the host model's)
# ---------------------------------------------------------------------------------------------
NY_MIN = 2000  # LZQ_NY_MIN (include/lzq.h)
# the y-grid runs from the -80 clip to the +50 clip: 32 passes of 64 lanes, each with its own
# truncation end, crossing every regime
FT_WINDOW = {"beta_over_H": 200.0, "T_max_over_Tp": 1.0e3, "T_min_over_Tp": 0.1}
ODE_WINDOW = {"T_min_over_Tp": 0.78, "T_max_over_Tp": 0.90}   # y from 32 down to 12: crosses y_dead
ODE_NT = 200                                                  # knots: not a multiple of 64


def ft_ygrid(c, n_y=NY_MIN):
    """numpy restatement of quad_setup's y-grid and c for the config c at n_y nodes (at least
    LZQ_NY_MIN, fpy:246; csrc/lzq_quad.h; fpy:234-247): (y_lo, y_hi, cneg, ys)."""
    n = max(int(n_y), NY_MIN)
    Tp, B = c["T_p_GeV"], c["beta_over_H"]

    def y_of_T(T):
        q = Tp / max(T, 1e-30)
        return 0.5 * B * (q * q - 1.0)

    y_lo = max(y_of_T(c["T_max_over_Tp"] * Tp), -80.0)
    y_hi = min(y_of_T(c["T_min_over_Tp"] * Tp), 50.0)
    step = (y_hi - y_lo) / float(n - 1)
    ys = np.arange(n, dtype=np.float64) * step + y_lo
    ys[-1] = y_hi
    return y_lo, y_hi, -(c["I_p"] / 6.0), ys


def ft_pick(g, I_p, ys):
    """The nodes of the F table that are compared with the reference: every 16th, the last, and
    all inside the three transition zones of grid g."""
    y_clamp, y_sat, y_dead = g.boundaries(I_p)
    pick = (np.arange(ys.size) % 16 == 0) | (np.abs(ys - y_clamp) <= 0.5) | (np.abs(ys - y_sat) <= 0.25) \
        | ((ys >= y_dead - 2.0) & (ys <= y_dead + 0.2))
    pick[-1] = True
    return np.nonzero(pick)[0]


def ode_knot_y(c, nt=ODE_NT):
    """(T, T_p / T, y) at the nt knots of build_tables' linspace(T_lo, T_hi, nt) over main()'s window
    of config c, in the device's operations (lzq_physics.h linspace_at, y_of_T)."""
    Tp, B = c["T_p_GeV"], c["beta_over_H"]
    T_lo, T_hi = c["T_min_over_Tp"] * Tp, c["T_max_over_Tp"] * Tp
    step = (T_hi - T_lo) / float(nt - 1)
    Ts = np.arange(nt, dtype=np.float64) * step + T_lo
    Ts[-1] = T_hi
    q = Tp / np.maximum(Ts, 1e-30)
    return Ts, q, 0.5 * B * (q * q - 1.0)
