"""High-precision reference of the Y_B y-quadrature and of the epilogue (TEST INFRASTRUCTURE; mpmath,
60 digits), with F_j GIVEN: everything yb_wave / reuse_wave (csrc/lzq_quad.h) do with the z-sums once
they exist, fpy:247-267, and epilogue_pre / epilogue_finish, fpy:372-384, 413-417.

    y_j      the device's nodes, numpy.linspace(y_lo, y_hi, n) (zsum_ref.ft_ygrid), taken as exact
    w_j      (y_{j+1} - y_{j-1}) / 2, one-sided and halved at the two ends                      fpy:267
    d_j      max(1 + 2 y_j / B, 1e-12),  T_j = T_p / sqrt(d_j),  |dT/dy| = (T_p / B) d_j^-1.5   fpy:252-255
    I_j      P J(T) pref0 e^clip(y, -50, 50) F_j / (s H T) |dT/dy|, 0 for y > 50                fpy:158-165, 258-265
    W_j      exp(-(y_j / max(sigma, 1e-6))^2 / 2)                                               fpy:262
    Y_B      sum_j w_j I_j W_j

F_j are doubles handed in and taken as exact, as zsum_ref.py takes the z tables: on the GPU they are the
device's own (the table lzq_sweep_grid_ztables builds), so the comparison measures the per-y arithmetic,
the weights, the lane sums and the butterfly, and not the z-sum (pinned by tests/test_gpu_zsum.py).  The
constants are the doubles of csrc/lzq_physics.h / physics_host.py; J's branch T > m/3 is decided on the
exact T.

The tolerance is derived, not tuned.  u = 2^-53; "1 ulp" is counted as 2 u.

Relative part of one node's term w_j I_j W_j, by counting the roundings of y_factors, integrand_from and
y_weight in the device's operation order (documented bounds: exp_sc 1 ulp, rsqrt_pos 2 ulp, sqrt and
every +, *, / correctly rounded; a product of k rounded factors adds their errors and k - 1):

    pexp   = pref0 e^y     H_p = 1.66 sqrt(g*) T_p T_p / M_Pl (5), beta (1), / v_w (1), * (I_p/2) (1),
                           exp_sc (2), the product (1)                                                  11
    Av     = pexp F        the product                                                                  12
    T      = T_p rs        its own product (1); rs's error is the common mode below
    T3     = (T T) T       two products and three T                                                      5
    n_eq   = c_rel T3      c_rel: pi pi, 3 zeta3, the quotient, g (4); the product (1); T3 (5)          10
    PJ     = P (flux/4 n_eq vbar)   flux/4 and vbar = 1 are exact: two products                         12
    SB     = PJ Av W       two products (W's own error is the window part below)                        26
    H      = H0 T T / M_Pl H0 (2), two products and two T (4), 1/M_Pl (1), the product (1)               8
    sE     = s0 T3         s0: pi pi, / 45, g*s (3); the product (1); T3 (5)                             9
    sHT    = sE H T        two products and one T                                                       20
    |dT/dy|= dT0 rs rs rs  dT0 (1), two products, the product with dT0                                   4
    I      = SB / sHT |dT/dy|   the quotient and the product                                            52
    w      = (dl + dr) / 2 dl and dr round by at most u of themselves, their sum once; halving exact     2
    fma(w, I, acc)         one rounding                                                      K_REL  =   55

Non-relativistic nodes (T <= m/3) replace n_eq and vbar:

    c_nr   = g x sqrt(x), x = m / (2 pi)      the quotient (1) enters 1.5 times, sqrt, product, g       4.5
    T sqrt T               T 1.5 times, sqrt, product                                                   3.5
    exp_sc(-m/T)           its value (2); its ARGUMENT is the K_X term below
    n_eq                   two products                                                                 12
    vbar   = sqrt(8 T / v0)   v0 = pi m (1), the quotient (1), T (1), halved by the sqrt, sqrt (1)      2.5
    PJ                     three products                                                               17.5
                                                                                             K_NR   =   60.5

Amplified parts.  rs = rsqrt_pos(d) carries two errors that are common to every factor it enters: its own
4 u and half the relative error of d, where d = fl(1 + fl(2y/B)) is wrong by u (1 + A), A = |2y/B| / d
(the cancellation in 1 + 2y/B; A = 0 on the 1e-12 floor, which is exact).  The term depends on rs as

    relativistic       T^3 / T^6 * rs^3            = rs^0:   the term is analytically independent of d,
    non-relativistic   T^2 e^(-m/T) / T^6 * rs^3   = rs^(X - 1), X = m/T.

This independence IS used for the two common-mode errors of rs on relativistic nodes (they cancel to first
order; the second order, 72 eps^2 -- (X^2/2 + 72) eps^2 on a non-relativistic node --, is added) and is NOT
used for anything else: every T above is counted with its own rounding as if the factors were independent.
On non-relativistic nodes the exponent X - 1 is used as it stands, so

    K_X  = 6.5   X u:   the quotient m/T (1), T's own product (1), rs's 4 u and d's own u/2 through X - 1 <= X
    K_D  = 0.5   (X - 1) A u:  the cancellation's share, the only part 1/d multiplies: "sensitivity / denom"
                 with sensitivity (X - 1) |2y/B|; on a relativistic node the sensitivity is 0
    K_W  = 5     (q^2/2) u where the Gaussian is in play: 1/sigma (1), y/sigma (1), twice in q q, the square (1);
                 plus 2 u for exp_sc's value.  A window that is exactly 1 (a plateau over the grid, a node
                 probe at its own node) adds nothing.
    |y| does not appear: e^y's argument is the exact double y, clipped exactly, and the c of F is in F.

So on an amplification-free node the relative tolerance is 55 u (6.1e-15) and never more than K_NR = 60.5 u,
below the 128 u this module asserts as its cap; K_X <= 8 is asserted too.

Absolute part, for the subnormal range.  Every intermediate the device rounds -- exp_sc(-m/T), n_eq,
flux/4 n_eq, J, P J, pexp, A/V, PJ Av, W, SB, the quotient, I and w I -- whose exact value v lies below
2^-1022 is rounded on the subnormal grid, an error of up to 2^-1074, which reaches the term multiplied by
every factor applied afterwards: 2^-1074 (term / v) is added for each.  Where F_j = 0, or the exact
exp(-m/T) of a non-relativistic node or the exact W is below 2^-1075, the device's term must be exactly
+0 (exp_sc returns 0 there and every later product keeps it).

Sums.  The node tolerances add (the terms are non-negative), plus ACC_MARGIN = 4 times the MEASURED
accumulation error: |plain - exact| with plain the left-to-right FP64 sum of the correctly rounded terms,
on the same case (zsum_ref.py's rule; the device adds per lane and then over 64 lanes).

No node is left out: each is compared relatively with its absolute part, or for an exact zero.  A node
whose exact T lies within 2^-40 of m/3, whose exact d within 2^-40 of the floor, or whose exponential
within 1e-9 of the 2^-1075 threshold cannot be decided between device and reference: Nodes.undecided lists
them and the case list must have none (asserted where the cases are built).
"""
import math

import mpmath as mp
import numpy as np

import zsum_ref as Z
from conftest import BASE_CFG, full_cfg, pkg

DPS = Z.DPS
U = Z.U
ACC_MARGIN = Z.ACC_MARGIN
K_REL, K_NR, K_X, K_D, K_W, K_WEXP = 55.0, 60.5, 6.5, 0.5, 5.0, 2.0
CAP_U = 128.0
assert max(K_REL, K_NR) <= CAP_U and K_X <= 8.0
UNDECIDED = 2.0 ** -40
# csrc/lzq_physics.h (fpy:33-39); tests/test_yquad_host.py reads them back from the header
ZETA3, S0_M3, GEV_TO_KG, M_PROTON_KG = 1.202056903159594, 2891.0 * 1e6, 1.78266192e-27, 1.67262192369e-27

ZGRID = (13, 3.0)                  # F is an input: the z grid is immaterial
NY = 2000
NYS_MORE = (2048, 2049, 2050, 2113, 4000)   # the end of the grid on a pass boundary, 1 and 2 past, inside a group
CASES = {
    "shipped": {},
    "clips": dict(Z.FT_WINDOW),
    "heavy": {"m_chi_GeV": 3000.0},
    "branch": {"m_chi_GeV": 600.7},
    "underflow": {"m_chi_GeV": 6e4},
    "dead source": {"m_chi_GeV": 1e6},
    "small denom": {"beta_over_H": 60.0, "T_max_over_Tp": 30.0, "T_min_over_Tp": 0.05, "m_chi_GeV": 1e5},
    "denom floor": {"T_max_over_Tp": 1e7},
    "low B": {"beta_over_H": 1.0, "T_max_over_Tp": 30.0, "T_min_over_Tp": 0.05, "m_chi_GeV": 100.0},
    "narrow": {"T_max_over_Tp": 1.1, "T_min_over_Tp": 0.9},
}
MULTI_NY = ("shipped", "branch")   # the cases that also run at NYS_MORE
DEFECTS = {"a": "first and last weights not halved", "b": "the last node counted once more",
           "c": "e^y without the +-50 clip", "d": "reciprocal square root off by 2^-43",
           "e": "exponential's series stopped at r^9", "f": "one lane dropped from the 64-lane sum"}


def cfg_of(case, **over):
    return full_cfg({**BASE_CFG, **CASES[case], **over})


def ygrid(c, n_y=NY):
    """(y_lo, y_hi, step, ys): the device's y-grid (quad_setup, y_node) in numpy doubles."""
    y_lo, y_hi, _, ys = Z.ft_ygrid(c, n_y)
    return y_lo, y_hi, (y_hi - y_lo) / float(ys.size - 1), ys


def probe_indices(n):
    """The probed nodes: every one at NY, else the first 65, the last 130 and every 16th between."""
    if n == NY:
        return np.arange(n)
    j = np.arange(n)
    return j[(j < 65) | (j >= n - 130) | (j % 16 == 0)]


def host_F(c, ys, nz=ZGRID[0], z_max=ZGRID[1]):
    """F_j in plain numpy doubles from the library's host tables (any doubles do: F is an input)."""
    _, g4, om = pkg("_native").ztables(nz, z_max)
    cc = -(c["I_p"] / 6.0) * np.exp(np.clip(ys, -50.0, 50.0))
    return np.array([float(np.sum(om * np.exp(x * g4))) for x in cc])


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
class Nodes:
    """Per node of one (config, n_y, F): the exact term without the window R0 = w I (mp), the
    relative tolerance without the window part, what the absolute part needs, and the flags."""


def _mpf(x):
    return mp.mpf(float(x))


def nodes_ref(c, ys, F):
    with mp.workdps(DPS):
        ph = pkg("physics_host")
        pi, zeta = mp.mpf(ph.PI), mp.mpf(ZETA3)
        pref0, _ = Z.kernel_constants(c)
        B, Tp, m, g = max(_mpf(c["beta_over_H"]), mp.mpf(1e-30)), _mpf(c["T_p_GeV"]), _mpf(c["m_chi_GeV"]), _mpf(c["g_chi"])
        m3 = m / 3
        H0 = mp.mpf(1.66) * mp.sqrt(_mpf(c["g_star"])) / mp.mpf(ph.M_PL_GEV)
        s0 = 2 * pi * pi / 45 * _mpf(c["g_star_s"])
        fermion = str(c["chi_stats"]).lower().startswith("ferm")
        c_rel = g * (3 * zeta / (4 * pi * pi)) if fermion else g * (zeta / (pi * pi))
        x = m / (2 * pi)
        c_nr = g * x * mp.sqrt(x)
        v0 = pi * max(m, mp.mpf(1e-20))
        flux4, P, dT0 = _mpf(c["incident_flux_scale"]) / 4, _mpf(c["P_chi_to_B"]), Tp / B
        floor, half, minn = mp.mpf(1e-12), mp.ldexp(1, -1075), mp.ldexp(1, -1022)
        x_zero = -mp.log(half)                      # exp(-X) < 2^-1075  <=>  X > 1075 ln 2
        n = len(ys)
        ymp = [_mpf(y) for y in ys]
        nd = Nodes()
        nd.n, nd.ys = n, np.asarray(ys, dtype=np.float64)
        nd.R0, nd.rel0, nd.zero, nd.pre, nd.post = [], [], [], [], []
        nd.relativistic, nd.X, nd.denom, nd.undecided = np.zeros(n, bool), np.zeros(n), np.zeros(n), []
        nd.nearest_branch = math.inf
        for j in range(n):
            y = ymp[j]
            w = (ymp[min(j + 1, n - 1)] - ymp[max(j - 1, 0)]) / 2
            raw = 1 + 2 * y / B
            floored = raw <= floor
            d = floor if floored else raw
            if abs(raw / floor - 1) < UNDECIDED:
                nd.undecided.append((j, "denom floor", float(raw)))
            A = 0.0 if floored else float(abs(2 * y / B) / d)
            rs = 1 / mp.sqrt(d)
            T = Tp * rs
            adT = dT0 * rs ** 3
            sHT = s0 * T ** 3 * (H0 * T * T) * T
            dist = float(abs(T / m3 - 1))
            nd.nearest_branch = min(nd.nearest_branch, dist)
            if dist < UNDECIDED:
                nd.undecided.append((j, "T = m/3", dist))
            rel = T > m3
            Fj = _mpf(F[j])
            pexp = pref0 * mp.exp(min(max(y, mp.mpf(-50)), mp.mpf(50)))
            Av = pexp * Fj if y <= 50 else mp.mpf(0)
            zero = Av == 0
            chain = [pexp, Av]
            if rel:
                X = 0.0
                n_eq = c_rel * T ** 3
                chain += [n_eq, flux4 * n_eq]
                J = flux4 * n_eq
                tol = K_REL * U
                eps = (4.0 + 0.5 * (1.0 + A)) * U
                tol += 72.0 * eps * eps
            else:
                Xm = m / T
                X = float(Xm)
                if abs(Xm / x_zero - 1) < 1e-9:
                    nd.undecided.append((j, "exp(-m/T) at 2^-1075", X))
                e = mp.exp(-Xm)
                zero = zero or e < half
                n_eq = c_nr * T * mp.sqrt(T) * e
                vbar = mp.sqrt(8 * T / v0)
                J = flux4 * n_eq * vbar
                chain += [e, n_eq, flux4 * n_eq, J]
                eps = (4.0 + 0.5 * (1.0 + A)) * U
                tol = K_NR * U + K_X * X * U + K_D * abs(X - 1.0) * A * U + (0.5 * X * X + 72.0) * eps * eps
            PJ = P * J
            SB1 = PJ * Av
            Q1 = SB1 / sHT
            I1 = Q1 * adT
            R0 = w * I1
            chain += [PJ, SB1]
            nd.relativistic[j], nd.X[j], nd.denom[j] = bool(rel), X, float(d)
            nd.zero.append(bool(zero))
            nd.R0.append(mp.mpf(0) if zero else R0)
            nd.rel0.append(tol)
            # absolute part: sum of term / v over the subnormal intermediates before the window, and the
            # later ones (each still to be multiplied by W) for window_abs
            nd.pre.append(mp.mpf(0) if zero else sum((1 / v for v in chain if v < minn), mp.mpf(0)))
            nd.post.append(None if zero else (SB1, Q1, I1, R0))
        return nd


class Win:
    """A window at the nodes: W (mp), its relative tolerance, and where it must be an exact zero.
    exact = True: W is 1 or 0 exactly and is rounded nowhere."""


def win_one(nd, only=None):
    """W = 1 at every node (a plateau over the whole grid), or at node `only` alone and exactly 0
    elsewhere (a node probe)."""
    w = Win()
    one, nul = mp.mpf(1), mp.mpf(0)
    w.W = [one if only is None or j == only else nul for j in range(nd.n)]
    w.rel = [0.0] * nd.n
    w.zero = [not (only is None or j == only) for j in range(nd.n)]
    w.exact, w.undecided = True, []
    return w


def win_gauss(nd, sigma):
    w = Win()
    w.W, w.rel, w.zero, w.undecided, w.exact = [], [], [], [], False
    with mp.workdps(DPS):
        sig = max(_mpf(sigma), mp.mpf(1e-6))
        half = mp.ldexp(1, -1075)
        x_zero = -mp.log(half)
        for j, y in enumerate(nd.ys):
            a = (_mpf(y) / sig) ** 2 / 2
            if a > 0 and abs(a / x_zero - 1) < 1e-9:
                w.undecided.append((j, "W at 2^-1075", float(a)))
            W = mp.exp(-a) if a < 4000 else mp.mpf(0)
            w.zero.append(W < half)
            w.W.append(W)
            w.rel.append((K_WEXP + K_W * float(min(a, 4000))) * U)
    return w


def node_tol(nd, win, j):
    """(exact term, tolerance) of node j under the window, both mp; (0, None): must be exactly +0."""
    if nd.zero[j] or win.zero[j]:
        return mp.mpf(0), None
    W = win.W[j]
    R = nd.R0[j] * W
    minn, tiny = mp.ldexp(1, -1022), mp.ldexp(1, -1074)
    ab = R * nd.pre[j]
    post = nd.post[j]
    if post[3] * W < minn or post[0] * W < minn or post[1] * W < minn or post[2] * W < minn or W < minn:
        # term / v for v = W, SB, the quotient, I, w I: the factors applied after each
        if W < minn and not win.exact:
            ab += nd.R0[j]
        for v1 in post:
            if v1 * W < minn:
                ab += nd.R0[j] / v1
    return R, (nd.rel0[j] + win.rel[j]) * R + tiny * ab


def is_pos_zero(x):
    return x == 0.0 and math.copysign(1.0, x) > 0


def compare_nodes(got, nd, win, idx=None, probe=False):
    """got[i] against the term of node idx[i] (all nodes if idx is None).  probe: the window is the
    node's own probe (W = 1 there).  Returns (worst relative error over the normal-range terms, worst
    error / tolerance, failures)."""
    idx = range(nd.n) if idx is None else idx
    worst = ratio = 0.0
    bad = []
    one = None
    with mp.workdps(DPS):
        if probe:
            one = win_one(nd)
        for x, j in zip(got, idx):
            x, j = float(x), int(j)
            R, t = node_tol(nd, one if probe else win, j)
            if t is None:
                if not is_pos_zero(x):
                    bad.append((j, nd.ys[j], x, 0.0, "must be exactly +0"))
                continue
            if not math.isfinite(x) or x < 0.0 or (x == 0.0 and not is_pos_zero(x)):
                bad.append((j, nd.ys[j], x, float(R), "NaN, negative or -0"))
                ratio = math.inf
                continue
            e = abs(mp.mpf(x) - R)
            q = float(e / t)
            ratio = max(ratio, q)
            if R > mp.ldexp(1, -1000):
                worst = max(worst, float(e / R))
            if q > 1.0:
                bad.append((j, nd.ys[j], x, float(R), float(t / R)))
    return worst, ratio, bad


def sum_ref(nd, win):
    """(exact sum, tolerance, measured accumulation error) of the case under the window, mp."""
    with mp.workdps(DPS):
        S = T = mp.mpf(0)
        plain = 0.0
        for j in range(nd.n):
            R, t = node_tol(nd, win, j)
            if t is None:
                continue
            S += R
            T += t
            plain += float(R)
        acc = abs(mp.mpf(plain) - S)
        return S, T + ACC_MARGIN * acc, acc


def compare_sum(x, ref):
    """(relative error, error / tolerance, failure or None) of the sum x against sum_ref's triple."""
    S, tol, _ = ref
    x = float(x)
    with mp.workdps(DPS):
        if S == 0:
            return 0.0, 0.0, None if is_pos_zero(x) else (x, 0.0, "must be exactly +0")
        if not math.isfinite(x) or x < 0.0:
            return math.inf, math.inf, (x, float(S), "NaN or negative")
        e = abs(mp.mpf(x) - S)
        q = float(e / tol)
        return float(e / S), q, None if q <= 1.0 else (x, float(S), float(tol / S))


# ---------------------------------------------------------------------------------------------
# a plain FP64 model of the same loop, with switchable seeded defects
# ---------------------------------------------------------------------------------------------
def _exp_r9(x):
    """exp with the Taylor series of exp_sc stopped at r^9: numpy's exp less the dropped terms
    r^10/10! .. r^13/13! (relative to e^r), r = x - round(x / ln 2) ln 2."""
    x = np.asarray(x, dtype=np.float64)
    r = x - np.rint(x / math.log(2.0)) * math.log(2.0)
    tail = sum(r ** i / math.factorial(i) for i in range(10, 14))
    return np.exp(x) * (1.0 - tail * np.exp(-r))


def model(c, ys, F, sigma=None, defect=None):
    """(terms w_j I_j W_j, Y_B) in numpy doubles, the formula in quad_setup's / y_factors' operation
    order, numpy's exp and sqrt; the sum per lane over the passes and then the xor butterfly of
    wave_sum.  sigma None: W = 1 exactly.  defect: a key of DEFECTS."""
    ph = pkg("physics_host")
    ex = _exp_r9 if defect == "e" else np.exp
    ys = np.asarray(ys, dtype=np.float64)
    n = ys.size
    B, Tp, m = c["beta_over_H"], c["T_p_GeV"], c["m_chi_GeV"]
    pi = ph.PI
    pref0 = (c["I_p"] / 2.0) * ((B * ph.H_std(Tp, c["g_star"])) / max(c["v_w"], 1e-12))
    Bc = max(B, 1e-30)
    dT0 = -(Tp / Bc)
    H0, s0 = 1.66 * math.sqrt(c["g_star"]), (2.0 * (pi * pi) / 45.0) * c["g_star_s"]
    fermion = str(c["chi_stats"]).lower().startswith("ferm")
    c_rel = c["g_chi"] * (3.0 * ZETA3 / (4.0 * (pi * pi))) if fermion else c["g_chi"] * (ZETA3 / (pi * pi))
    x = m / (2.0 * pi)
    c_nr = c["g_chi"] * (x * math.sqrt(x))
    v0 = pi * max(m, 1e-20)
    d = np.diff(ys)
    w = 0.5 * (np.concatenate([[0.0], d]) + np.concatenate([d, [0.0]]))
    if defect == "a":
        w[0], w[-1] = d[0], d[-1]
    expy = ex(ys if defect == "c" else np.clip(ys, -50.0, 50.0))
    denom = np.maximum(1.0 + 2.0 * ys / Bc, 1e-12)
    rs = 1.0 / np.sqrt(denom)
    if defect == "d":
        rs = rs * (1.0 + 2.0 ** -43)
    T = Tp * rs
    dTdy = dT0 * ((rs * rs) * rs)
    H = H0 * T * T * (1.0 / ph.M_PL_GEV)
    T3 = (T * T) * T
    sE = s0 * T3
    rel = T > m / 3.0
    with np.errstate(under="ignore"):
        n_nr = c_nr * (T * np.sqrt(T)) * ex(-m / np.maximum(T, 1e-30))
        n_eq = np.where(rel, c_rel * T3, n_nr)
        vbar = np.where(rel, 1.0, np.sqrt(np.maximum(8.0 * T / v0, 0.0)))
        PJ = c["P_chi_to_B"] * (c["incident_flux_scale"] * 0.25 * n_eq * vbar)
        if sigma is None:
            W = np.ones(n)
        else:
            q = ys * (1.0 / max(sigma, 1e-6))
            W = ex(-0.5 * (q * q))
        Av = np.where(ys > 50.0, 0.0, (pref0 * expy) * np.asarray(F, dtype=np.float64))
        terms = w * (PJ * Av * W / (sE * H * T) * np.abs(dTdy))
        lanes = np.zeros(64)
        for base in range(0, n, 64):
            t = terms[base:base + 64]
            lanes[:t.size] = lanes[:t.size] + t
        if defect == "b" and n % 64:
            lanes[n % 64] += terms[-1]          # the tail lane next to the last node, weight not zeroed
        if defect == "f":
            lanes[37] = 0.0
        for off in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[np.arange(64) ^ off]
    return terms, float(lanes[0])


# ---------------------------------------------------------------------------------------------
# the epilogue
# ---------------------------------------------------------------------------------------------
# Counted roundings (u); libm pow 2 ulp = 4 u, libm exp 1 ulp = 2 u (csrc/lzq_physics.h).  T_hi = fl(T_max T_p) (1).
#   rho_B   = (Y_B S0) m_p                                                                     2
#   Y_chi   thermal, relativistic: c_rel (4), pow(T, 3) (4 + 3), product (1); s: s0 (3), pow (4 + 3),
#           product (1); the quotient (1)                                                      24
#           thermal, non-relativistic: m/(2 pi) (1) through pow 1.5 (4 + 1.5), g (1); pow(T, 1.5) (4 + 1.5);
#           exp (2); two products; / s (11 + 1) = 28, and (m/T_hi) (quotient + T_hi) = 2 X
#           n_chi_at_Tp / s(T_p): s0 (3), pow (4), product (1), the quotient (1)                9
#           Y_chi_init and 1e-12: exact                                                         0
#   rho_DM  = (Y_chi S0) (m GeV_to_kg): Y_chi's and three products
#   DM/B    = rho_DM / max(rho_B, 1e-300): rho_DM's, rho_B's and the quotient
EPI_FIELDS = ("Y_chi", "rho_B_kg_m3", "rho_DM_kg_m3", "DM_over_B")


def epilogue_ref(c, Y_B):
    """{field: (value mp, relative tolerance)} from the device's Y_B as an exact double; None: an
    invalid regime (the four fields epilogue_finish sets and Y_chi are NaN)."""
    r = str(c["regime"]).lower()
    if not (r.startswith("therm") or r.startswith("non")):
        return None
    with mp.workdps(DPS):
        ph = pkg("physics_host")
        pi, zeta = mp.mpf(ph.PI), mp.mpf(ZETA3)
        Tp, m, g = _mpf(c["T_p_GeV"]), _mpf(c["m_chi_GeV"]), _mpf(c["g_chi"])
        s0 = 2 * pi * pi / 45 * _mpf(c["g_star_s"])
        if r.startswith("therm"):
            T = _mpf(c["T_max_over_Tp"]) * Tp
            dist = abs(T / (m / 3) - 1)
            assert dist == 0 or dist > UNDECIDED, "T_hi undecidably close to m/3"
            if T > m / 3:
                fermion = str(c["chi_stats"]).lower().startswith("ferm")
                c_rel = g * (3 * zeta / (4 * pi * pi)) if fermion else g * (zeta / (pi * pi))
                Ychi, ky = c_rel * T ** 3 / (s0 * T ** 3), 24.0
            else:
                x = m / (2 * pi)
                Ychi = g * x * mp.sqrt(x) * T * mp.sqrt(T) * mp.exp(-m / T) / (s0 * T ** 3)
                ky = 28.0 + 2.0 * float(m / T)
        elif c["Y_chi_init"] is not None:
            Ychi, ky = _mpf(c["Y_chi_init"]), 0.0
        elif c["n_chi_at_Tp_GeV3"] is not None:
            Ychi, ky = _mpf(c["n_chi_at_Tp_GeV3"]) / max(s0 * Tp ** 3, mp.mpf(1e-300)), 9.0
        else:
            Ychi, ky = mp.mpf(1e-12), 0.0
        S0 = mp.mpf(S0_M3)
        rho_B = _mpf(Y_B) * S0 * mp.mpf(M_PROTON_KG)
        rho_DM = Ychi * S0 * (m * mp.mpf(GEV_TO_KG))
        ratio = rho_DM / max(rho_B, mp.mpf(1e-300))
        kb = 2.0 if rho_B > mp.mpf(1e-300) else 0.0
        return {"Y_chi": (Ychi, ky * U), "rho_B_kg_m3": (rho_B, 2.0 * U), "rho_DM_kg_m3": (rho_DM, (ky + 3.0) * U),
                "DM_over_B": (ratio, (ky + 3.0 + kb + 1.0) * U)}
