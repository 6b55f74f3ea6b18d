"""References of the wash-out / depletion quadrature (csrc/lzq_wash.h; TEST INFRASTRUCTURE).

(1) omega(T) = exp(-Gamma log(T / T_lo)) in mpmath, and the counted tolerance of its FP64 builds;
(2) the window W_j omega_j as a yquad_ref.Win, so the device's yields are held to tests/yquad_ref.py
    unchanged;
(3) a numpy restatement of the definition on the reference's y-grid (fpy:231-267 with the factor and the
    second sum), with switchable seeded defects.

The count.  u = 2^-53.  With q = fl(T / T_lo), L = |log q| and e = -fl(Gamma fl(log q)), every error
of the exponent e is an absolute error of e and so a relative error of omega = exp(e):

    q        the quotient rounds once: u relative, which moves log q by u absolutely           Gamma u
    log      the library's: an error of the value's own size, L u                            Gamma L u
    product  Gamma fl(log q) rounds once, and the sign is exact; with the two end effects
             of a value that sits at the top of its binade                                   2 Gamma u
    exp      the library's (libm on the host, exp_sc on the device), 1 ulp of the value            2 u

so |omega - exact| <= (Gamma (L + 3) + 2) u omega.  This is the figure the feature's specification gives
and it is used as it stands.  It takes the logarithm's error as L u, half of a strict "1 ulp = 2 u of
the value" reading (under which, and with the product's own L u, the sum would be Gamma (3 L + 1) + 2):
it holds for logarithms good to half an ulp or so, which glibc's and the device library's are.  `t_u`
adds Gamma t_u u for a T that is itself off by t_u u relative (the device forms T = T_p rsqrt_pos(d):
rsqrt_pos 2 ulp = 4 u, the product u, against the host's division and sqrt, 2 u: t_u = 7).

Subnormal band: an exact omega below 2^-1022 is rounded on the subnormal grid: 2^-1074 absolute is added.
Below 2^-1075 the builds must return exactly +0 (the exponent is then below -745.13).  Gamma = 0 (after
the max) must give exactly 1.0.
"""
import math

import mpmath as mp
import numpy as np

import yquad_ref as Y
from conftest import pkg

DPS = 40
U = 2.0 ** -53
T_U_DEVICE = 7.0
TINY = 2.0 ** -1074


def count(gamma, L, t_u=0.0):
    """The relative tolerance of omega at Gamma (after the max) and L = |log(T / T_lo)|."""
    return (gamma * (L + 3.0 + t_u) + 2.0) * U


def T_lo_of(c):
    return max(c["T_min_over_Tp"] * c["T_p_GeV"], 1e-30)


def T_of_y(c, ys):
    """T(y) as the host build forms it (csrc/lzq_wash.h wash_T_of_y_host): IEEE /, + and sqrt, which
    numpy reproduces bit for bit."""
    ys = np.asarray(ys, dtype=np.float64)
    denom = np.maximum(1.0 + 2.0 * ys / max(c["beta_over_H"], 1e-30), 1e-12)
    return c["T_p_GeV"] / np.sqrt(denom)


def omega_mp(gamma_raw, T, T_lo):
    """(omega in mp, L) with T and T_lo taken as exact doubles."""
    with mp.workdps(DPS):
        g = max(mp.mpf(float(gamma_raw)), mp.mpf(0))
        lg = mp.log(mp.mpf(float(T)) / mp.mpf(float(T_lo)))
        return (mp.mpf(1) if g == 0 else mp.exp(-g * lg)), float(abs(lg))


def check_factor(got, gamma_raw, T, T_lo, scale=1.0, t_u=0.0):
    """None if the FP64 value `got` is within scale x the count of the exact omega, else a message.
    Exact 1.0 for Gamma <= 0, exact +0 below the subnormal band."""
    got = float(got)
    g = max(float(gamma_raw), 0.0)
    if g == 0.0:
        return None if got == 1.0 else f"Gamma = {gamma_raw}: {got!r} is not exactly 1.0"
    w, L = omega_mp(gamma_raw, T, T_lo)
    with mp.workdps(DPS):
        if w < mp.ldexp(1, -1075) * (1 - mp.mpf(1e-9)):
            ok = got == 0.0 and math.copysign(1.0, got) > 0
            return None if ok else f"Gamma = {g}, L = {L}: {got!r} must be exactly +0"
        tol = scale * count(g, L, t_u) * w + (mp.mpf(TINY) if w < mp.ldexp(1, -1021) else 0)
        err = abs(mp.mpf(got) - w)
        if err <= tol:
            return None
        return f"Gamma = {g}, L = {L}: {got!r} vs {mp.nstr(w, 20)}: error {float(err / w):.3e} > {float(tol / w):.3e}"


def win_wash(nd, base_win, c, gamma_raw, t_u=T_U_DEVICE, only=None):
    """yquad_ref's window W_j omega_j: base_win (a yquad_ref.Win: win_one, win_gauss) times the exact
    omega at the exact T_j of the node, its tolerance the window's plus the factor's count.  only: the
    nodes that will be read (a node probe); the others keep base_win's entries."""
    w = Y.Win()
    g = max(float(gamma_raw), 0.0)
    T_lo = T_lo_of(c)
    w.W, w.rel, w.zero, w.undecided = [], [], [], list(base_win.undecided)
    w.exact = base_win.exact and g == 0.0
    with mp.workdps(Y.DPS):
        B, Tp = max(mp.mpf(c["beta_over_H"]), mp.mpf(1e-30)), mp.mpf(c["T_p_GeV"])
        half = mp.ldexp(1, -1075)
        for j, y in enumerate(nd.ys):
            if g == 0.0 or base_win.zero[j] or (only is not None and j not in only):
                w.W.append(base_win.W[j]), w.rel.append(base_win.rel[j]), w.zero.append(base_win.zero[j])
                continue
            d = max(1 + 2 * mp.mpf(float(y)) / B, mp.mpf(1e-12))
            lg = mp.log(Tp / mp.sqrt(d) / mp.mpf(T_lo))
            om = mp.exp(-mp.mpf(g) * lg)
            if om > 0 and abs(mp.log(om) / mp.log(half) - 1) < 1e-9:
                w.undecided.append((j, "omega at 2^-1075", float(lg)))
            w.zero.append(om < half)
            w.W.append(base_win.W[j] * om)
            # (the product W omega rounds once more)
            w.rel.append(base_win.rel[j] + count(g, float(abs(lg)), t_u) + U)
    return w


# ---------------------------------------------------------------------------------------------
# the numpy restatement of the definition, with seeded defects
# ---------------------------------------------------------------------------------------------
DEFECTS = {"a": "T_p in place of T_lo", "b": "the exponent's sign flipped",
           "c": "depletion subtracting the washed Y_B", "d": "Gamma not clamped at 0"}


def Y_chi0(c):
    """fpy:389-400, the ODE branch's initial Y_chi (its `else` included: an unknown regime starts
    thermal there, where the fast path of fpy:376-384 has no value and the kernels give NaN)."""
    ph = pkg("physics_host")
    r = str(c["regime"]).lower()
    if r.startswith("non"):
        if c["Y_chi_init"] is not None:
            return float(c["Y_chi_init"])
        if c["n_chi_at_Tp_GeV3"] is not None:
            return float(c["n_chi_at_Tp_GeV3"]) / max(ph.s_entropy(c["T_p_GeV"], c["g_star_s"]), 1e-300)
        return 1.0e-12
    T, m, g = c["T_max_over_Tp"] * c["T_p_GeV"], c["m_chi_GeV"], c["g_chi"]
    if T > m / 3.0:                                                                   # fpy:90-105
        fermion = str(c["chi_stats"]).lower().startswith("ferm")
        n = g * (3.0 * Y.ZETA3 / (4.0 * ph.PI ** 2)) * T ** 3 if fermion else g * (Y.ZETA3 / ph.PI ** 2) * T ** 3
    else:
        n = g * (m * T / (2.0 * ph.PI)) ** 1.5 * math.exp(-m / max(T, 1e-30))
    return n / ph.s_entropy(T, c["g_star_s"])


def cont_F(c, ys, z_max=30.0):
    """yquad_ref.host_F on the continuum z rule's host tables (lzq_cont_tables)."""
    _, g4, om = pkg("_native").cont_tables(z_max)
    cc = -(c["I_p"] / 6.0) * np.exp(np.clip(ys, -50.0, 50.0))
    return np.array([float(np.sum(om * np.exp(x * g4))) for x in cc])


def restate(c, n_y=8000, nz=1200, z_max=30.0, defect=None, terms=None, continuum=False):
    """(Y_B, Y_chi, terms) of the definition in numpy doubles on the reference's y-grid: the fast
    path's terms w_j g_j (yquad_ref.model: fpy:247-267 in numpy, A/V restated from the library's host z
    tables), times omega_j; Y_chi = Y_chi0 - [deplete] sum of the unwashed terms.  A zero-width or
    inverted T window is the fast path's exact 0.0 (fpy:242-243).  terms: reuse those of an earlier call."""
    y_lo, y_hi, _, ys = Y.ygrid(c, n_y)
    dep = bool(c["deplete_DM_from_source"])
    if not y_hi > y_lo:
        return 0.0, Y_chi0(c), None
    if terms is None:
        F = cont_F(c, ys, z_max) if continuum else Y.host_F(c, ys, nz, z_max)
        terms, _ = Y.model(c, ys, F, sigma=c["source_shape_sigma_y"])
    g = float(c["Gamma_wash_over_H"])
    if defect != "d":
        g = max(g, 0.0)
    T_ref = c["T_p_GeV"] if defect == "a" else T_lo_of(c)
    sign = 1.0 if defect == "b" else -1.0
    with np.errstate(over="ignore", under="ignore"):
        om = np.ones_like(ys) if g == 0.0 else np.exp(sign * g * np.log(T_of_y(c, ys) / T_ref))
    YB = float(np.sum(terms * om))
    YB0 = YB if defect == "c" else float(np.sum(terms))
    return YB, (Y_chi0(c) - YB0 if dep else Y_chi0(c)), terms


def ode_params(c):
    """The ODE_DTYPE record of a config."""
    return pkg("wash").from_config(c)
