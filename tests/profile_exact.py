"""Exact references for the bounce-profile LZ path (TEST INFRASTRUCTURE): what the crossings and the
propagation of csrc/lzq_profile.hip ARE on given interval rows, computed by methods that share
nothing with the kernels or with tests/profile_ref.py (only `fractions` and `mpmath` are imported).

  crossings_exact  -- eqs.(5)-(8) in exact rational arithmetic on the rows' doubles: Sturm
                      sequences, bisection, signs at rational sample points;
  propagate_exact  -- i dpsi/dt = (Delta sigma_z + m sigma_x) psi, xi = v_w t, by its power series on
                      every knot interval (H is a polynomial there) at 40 digits, between the chi-like
                      second-order dressed states at the two ends.

Rows are ascending local coefficients [n-1][4] of t = xi - xi_j; floats or Fractions.
"""
import math
from collections import namedtuple
from fractions import Fraction

import mpmath
from mpmath import mp, mpf, mpc

DPS = 40
EPS = Fraction(1, 2 ** 53)


def dm_rows(coef8, yB, ychi, lam):
    """Exact rows of Delta = y_B phi - y_chi Phi (eq.5) and m = lambda phi (eq.7) from 8-double
    rows (phi c0..c3, Phi c0..c3): Fractions, nothing rounded."""
    yB, ychi, lam = Fraction(yB), Fraction(ychi), Fraction(lam)
    D = [[yB * Fraction(float(r[k])) - ychi * Fraction(float(r[4 + k])) for k in range(4)] for r in coef8]
    M = [[lam * Fraction(float(r[k])) for k in range(4)] for r in coef8]
    return D, M


# ---- polynomials over the rationals (ascending coefficients) --------------------------------
def _trim(p):
    p = list(p)
    while p and p[-1] == 0:
        p.pop()
    return p


def _ev(p, t):
    v = Fraction(0)
    for c in reversed(p):
        v = v * t + c
    return v


def _der(p):
    return _trim([k * p[k] for k in range(1, len(p))])


def _divmod(a, b):
    a, q = list(a), [Fraction(0)] * max(len(a) - len(b) + 1, 0)
    while len(a) >= len(b) and a:
        f, s = a[-1] / b[-1], len(a) - len(b)
        q[s] = f
        for k in range(len(b)):
            a[s + k] -= f * b[k]
        a = _trim(a[:-1]) if a[-1] == 0 else _trim(a)
    return _trim(q), _trim(a)


def _gcd(a, b):
    while b:
        a, b = b, _divmod(a, b)[1]
    return a


def _sturm(q):
    ch = [q, _der(q)]
    while ch[-1]:
        r = _divmod(ch[-2], ch[-1])[1]
        ch.append([-c for c in r])
    return ch[:-1]


def _sgn(v):
    return (v > 0) - (v < 0)


def _ints(p):
    """p times the (positive) common denominator of its coefficients: integers, the same signs."""
    den = 1
    for c in p:
        den = den * c.denominator // math.gcd(den, c.denominator)
    return [int(c * den) for c in p]


def _sign_at(pi, t):
    """Sign of the integer-coefficient polynomial pi at the rational t (integer arithmetic)."""
    num, den = t.numerator, t.denominator
    v, dk = 0, 1
    for c in reversed(pi):
        v = v * num + c * dk
        dk *= den
    return _sgn(v)


def _var(chi, t):
    s = [v for v in (_sign_at(p, t) for p in chi) if v != 0]
    return sum(1 for a, b in zip(s, s[1:]) if a != b)


def _no_root_hull(p, L):
    """True only if the cubic p has no root in [0, L] (most intervals of a profile), decided in
    doubles: its four Bernstein coefficients on [0, L] have one sign, each beyond 2^-30 S
    (S = sum |c_k| L^k; their rounding error is below 2^-49 S, and the values of p on [0, L] lie in
    their hull).  Anything closer goes to the exact path."""
    c = [float(v) for v in p] + [0.0] * (4 - len(p))
    l1, l2, l3 = float(L), float(L) ** 2, float(L) ** 3
    S = abs(c[0]) + abs(c[1]) * l1 + abs(c[2]) * l2 + abs(c[3]) * l3
    if not S < float("inf"):
        return False
    b = (c[0], c[0] + c[1] * l1 / 3, c[0] + 2 * c[1] * l1 / 3 + c[2] * l2 / 3, c[0] + c[1] * l1 + c[2] * l2 + c[3] * l3)
    m = S * 2.0 ** -30
    return all(v > m for v in b) or all(v < -m for v in b)


def _polish(q, lo, hi, L):
    """The simple root of q isolated in [lo, hi] (hi - lo <= 2^-64 L) to ~2^-190 L: three Newton
    steps in rationals, each rounded to 2^-200 L; it must stay inside its bracket."""
    dq, x, unit = _der(q), (lo + hi) / 2, L / 2 ** 200
    for _ in range(3):
        x = x - _ev(q, x) / _ev(dq, x)
        x = round(x / unit) * unit
        assert lo <= x <= hi, (lo, x, hi)
    return x


def roots_in(p, L, bits=64):
    """(lo, hi) (Fractions) of the distinct real roots of the nonzero polynomial p in [0, L],
    ascending: lo == hi, the root met exactly or isolated by Sturm's theorem and bisection to
    2^-bits L, then polished to 2^-190 L."""
    p = _trim(p)
    if len(p) <= 1:
        return []
    if len(p) <= 4 and _no_root_hull(p, L):
        return []
    q = _divmod(p, _gcd(p, _der(p)))[0]            # squarefree: the same distinct roots, all simple
    out = []
    for e in (Fraction(0), L):                     # roots on the ends: recorded, divided out
        if _ev(q, e) == 0:
            out.append((e, e))
            q = _divmod(q, [-e, Fraction(1)])[0]
    if len(q) > 1:
        ch, qi = [_ints(c) for c in _sturm(q)], _ints(q)
        work = [(Fraction(0), L, _var(ch, Fraction(0)) - _var(ch, L))]   # roots in (lo, hi), q != 0 at both
        while work:
            lo, hi, n = work.pop()
            if n == 0:
                continue
            if n == 1:
                s = _sign_at(qi, lo)
                while hi - lo > L / 2 ** bits:
                    mid = (lo + hi) / 2
                    v = _sign_at(qi, mid)
                    if v == 0:
                        lo = hi = mid
                    elif v == s:
                        lo = mid
                    else:
                        hi = mid
                if lo != hi:
                    lo = hi = _polish(q, lo, hi, L)
                out.append((lo, hi))
                continue
            for f in (Fraction(1, 2), Fraction(2, 5), Fraction(3, 5), Fraction(3, 7), Fraction(4, 7)):
                mid = lo + (hi - lo) * f
                if _sign_at(qi, mid) != 0:
                    break
            vm = _var(ch, mid)
            work.append((lo, mid, _var(ch, lo) - vm))
            work.append((mid, hi, vm - _var(ch, hi)))
    return sorted(out)


# ---- crossings --------------------------------------------------------------------------------
Crossing = namedtuple("Crossing", "xi dprime m delta rho d_dprime d_m d_delta interval t")


def _mpf(fr):
    return mpf(fr.numerator) / mpf(fr.denominator)


def _resolution(xk, row, t, J=0):
    """rho at local point t of `row` (Fractions), J the jump of Delta there: see crossings_exact."""
    S = sum(abs(c) * t ** k for k, c in enumerate(row))
    ulp = Fraction(math.ulp(abs(float(xk + t))))
    d, k, fact = _trim(row), 0, 1
    while True:
        d, k = _der(d), k + 1
        fact *= k
        if not d:
            return None                                  # constant row: no resolution (never a root)
        v = abs(_ev(d, t))
        if v != 0:
            w = max(8 * EPS * S, J) * fact / v
            return 2 * ulp + (w if k == 1 else Fraction(float(w) ** (1.0 / k)) * Fraction(1 + 2 ** -40))


def crossings_exact(knots, rows_D, rows_M, v_w):
    """Every crossing of Delta over the profile, [Crossing], in exact rational arithmetic.

    Per interval the distinct real roots of the exact cubic in [0, L] are isolated (Sturm sequence,
    bisection); an identically-zero row has no roots and no sign.  Delta's sign is taken at the
    exact midpoints between consecutive roots and knots, each interval from its own row, so the
    jump between row j at L and row j+1 at 0 is part of the sequence.  A crossing is a change
    between consecutive nonzero signs, located at the end of the earlier sign's stretch: the root's
    bracket, the knot for a jump, a zero stretch's first point.  Zeros on the first or last knot
    have no sign on one side: not crossings.

    Resolution.  A double-precision evaluation of the row by Horner's rule at t returns Delta(t)
    with a forward error of at most gamma_6 S(t), S = sum |c_k| t^k (three multiply-adds; gamma_6 ~
    6 2^-53, rounded up to 8 2^-53).  Any double-precision method locates the root only where two
    such evaluations can still be told from zero: carried to the root with slope Delta', that is
    +- 8 2^-53 S/|Delta'| in t, plus one rounding each for t and for xi = x_j + t:
        rho = 2 ulp(xi) + 8 2^-53 S / |Delta'|
    (where Delta' = 0 at the root, its first non-vanishing derivative of order k takes its place:
    (8 2^-53 S k!/|Delta^(k)|)^(1/k), the same argument on the leading Taylor term).
    That formula is a root's.  A sign change located ON a junction (a jump, or a root on the knot)
    has no root to carry an error to, and needs its own statement: the two rows are two
    double-precision representations of ONE function and disagree at the knot by
    J = |Delta_j(L) - Delta_{j+1}(0)| (from the rows alone, in exact arithmetic; the spline's
    rounding, which S of the cancelling Delta row does not bound), so near the knot that function
    is known to max(8 2^-53 S, J) and its zero to that over |Delta'|:
        rho_junction = 2 ulp(xi) + max(8 2^-53 S, J) / |Delta'|.
    Sign changes closer than the larger rho of the pair cannot be told apart: a run of them counts
    by parity, an odd run as one crossing (its middle member, rho widened by the run's extent), an
    even run as none.

    Returns xi*, Delta'*, m*, delta_LZ = m*^2 / (2 v_w |Delta'*|) (eqs.(6)-(8)) as 40-digit mpf, rho,
    and |d/dxi| of the three at xi* (what rho moves them by)."""
    xs = [Fraction(float(x)) for x in knots]
    nI = len(xs) - 1
    D = [[Fraction(c) for c in r] for r in rows_D]
    M = [[Fraction(c) for c in r] for r in rows_M]
    # stretches of constant sign: (sign, interval, t_end)
    st = []
    for j in range(nI):
        L = xs[j + 1] - xs[j]
        if not _trim(D[j]):
            st.append((0, j, L))
            continue
        cuts = [Fraction(0)] + [(lo + hi) / 2 for lo, hi in roots_in(D[j], L)] + [L]
        for a, b in zip(cuts, cuts[1:]):
            if b > a:
                st.append((_sgn(_ev(D[j], (a + b) / 2)), j, b))
    changes, last = [], None
    for s, j, b in st:
        if s == 0:
            continue
        if last is not None and s != last[0]:
            changes.append((last[1], last[2]))
        last = (s, j, b)
    with mp.workdps(DPS):
        ev = []
        for j, t in changes:
            J = 0
            if t == xs[j + 1] - xs[j] and j + 1 < nI:      # at a junction: the two rows' disagreement
                J = abs(_ev(D[j], t) - D[j + 1][0])
            rho = _resolution(xs[j], D[j], t, J)
            ev.append([xs[j] + t, rho, j, t])
        # clusters of unresolvable sign changes, by parity
        groups = []
        for e in ev:
            if groups and e[0] - groups[-1][-1][0] <= max(e[1], groups[-1][-1][1]):
                groups[-1].append(e)
            else:
                groups.append([e])
        out = []
        vw = max(mpf(float(v_w)), mpf("1e-12"))
        for g in groups:
            if len(g) % 2 == 0:
                continue
            xi, _, j, t = g[len(g) // 2]
            rho = max(e[1] for e in g) + (g[-1][0] - g[0][0])
            d1, d2 = _ev(_der(D[j]), t), _ev(_der(_der(D[j])), t)
            m, m1 = _ev(M[j], t), _ev(_der(M[j]), t)
            dp, mm = _mpf(d1), _mpf(m)
            delta = mm * mm / (2 * vw * abs(dp)) if d1 != 0 else mpf("inf")
            dd = abs(delta * (2 * _mpf(m1) / mm - _mpf(d2) / dp)) if d1 != 0 and m != 0 else mpf(0)
            out.append(Crossing(_mpf(xi), dp, mm, delta, _mpf(rho), abs(_mpf(d2)), abs(_mpf(m1)), dd, j, _mpf(t)))
    return out


# ---- propagation ------------------------------------------------------------------------------
def dressed_chi_like_exact(D, Dd, Ddd, m, md, mdd):
    """The chi-like second-order dressed state of H = D sigma_z + m sigma_x (PAPER):
    theta = atan2(m, D)/2, eps = theta'/(2E), beta = -i eps - eps'/(2E) with E = sqrt(D^2 + m^2),
    theta' = (m' D - m D')/(2 E^2) and its derivative carrying m'' and D'';
    |+> = (cos - sin beta, sin + cos beta)/n, |-> = (-sin - cos beta*, cos - sin beta*)/n; the
    chi-like one is the state whose first (chi) component is the larger."""
    E2 = D * D + m * m
    E = mpmath.sqrt(E2)
    th = mpmath.atan2(m, D) / 2
    c, s = mpmath.cos(th), mpmath.sin(th)
    w = md * D - m * Dd
    thd = w / (2 * E2)
    Ed = (D * Dd + m * md) / E
    wd = mdd * D - m * Ddd                         # (m' D - m D')' : the m' D' terms cancel
    thdd = wd / (2 * E2) - w * (2 * E * Ed) / (2 * E2 * E2)
    eps = thd / (2 * E)
    epsd = thdd / (2 * E) - thd * Ed / (2 * E2)
    beta = mpc(-epsd / (2 * E), -eps)
    n = mpmath.sqrt(1 + abs(beta) ** 2)
    plus = ((c - s * beta) / n, (s + c * beta) / n)
    minus = ((-s - c * mpmath.conj(beta)) / n, (c - s * mpmath.conj(beta)) / n)
    return plus if abs(plus[0]) >= abs(plus[1]) else minus


def _shift(c, s):
    """Coefficients of c(s + tau) in tau (cubic)."""
    c0, c1, c2, c3 = c
    return [c0 + s * (c1 + s * (c2 + s * c3)), c1 + s * (2 * c2 + 3 * c3 * s), c2 + 3 * c3 * s, c3]


def _edge_exact(cD, cM, t, v):
    d, m = _shift(cD, t), _shift(cM, t)
    return dressed_chi_like_exact(d[0], v * d[1], v * v * 2 * d[2], m[0], v * m[1], v * v * 2 * m[2])


BITS = 200            # fixed-point fraction bits of the series sums (60 digits)


def _fix(v):
    return int(mpmath.floor(mpmath.ldexp(v, BITS) + mpf(0.5)))


def propagate_exact(knots, rows_D, rows_M, v_w, terms=60):
    """P = 1 - |<u_end|psi>|^2 through the whole profile at 40 digits.  On a knot interval
    d psi/d xi = -(i/v_w) (Delta(xi) sigma_z + m(xi) sigma_x) psi has polynomial coefficients, so about
    any point s, psi(s + h u) = sum b_n u^n with the four-term recurrence
        (n + 1) b_{n+1} = -i sum_{k=0..3} (Delta_k sigma_z + m_k sigma_x) (h^{k+1} / v_w) b_{n-k},
    Delta_k, m_k the Taylor coefficients at s, and the sub-step's end is u = 1: the plain sum of the
    b_n.  Sub-steps keep (h / v_w) sum_k (|Delta_k| + |m_k|) h^k <= 1/2 (bounded over the interval by
    the rows' absolute sums), so the terms fall like (1/2)^n / n!; `terms` >= 60 of them, the last four
    asserted below 1e-35.  The sums run in 200-bit fixed point (integers: every operation rounds by
    at most 2^-200, a few thousand of them per sub-step); rows, edge states and P in mpmath."""
    assert terms >= 60
    with mp.workdps(DPS + 25):
        v = mpf(float(v_w))
        xs = [mpf(float(x)) for x in knots]
        rD = [[_mpf(Fraction(c)) for c in r] for r in rows_D]
        rM = [[_mpf(Fraction(c)) for c in r] for r in rows_M]
        p0, p1 = _edge_exact(rD[0], rM[0], mpf(0), v)
        p = [_fix(p0.real), _fix(p0.imag), _fix(p1.real), _fix(p1.imag)]
        tiny = _fix(mpf("1e-35"))
        for j in range(len(xs) - 1):
            L = xs[j + 1] - xs[j]
            bound = sum((abs(rD[j][k]) + abs(rM[j][k])) * L ** k for k in range(4))
            nsub = max(1, int(mpmath.ceil(2 * bound * L / v)))
            h = L / nsub
            for i in range(nsub):
                d, m = _shift(rD[j], i * h), _shift(rM[j], i * h)
                hk = [(k, _fix(d[k] * h ** (k + 1) / v), _fix(m[k] * h ** (k + 1) / v)) for k in range(4)]
                hk = [t for t in hk if t[1] or t[2]]
                b = [p]                                  # b_n = (re psi_1, im psi_1, re psi_2, im psi_2)
                tot = list(p)
                for n in range(terms):
                    u = [0, 0, 0, 0]
                    for k, dk, mk in hk:
                        if k <= n:
                            c = b[n - k]
                            u[0] += dk * c[0] + mk * c[2]
                            u[1] += dk * c[1] + mk * c[3]
                            u[2] += mk * c[0] - dk * c[2]
                            u[3] += mk * c[1] - dk * c[3]
                    q = (n + 1) << BITS                  # b_{n+1} = -i u / (n + 1): (re, im) -> (im, -re)
                    nb = [u[1] // q, -u[0] // q, u[3] // q, -u[2] // q]
                    b.append(nb)
                    tot = [t + w for t, w in zip(tot, nb)]
                    if n >= terms - 4:
                        assert max(abs(w) for w in nb) < tiny, (j, i, n)
                p = tot
        s0, s1 = (mpc(mpmath.ldexp(mpf(p[0]), -BITS), mpmath.ldexp(mpf(p[1]), -BITS)),
                  mpc(mpmath.ldexp(mpf(p[2]), -BITS), mpmath.ldexp(mpf(p[3]), -BITS)))
        u0, u1 = _edge_exact(rD[-1], rM[-1], xs[-1] - xs[-2], v)
        amp = mpmath.conj(u0) * s0 + mpmath.conj(u1) * s1
        nrm = abs(s0) ** 2 + abs(s1) ** 2
        assert abs(nrm - 1) < mpf("1e-45"), nrm            # unitarity of the series solution
        with mp.workdps(DPS):
            return +(1 - abs(amp) ** 2 / nrm)
