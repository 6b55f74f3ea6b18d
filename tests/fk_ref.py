"""References and counted tolerances of the momentum-averaged LZ probability P-bar (TEST INFRASTRUCTURE;
csrc/lzq_fk.h fk_pbar).

Two references:

* pbar_quad: the definition of include/lzq.h by mpmath.quad, 40 digits -- what the rule approximates
  (tests/golden/fk_pbar_box.json holds it on the box; tools/fk_rule_error.py writes that file);
* pbar_rule_ld: the RULE itself, the sums over the library's own node table, in numpy's long double
  (x87, 64-bit mantissa: 2^-64 per operation, < 300 * 2^-63 = 3.3e-17 over a sum) -- what the
  arithmetic of a build of fk_pbar approximates.  Its inputs (mu, g, the table) are doubles taken as
  exact, as tests/yquad_ref.py takes F_j.

The tolerance of a build against pbar_rule_ld is counted, not tuned (u = 2^-53; "1 ulp" is 2 u, the bound
of the device library's and libm's exp, log and expm1), per node i in fk_pbar's operation order:

    a     = t (t + 2 mu)         the sum (1), the product (1); 2 mu is exact                       2
    w     = a we / (1 +- x e)    x = e^-mu: exp (2), its argument -mu exact, and the product x e (1),
                                 both times amp = x e / |1 +- x e| (the boson's difference cancels
                                 at small mu + t); the sum (1); a (2), the product a we (1) and the
                                 quotient (1)                                          5 + 3 amp
    q     = a / (eps eps)        a (2), eps = t + mu (1) twice, the product (1), the quotient (1)  6
    L     = log q                2 |L| relative, 6 absolute from q
    arg   = hp L + lr            hp = -p/2 exact; lr = p log v_ref: log (2), product (1): 3 |lr|;
                                 the product hp L (1): |hp L|; the sum (1): |arg|
            absolute error       6 |hp| + 3 |hp L| + 3 |lr| + |arg|
    F     = exp(arg)             exp (2) + arg's absolute error
    x     = g F                  (1)
    b     = -expm1(-x)           expm1 (2); d ln b / d ln x = x e^-x / (1 - e^-x) <= 1
    term  = w b                  (1)

and p = 0: b = -expm1(-g) once (2), term (1).  The two sums are over N non-negative terms in node
order, at most (N - 1) u each (the worst case of recursive summation, not a measured one); the
quotient 1.  A sum's relative error from its terms' is their mean weighted by the terms, so

    tol(mu, g, block) = [mean_term(w + b + 1) + mean_w(w) + 2 (N - 1) + 1] u + 3.3e-17.
"""
import math

import mpmath as mp
import numpy as np

from conftest import pkg

U = 2.0 ** -53
LD_ERR = 300 * 2.0 ** -63


def table():
    return pkg("fk").nodes()


def pbar_rule_ld(mu, g, p, v_ref, stats, tab=None):
    """The rule's sums in long double for arrays mu, g (broadcast): np.longdouble array."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, "needs the x87 long double"
    t, we, e = (np.asarray(x, dtype=ld) for x in (table() if tab is None else tab))
    mu, g = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(g, dtype=np.float64))
    out = np.empty(mu.shape, dtype=ld)
    for k in np.ndindex(mu.shape):
        m, gg = ld(mu[k]), ld(g[k])
        x = np.exp(-m)
        a = t * (t + 2 * m)
        w = a * we / (1 + (x if stats == 0 else -x) * e)
        if p == 0:
            F = ld(1)
        else:
            eps = t + m
            F = np.exp(ld(p) * np.log(ld(v_ref)) - ld(p) / 2 * np.log(a / (eps * eps)))
        with np.errstate(over="ignore", invalid="ignore"):
            xx = np.where(np.isinf(gg), ld(np.inf), gg * F)
        b = -np.expm1(-xx)
        out[k] = np.sum(w * b) / np.sum(w)
    return out


def to_mp(x):
    """A long double as an exact mpf."""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))


def pbar_tol(mu, g, p, v_ref, stats, tab=None):
    """The counted relative tolerance (docstring) of one build of fk_pbar at scalar mu, g."""
    t, we, e = table() if tab is None else tab
    n = t.size
    x = math.exp(-mu)
    a = t * (t + 2.0 * mu)
    D = 1.0 + (x if stats == 0 else -x) * e
    w = a * we / D
    k_w = 4.0 + 3.0 * (x * e / np.abs(D)) + 1.0
    if p == 0:
        k_b = np.full(n, 2.0)
        b = np.full(n, -math.expm1(-g))
    else:
        eps = t + mu
        L = np.log(a / (eps * eps))
        hp, lr = -0.5 * p, p * math.log(v_ref)
        arg_abs = 6.0 * abs(hp) + 3.0 * np.abs(hp * L) + 3.0 * abs(lr) + np.abs(hp * L + lr)
        k_b = (2.0 + arg_abs) + 1.0 + 2.0
        with np.errstate(over="ignore"):
            b = -np.expm1(-(g * np.exp(hp * L + lr)))
    term = w * b
    k_num = float(np.sum(term * (k_w + k_b + 1.0)) / np.sum(term)) if np.sum(term) > 0 else 0.0
    k_den = float(np.sum(w * k_w) / np.sum(w))
    return (k_num + k_den + 2.0 * (n - 1) + 1.0) * U + LD_ERR


def pbar_quad(mu, g, p, v_ref, stats):
    import importlib.util
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("fk_rule_error", os.path.join(here, "..", "tools", "fk_rule_error.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.pbar_mp(mu, g, p, v_ref, stats)
