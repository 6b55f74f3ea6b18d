"""The bounce-profile kernels (csrc/lzq_profile.hip) against EXACT references (tests/profile_exact.py):
what the right answer is, by methods that share nothing with the kernels or with the restatement
tests/profile_ref.py.

* propagation: 17 curved profiles solved by power series at 40 digits (golden_profile_exact.json):
  the cubic terms of the Magnus polynomials, the m', m'' terms of the dressed edge states and the
  step rule on curved intervals;
* crossings: exact rational arithmetic (Sturm sequences) on the very rows the kernel reads: random
  multi-crossing profiles, zeros on knots to rounding (the case the walk got wrong before Delta had
  one value per knot: 57 of 3000 seeded draws reported a count whose parity contradicted Delta's
  end signs), and hand-built rows with literal expectations;
* the four cos/sinc ranges of a Magnus step (|n|^2 <= 1/8, <= 1/4, <= 1, beyond), reached only at
  0.5 - 2.5 steps per radian.
"""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg
import profile_cases as C
import profile_exact as X
import profile_ref as R

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(GOLDEN, "golden_profile_exact.json")))
RND = 1e-11   # kernel vs restatement rounding bound (tests/test_gpu_profile.py)


def unhex(a, shape=(-1,)):
    return np.array([float.fromhex(v) for v in a]).reshape(shape)


def rows_shape(engine, knots, coef8):
    """Shapes from given rows (as test_gpu_profile._linear_shape): [n_knots] / [n_knots - 1, 8] or
    batches of them."""
    k, c = np.asarray(knots, float), np.asarray(coef8, float)
    if k.ndim == 1:
        k, c = k[None], c[None]
    return pkg("engine").ProfileShapes(torch.as_tensor(k, device=engine.device), torch.as_tensor(c, device=engine.device))


def crossings(engine, sh, pts, max_cross=8):
    return {k: v.cpu().numpy() for k, v in engine.profile_crossings(sh, pts, max_cross).items()}


# ---- 1. propagation against the exact solution ------------------------------------------------
def test_propagation_matches_exact(gpu_engine):
    """Every fixture case at 4 and 16 steps per radian: |P_gpu - P_exact| <= e_ref(spr) + 1e-11, e_ref
    the scheme's truncation error (the restatement's distance from the exact P, measured on the CPU,
    in the fixture) and 1e-11 the kernel-vs-restatement rounding bound; through the device splines
    the same plus dP_spline (the fixture's measured effect of the spline-coefficient bound on P).
    lambda = 0: P <= 1e-15."""
    worst = {(spr, via): 0.0 for spr in (4, 16) for via in ("rows", "splines")}
    for name, s in GOLD["shapes"].items():
        cases = [c for c in GOLD["cases"] if c["shape"] == name]
        x = unhex(s["knots"])
        shapes = {"rows": rows_shape(gpu_engine, x, unhex(s["coef"], (len(x) - 1, 8))),
                  "splines": gpu_engine.profile_shapes(x, unhex(s["phi"]), unhex(s["Phi"]))}
        pts = gpu_engine.profile_points(*zip(*(c["point"] for c in cases)), 0)
        for via, sh in shapes.items():
            for spr in (4, 16):
                got = gpu_engine.lz_propagate_profile(sh, pts, float(spr)).cpu().numpy()
                for c, P in zip(cases, got):
                    err = abs(P - float(c["P"]))
                    gate = c["e_ref"][str(spr)] + RND + (c["dP_spline"] if via == "splines" else 0.0)
                    worst[spr, via] = max(worst[spr, via], err)
                    assert 0.0 <= P <= 1.0 and err <= gate, (c["name"], via, spr, P, c["P"], err, gate)
                    if c["point"][2] == 0.0:
                        assert P <= 1e-15, (c["name"], via, spr, P)
    for (spr, via), w in sorted(worst.items()):
        print(f"profile propagation vs exact, {spr} steps/rad, {via}: worst |P - P_exact| = {w:.3g}")


# ---- 2. crossings against the exact ones, generic profiles ------------------------------------
def test_crossings_match_exact(gpu_engine):
    """The random multi-crossing profiles of test_crossings_match_restatement, rows from scipy handed
    over as they are: counts equal; |xi - xi_exact| <= rho; Delta', m, delta_LZ within rho x |their
    xi-derivative| + 8 ulp."""
    rng = np.random.default_rng(7)
    shapes = [C.wiggly(60, s) for s in range(4)]
    c8 = [C.rows8(*s) for s in shapes]
    sh = rows_shape(gpu_engine, np.stack([s[0] for s in shapes]), np.stack(c8))
    n = 64
    yB, ychi = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    lam, vw, shp = rng.uniform(0.01, 0.5, n), rng.uniform(0.1, 0.9, n), rng.integers(0, 4, n)
    cr = crossings(gpu_engine, sh, gpu_engine.profile_points(yB, ychi, lam, vw, shp))
    total, worst = 0, 0.0
    for i in range(n):
        s = shp[i]
        ref = X.crossings_exact(shapes[s][0], C.rows_D(c8[s], yB[i], ychi[i]), lam[i] * c8[s][:, :4], vw[i])
        assert cr["count"][i] == len(ref), (i, cr["count"][i], [float(e.xi) for e in ref])
        total += len(ref)
        for k, e in enumerate(ref):
            worst = max(worst, float(abs(cr["xi"][i, k] - e.xi) / e.rho))
            assert abs(cr["xi"][i, k] - e.xi) <= e.rho, (i, k, cr["xi"][i, k], e)
            for key, val, der in (("dprime", e.dprime, e.d_dprime), ("m_mix", e.m, e.d_m), ("delta_lz", e.delta, e.d_delta)):
                assert abs(cr[key][i, k] - val) <= e.rho * der + 8 * math.ulp(abs(float(val))), (i, k, key, cr[key][i, k], e)
    assert total >= 2 * n
    print(f"crossings vs exact: {total} crossings, worst |xi - xi_exact| / rho = {worst:.3g}")


# ---- 3. zeros on knots to rounding --------------------------------------------------------------
BATCHES = C.knot_zero_batches()


@pytest.mark.parametrize("n_knots", C.KNOT_COUNTS)
def test_knot_zero_counts(gpu_engine, n_knots):
    """Delta vanishes on an interior knot to rounding (profile_cases.knot_zero_profile; 4 knot counts x
    512 shapes, one point each, none skipped): the count's parity matches Delta's end signs, the count
    is crossings_exact's, and no two reported crossings lie within 2 rho of each other.  (Where the
    two rows' own disagreement at the knot exceeds a root's rho -- shallow Delta', 1 draw of the 2048:
    sign changes 1.6e-13 and 1.1e-12 either side of the knot from a 2.5e-16 jump -- crossings_exact
    counts them as one by its junction resolution; see its docstring.)"""
    draws = BATCHES[n_knots]
    c8 = [C.rows8(x, phi, Phi) for x, phi, Phi, _, _, _ in draws]
    sh = rows_shape(gpu_engine, np.stack([d[0] for d in draws]), np.stack(c8))
    yB, ychi = np.array([d[3] for d in draws]), np.array([d[4] for d in draws])
    cr = crossings(gpu_engine, sh, gpu_engine.profile_points(yB, ychi, 0.1, 0.3, np.arange(len(draws))))
    checked = 0
    for i, (x, _, _, yb, yc, k) in enumerate(draws):
        sa, sb = C.end_signs(x, c8[i], yb, yc)
        assert sa != 0 and sb != 0, (n_knots, i)
        cnt = int(cr["count"][i])
        assert (cnt % 2 == 1) == (sa != sb), (n_knots, i, k, cnt, sa, sb)
        ref = X.crossings_exact(x, C.rows_D(c8[i], yb, yc), 0.1 * c8[i][:, :4], 0.3)
        assert cnt == len(ref), (n_knots, i, k, cnt, cr["xi"][i, :cnt], [float(e.xi) for e in ref])
        rho = max(float(e.rho) for e in ref) if ref else 0.0
        assert all(b - a > 2 * rho for a, b in zip(cr["xi"][i, :cnt], cr["xi"][i, 1:cnt])), (n_knots, i, cr["xi"][i, :cnt])
        checked += 1
    assert checked == C.PER_COUNT


# ---- 4. hand-built rows ---------------------------------------------------------------------------
def _hand(engine, knots, rows, max_cross=4):
    sh = rows_shape(engine, np.array(knots, float), C.hand_rows8(rows))
    return crossings(engine, sh, engine.profile_points(0.0, -1.0, 1.0, C.HAND_VW, 0), max_cross)


@pytest.mark.parametrize("case", C.HAND, ids=[c[0] for c in C.HAND])
def test_hand_built_rows(gpu_engine, case):
    """Exact dyadic rows, y_B = 0, y_chi = -1, lambda = 1 (Delta is the Phi row, m = 1): literal
    expectations.  A zero on an interior knot is a crossing iff the signs around it differ; zeros on
    the first and last knot are not crossings; a zero interval between + and - is one crossing at the
    first zero met; tangent roots are none; roots come in order."""
    name, knots, rows, expect = case
    cr = _hand(gpu_engine, knots, rows)
    assert cr["count"][0] == len(expect), (name, cr["count"][0], cr["xi"][0])
    ref = X.crossings_exact(knots, rows, [[1, 0, 0, 0]] * len(rows), C.HAND_VW)
    assert len(ref) == len(expect)
    for k, ((xi, dp), e) in enumerate(zip(expect, ref)):
        assert abs(cr["xi"][0, k] - xi) <= e.rho, (name, k, cr["xi"][0, k], xi, e.rho)
        assert abs(cr["dprime"][0, k] - dp) <= e.rho * e.d_dprime + 8 * math.ulp(abs(dp)), (name, k, cr["dprime"][0, k], dp)
        assert cr["m_mix"][0, k] == 1.0
        d = 1.0 / abs(dp)
        assert abs(cr["delta_lz"][0, k] - d) <= e.rho * e.d_delta + 8 * math.ulp(d), (name, k, cr["delta_lz"][0, k], d)


def test_triple_root_by_residual(gpu_engine):
    """(t - 1)^3: one crossing; where exactly is beyond double precision (rho ~ 2e-5), so it is judged
    by the residual: |Delta(xi*)| <= 8 2^-53 S, S = sum |c_k| t^k, evaluated exactly."""
    _, knots, rows = C.TRIPLE
    cr = _hand(gpu_engine, knots, rows)
    assert cr["count"][0] == 1
    t = Fraction(float(cr["xi"][0, 0]))
    res = abs(sum(Fraction(c) * t ** k for k, c in enumerate(rows[0])))
    S = sum(abs(Fraction(c)) * t ** k for k, c in enumerate(rows[0]))
    assert 0 < t < 2 and res <= 8 * X.EPS * S, (float(t), float(res), float(8 * X.EPS * S))


@pytest.mark.parametrize("max_cross", [0, 1, 2])
def test_max_cross_overflow(gpu_engine, max_cross):
    """3 crossings against max_cross 0, 1, 2 in a two-point batch: count is the total, only the first
    max_cross entries are written, and the neighbouring point's entries (its own crossing, its unused
    slots, the buffer's tail) are intact."""
    _, knots, rows, expect = next(c for c in C.HAND if c[0] == "three simple roots")
    _, knots1, rows1, expect1 = next(c for c in C.HAND if c[0] == "linear")
    k2 = np.stack([np.array(knots, float), np.array(knots1, float)])
    sh = rows_shape(gpu_engine, k2, np.stack([C.hand_rows8(rows), C.hand_rows8(rows1)]))
    pts = gpu_engine.profile_points(0.0, -1.0, 1.0, C.HAND_VW, [0, 1])
    vp, SENT, tail = pkg("engine")._vp, -7.0, 8
    bufs = [torch.full((2 * max_cross + tail,), SENT, dtype=torch.float64, device=gpu_engine.device) for _ in range(4)]
    count = torch.full((2,), -5, dtype=torch.int32, device=gpu_engine.device)
    with torch.cuda.device(gpu_engine.device):
        gpu_engine._check(gpu_engine.lib.lzq_profile_crossings(
            vp(sh.knots), vp(sh.coef), 2, 4, vp(pts), 2, max_cross, *(vp(b) for b in bufs), vp(count), gpu_engine._stream()))
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [3, 1]
    xi, dp = bufs[0].cpu().numpy(), bufs[1].cpu().numpy()
    want = np.full(2 * max_cross + tail, SENT)
    want_dp = want.copy()
    for k in range(max_cross):
        want[k], want_dp[k] = expect[k]
    if max_cross >= 1:
        want[max_cross], want_dp[max_cross] = expect1[0]
    assert np.allclose(xi, want, rtol=0, atol=1e-13) and np.allclose(dp, want_dp, rtol=0, atol=1e-12), (xi, want)
    assert (xi[max_cross + min(max_cross, 1):] == SENT).all() and (xi[2 * max_cross:] == SENT).all()
    for b in bufs[2:]:
        assert (b.cpu().numpy()[2 * max_cross:] == SENT).all()


# ---- 5. the step-angle branches -------------------------------------------------------------------
def test_step_angle_branches(gpu_engine):
    """0.5, 1, 1.5 and 2.5 steps per radian on the four coupling sets of
    test_propagation_matches_restatement: P within 1e-11 of the restatement, 0 <= P <= 1.  Every
    other profile test runs at >= 3 steps per radian, where |n|^2 <~ 0.12 and only the first range of
    cos_sinc_step executes; here all four do (checked with the restatement's steps in
    test_profile_exact_host.test_step_angles_reach_every_range: at 0.5 steps per radian alone the 165
    steps fall 67 / 26 / 37 / 35 into |n|^2 <= 1/8, <= 1/4, <= 1, > 1)."""
    shapes = [C.wiggly(24, s, span=4.0) for s in range(2)]
    c8 = [C.rows8(*s) for s in shapes]
    sh = rows_shape(gpu_engine, np.stack([s[0] for s in shapes]), np.stack(c8))
    pts = gpu_engine.profile_points(*zip(*C.COUPLINGS))
    worst = 0.0
    for spr in (0.5, 1.0, 1.5, 2.5):
        got = gpu_engine.lz_propagate_profile(sh, pts, spr).cpu().numpy()
        for i, (yB, ychi, lam, vw, s) in enumerate(C.COUPLINGS):
            ref = R.propagate_profile(shapes[s][0], c8[s][:, :4], c8[s][:, 4:], yB, ychi, lam, vw, spr=spr)
            worst = max(worst, abs(got[i] - ref))
            assert 0.0 <= got[i] <= 1.0 and abs(got[i] - ref) <= RND, (spr, i, got[i], ref)
    print(f"profile propagation at 0.5 - 2.5 steps/rad vs restatement: worst {worst:.3g}")
