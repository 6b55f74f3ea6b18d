"""Wash-out and source depletion on the y-grid quadrature (csrc/lzq_wash.hip: lzq_wash_factor_batch,
lzq_yields_batch_reuse_wash, lzq_sweep_grid_from_ztables_wash, lzq_sweep_grid_solve_wash) on an MI355X.

* the factor omega alone against the host build, within twice the count of tests/wash_ref.py;
* Gamma = 0 without depletion: the three entry points return their namesakes' bits;
* the yields against the mpmath reference of tests/yquad_ref.py (unchanged), its window W_j omega_j and its
  tolerance the window's plus the factor's count: node probes and full sums;
* depletion: Y_chi = fl(Y_chi0 - Y_B0) bit for bit, the negative Y_chi of the reference's flux = 1e-3 case;
* the sigma_v = 0 cases of tests/golden/golden_ode.json within the bound tests/test_wash_host.py measured;
* the grid decode against the explicit-points call, the solve against the forward kernel and scipy's
  brentq on the host restatement, the refusals.

Shapes: n_y = 2000 and 2049 (a partial last pass and its tail lanes), the (13, 3) and (1200, 30) z grids
and the continuum table, a few dozen points per call.
"""
import ctypes
import math

import mpmath as mp
import numpy as np
import pytest
import torch

import wash_ref as WR
import yquad_ref as Y
from conftest import BASE_CFG, full_cfg, golden, pkg
from test_gpu_yquad import device_ref
from test_wash_host import bound_for, golden_cases
from test_yquad_host import probe_block

pytestmark = pytest.mark.gpu
SMALL, DEFAULT = Y.ZGRID, (1200, 30.0)
DEP = {"deplete_DM_from_source": True}
NONE = {}
FLAT = {"kind": "plateau", "half_width": 200.0}
COL = {k: i for i, k in enumerate(("Y_B", "Y_chi", "rho_B_kg_m3", "rho_DM_kg_m3", "DM_over_B", "P_used"))}


def same(a, b):
    a, b = (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64),
                                                 np.ascontiguousarray(b).view(np.int64))


def blocks(rows):
    """ODE_DTYPE records from (Gamma, deplete) pairs."""
    rec = np.zeros(len(rows), dtype=pkg("_native").ODE_DTYPE)
    rec["Gamma_wash_over_H"] = [g for g, _ in rows]
    rec["deplete_DM_from_source"] = [int(d) for _, d in rows]
    return rec


# ---------------------------------------------------------------------------------------------
# the factor
# ---------------------------------------------------------------------------------------------
def test_factor_against_host(gpu_engine):
    """4096 (Gamma, y) pairs: 8 Gammas x 512 nodes of main()'s window, ends included."""
    W, cfgm = pkg("wash"), pkg("config")
    c = full_cfg(BASE_CFG)
    ys = np.ascontiguousarray(Y.ygrid(c, 2000)[3][np.linspace(0, 1999, 512).astype(int)])
    T, T_lo = WR.T_of_y(c, ys), WR.T_lo_of(c)
    L = np.abs(np.log(T / T_lo))
    worst, worst0, n = 0.0, 0.0, 0
    for g in (0.0, -2.0, 1e-12, 0.3, 5.0, 50.0, 85.0, 800.0):
        blk = {"Gamma_wash_over_H": g}
        dev = gpu_engine.wash_factor(cfgm.to_point(c), blk, ys).cpu().numpy()
        host = W.factor_host(cfgm.to_point(c), blk, ys)
        n += dev.size
        if g <= 0.0:
            assert np.all(dev == 1.0) and np.all(host == 1.0)
            continue
        tol = 2.0 * WR.count(g, L, WR.T_U_DEVICE) * host + np.where(host < 2.0 ** -1021, WR.TINY, 0.0)
        assert np.all(np.abs(dev - host) <= tol), (g, np.max(np.abs(dev - host) / np.maximum(tol, 1e-320)))
        big = host > 2.0 ** -1000
        worst = max(worst, float(np.max(np.abs(dev - host)[big] / tol[big])) if big.any() else 0.0)
        tol0 = 2.0 * WR.count(g, L) * host                   # (reported, not asserted: the count without T's term)
        worst0 = max(worst0, float(np.max(np.abs(dev - host)[big] / tol0[big])) if big.any() else 0.0)
        if g == 800.0:   # T/T_lo = 5000 at node 0: e^-6814 is exactly +0 in both builds
            assert dev[0] == 0.0 and not np.signbit(dev[0]) and host[0] == 0.0
        if g == 85.0:    # e^-724: the subnormal band at node 0
            assert 0.0 < host[0] < 2.0 ** -1000 and dev[0] >= 0.0
    assert n == 4096
    # T = T_lo exactly (y = 0, T_min = T_p): log 1 = 0, omega = 1 whatever Gamma
    c1 = full_cfg({**BASE_CFG, "T_min_over_Tp": 1.0})
    assert gpu_engine.wash_factor(cfgm.to_point(c1), {"Gamma_wash_over_H": 800.0}, [0.0]).cpu().numpy()[0] == 1.0
    print(f"omega, device against host: {n} pairs, worst |difference| / (2 x count) {worst:.3f} with the device's T "
          f"counted (t_u = {WR.T_U_DEVICE}), {worst0:.3f} of 2 x (Gamma (L + 3) + 2) u without it")


# ---------------------------------------------------------------------------------------------
# Gamma = 0 without depletion: the namesakes' bits
# ---------------------------------------------------------------------------------------------
def identity_points(n=36):
    """n points on 3 z-sum classes (I_p), differing in P, sigma_y, flux and m_chi."""
    cfgm = pkg("config")
    pts = []
    for i in range(n):
        pts.append(cfgm.to_point(full_cfg({**BASE_CFG, "I_p": (0.34, 0.2, 0.5)[i % 3], "P_chi_to_B": 0.05 + 0.02 * i,
                                           "source_shape_sigma_y": 3.0 + i, "m_chi_GeV": 0.95 * (1 + i % 5),
                                           "incident_flux_scale": 1.07e-9 * (1 + i % 7)})))
    return np.concatenate(pts)


def window_records(n):
    W = pkg("window")
    return np.concatenate([W.to_window({"kind": "plateau", "y0": -3.0 + 0.3 * i, "half_width": 1.0 + 0.1 * i,
                                        "sigma_lo": 2.0, "sigma_hi": 4.0}) for i in range(n)])


@pytest.mark.parametrize("n_y,grid", [(2000, SMALL), (2049, DEFAULT), (2049, "continuum")])
def test_identity_with_the_namesakes(gpu_engine, n_y, grid):
    eng = gpu_engine
    cont = grid == "continuum"
    kw = dict(n_y=n_y, continuum=True) if cont else dict(n_y=n_y, nz=grid[0], z_max=grid[1])
    pts = identity_points()
    wins = window_records(pts.size)
    # explicit points, the point's Gaussian and a block per point
    for win in (None, wins):
        want = eng.yields(pts, reuse=True, window=win, **kw)
        assert eng.last_yields_path == "tables"
        assert same(eng.yields(pts, wash=NONE, window=win, **kw), want)
        assert same(eng.yields(pts, wash=blocks([(-1.0, 0)] * pts.size), window=win, **kw), want)   # max(., 0)
    # grid and solve, with a window axis in the second case
    c = full_cfg(BASE_CFG)
    axes = [("I_p", np.array([0.34, 0.2])), ("delta_LZ", np.linspace(0.01, 0.2, 5)), ("incident_flux_scale", np.array([1.07e-9, 3e-9]))]
    waxes = axes + [("window_y0", np.array([-1.0, 0.5]))]
    sv = {"field": "P_chi_to_B", "lo": 1e-3, "hi": 1.0}
    for ax, win in ((axes, None), (waxes, {"kind": "plateau", "half_width": 2.0, "sigma": 3.0})):
        total = int(np.prod([len(v) for _, v in ax]))
        want = eng.sweep(c, ax, 0, total, reuse=True, window=win, **kw)
        assert same(eng.sweep(c, ax, 0, total, wash=NONE, window=win, **kw), want)
        sax = [a for a in ax if a[0] != "delta_LZ"]
        total = int(np.prod([len(v) for _, v in sax]))
        rec0, sol0 = eng.sweep(c, sax, 0, total, solve=sv, window=win, **kw)
        rec1, sol1 = eng.sweep(c, sax, 0, total, solve=sv, window=win, wash=NONE, **kw)
        assert same(rec1, rec0) and same(sol1, sol0)
        assert (sol0.cpu().numpy()[:, 5] == 0.0).any()


# ---------------------------------------------------------------------------------------------
# the yields against mpmath
# ---------------------------------------------------------------------------------------------
def gamma_subnormal(c, y):
    """The Gamma that puts omega(T(y)) at e^-715, inside the subnormal band."""
    return 715.0 / math.log(float(WR.T_of_y(c, [y])[0]) / WR.T_lo_of(c))


@pytest.mark.parametrize("case,n_y,grid", [("shipped", 2000, SMALL), ("branch", 2049, SMALL), ("shipped", 2049, DEFAULT)])
def test_node_probes_against_mp(gpu_engine, case, n_y, grid):
    """fl(w_j I_j omega_j) at nodes 0, 63, 64, n_y - 1 and where T crosses m/3, for Gamma = 0.5, 50 and
    the node's own subnormal Gamma: a plateau block that is 1 at one node."""
    cfgm, W = pkg("config"), pkg("window")
    c, (y_lo, y_hi, step, ys), F, nd = device_ref(gpu_engine, case, grid, n_y)
    nodes = [0, 63, 64, n_y - 1]
    flips = np.nonzero(np.diff(nd.relativistic.astype(int)))[0]
    if case == "branch":
        assert flips.size == 1
    nodes += [int(j) for f in flips for j in (f, f + 1)]
    rows = []          # (node, Gamma)
    for j in nodes:
        gs = [0.5, 50.0]
        if float(WR.T_of_y(c, [ys[j]])[0]) > WR.T_lo_of(c) * 1.001:
            gs.append(gamma_subnormal(c, ys[j]))
        rows += [(j, g) for g in gs]
    pts = np.repeat(cfgm.to_point(c), len(rows))
    wins = np.concatenate([W.to_window(probe_block(ys[j], step)) for j, _ in rows])
    out = gpu_engine.yields(pts, wash=blocks([(g, 0) for _, g in rows]), window=wins, n_y=n_y, nz=grid[0],
                            z_max=grid[1]).cpu().numpy()
    worst = 0.0
    one = Y.win_one(nd)
    for (j, g), got in zip(rows, out[:, 0]):
        win = WR.win_wash(nd, one, c, g, only=(j,))
        _, ratio, bad = Y.compare_nodes([got], nd, win, idx=[j])
        assert not bad, (j, g, bad)
        worst = max(worst, ratio)
    sub = [got for (j, g), got in zip(rows, out[:, 0]) if g > 60.0]
    assert all(0.0 <= x < 2.0 ** -1000 for x in sub) and len(sub) >= 4
    print(f"wash node probes [{case}, n_y = {n_y}, z grid {grid}]: {len(rows)} probes, worst err/tol {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("case,n_y,grid", [("shipped", 2000, SMALL), ("branch", 2049, SMALL), ("shipped", 2049, DEFAULT)])
def test_sums_against_mp(gpu_engine, case, n_y, grid):
    """Y_B under sigma_y = 9 and under W = 1, Gamma = 0.5 and 50."""
    cfgm = pkg("config")
    c, (y_lo, y_hi, step, ys), F, nd = device_ref(gpu_engine, case, grid, n_y)
    kw = dict(n_y=n_y, nz=grid[0], z_max=grid[1])
    gs = (0.5, 50.0)
    pts = np.repeat(cfgm.to_point(dict(c, source_shape_sigma_y=9.0)), len(gs))
    gauss = gpu_engine.yields(pts, wash=blocks([(g, 0) for g in gs]), **kw).cpu().numpy()
    flat = gpu_engine.yields(pts, wash=blocks([(g, 0) for g in gs]), window=FLAT, **kw).cpu().numpy()
    worst = 0.0
    for name, base, recs in (("sigma_y = 9", Y.win_gauss(nd, 9.0), gauss), ("W = 1", Y.win_one(nd), flat)):
        for g, rec in zip(gs, recs):
            win = WR.win_wash(nd, base, c, g)
            assert not win.undecided
            rel, ratio, bad = Y.compare_sum(rec[0], Y.sum_ref(nd, win))
            print(f"wash Y_B [{case}, n_y = {n_y}, z grid {grid}, {name}, Gamma = {g}]: {float(rec[0])!r}, "
                  f"rel err {rel:.3e}, err/tol {ratio:.3f}")
            assert bad is None, (name, g, bad)
            worst = max(worst, ratio)
    assert worst < 1.0


def test_dead_source(gpu_engine):
    """m_chi = 1e6: every term underflows, Y_B is exactly +0 and depletion leaves Y_chi0."""
    c = Y.cfg_of("dead source")
    out = gpu_engine.yields(np.repeat(pkg("config").to_point(c), 2), wash=blocks([(0.5, 1), (0.0, 1)]), n_y=2000,
                            nz=SMALL[0], z_max=SMALL[1]).cpu().numpy()
    for rec in out:
        assert Y.is_pos_zero(float(rec[0])) and rec[1] == c["Y_chi_init"]


# ---------------------------------------------------------------------------------------------
# depletion
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_y,grid", [(2000, SMALL), (2049, DEFAULT)])
def test_depletion_bits(gpu_engine, n_y, grid):
    cfgm = pkg("config")
    c = full_cfg(BASE_CFG)
    big = dict(c, incident_flux_scale=1e-3)
    pts = np.concatenate([cfgm.to_point(x) for x in (c, c, c, c, big, big)])
    rows = [(0.0, 0), (0.0, 1), (0.5, 1), (0.5, 0), (0.0, 0), (0.7, 1)]
    out = gpu_engine.yields(pts, wash=blocks(rows), n_y=n_y, nz=grid[0], z_max=grid[1]).cpu().numpy()
    Y0 = np.float64(c["Y_chi_init"])
    for b, lo, hi in ((0, 1, 4), (4, 5, 6)):
        base, YB0 = out[b], out[b, 0]
        assert base[1] == Y0
        for (g, dep), rec in zip(rows[lo:hi], out[lo:hi]):
            want = Y0 - YB0 if dep else Y0                   # one IEEE subtraction
            assert same(rec[1:2], np.array([want])), (g, dep)
            if g == 0.0:
                assert same(rec[0:1], base[0:1])             # the second accumulator is the first's twin
            else:
                assert 0.0 < rec[0] < YB0
            # the epilogue on (Y_B, Y_chi), fpy:413-417 in its operation order
            rho_dm = (rec[1] * Y.S0_M3) * (np.float64(c["m_chi_GeV"]) * Y.GEV_TO_KG)
            rho_b = (rec[0] * Y.S0_M3) * Y.M_PROTON_KG
            assert same(rec[2:5], np.array([rho_b, rho_dm, rho_dm / max(rho_b, 1e-300)]))
    # the reference's flux = 1e-3 case: a negative Y_chi, not clamped, and the ratio the epilogue forms from it
    assert out[5, 1] < 0.0 and out[5, 3] < 0.0 and out[5, 4] < 0.0
    print(f"depletion [n_y = {n_y}, z grid {grid}]: Y_chi = {out[1, 1]!r} (DM/B {out[1, 4]!r}); flux 1e-3: Y_chi = {out[5, 1]!r}")


# ---------------------------------------------------------------------------------------------
# the reference program's tight solves
# ---------------------------------------------------------------------------------------------
def test_golden_cases(gpu_engine):
    cfgm, W = pkg("config"), pkg("wash")
    cases = golden_cases()
    # an unknown regime starts thermal in the ODE branch (fpy:399-400); the kernels give NaN for it as
    # the fast path has no value, so that case runs as what the reference integrated
    cfgs = [dict(c, regime="thermal") if not str(c["regime"]).lower().startswith(("non", "therm")) else c
            for _, c, _ in cases]
    pts = np.concatenate([cfgm.to_point(c) for c in cfgs])
    ode = np.concatenate([W.from_config(c) for c in cfgs])
    out = gpu_engine.yields(pts, wash=ode, n_y=8000).cpu().numpy()
    worst = {}
    for (i, c, tight), rec in zip(cases, out):
        if tight is None:                                    # zero-width / inverted window: the fast path's 0.0
            assert Y.is_pos_zero(float(rec[0])) and rec[1] == c["Y_chi_init"]
            continue
        for k in ("Y_B", "Y_chi"):
            d = abs(rec[COL[k]] - tight[k]) / abs(tight[k])
            worst[bound_for(c)] = max(worst.get(bound_for(c), 0.0), d)
            assert d <= bound_for(c), (i, k, rec[COL[k]], tight[k], d)
    print("golden sigma_v = 0 cases, device against `tight`: " +
          ", ".join(f"worst {w:.3e} (bound {b:.3e})" for b, w in sorted(worst.items())))


# ---------------------------------------------------------------------------------------------
# the grid decode
# ---------------------------------------------------------------------------------------------
def expand(eng, c, axes, wash):
    """(points, ODE records, window records or None) of the grid in C order, last axis fastest."""
    cfgm, W = pkg("config"), pkg("window")
    names = [n for n, _ in axes]
    grids = np.meshgrid(*[np.asarray(v, dtype=np.float64) for _, v in axes], indexing="ij")
    cols = {n: g.reshape(-1) for n, g in zip(names, grids)}
    total = grids[0].size
    pts = np.repeat(cfgm.to_point(c), total)
    ode = np.repeat(pkg("wash").to_wash(wash), total)
    win = None
    for n, v in cols.items():
        if n == "delta_LZ":
            pts["P_chi_to_B"] = eng.p_closed_form(v).cpu().numpy()
        elif n == "Gamma_wash_over_H":
            ode[n] = v
        elif n == "deplete_DM_from_source":
            ode[n] = (v != 0.0).astype(np.int32)
        elif n == "window_y0":
            win = np.repeat(W.to_window(WIN_BASE), total)
            win["y0"] = v
        else:
            pts[n] = v
    return pts, ode, win


WIN_BASE = {"kind": "plateau", "half_width": 2.0, "sigma_lo": 3.0, "sigma_hi": 5.0}
GRID = [("delta_LZ", np.linspace(0.01, 0.2, 5)), ("Gamma_wash_over_H", np.array([0.0, 0.3, 5.0, 50.0])),
        ("deplete_DM_from_source", np.array([0.0, 1.0]))]


@pytest.mark.parametrize("windowed,n_y,grid", [(False, 2000, SMALL), (True, 2049, DEFAULT), (True, 2000, "continuum")])
def test_grid_against_explicit_points(gpu_engine, windowed, n_y, grid):
    eng = gpu_engine
    cont = grid == "continuum"
    kw = dict(n_y=n_y, continuum=True) if cont else dict(n_y=n_y, nz=grid[0], z_max=grid[1])
    c = full_cfg(BASE_CFG)
    axes = ([("window_y0", np.array([-2.0, 1.0]))] if windowed else []) + GRID
    win = WIN_BASE if windowed else None
    total = int(np.prod([len(v) for _, v in axes]))
    assert total == (80 if windowed else 40)
    pts, ode, wins = expand(eng, c, axes, {"Gamma_wash_over_H": 7.0})
    want = eng.yields(pts, wash=ode, window=wins, **kw).cpu().numpy()
    assert np.all(np.isfinite(want)) and len({float(x) for x in want[:, 0]}) >= total // 2
    whole = eng.sweep(c, axes, 0, total, wash={"Gamma_wash_over_H": 7.0}, window=win, **kw).cpu().numpy()
    assert same(whole, want)
    for chunk in (7, 32):                                    # two chunkings
        got = np.concatenate([eng.sweep(c, axes, s, min(chunk, total - s), wash={"Gamma_wash_over_H": 7.0}, window=win,
                                        **kw).cpu().numpy() for s in range(0, total, chunk)])
        assert same(got, want)
    assert same(eng.sweep(c, axes, 11, 13, wash=NONE, window=win, **kw), want[11:24])   # start != 0


def test_wash_axis_refused_elsewhere(gpu_engine):
    """A LZQ_F_GAMMA_WASH axis is an unknown field to every entry point but the *_wash ones."""
    eng, nat, cfgm = gpu_engine, pkg("_native"), pkg("config")
    L = eng.lib
    vals = torch.tensor([0.0, 1.0], dtype=torch.float64, device=eng.device)
    arr = (nat.LzqAxis * 1)()
    arr[0].field, arr[0].n, arr[0].values = nat.WASH_FIELD["Gamma_wash_over_H"], 2, vals.data_ptr()
    base = cfgm.to_ctypes_point(cfgm.to_point(full_cfg(BASE_CFG)))
    win = nat.LzqWindow.from_buffer_copy(pkg("window").to_window(FLAT).tobytes())
    work = torch.zeros(2006, dtype=torch.float64, device=eng.device)
    out = torch.zeros((2, 6), dtype=torch.float64, device=eng.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    calls = [
        L.lzq_sweep_grid(ctypes.byref(base), arr, 1, 0, 2, 2000, 13, 3.0, None, vp(out), None),
        L.lzq_sweep_grid_from_ztables(ctypes.byref(base), arr, 1, 0, 2, 2000, 13, 3.0, None, vp(work), 2006, vp(out), None),
        L.lzq_sweep_grid_from_ztables_window(ctypes.byref(base), ctypes.byref(win), arr, 1, 0, 2, 2000, 13, 3.0, None,
                                             vp(work), 2006, None, vp(out), None),
        L.lzq_sweep_grid_ztables(ctypes.byref(base), arr, 1, 2000, 13, 3.0, vp(work), 2006, None),
    ]
    for rc in calls:
        assert rc == -1
    assert b"unknown field 96" in L.lzq_last_error()
    with pytest.raises(ValueError, match="unknown sweep field"):
        eng.sweep(full_cfg(BASE_CFG), [("Gamma_wash_over_H", [0.0, 1.0])], 0, 2, n_y=2000)
    # two axes writing one wash field
    with pytest.raises(nat.LzqError, match="writes a wash field"):
        eng.sweep(full_cfg(BASE_CFG), [("Gamma_wash_over_H", [0.0]), ("Gamma_wash_over_H", [1.0])], 0, 1, n_y=2000,
                  nz=13, z_max=3.0, wash=NONE)
    with pytest.raises(ValueError, match="sigma_v_chi_GeV_m2"):
        eng.sweep(full_cfg(BASE_CFG), [], 0, 1, n_y=2000, nz=13, z_max=3.0, wash={"sigma_v_chi_GeV_m2": 1e-20})
    # a refused block in device memory: NaN yields, no table read
    bad = blocks([(math.nan, 0), (0.5, 0)])
    rec = eng.yields(np.repeat(cfgm.to_point(full_cfg(BASE_CFG)), 2), wash=eng.ode_params_to_device(bad), n_y=2000,
                     nz=13, z_max=3.0).cpu().numpy()
    assert np.all(np.isnan(rec[0, :5])) and np.all(np.isfinite(rec[1]))


# ---------------------------------------------------------------------------------------------
# the solve
# ---------------------------------------------------------------------------------------------
def host_ratio(c, n_y, grid, terms_box, cont=False):
    """DM/B(Gamma) of the host restatement (fpy:413-417 on its Y_B, Y_chi)."""
    def f(g):
        YB, Ychi, terms_box[0] = WR.restate(dict(c, Gamma_wash_over_H=g), n_y=n_y, nz=grid[0], z_max=grid[1],
                                            terms=terms_box[0], continuum=cont)
        return (Ychi * Y.S0_M3) * (c["m_chi_GeV"] * Y.GEV_TO_KG) / max((YB * Y.S0_M3) * Y.M_PROTON_KG, 1e-300)
    return f


@pytest.mark.parametrize("windowed,cont", [(False, False), (True, False), (False, True)],
                         ids=["sigma_y=9", "W=1", "continuum-sigma_y=9"])
def test_solve_gamma_for_the_planck_ratio(gpu_engine, windowed, cont):
    """The shipped point with depletion: depletion alone gives DM/B = 4.676, so a Gamma_wash/H with
    DM/B = 5.357 exists."""
    from scipy.optimize import brentq
    eng = gpu_engine
    n_y, grid, xtol = 2049, DEFAULT, 1e-12
    kw = dict(n_y=n_y, continuum=True) if cont else dict(n_y=n_y, nz=grid[0], z_max=grid[1])
    c = full_cfg(dict(BASE_CFG, deplete_DM_from_source=True))
    win = FLAT if windowed else None
    sv = {"field": "Gamma_wash_over_H", "lo": 0.0, "hi": 5.0, "xtol": xtol}
    rec, sol = eng.solve_point(c, sv, wash=DEP, window=win, **kw)
    rec, sol = rec.cpu().numpy(), sol.cpu().numpy()
    x = float(sol[0])
    assert sol[5] == 0.0 and 0.0 < x < 5.0 and sol[1] <= x <= sol[2] and sol[4] <= 64
    assert abs(rec[4] / 5.357 - 1.0) <= 1e-11
    # the stored record is the forward grid kernel's at x, bit for bit
    fwd = eng.sweep(c, [("Gamma_wash_over_H", np.array([x]))], 0, 1, wash=DEP, window=win, **kw)
    assert same(fwd.cpu().numpy()[0], rec)
    # scipy on the host restatement (W = 1: its sigma is the plateau's, wide enough to be 1 on the grid)
    box = [None]
    f = host_ratio(dict(c, source_shape_sigma_y=1e9) if windowed else c, n_y, grid, box, cont)
    x_ref = brentq(lambda g: f(g) - 5.357, 0.0, 5.0, xtol=1e-15, rtol=1e-15)
    h = 1e-4 * x_ref
    S = (math.log(f(x_ref + h)) - math.log(f(x_ref - h))) / (math.log(x_ref + h) - math.log(x_ref - h))
    print(f"Gamma_wash/H with DM/B = 5.357, depletion on [{'W = 1' if windowed else 'sigma_y = 9'}, "
          f"{'continuum' if cont else grid}, n_y = {n_y}]: "
          f"{x!r} (brentq on the host restatement {x_ref!r}, log slope {S:.3f}), {int(sol[4])} evaluations")
    assert abs(x / x_ref - 1.0) <= xtol + 1e-11 / abs(S)


def test_solve_statuses(gpu_engine):
    eng, nat = gpu_engine, pkg("_native")
    kw = dict(n_y=2000, nz=SMALL[0], z_max=SMALL[1])
    c = full_cfg(dict(BASE_CFG, deplete_DM_from_source=True))
    axes = [("I_p", np.array([0.34, 0.3])), ("deplete_DM_from_source", np.array([0.0, 1.0]))]
    ends = eng.sweep(c, axes + [("Gamma_wash_over_H", np.array([0.0, 2.0]))], 0, 8, wash=NONE, **kw).cpu().numpy()
    target = float(math.sqrt(ends[0, 4] * ends[1, 4]))
    sv = {"field": "Gamma_wash_over_H", "lo": 0.0, "hi": 2.0, "target": {"field": "DM_over_B", "value": target}}
    rec, sol = eng.sweep(c, axes, 0, 4, solve=sv, wash=NONE, **kw)
    sol = sol.cpu().numpy()
    assert sol[0, 5] == nat.SOLVE_OK and abs(rec.cpu().numpy()[0, 4] / target - 1.0) <= 1e-11
    # chunk independence
    r2, s2 = eng.sweep(c, axes, 1, 3, solve=sv, wash=NONE, **kw)
    assert same(r2, rec[1:]) and same(s2.cpu().numpy(), sol[1:])
    # a bracket without a sign change
    _, s3 = eng.sweep(c, axes, 0, 4, solve=dict(sv, hi=1e-6), wash=NONE, **kw)
    assert np.all(s3.cpu().numpy()[:, 5] == nat.SOLVE_NO_BRACKET)
    # a flipped header word of the z-sum tables: NaN records, BAD_TABLE
    eng.sweep(c, axes, 0, 4, solve=sv, wash=NONE, **kw)
    word = eng._zwork[3].clone()
    eng._zwork[3] = -word
    try:
        r4, s4 = eng.sweep(c, axes, 0, 4, solve=sv, wash=NONE, **kw)
        fwd = eng.sweep(c, axes, 0, 4, wash=NONE, **kw).cpu().numpy()
    finally:
        eng._zwork[3] = word
        eng._ztab_key = None
    r4, s4 = r4.cpu().numpy(), s4.cpu().numpy()
    assert np.all(s4[:2, 5] == nat.SOLVE_BAD_TABLE) and np.all(np.isnan(r4[:2])) and np.all(np.isnan(s4[:2, 0]))
    assert same(s4[2:], sol[2:]) and same(r4[2:], rec.cpu().numpy()[2:])   # the second table is intact
    assert np.all(np.isnan(fwd[:2, [0, 2, 4]])) and np.all(np.isnan(fwd[1, [1, 3]])) and np.all(np.isfinite(fwd[2:]))


# ---------------------------------------------------------------------------------------------
# the sweep driver
# ---------------------------------------------------------------------------------------------
def test_wash_rule_sweep_solve_block_at_two_world_sizes(tmp_path):
    """A "wash_rule": "quadrature" spec with a solve section, fit-only (--no-table): the same "solve" block
    from one rank and from two (gloo, both on the one GPU), in fresh child processes."""
    import json
    import sys
    from conftest import PKG_NAME
    from test_gpu_dist import run, torchrun
    spec = {"name": "wash", "n_y": 2000, "nz": 13, "z_max": 3.0, "wash_rule": "quadrature",
            "base": {"deplete_DM_from_source": True},
            "axes": [{"field": "I_p", "values": [0.34, 0.3]}, {"field": "delta_LZ", "linspace": [0.01, 0.03, 9]},
                     {"field": "deplete_DM_from_source", "values": [0.0, 1.0]}],
            "solve": {"field": "Gamma_wash_over_H", "lo": 0.0, "hi": 20.0, "target": {"field": "DM_over_B", "value": 40.0}}}
    path = tmp_path / "spec.json"
    path.write_text(json.dumps(spec))
    args = ["--spec", str(path), "--chunk", "7", "--fit", "paper", "--no-table"]
    one, two = tmp_path / "w1", tmp_path / "w2"
    run([sys.executable, "-m", PKG_NAME + ".sweep", *args, "--out", str(one)], 300)
    run(torchrun(2) + ["-m", PKG_NAME + ".sweep", *args, "--out", str(two), "--dist-backend", "gloo"], 300)
    blocks_ = []
    for d in (one, two):
        with open(d / "summary.json") as f:
            blocks_.append(json.load(f)["solve"])
        assert not (d / "table.npy").exists() and not (d / "solve.npy").exists()
    assert blocks_[0] == blocks_[1]
    b = blocks_[0]
    assert b["field"] == "Gamma_wash_over_H" and sum(b["status"].values()) == 36 and b["status"]["ok"] > 0
    assert b["x"] is not None and 0.0 < b["x"]["min"] <= b["x"]["max"] < 20.0
    print(f"wash_rule sweep, solve block: {b['status']}, x {b['x']}")
