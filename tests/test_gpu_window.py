"""The source activity window W(y) on the GPU (include/lzq.h lzq_window; csrc/lzq_window.hip): the
plateau family and tabulated profiles in place of the Gaussian proxy of fpy:262.  Needs an MI355X.

Pinned to tests/golden/golden_window.json, which tests/golden/make_golden_window.py made by running
the reference with source_shape_sigma_y = 1e300 (its own window exactly 1) and bs.aov wrapped to
return A/V(y) W(y), W written in plain Python from the definition.

Tolerances: north_star's 1e-8 gate and the golden tests' 1e-11 guard band on Y_B, exact zeros where
the reference has them.  W alone: the table kind is the host build's bits; the Gaussian kinds are
held to 2 ulp of mpmath's exp at the host's q (exp_sc documents <= 1 ulp).  Everything else is
equality of bits.

Measured on an MI355X (the prints below): worst Y_B error against the reference 7.9e-14, dense,
reuse and facade alike; worst W error of the Gaussian kinds 0.81 ulp.
"""
import numpy as np
import pytest
import torch

from conftest import BASE_CFG, full_cfg, golden, pkg, rel_err
from test_window_host import GAUSS_KINDS, edge_ys, exp_ulps, table_cases, win, around

pytestmark = pytest.mark.gpu
GATE = 1e-8
GUARD = 1e-11
ZGRIDS = [(1200, 30.0), (13, 3.0)]


def bits(t):
    return t.contiguous().view(torch.int64)


def same(a, b):
    """Equal bits (NaN rows included)."""
    return torch.equal(bits(a), bits(b))


def _groups():
    """The fixtures by (table set, n_y, nz, z_max): one batch per launch shape."""
    d = golden("golden_window.json")
    out = {}
    for r in d["cases"]:
        out.setdefault((r["tables"], r["n_y"], r["nz"], r["z_max"]), []).append(r)
    return d["tables"], out


def _tables(sets, name):
    return None if name is None else pkg("window").WindowTables(sets[name]["u"], sets[name]["W"])


def _check(got, ref, what):
    if ref == 0.0:
        assert got == 0.0, (what, got)
        return 0.0
    e = rel_err(got, ref)
    assert e < GATE and e < GUARD, (what, got, ref, e)
    return e


def test_fixtures_dense_reuse_and_facade(gpu_engine):
    """Every fixture through Engine.yields, dense and from shared z-sum tables, and through the
    facade (bs.window)."""
    cfgm, W, B = pkg("config"), pkg("window"), pkg("boltzmann")
    sets, groups = _groups()
    worst = {"dense": 0.0, "reuse": 0.0, "facade": 0.0}
    n = 0
    for (tname, n_y, nz, z_max), rows in groups.items():
        tabs = _tables(sets, tname)
        cfgs = [full_cfg(r["config"]) for r in rows]
        pts = np.concatenate([cfgm.to_point(c) for c in cfgs])
        wins = np.concatenate([W.to_window(r["window"]) for r in rows])
        dense = gpu_engine.yields(pts, n_y=n_y, nz=nz, z_max=z_max, window=wins, window_tables=tabs)
        assert gpu_engine.last_yields_path == "dense"
        # the batch twice over: every z-sum key is then shared, so the tables path is taken
        reuse = gpu_engine.yields(np.concatenate([pts, pts]), n_y=n_y, nz=nz, z_max=z_max, reuse=True,
                                  window=np.concatenate([wins, wins]), window_tables=tabs)
        assert gpu_engine.last_yields_path == "tables"
        assert same(reuse[:len(rows)], dense) and same(reuse[len(rows):], dense)
        for r, c, row in zip(rows, cfgs, dense.cpu().numpy()):
            worst["dense"] = max(worst["dense"], _check(row[0], r["Y_B"], r["window"]))
            worst["reuse"] = worst["dense"]
            cfg = cfgm.Config(**c)
            bs = B.BoltzmannSystem(cfg, cfg.P_chi_to_B)
            bs.aov = B.AoverVKernel(cfg.I_p, cfg.beta_over_H, cfg.T_p_GeV, cfg.v_w, cfg.g_star, z_max=z_max, nz=nz)
            bs.window, bs.window_tables = r["window"], tabs
            got = bs.integrate_YB_by_quadrature(cfg.T_min_over_Tp * cfg.T_p_GeV, cfg.T_max_over_Tp * cfg.T_p_GeV,
                                                n_y=n_y)
            worst["facade"] = max(worst["facade"], _check(got, r["Y_B"], r["window"]))
            assert got == row[0]
            n += 1
    assert n == len(golden("golden_window.json")["cases"]) >= 45   # no fixture is skipped
    print("window fixtures vs reference, worst Y_B rel err:", {k: f"{v:.3e}" for k, v in worst.items()})


def test_facade_S_B_T_and_ode_operators(gpu_engine):
    cfgm, B = pkg("config"), pkg("boltzmann")
    cfg = cfgm.Config(**full_cfg(BASE_CFG))
    bs = B.BoltzmannSystem(cfg, cfg.P_chi_to_B)
    plain = bs.S_B_T(95.0)
    bs.window = win("gauss", sigma_hi=cfg.source_shape_sigma_y)
    # y/sigma against y (1/sigma): q differs by an ulp, W by q^2 2^-52 (q = 0.6 here)
    assert rel_err(bs.S_B_T(95.0), plain) < 1e-14
    bs.window = win("plateau", half_width=200.0)
    assert bs.S_B_T(95.0) > plain
    with pytest.raises(NotImplementedError):
        bs.build_tables(60.0, 160.0)
    bs.window = None
    bs.build_tables(60.0, 160.0)
    bs.window = win("gauss")
    with pytest.raises(NotImplementedError):
        bs.rhs(1.0, [1e-10, 0.0])


def test_window_alone_against_the_host_build(gpu_engine):
    """lzq_window_batch against lzq_window_eval_host at the edges: an ulp either side of
    |u| = half_width and u = 0, every knot, both table ends."""
    W = pkg("window")
    worst = 0.0
    for w in GAUSS_KINDS:
        ys = edge_ys(w)
        q, _ = W.eval_host(w, ys)
        dev = gpu_engine.window(w, ys).cpu().numpy()
        e = max(exp_ulps(Wi, qi) for Wi, qi in zip(dev, q))
        assert e <= 2.0, (w, e)
        worst = max(worst, e)
    print(f"device W (Gaussian kinds) vs mpmath exp at the host's q: worst {worst:.3f} ulp")
    for name, t, w in table_cases():
        ys = list(np.linspace(-80.0, 50.0, 523))
        for uk in t["u"]:
            ys += around(w["y0"] + w["scale"] * uk, 3)
        tabs = W.WindowTables(t["u"], t["W"])
        _, host = W.eval_host(w, ys, tabs)
        dev = gpu_engine.window(w, ys, tabs).cpu().numpy()
        assert np.array_equal(dev, host), (name, w)


def _batch(cfgm):
    """48 points over 4 z-sum keys (so the tables path applies), with an empty-window point and an
    `auto`-regime (NaN) point among them."""
    rng = np.random.default_rng(11)
    keys = [dict(I_p=0.34, beta_over_H=100.0, T_p_GeV=100.0), dict(I_p=0.8, beta_over_H=400.0, T_p_GeV=30.0),
            dict(I_p=0.1, beta_over_H=20.0, T_p_GeV=700.0), dict(I_p=0.34, beta_over_H=100.0, T_p_GeV=100.0,
                                                                 T_min_over_Tp=6.0)]   # the last: y_hi <= y_lo
    cfgs = []
    for i in range(48):
        c = full_cfg(BASE_CFG)
        c.update(keys[i % 4])
        c.update(m_chi_GeV=float(10 ** rng.uniform(-1, 3.5)), source_shape_sigma_y=float(rng.uniform(2.0, 30.0)),
                 P_chi_to_B=float(rng.uniform(0, 1)), incident_flux_scale=float(10 ** rng.uniform(-10, -6)))
        cfgs.append(c)
    cfgs[5]["regime"] = "auto"
    return cfgs, np.concatenate([cfgm.to_point(c) for c in cfgs])


@pytest.mark.parametrize("nz,z_max", ZGRIDS)
@pytest.mark.parametrize("reuse", [False, True])
def test_equal_bits(gpu_engine, nz, z_max, reuse):
    cfgm, W = pkg("config"), pkg("window")
    cfgs, pts = _batch(cfgm)
    kw = dict(n_y=2000, nz=nz, z_max=z_max, reuse=reuse)
    path = "tables" if reuse else "dense"
    head = gpu_engine.yields(pts, **kw)
    assert torch.isnan(head[5, 0]) and float(head[3, 0]) == 0.0 and float(head[0, 0]) > 0.0
    # a GAUSS block with the point's own sigma_y is the headline
    own = np.concatenate([W.to_window(win("gauss", sigma_hi=c["source_shape_sigma_y"])) for c in cfgs])
    g = gpu_engine.yields(pts, window=own, **kw)
    assert gpu_engine.last_yields_path == path
    assert same(g, head)
    # PLATEAU(0, 0, sigma, sigma) is GAUSS(sigma)
    plat = np.concatenate([W.to_window(win("plateau", sigma_lo=c["source_shape_sigma_y"],
                                           sigma_hi=c["source_shape_sigma_y"])) for c in cfgs])
    assert same(gpu_engine.yields(pts, window=plat, **kw), head)
    # a plateau over the whole range is the headline at sigma_y = 1e300 (one block for all points)
    flat = pts.copy()
    flat["source_shape_sigma_y"] = 1e300
    assert same(gpu_engine.yields(pts, window=win("plateau", y0=3.0, half_width=200.0), **kw),
                gpu_engine.yields(flat, **kw))


@pytest.mark.parametrize("nz,z_max", ZGRIDS)
def test_dense_equals_reuse_and_points_are_independent(gpu_engine, nz, z_max):
    """Every kind in one batch: dense = reuse; a point's record does not depend on its neighbours
    (permuted, split)."""
    cfgm, W = pkg("config"), pkg("window")
    t = golden("golden_window.json")["tables"]["k1024"]
    tabs = gpu_engine.window_tables_to_device(W.WindowTables(t["u"], t["W"]))
    cfgs, pts = _batch(cfgm)
    rng = np.random.default_rng(2)
    blocks = []
    for i in range(len(cfgs)):
        k = i % 3
        if k == 0:
            blocks.append(win("gauss", sigma_hi=float(rng.uniform(1, 20))))
        elif k == 1:
            blocks.append(win("plateau", y0=float(rng.uniform(-60, 70)), half_width=float(rng.uniform(0, 30)),
                              sigma_lo=float(10 ** rng.uniform(-3, 1.3)), sigma_hi=float(10 ** rng.uniform(-3, 1.3))))
        else:
            blocks.append(win("table", table=int(rng.integers(0, 2)), y0=float(rng.uniform(-10, 10)),
                              scale=float(rng.uniform(0.2, 4.0))))
    wins = np.concatenate([W.to_window(b) for b in blocks])
    kw = dict(n_y=2000, nz=nz, z_max=z_max, window_tables=tabs)
    dense = gpu_engine.yields(pts, window=wins, **kw)
    assert gpu_engine.last_yields_path == "dense"
    reuse = gpu_engine.yields(pts, window=wins, reuse=True, **kw)
    assert gpu_engine.last_yields_path == "tables"
    assert same(dense, reuse)
    ok = [i for i in range(len(cfgs)) if i % 4 != 3 and i != 5]
    assert float(dense[ok, 0].min()) >= 0.0 and int((dense[ok, 0] > 0).sum()) > len(ok) // 2
    perm = rng.permutation(len(cfgs))
    for r in (False, True):
        p = gpu_engine.yields(pts[perm], window=wins[perm], reuse=r, **kw)
        assert same(p, dense[torch.as_tensor(perm, device=dense.device)])
        parts = [gpu_engine.yields(pts[a:b], window=wins[a:b], reuse=r, **kw) for a, b in ((0, 1), (1, 18), (18, 48))]
        assert same(torch.cat(parts), dense)


def test_bad_blocks_and_arguments(gpu_engine):
    cfgm, W, N = pkg("config"), pkg("window"), pkg("_native")
    pts = np.repeat(cfgm.to_point(full_cfg(BASE_CFG)), 4)
    with pytest.raises(N.LzqError, match="sigma"):
        gpu_engine.yields(pts, window=win("gauss", sigma_hi=0.0))
    with pytest.raises(N.LzqError, match="table index"):
        gpu_engine.yields(pts, window=win("table"))
    with pytest.raises(ValueError):
        gpu_engine.yields(pts, window=win("gauss"), aov=full_cfg(BASE_CFG))
    with pytest.raises(ValueError):
        gpu_engine.yields(pts, window=np.repeat(W.to_window(win("gauss")), 3))
    # a block that reaches the kernels unchecked (device records) gives NaN, never a number
    recs = np.repeat(W.to_window(win("gauss", sigma_hi=9.0)), 4)
    recs["sigma_hi"][1] = -1.0
    recs["kind"][2] = 9
    recs["kind"][3], recs["table"][3] = N.WIN_TABLE, 5
    d_win = torch.from_numpy(recs.view(np.uint8).copy()).to(gpu_engine.device)
    for r in (False, True):
        out = gpu_engine.yields(pts, window=d_win, reuse=r, n_y=2000).cpu().numpy()
        assert out[0, 0] > 0 and np.isnan(out[1:, 0]).all()


def test_ode_takes_no_window(gpu_engine):
    cfgm, S = pkg("config"), pkg("sweep")
    c = dict(full_cfg(BASE_CFG), Gamma_wash_over_H=0.5, T_max_over_Tp=1.6, T_min_over_Tp=0.6)
    with pytest.raises(NotImplementedError):
        gpu_engine.ode(cfgm.to_point(c), cfgm.to_ode_params(c), window=win("gauss"))
    spec = S.SweepSpec("w", c, [("window_y0", np.array([0.0, 1.0]))], n_y=2000,
                       window=S.WindowSpec({"kind": "plateau"}))
    with pytest.raises(ValueError, match="ODE"):
        S.run_sweep(spec, gpu_engine, log=lambda s: None)


# ---- a window sweep end to end -----------------------------------------------------------------
def _sweep_spec(kind="plateau"):
    S = pkg("sweep")
    if kind == "table":
        t = golden("golden_window.json")["tables"]["k1024"]
        return S.SweepSpec("wt", full_cfg(BASE_CFG), [("window_table", np.array([0.0, 1.0])),
                                                      ("window_scale", np.array([0.5, 1.0, 3.0])),
                                                      ("delta_LZ", np.logspace(-3, 0, 4))], n_y=2000,
                           window=S.WindowSpec({"kind": "table", "y0": 2.0}, t["u"], t["W"]))
    return S.SweepSpec("w345", full_cfg(BASE_CFG), [("window_y0", np.array([-6.0, 0.0, 8.0])),
                                                    ("window_sigma", np.array([2.0, 5.0, 9.0, 20.0])),
                                                    ("delta_LZ", np.logspace(-3, 0, 5))], n_y=2000,
                       window=S.WindowSpec({"kind": "plateau", "half_width": 3.0}))


@pytest.fixture(scope="module")
def sweep_table(gpu_engine):
    """The 3 x 4 x 5 grid, dense in one chunk: the table every variant has to reproduce."""
    return pkg("sweep").run_sweep(_sweep_spec(), gpu_engine, chunk=1 << 20, log=lambda s: None)


@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("chunk", [1 << 20, 7])
def test_window_sweep_variants_and_fit(gpu_engine, sweep_table, chunk, reuse):
    S, F, cfgm, W = pkg("sweep"), pkg("fit"), pkg("config"), pkg("window")
    spec = _sweep_spec()
    assert spec.total == 60
    table = S.run_sweep(spec, gpu_engine, chunk=chunk, log=lambda s: None, reuse=reuse)
    assert same(table, sweep_table)
    if reuse:
        assert gpu_engine.last_yields_path == "tables"
    # per-point Engine.yields with the block and P that the grid index decodes to
    t = table.cpu().numpy()
    for i in (0, 4, 5, 23, 38, 59):
        p = spec.point_params(i)
        c = dict(spec.base, P_chi_to_B=float(gpu_engine.p_closed_form([p["delta_LZ"]]).cpu().numpy()[0]))
        one = gpu_engine.yields(cfgm.to_point(c), n_y=2000,
                                window=win("plateau", y0=p["window_y0"], half_width=3.0, sigma_lo=p["window_sigma"],
                                           sigma_hi=p["window_sigma"])).cpu().numpy()[0]
        assert np.array_equal(one.view(np.int64), t[i].view(np.int64)), i
    assert len(np.unique(t[:, 0])) == 60   # both window axes and delta_LZ move Y_B
    # with a fit: the device state equals HostFit on that table
    yb, dm = np.median(t[:, 0]), np.median(t[:, 4])
    fit = F.FitSpec.from_json({"terms": [{"field": "Y_B", "target": float(yb), "sigma": float(abs(yb))},
                                         {"field": "DM_over_B", "target": float(dm), "sigma": float(abs(dm))}],
                               "levels": [0.5, 2.0], "maps": [["window_y0", "window_sigma"], ["delta_LZ"]],
                               "select": {"level": 2.0, "cap": 20}})
    tab2, res = S.run_sweep(spec, gpu_engine, chunk=chunk, log=lambda s: None, reuse=reuse, fit=fit)
    assert same(tab2, sweep_table)
    h = F.HostFit(fit, fit.resolve(spec))
    h.update(t, 0)
    assert F.differences(res, h.result()) == []


@pytest.mark.parametrize("kind", ["crossings", "profile"])
def test_crossing_and_profile_specs_carry_a_window(gpu_engine, kind):
    """Their P goes in as the per-point override: with a GAUSS window of the base's own sigma_y the
    rows are the spec's without a window, bit for bit; another sigma moves them."""
    S = pkg("sweep")
    base = full_cfg(BASE_CFG)
    if kind == "crossings":
        axes = [("m_mix", np.logspace(-2, -0.5, 3)), ("dprime", np.logspace(-1, 0.5, 4))]
        extra = dict(crossings=S.CrossingSpec(n_cross=3))
    else:
        axes = [("y_B", np.linspace(0.5, 2.0, 3)), ("lambda_tr_eff", np.logspace(-2, 0, 4))]
        extra = dict(profile=S.ProfileSpec())
    plain = S.run_sweep(S.SweepSpec("p", base, axes, n_y=2000, **extra), gpu_engine, log=lambda s: None)
    sig = np.array([base["source_shape_sigma_y"], 4.0])
    spec = S.SweepSpec("pw", base, axes + [("window_sigma_hi", sig)], n_y=2000, window=S.WindowSpec({"kind": "gauss"}),
                       **extra)
    for chunk, reuse in ((1 << 20, False), (5, True)):
        w = S.run_sweep(spec, gpu_engine, chunk=chunk, log=lambda s: None, reuse=reuse)
        assert same(w[0::2], plain)
        assert bool((w[1::2, 0] < w[0::2, 0]).any()) and not bool((w[1::2, 0] > w[0::2, 0]).any())


def test_table_window_sweep(gpu_engine):
    S = pkg("sweep")
    spec = _sweep_spec("table")
    a = S.run_sweep(spec, gpu_engine, chunk=1 << 20, log=lambda s: None)
    b = S.run_sweep(spec, gpu_engine, chunk=5, log=lambda s: None, reuse=True)
    assert same(a, b) and bool((a[:, 0] > 0).all()) and len(np.unique(a[:, 0].cpu().numpy())) == 24
