"""One parameter per grid point solved for a target yield on the device (lzq_sweep_grid_solve;
csrc/lzq_solve.hip, the rule in csrc/lzq_solve.h).  Needs an MI355X.

Roots are pinned to the reference's own (tests/golden/golden_solve.json: scipy's brentq on the
reference) within |x/x_ref - 1| <= xtol + 1e-11/|S| -- the suite's guard band on yields against the
reference is 1e-11, and a relative error eps in the field moves the root by eps/|S|, S the fixture's
logarithmic slope.  Everything else is equality of bits: the stored record against the forward sweep
at x*, the bracket's signs by forward sweeps at its ends, equivalent forms, and splits of the range.
n_y = 2000 and the (13, 3.0) z grid unless a test says otherwise.
"""
import math

import numpy as np
import pytest
import torch

from conftest import BASE_CFG, full_cfg, golden, pkg

pytestmark = pytest.mark.gpu
ZS = dict(nz=13, z_max=3.0)
PLATEAU = {"kind": "plateau", "y0": -5.0, "half_width": 3.0, "sigma_lo": 4.0, "sigma_hi": 6.0}
M_CHI = ("m_chi_GeV", np.linspace(0.8, 1.2, 10))
V_W = ("v_w", np.linspace(0.25, 0.40, 7))
HW = {"field": "window_half_width", "lo": 0.0, "hi": 40.0}
DMB = 4  # DM_over_B's column
XTOL = 1e-12


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def solve(eng, cfg, axes, sv, start=0, count=None, window=None, tables=None, n_y=2000, **z):
    total = int(np.prod([len(v) for _, v in axes])) if axes else 1
    count = total - start if count is None else count
    rec, sol = eng.sweep(cfg, axes, start, count, n_y=n_y, window=window, window_tables=tables, solve=sv, **(z or ZS))
    torch.cuda.synchronize()
    return rec.cpu().numpy(), sol.cpu().numpy()


def forward(eng, cfg, axes, window=None, tables=None, n_y=2000, **z):
    total = int(np.prod([len(v) for _, v in axes]))
    out = eng.sweep(cfg, axes, 0, total, n_y=n_y, reuse=True, window=window, window_tables=tables, **(z or ZS))
    assert eng.last_reuse == "tables"
    return out.cpu().numpy()


def forward_at(eng, cfg, axes, field, xs, window=None):
    """The forward sweep of every grid point with `field` set to that point's own xs[i]: the grid with
    one more (fastest) axis holding all the xs, its diagonal taken."""
    n = len(xs)
    out = forward(eng, cfg, list(axes) + [(field, np.asarray(xs, dtype=np.float64))], window=window)
    return out.reshape(n, n, 6)[np.arange(n), np.arange(n)]


# ---- (a) every fixture as a one-point grid -------------------------------------------------------
CASES = golden("golden_solve.json")["cases"]
TABLES = golden("golden_solve.json")["tables"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_fixture_roots(gpu_engine, case):
    sv = dict(case["solve"], xtol=XTOL)
    t = TABLES[case["tables"]] if case["tables"] else None
    rec, sol = solve(gpu_engine, full_cfg(case["config"]), [], sv, window=case["window"],
                     tables=(t["u"], t["W"]) if t else None, n_y=case["n_y"], nz=case["nz"], z_max=case["z_max"])
    x, x_lo, x_hi, residual, evals, status = sol[0]
    err = abs(x / case["x_ref"] - 1.0)
    tol = XTOL + 1e-11 / abs(case["log_slope"])
    print(f"{case['name']}: x = {x!r} x_ref = {case['x_ref']!r} err = {err:.3e} tol = {tol:.3e} evals = {evals:.0f} "
          f"status = {status:.0f} residual = {residual:.3e}")
    assert status == 0 and 2 <= evals <= 64
    assert x_lo <= x <= x_hi
    assert (x_hi - x_lo) <= XTOL * max(abs(x_lo), abs(x_hi)) or np.nextafter(x_lo, x_hi) == x_hi
    assert err <= tol
    col = pkg("_native").YIELD_FIELDS.index(sv["target"]["field"])
    assert residual == rec[0, col] - sv["target"]["value"]


# ---- (b) the record, the bracket's signs and the residual on a 70-point grid ------------------------
@pytest.fixture(scope="module")
def hw_grid(gpu_engine):
    """The 10 x 7 (m_chi, v_w) grid with a plateau window; its DM_over_B at both ends of the
    half-width range, and a target every point brackets."""
    cfg = full_cfg(BASE_CFG)
    ends = forward(gpu_engine, cfg, [M_CHI, V_W, ("window_half_width", np.array([HW["lo"], HW["hi"]]))],
                   window=PLATEAU).reshape(70, 2, 6)[:, :, DMB]
    d_lo, d_hi = ends[:, 0], ends[:, 1]
    assert d_hi.max() < d_lo.min()                     # DM_over_B falls as the window widens
    target = float(math.sqrt(d_hi.max() * d_lo.min()))
    sv = dict(HW, target={"field": "DM_over_B", "value": target}, xtol=XTOL)
    rec, sol = solve(gpu_engine, cfg, [M_CHI, V_W], sv, window=PLATEAU)
    return cfg, sv, d_lo, d_hi, rec, sol


def test_record_bracket_and_residual(gpu_engine, hw_grid):
    cfg, sv, _, _, rec, sol = hw_grid
    t = sv["target"]["value"]
    x, x_lo, x_hi, residual, evals, status = sol.T
    assert np.all(status == 0) and np.all((evals >= 3) & (evals <= 64))
    assert np.all((x_lo <= x) & (x <= x_hi) & (sv["lo"] <= x_lo) & (x_hi <= sv["hi"]))
    assert np.all((x == x_lo) | (x == x_hi))
    assert np.all((x_hi - x_lo <= XTOL * np.maximum(np.abs(x_lo), np.abs(x_hi))) | (np.nextafter(x_lo, x_hi) == x_hi))
    assert len(np.unique(x)) >= 50      # (m_chi v_w decides the root: equal products coincide)
    # the stored record is the forward sweep's at x*, bit for bit
    at_x = forward_at(gpu_engine, cfg, [M_CHI, V_W], "window_half_width", x, window=PLATEAU)
    assert same(rec, at_x)
    # residual = f(x*) as numpy forms it
    assert same(residual, rec[:, DMB] - t)
    # f at the bracket's ends: opposite strict signs, or an exact zero
    f_lo = forward_at(gpu_engine, cfg, [M_CHI, V_W], "window_half_width", x_lo, window=PLATEAU)[:, DMB] - t
    f_hi = forward_at(gpu_engine, cfg, [M_CHI, V_W], "window_half_width", x_hi, window=PLATEAU)[:, DMB] - t
    assert np.all(((f_lo < 0) != (f_hi < 0)) & (f_lo != 0) & (f_hi != 0) | ((f_lo == 0) & (f_hi == 0) & (x_lo == x_hi)))
    assert np.all(np.abs(residual) == np.minimum(np.abs(f_lo), np.abs(f_hi)))
    print(f"70-point half-width solve: evals mean {evals.mean():.2f} max {evals.max():.0f}, "
          f"max |residual|/target {np.abs(residual).max() / t:.3e}")


# ---- (c) equal bits across equivalent forms -------------------------------------------------------
def test_gauss_block_equals_the_points_gaussian(gpu_engine):
    cfg = full_cfg(BASE_CFG)
    axes = [("m_chi_GeV", np.linspace(0.5, 2.0, 17))]
    ends = forward(gpu_engine, cfg, axes + [("source_shape_sigma_y", np.array([1.0, 50.0]))]).reshape(17, 2, 6)[:, :, DMB]
    assert ends[:, 1].max() < ends[:, 0].min()
    target = {"field": "DM_over_B", "value": float(math.sqrt(ends[:, 1].max() * ends[:, 0].min()))}
    a = solve(gpu_engine, cfg, axes, {"field": "source_shape_sigma_y", "lo": 1.0, "hi": 50.0, "target": target})
    b = solve(gpu_engine, cfg, axes, {"field": "window_sigma", "lo": 1.0, "hi": 50.0, "target": target},
              window={"kind": "gauss", "sigma_hi": cfg["source_shape_sigma_y"]})
    assert np.all(a[1][:, 5] == 0) and len(np.unique(a[1][:, 0])) == 17
    assert same(a[1], b[1])      # x, bracket, residual, evaluations, status
    assert same(a[0], b[0])      # the record


# ---- (d) equal bits across splits ----------------------------------------------------------------
def test_split_ranges_equal_the_whole(gpu_engine, hw_grid):
    cfg, sv, _, _, rec, sol = hw_grid
    for start, count in ((0, 1), (0, 5), (0, 17), (17, 5), (22, 48), (69, 1), (70, 0), (16, 17)):
        r, s = solve(gpu_engine, cfg, [M_CHI, V_W], sv, start, count, window=PLATEAU)
        assert r.shape == s.shape == (count, 6)
        assert same(r, rec[start:start + count]) and same(s, sol[start:start + count]), (start, count)


def test_start_past_2_to_32(gpu_engine):
    """A 256^5 grid: five points from flat index 2^32 + 12345 on equal those of the one-point grids
    of their decoded coordinates."""
    cfg = full_cfg(BASE_CFG)
    names = ("g_chi", "v_w", "g_star_s", "incident_flux_scale", "m_chi_GeV")
    base = (2.0, 0.30, 106.75, 1.07e-9, 0.95)
    axes = [(n, b * np.linspace(0.9, 1.1, 256)) for n, b in zip(names, base)]
    start = (1 << 32) + 12345
    first = [(n, np.array([v[c]])) for (n, v), c in zip(axes, np.unravel_index(start, (256,) * 5))]
    ends = forward(gpu_engine, cfg, first + [("window_half_width", np.array([HW["lo"], HW["hi"]]))], window=PLATEAU)
    sv = dict(HW, target={"field": "DM_over_B", "value": float(math.sqrt(ends[0, DMB] * ends[1, DMB]))}, xtol=XTOL)
    rec, sol = solve(gpu_engine, cfg, axes, sv, start, 5, window=PLATEAU)
    assert np.all(sol[:, 5] == 0)
    for i in range(5):
        coords = np.unravel_index(start + i, (256,) * 5)
        one = [(n, np.array([v[c]])) for (n, v), c in zip(axes, coords)]
        r1, s1 = solve(gpu_engine, cfg, one, sv, window=PLATEAU)
        assert same(r1[0], rec[i]) and same(s1[0], sol[i]), i


# ---- (e) statuses ----------------------------------------------------------------------------------
def _assert_refused(rec, sol, rows, status, sv):
    assert np.all(sol[rows, 5] == status)
    assert np.all(np.isnan(rec[rows])) and np.all(np.isnan(sol[rows][:, [0, 3]]))
    assert np.all(sol[rows, 1] == sv["lo"]) and np.all(sol[rows, 2] == sv["hi"])


def test_some_points_without_a_bracket(gpu_engine, hw_grid):
    cfg, _, d_lo, d_hi, _, _ = hw_grid
    target = float(np.median(d_lo))            # about half the points start below it at both ends
    sv = dict(HW, target={"field": "DM_over_B", "value": target}, xtol=XTOL)
    rec, sol = solve(gpu_engine, cfg, [M_CHI, V_W], sv, window=PLATEAU)
    f_lo, f_hi = d_lo - target, d_hi - target
    none = (f_lo != 0) & (f_hi != 0) & ((f_lo < 0) == (f_hi < 0))
    assert 10 <= none.sum() <= 60
    assert np.array_equal(sol[:, 5] == 2, none)
    _assert_refused(rec, sol, none, 2, sv)
    assert np.all(sol[none, 4] == 2)           # detected after the two ends
    ok = ~none
    assert np.all(sol[ok, 5] == 0) and np.all(np.isfinite(rec[ok])) and np.all(np.isfinite(sol[ok]))
    S = pkg("solve").summary(sv, sol)
    assert S["status"]["no_bracket"] == int(none.sum()) and S["status"]["ok"] == int(ok.sum())


def test_empty_y_range_has_no_bracket(gpu_engine):
    cfg = full_cfg(dict(BASE_CFG, T_max_over_Tp=0.5, T_min_over_Tp=2.0))   # y_hi <= y_lo: Y_B = 0 (fpy:242-243)
    sv = dict(HW, target={"field": "DM_over_B", "value": 40.0})
    rec, sol = solve(gpu_engine, cfg, [("m_chi_GeV", np.linspace(0.8, 1.2, 5))], sv, window=PLATEAU)
    _assert_refused(rec, sol, np.arange(5), 2, sv)
    assert np.all(sol[:, 4] == 2)


def test_bad_value_in_a_device_resident_window_axis(gpu_engine):
    cfg = full_cfg(BASE_CFG)
    sig = torch.tensor([6.0, -1.0, 5.5, float("nan"), 6.5], dtype=torch.float64, device=gpu_engine.device)
    # (the half-width fixture's target: the middle of this window's range on the base configuration)
    sv = dict(HW, target=next(c for c in CASES if c["name"] == "plateau_half_width")["solve"]["target"])
    rec, sol = solve(gpu_engine, cfg, [("window_sigma_hi", sig)], sv, count=5, window=PLATEAU)
    bad = np.array([False, True, False, True, False])
    _assert_refused(rec, sol, bad, 3, sv)
    assert np.all(sol[bad, 4] == 1)            # refused at the first evaluation
    assert np.all(sol[~bad, 5] == 0) and np.all(np.isfinite(rec[~bad]))


def test_max_evals_three(gpu_engine, hw_grid):
    cfg, sv, _, _, _, full = hw_grid
    sv3 = dict(sv, max_evals=3)
    rec, sol = solve(gpu_engine, cfg, [M_CHI, V_W], sv3, window=PLATEAU)
    x, x_lo, x_hi, residual, evals, status = sol.T
    assert np.all(status == 1) and np.all(evals == 3)
    assert np.all((sv["lo"] <= x_lo) & (x_lo < x_hi) & (x_hi <= sv["hi"]) & ((x == x_lo) | (x == x_hi)))
    assert np.all((x_lo <= full[:, 0]) & (full[:, 0] <= x_hi))     # the bracket still holds the root
    assert same(rec, forward_at(gpu_engine, cfg, [M_CHI, V_W], "window_half_width", x, window=PLATEAU))
    assert same(residual, rec[:, DMB] - sv["target"]["value"])


def test_bad_table_status(gpu_engine):
    """Tables built for another n_y: the header does not match, tested once at lo."""
    import ctypes
    N = pkg("_native")
    cfg = full_cfg(BASE_CFG)
    eng = gpu_engine
    forward(eng, cfg, [M_CHI], n_y=2000)                       # leaves the n_y = 2000 table in the workspace
    base = pkg("config").to_ctypes_point(pkg("config").to_point(cfg))
    vals = torch.tensor(M_CHI[1], dtype=torch.float64, device=eng.device)
    ax = (N.LzqAxis * 1)()
    ax[0].field, ax[0].n, ax[0].values = N.FIELD["m_chi_GeV"], 10, vals.data_ptr()
    sv = {"field": "source_shape_sigma_y", "lo": 1.0, "hi": 50.0}
    out = torch.zeros((10, 6), dtype=torch.float64, device=eng.device)
    sol = torch.zeros((10, 6), dtype=torch.float64, device=eng.device)
    work = torch.zeros(3000 + N.REUSE_TABLE_HEADER, dtype=torch.float64, device=eng.device)
    work[:eng._zwork.numel()][:2006] = eng._zwork[:2006]
    rc = eng.lib.lzq_sweep_grid_solve(ctypes.byref(base), None, ax, 1, ctypes.byref(pkg("solve").to_ctypes(sv)), 0, 10,
                                      3000, 13, 3.0, None, work.data_ptr(), work.numel(), None, out.data_ptr(),
                                      sol.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    _assert_refused(out.cpu().numpy(), sol.cpu().numpy(), np.arange(10), 4, sv)


def test_refusals_raise_before_any_launch(gpu_engine):
    cfg = full_cfg(BASE_CFG)
    with pytest.raises(ValueError, match="changes the z-sum tables"):
        gpu_engine.sweep(cfg, [M_CHI], 0, 10, n_y=2000, solve={"field": "I_p", "lo": 0.1, "hi": 1.0}, **ZS)
    with pytest.raises(ValueError, match="needs a window"):
        gpu_engine.sweep(cfg, [M_CHI], 0, 10, n_y=2000, solve=HW, **ZS)
    with pytest.raises(ValueError, match="writes the solve field"):
        gpu_engine.sweep(cfg, [M_CHI], 0, 10, n_y=2000, solve={"field": "m_chi_GeV", "lo": 0.1, "hi": 1.0}, **ZS)
    with pytest.raises(ValueError, match="P override"):
        gpu_engine.sweep(cfg, [M_CHI], 0, 10, n_y=2000, P_points=torch.full((10,), 0.1, dtype=torch.float64),
                         solve={"field": "P_chi_to_B", "lo": 0.01, "hi": 1.0}, **ZS)


# ---- LZ fields: the closed form inside the solve ---------------------------------------------------
def test_lz_fields_agree_with_the_P_solve(gpu_engine):
    """delta_LZ and m_mix (with a dprime axis) solved for the Planck ratio give the P of the P solve
    through the closed form, and their records equal the forward sweep's at x*."""
    cfg = full_cfg(BASE_CFG)
    rp, sp = solve(gpu_engine, cfg, [], {"field": "P_chi_to_B", "lo": 0.01, "hi": 1.0})
    rd, sd = solve(gpu_engine, cfg, [], {"field": "delta_LZ", "lo": 1e-3, "hi": 3.0})
    assert sp[0, 5] == 0 == sd[0, 5]
    P = 1.0 - math.exp(-2.0 * math.pi * sd[0, 0])
    assert abs(P / sp[0, 0] - 1.0) <= 1e-11 and abs(rd[0, 5] / sp[0, 0] - 1.0) <= 1e-11
    assert same(rd, forward(gpu_engine, cfg, [("delta_LZ", np.array([sd[0, 0]]))]))
    dpr = ("dprime", np.array([0.5, 2.0, 7.0]))
    rm, sm = solve(gpu_engine, cfg, [dpr], {"field": "m_mix", "lo": 1e-3, "hi": 10.0})
    assert np.all(sm[:, 5] == 0)
    delta = sm[:, 0] ** 2 / (2.0 * cfg["v_w"] * dpr[1])
    assert np.all(np.abs(delta / sd[0, 0] - 1.0) <= 1e-10)
    at = forward(gpu_engine, cfg, [dpr, ("m_mix", sm[:, 0])]).reshape(3, 3, 6)[np.arange(3), np.arange(3)]
    assert same(rm, at)


@pytest.mark.parametrize("window", [None, PLATEAU], ids=["gauss", "block"])
def test_v_w_solve_over_lz_axes_moves_P_with_it(gpu_engine, window):
    """v_w enters the P of m_mix / dprime axes (PAPER eq.(8)): a v_w solve on such a grid (the built-in
    C2's axes) re-forms P at every x, so its record is the forward sweep's with v_w as an axis, bit for
    bit, in both instantiations."""
    cfg = full_cfg(BASE_CFG)
    axes = [("dprime", np.array([1.0, 1.7, 3.0])), ("m_mix", np.array([0.3, 0.4, 0.5, 0.6]))]
    ends = forward(gpu_engine, cfg, axes + [("v_w", np.array([0.01, 1.0]))], window=window).reshape(12, 2, 6)
    assert np.all(ends[:, 0, 5] > ends[:, 1, 5]) and len(np.unique(ends[:, 1, 5])) == 12   # P_used moves with v_w
    d_lo, d_hi = ends[:, 0, DMB], ends[:, 1, DMB]
    assert d_lo.max() < d_hi.min()
    sv = {"field": "v_w", "lo": 0.01, "hi": 1.0, "xtol": XTOL,
          "target": {"field": "DM_over_B", "value": float(math.sqrt(d_lo.max() * d_hi.min()))}}
    rec, sol = solve(gpu_engine, cfg, axes, sv, window=window)
    assert np.all(sol[:, 5] == 0) and len(np.unique(sol[:, 0])) == 12
    at_x = forward_at(gpu_engine, cfg, axes, "v_w", sol[:, 0], window=window)
    assert same(rec, at_x)
    delta = axes[1][1][None, :] ** 2 / (2.0 * sol[:, 0].reshape(3, 4) * axes[0][1][:, None])
    assert np.allclose(rec[:, 5].reshape(3, 4), 1.0 - np.exp(-2.0 * np.pi * delta), rtol=1e-12, atol=0)
    assert same(sol[:, 3], rec[:, DMB] - sv["target"]["value"])
    for k, xs in ((1, sol[:, 1]), (2, sol[:, 2])):                   # the bracket's signs, by forward sweeps
        f = forward_at(gpu_engine, cfg, axes, "v_w", xs, window=window)[:, DMB] - sv["target"]["value"]
        assert np.all(f <= 0) if k == 1 else np.all(f >= 0)
    # a per-point override still decides P
    Pp = torch.full((12,), 0.2, dtype=torch.float64, device=gpu_engine.device)
    r2, s2 = gpu_engine.sweep(cfg, axes, 0, 12, n_y=2000, window=window, solve=dict(sv, target={"field": "DM_over_B", "value": 5.0}),
                              P_points=Pp, **ZS)
    assert np.all(r2.cpu().numpy()[s2.cpu().numpy()[:, 5] == 0, 5] == 0.2)


# ---- (f) the paper's P_eff --------------------------------------------------------------------------
def test_P_eff_of_the_shipped_configuration(gpu_engine):
    """PAPER eqs.(22)-(24): the P at which the shipped configuration gives the Planck ratio 5.357, at
    main()'s n_y = 8000 on the (1200, 30) grid: 0.15850 to the digits the paper prints, and the
    reference's own root within the fixture tolerance."""
    case = next(c for c in CASES if c["name"] == "P_shipped_8000")
    rec, sol = gpu_engine.solve_point(full_cfg(BASE_CFG), {"field": "P_chi_to_B", "lo": 0.01, "hi": 1.0}, n_y=8000)
    x, status = float(sol[0]), float(sol[5])
    print(f"P_eff = {x!r} (reference root {case['x_ref']!r}), evals = {float(sol[4]):.0f}")
    assert status == 0 and f"{x:.9f}".startswith("0.15850")
    assert abs(x / case["x_ref"] - 1.0) <= XTOL + 1e-11 / abs(case["log_slope"])
    assert float(rec[5]) == x and abs(float(rec[4]) / 5.357 - 1.0) <= 1e-11


# ---- (g) the sweep driver: files, summary block, resume ------------------------------------------------
def test_sweep_cli_with_solve_and_fit(gpu_engine, hw_grid, tmp_path):
    import json
    import os
    S = pkg("sweep")
    T = hw_grid[1]["target"]["value"]      # bracketed by every point of the 10 x 7 grid
    spec_d = {"name": "hw", "n_y": 2000, "nz": 13, "z_max": 3.0,
              "axes": [{"field": "m_chi_GeV", "values": [float(v) for v in M_CHI[1]]},
                       {"field": "v_w", "values": [float(v) for v in V_W[1][:3]]}],
              "window": dict(PLATEAU), "solve": dict(HW, target={"field": "DM_over_B", "value": T})}
    path, out = str(tmp_path / "spec.json"), str(tmp_path / "out")
    with open(path, "w") as f:
        json.dump(spec_d, f)
    S.main(["--spec", path, "--out", out, "--chunk", "16", "--fit", "paper"])
    table, sol = np.load(os.path.join(out, "table.npy")), np.load(os.path.join(out, "solve.npy"))
    assert table.shape == sol.shape == (30, 6) and np.all(sol[:, 5] == 0)
    assert same(sol[:, 3], table[:, DMB] - T)
    with open(os.path.join(out, "summary.json")) as f:
        summ = json.load(f)
    assert summ["solve"] == json.loads(json.dumps(pkg("solve").summary(spec_d["solve"], sol)))
    assert summ["solve"]["status"]["ok"] == 30 and summ["solve"]["field"] == "window_half_width"
    assert summ["spec_def"]["solve"]["target"] == {"field": "DM_over_B", "value": T} and "fit" in summ
    assert os.path.exists(os.path.join(out, "fit.json"))
    shards = sorted(f for f in os.listdir(out) if f.startswith("shard_") and not f.endswith(".solve.npy"))
    assert len(shards) == 2 and all(os.path.exists(os.path.join(out, f[:-4] + ".solve.npy")) for f in shards)
    # the same through run_sweep, resumed from those checkpoints: nothing recomputed, the same bits
    spec = S.spec_from_json(spec_d)
    logs = []
    t2 = S.run_sweep(spec, gpu_engine, chunk=16, out_dir=out, resume=True, log=logs.append)
    assert sum("resumed" in m for m in logs) == 2 and not any("launched" in m for m in logs)
    assert same(t2, table) and same(S.run_sweep.solve, sol)
    # and computed afresh by the engine in one piece
    rec, s1 = solve(gpu_engine, full_cfg(spec.base), spec.axes, spec.solve, window=PLATEAU)
    assert same(rec, table) and same(s1, sol)
    # --no-table: the same summary block, no solve.npy, no table
    out2 = str(tmp_path / "out2")
    S.main(["--spec", path, "--out", out2, "--chunk", "16", "--fit", "paper", "--no-table"])
    with open(os.path.join(out2, "summary.json")) as f:
        assert json.load(f)["solve"] == summ["solve"]
    assert not os.path.exists(os.path.join(out2, "solve.npy")) and not os.path.exists(os.path.join(out2, "table.npy"))
    # a shard without its sibling is an error
    os.remove(os.path.join(out, shards[0][:-4] + ".solve.npy"))
    with pytest.raises(RuntimeError, match="no solve record"):
        S.run_sweep(spec, gpu_engine, chunk=16, out_dir=out, resume=True, log=logs.append)
