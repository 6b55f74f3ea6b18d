"""A/V in the continuum limit of the z grid on the device (csrc/lzq_cont.hip): the
continuum node table through the z-sum kernels, the live-range table kernel, and the *_cont entry
points up to Engine.aov / yields / sweep / solve_point.  Needs an MI355X.

References: the 60-digit sum over the table's own doubles (tests/zsum_ref.py on the duck-typed grid of
tests/test_cont_host.py) within zsum_ref.tol, and the fixture tests/golden/golden_cont.json (the
reference's y-quadrature on the z-integral by mpmath.quad) with the rule error on top.  n_y = 2000
throughout.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import zsum_ref as Z
from conftest import BASE_CFG, full_cfg, golden, pkg, rel_err
from test_cont_host import Z_MAX, cont_grid, fixture_items, rule_error
from test_gpu_zsum import bits, tuned

pytestmark = pytest.mark.gpu
I_P = BASE_CFG["I_p"]
N_Y = 2000
HDR = 6              # LZQ_REUSE_TABLE_HEADER
GUARD = 1e-11        # the project's GPU golden gate (tests/test_gpu_window.py)
FX = golden("golden_cont.json")


class skip_form:
    """LZQ_TUNE_CONT_SKIP for a block, restored on exit."""

    def __init__(self, eng, on):
        self.eng, self.on = eng, on

    def __enter__(self):
        self.prev = self.eng.tune_cont_skip(self.on)

    def __exit__(self, *exc):
        self.eng.tune_cont_skip(self.prev)
        return False


def tbits(t):
    return bits(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))


def same(a, b):
    return a.shape == b.shape and np.array_equal(tbits(a), tbits(b))


# ---------------------------------------------------------------------------------------------
# A/V
# ---------------------------------------------------------------------------------------------
def panel_edges_y(g, I_p):
    """The y at which a wavefront's live range gains or loses a panel: its smallest a = (I_p/6) e^y
    puts the truncation threshold 1080 octaves (lzq_quad.h zsum_dispatch) on the gamma4 of a panel's
    first node.  Those inside (-50, 50)."""
    k = Z.LOG2E * (I_p / 6.0)
    ys = [math.log(1080.0 / (k * float(g.g4[p]))) for p in range(0, g.g4.size, 20)]
    return [y for y in ys if -50.0 < y < 50.0]


def aov_y_set(g, I_p):
    """Module order, not sorted: 64 consecutive values share a wavefront."""
    ys = [-60.0, -50.0, math.nextafter(-50.0, -math.inf), math.nextafter(-50.0, math.inf)]
    ys += list(np.arange(-50.0, 50.01, 2.0))
    for yp in panel_edges_y(g, I_p):
        ys += [yp + (k + 0.5) * 0.004 for k in range(-16, 16)]
    ys += [50.0, math.nextafter(50.0, -math.inf), math.nextafter(50.0, math.inf), 60.0]
    return [float(y) for y in ys]


@pytest.mark.parametrize("variant", Z.VARIANTS)
def test_aov_vs_table_sum(gpu_engine, variant):
    """Engine.aov(continuum=True) against the 60-digit sum over its own tables within zsum_ref.tol, on
    the ladder, 16 y either side of every live-range change, the clips, and exact +0 above 50."""
    g = cont_grid()
    edges = panel_edges_y(g, I_P)
    assert len(edges) >= 15
    ys = aov_y_set(g, I_P)
    kernel = full_cfg(BASE_CFG)
    items = Z.av_ref(kernel, ys, g)
    acc = Z.accumulation([r for _, r, _ in items])
    with tuned(gpu_engine, exp=variant):
        got = gpu_engine.aov(kernel, ys, z_max=Z_MAX, continuum=True).cpu().numpy()
        with skip_form(gpu_engine, False):
            every = gpu_engine.aov(kernel, ys, z_max=Z_MAX, continuum=True).cpu().numpy()
    worst, ratio, bad = Z.compare(got, items, variant, acc)
    print(f"A/V_cont vs table sum [{variant}]: {len(ys)} y ({len(edges)} live-range changes), accumulation {acc:.2e}, "
          f"worst rel err {worst:.3e}, worst err/tol {ratio:.3f}")
    assert not bad, bad[:4]
    zeros = [(x, math.copysign(1.0, x)) for x, y in zip(got, ys) if y > 50.0]
    assert len(zeros) == 2 and all(z == (0.0, 1.0) for z in zeros)
    assert got[ys.index(-60.0)] == got[ys.index(-50.0)] > 0.0 and got[ys.index(50.0)] > 0.0
    assert np.array_equal(bits(got), bits(every))          # the live range skips exact +0 terms only


@pytest.mark.parametrize("variant", Z.VARIANTS)
def test_aov_vs_fixture(gpu_engine, variant):
    """Against the z-integral itself (the fixture), the same tolerance plus the rule error; where the
    reference grid's A/V is 0 (y > 27) the continuum's is not."""
    fx = FX["aov"]
    g = cont_grid()
    items = fixture_items(fx, g)
    acc = Z.accumulation([r for _, r, _ in items])
    extra = [rule_error(41)[0]] * len(items)
    with tuned(gpu_engine, exp=variant):
        got = gpu_engine.aov({**full_cfg(BASE_CFG), **fx["kernel"]}, fx["y"], z_max=fx["z_max"], continuum=True)
        got = got.cpu().numpy()
    worst, ratio, bad = Z.compare(got, items, variant, acc, extra_rel=extra)
    print(f"A/V_cont vs fixture [{variant}]: {len(items)} y, rule error {extra[0]:.2e}, worst rel err {worst:.3e}, "
          f"worst err/tol {ratio:.3f}")
    assert not bad, bad[:4]
    dark = [x for x, gv, y in zip(got, fx["A_over_V_grid"], fx["y"]) if gv == 0.0 and y <= 50.0]
    assert len(dark) >= 8 and all(x > 0.0 for x in dark)


@pytest.mark.parametrize("variant", Z.VARIANTS)
def test_wave_composition_bit_identical(gpu_engine, variant):
    """Equal y gives equal bits whatever shares its wavefront (the live range is the wavefront's, the
    zero / clamp-free / clamped loops are picked per wavefront): 1125 values, ragged, mixed regimes."""
    g = cont_grid()
    edges = panel_edges_y(g, I_P)
    y_zero, y_free, y_cl, y_top = -30.0, 0.0, 25.0, 49.5      # accumulate-only; clamp-free; clamped; a few panels live
    palette = [y_zero, y_free, y_cl, y_top, -60.0, 50.0, 60.0, edges[3], math.nextafter(edges[3], -math.inf),
               edges[10] + 0.01, 7.0, 12.0]

    def wave(fill):
        w = [fill] * 64
        for lane in (0, 17, 63):
            w[lane] = y_free
        return w

    top_but_one = [y_top] * 64
    top_but_one[5] = y_cl
    batches = {
        "free x 64": [y_free] * 64,
        "free among zero / clamped / top": wave(y_zero) + wave(y_cl) + wave(y_top),
        "clamped alone": [y_cl],                                       # tail lanes run y = 0
        "clamped among top": top_but_one,
        "two blocks, ragged": wave(y_cl) + wave(y_top) + [palette[i % len(palette)] for i in range(1125 - 128)],
    }
    assert len(batches["two blocks, ragged"]) == 1125
    seen = {}
    with tuned(gpu_engine, exp=variant):
        for name, ys in batches.items():
            out = gpu_engine.aov(full_cfg(BASE_CFG), ys, continuum=True).cpu().numpy()
            for y, b in zip(ys, bits(out)):
                seen.setdefault(y, {}).setdefault(int(b), []).append(name)
    for y, pats in seen.items():
        assert len(pats) == 1, (variant, y, {hex(b): sorted(set(n)) for b, n in pats.items()})
    val = {y: np.int64(next(iter(p))).view(np.float64) for y, p in seen.items()}
    assert all(val[y] > 0 for y in (y_zero, y_free, y_cl, y_top, 50.0)) and val[60.0] == 0.0


# ---------------------------------------------------------------------------------------------
# the z-sum tables: live-range kernel against every node
# ---------------------------------------------------------------------------------------------
FT_CFG = {**BASE_CFG, **Z.FT_WINDOW}     # y from the -80 clip to the +50 clip: every regime, 32 passes


class RawGrid:
    """The grid entry points through the raw ABI on base x axes."""

    def __init__(self, eng, cfg, axes):
        nat, cfgm = pkg("_native"), pkg("config")
        self.eng, self.nat = eng, nat
        self.base = cfgm.to_ctypes_point(cfgm.to_point(full_cfg(cfg)))
        self.vals = [torch.as_tensor(np.asarray(v, dtype=np.float64), device=eng.device) for _, v in axes]
        self.arr = (nat.LzqAxis * max(1, len(axes)))()
        for a, ((name, _), t) in enumerate(zip(axes, self.vals)):
            self.arr[a].field, self.arr[a].n, self.arr[a].values = nat.FIELD[name], t.numel(), t.data_ptr()
        self.n_axes = len(axes)
        self.total = int(np.prod([len(v) for _, v in axes])) if axes else 1
        self.need = eng.lib.lzq_sweep_grid_reuse_workspace(self.arr, self.n_axes, N_Y)

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.eng.device).cuda_stream)

    def work(self):
        return torch.full((self.need,), float("nan"), dtype=torch.float64, device=self.eng.device)

    def tables(self, cont, z_max=Z_MAX):
        w = self.work()
        p = ctypes.c_void_p(w.data_ptr())
        with torch.cuda.device(self.eng.device):
            if cont:
                rc = self.eng.lib.lzq_sweep_grid_ztables_cont(ctypes.byref(self.base), self.arr, self.n_axes, N_Y, z_max, p,
                                                              self.need, self.stream())
            else:
                rc = self.eng.lib.lzq_sweep_grid_ztables(ctypes.byref(self.base), self.arr, self.n_axes, N_Y, 1200, z_max,
                                                         p, self.need, self.stream())
        self.nat.check(rc, self.eng.lib)
        return w

    def integrate(self, w, cont, z_max=Z_MAX):
        out = torch.empty((self.total, 6), dtype=torch.float64, device=self.eng.device)
        p, o = ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(out.data_ptr())
        with torch.cuda.device(self.eng.device):
            if cont:
                rc = self.eng.lib.lzq_sweep_grid_from_ztables_cont(ctypes.byref(self.base), None, self.arr, self.n_axes, 0,
                                                                   self.total, N_Y, z_max, None, p, self.need, None, o,
                                                                   self.stream())
            else:
                rc = self.eng.lib.lzq_sweep_grid_from_ztables(ctypes.byref(self.base), self.arr, self.n_axes, 0, self.total,
                                                              N_Y, 1200, z_max, None, p, self.need, o, self.stream())
        self.nat.check(rc, self.eng.lib)
        return out.cpu().numpy()


@pytest.mark.parametrize("variant", Z.VARIANTS)
def test_skip_form_bit_identical(gpu_engine, variant):
    """LZQ_TUNE_CONT_SKIP 0 (the linspace grids' table kernel, every node) and 1 (the live-range
    kernel) write the same two tables (I_p = 0.05, 1.0), header and all 2000 F each; F against the
    60-digit sum at every 16th node."""
    rg = RawGrid(gpu_engine, FT_CFG, [("I_p", [0.05, 1.0])])
    assert rg.need == 2 * (N_Y + HDR)
    with tuned(gpu_engine, exp=variant):
        with skip_form(gpu_engine, True):
            live = rg.tables(True).cpu().numpy()
        with skip_form(gpu_engine, False):
            every = rg.tables(True).cpu().numpy()
    assert np.all(np.isfinite(live)) and np.array_equal(bits(live), bits(every))
    y_lo, y_hi, _, ys = Z.ft_ygrid(FT_CFG)
    g = cont_grid()
    for t, I_p in enumerate((0.05, 1.0)):
        tab = live[t * (N_Y + HDR):(t + 1) * (N_Y + HDR)]
        assert list(tab[:HDR]) == [y_lo, y_hi, float(N_Y), -(I_p / 6.0), -1.0, Z_MAX]
        F = tab[HDR:]
        assert np.all(F > 0.0)            # no lane is dead on the continuum table
        idx = np.arange(0, N_Y, 16)
        refs = Z.refs_for(g, I_p, [float(y) for y in ys[idx]])
        acc = Z.accumulation(refs)
        worst, ratio, bad = Z.compare(F[idx], Z.f_items(refs), variant, acc)
        print(f"continuum F table vs mp [{variant}, I_p = {I_p}]: {idx.size} of {N_Y} nodes, worst rel err {worst:.3e}, "
              f"worst err/tol {ratio:.3f}")
        assert not bad, bad[:4]


# ---------------------------------------------------------------------------------------------
# yields
# ---------------------------------------------------------------------------------------------
def test_yields_vs_fixture(gpu_engine):
    """The fixture's Y_B (the reference's y-quadrature on the z-integral) within the GPU golden gate;
    exact 0 for the empty window; z_max = 3 honoured; the live-range and every-node forms agree bit
    for bit through Y_B."""
    cfgm = pkg("config")
    worst, by_name = 0.0, {}
    for c in FX["cases"]:
        assert c["n_y"] == N_Y
        pt = cfgm.to_point(full_cfg(c["config"]))
        kw = dict(n_y=N_Y, z_max=c["z_max"], window=c["window"], continuum=True)
        got = gpu_engine.yields(pt, **kw)
        assert gpu_engine.last_yields_path == "tables"
        with skip_form(gpu_engine, False):
            assert same(gpu_engine.yields(pt, **kw), got), c["name"]
        yb = float(got[0, 0].item())
        by_name[c["name"]] = yb
        if c["Y_B"] == 0.0:
            assert yb == 0.0, (c["name"], yb)
            continue
        e = rel_err(yb, c["Y_B"])
        worst = max(worst, e)
        print(f"Y_B continuum [{c['name']}]: {yb!r} fixture {c['Y_B']!r} rel err {e:.3e}")
        assert e < GUARD, (c["name"], yb, c["Y_B"], e)
    print(f"Y_B continuum vs fixture: {len(FX['cases'])} cases, worst rel err {worst:.3e}")
    assert by_name["empty window"] == 0.0 and by_name["z_max=3"] != by_name["shipped"]
    # the reference grid's own number is another one (Y_B is not converged in it)
    grid = float(gpu_engine.yields(cfgm.to_point(full_cfg(BASE_CFG)), n_y=N_Y)[0, 0].item())
    assert 1.9 < by_name["shipped"] / grid < 2.2


def test_yields_groups_and_chunks(gpu_engine, monkeypatch):
    """Engine.yields(continuum=True) on explicit points: one table per distinct z-sum key, in chunks
    where the tables exceed the workspace cap -- the same bits as one point at a time."""
    cfgm, E = pkg("config"), pkg("engine")
    cfgs = [full_cfg({**BASE_CFG, "I_p": I_p, "P_chi_to_B": P}) for I_p in (0.05, 0.2, 0.34, 0.7, 1.0) for P in (0.1, 0.2)]
    pts = np.concatenate([cfgm.to_point(c) for c in cfgs])
    one = torch.cat([gpu_engine.yields(pts[i:i + 1], n_y=N_Y, continuum=True) for i in range(len(cfgs))])
    allp = gpu_engine.yields(pts, n_y=N_Y, continuum=True)
    assert gpu_engine.last_cont_chunks == 1 and same(allp, one)
    assert len(np.unique(one[:, 0].cpu().numpy())) == len(cfgs)
    monkeypatch.setattr(E, "REUSE_MAX_BYTES", 3 * (N_Y + HDR) * 8)     # three tables at a time
    chunked = gpu_engine.yields(pts, n_y=N_Y, continuum=True)
    assert gpu_engine.last_cont_chunks == 4 and same(chunked, one)


# ---------------------------------------------------------------------------------------------
# sweeps
# ---------------------------------------------------------------------------------------------
AXES = [("I_p", np.array([0.05, 1.0])), ("delta_LZ", np.logspace(-2, 0, 3))]


def test_sweep_equals_yields_chunks_window_and_mismatch(gpu_engine):
    S = pkg("sweep")
    spec = S.SweepSpec("c23", full_cfg(BASE_CFG), AXES, n_y=N_Y, z_rule="continuum")
    assert spec.to_json()["z_rule"] == "continuum" and S.spec_from_json(spec.to_json()).continuum
    assert S.spec_key(spec) != S.spec_key(S.SweepSpec("c23", full_cfg(BASE_CFG), AXES, n_y=N_Y))
    pts, _ = S.grid_records(spec, 0, spec.total, gpu_engine)
    ref = gpu_engine.yields(pts, n_y=N_Y, continuum=True)
    whole = gpu_engine.sweep(spec.base, AXES, 0, spec.total, n_y=N_Y, continuum=True)
    assert gpu_engine.last_reuse == "tables"
    assert bool((ref[:, 0] > 0).all()) and len(np.unique(ref[:, 0].cpu().numpy())) == spec.total
    assert same(whole, ref)
    parts = [gpu_engine.sweep(spec.base, AXES, s, min(4, spec.total - s), n_y=N_Y, continuum=True)
             for s in range(0, spec.total, 4)]
    assert same(torch.cat(parts), ref)
    assert same(S.run_sweep(spec, gpu_engine, chunk=5, log=lambda s: None), ref)
    # one window axis
    win = {"kind": "plateau", "half_width": 3.0}
    waxes = AXES + [("window_y0", np.array([-6.0, 4.0]))]
    wspec = S.SweepSpec("c232", full_cfg(BASE_CFG), waxes, n_y=N_Y, window=S.WindowSpec(win), z_rule="continuum")
    wpts, _ = S.grid_records(wspec, 0, wspec.total, gpu_engine)
    wref = gpu_engine.yields(wpts, n_y=N_Y, window=S.window_records(wspec, 0, wspec.total), continuum=True)
    wgot = gpu_engine.sweep(wspec.base, waxes, 0, wspec.total, n_y=N_Y, window=win, continuum=True)
    assert same(wgot, wref) and len(np.unique(wref[:, 0].cpu().numpy())) == wspec.total
    # a linspace call on continuum tables, and the reverse: NaN Y_B through the header match
    rg = RawGrid(gpu_engine, BASE_CFG, AXES)
    cont_t, lin_t = rg.tables(True), rg.tables(False)
    assert same(torch.as_tensor(rg.integrate(cont_t, True)), ref)
    assert np.all(np.isfinite(rg.integrate(lin_t, False)[:, 0]))
    assert np.all(np.isnan(rg.integrate(cont_t, False)[:, 0]))
    assert np.all(np.isnan(rg.integrate(lin_t, True)[:, 0]))
    assert np.all(np.isnan(rg.integrate(cont_t, True, z_max=20.0)[:, 0]))      # another z_max's table


def test_solve_for_P(gpu_engine):
    """The shipped configuration solved for P at DM/B = 5.357 on the continuum A/V: the stored record
    is the forward sweep's at x bit for bit, and x = P DM_over_B_cont / 5.357 from the fixture (Y_B is
    linear in P)."""
    cfg = full_cfg(BASE_CFG)
    sv = {"field": "P_chi_to_B", "lo": 0.01, "hi": 1.0, "target": {"field": "DM_over_B", "value": 5.357},
          "xtol": 1e-12}
    rec, sol = gpu_engine.solve_point(cfg, sv, n_y=N_Y, continuum=True)
    rec, sol = rec.cpu().numpy(), sol.cpu().numpy()
    x, status = float(sol[0]), sol[5]
    assert status == 0
    fwd = gpu_engine.sweep(cfg, [("P_chi_to_B", np.array([x]))], 0, 1, n_y=N_Y, continuum=True).cpu().numpy()
    assert np.array_equal(bits(rec), bits(fwd[0]))
    yb_fix = next(c for c in FX["cases"] if c["name"] == "shipped")["Y_B"]
    dmb_cont = float(fwd[0, 3]) / (yb_fix * (2891.0 * 1e6) * 1.67262192369e-27)     # fpy:36-39, 413-417
    x_ref = cfg["P_chi_to_B"] * dmb_cont / 5.357
    print(f"solve for P (continuum): x = {x!r}, P DM/B_cont / 5.357 = {x_ref!r}, rel err {abs(x / x_ref - 1):.3e}; "
          f"DM/B_cont at the shipped P = {dmb_cont:.6g}")
    assert abs(x / x_ref - 1.0) <= 1e-10
    assert 0.07 < x < 0.08          # the paper's P_eff = 0.1585 on the reference grid


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refusals(gpu_engine):
    nat, cfgm = pkg("_native"), pkg("config")
    cfg = full_cfg(BASE_CFG)
    pt = cfgm.to_point(cfg)
    for bad in (0.0, -30.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            gpu_engine.aov(cfg, [0.0], z_max=bad, continuum=True)
        with pytest.raises(ValueError):
            gpu_engine.yields(pt, n_y=N_Y, z_max=bad, continuum=True)
        with pytest.raises(ValueError):
            gpu_engine.sweep(cfg, AXES, 0, 6, n_y=N_Y, z_max=bad, continuum=True)
        y = torch.zeros(1, dtype=torch.float64, device=gpu_engine.device)
        a = cfgm.to_ctypes_aov(cfgm.to_aov(cfg))
        rc = gpu_engine.lib.lzq_aov_batch_cont(None, ctypes.byref(a), ctypes.c_void_p(y.data_ptr()), 1, bad,
                                               ctypes.c_void_p(y.data_ptr()), None)
        assert rc == -1                                                   # LZQ_EINVAL from the library itself
    with pytest.raises(ValueError):
        gpu_engine.yields(pt, n_y=N_Y, aov=cfg, continuum=True)
    with pytest.raises(ValueError):
        gpu_engine.yields(pt, n_y=N_Y, T_lo=[1.0], T_hi=[2.0], continuum=True)
    with pytest.raises(NotImplementedError):
        gpu_engine.ode(pt, cfgm.to_ode_params(cfg), continuum=True)
    S = pkg("sweep")
    with pytest.raises(ValueError):
        S.make_compute(S.SweepSpec("x", cfg, AXES, z_rule="gauss"), gpu_engine)
    with pytest.raises(ValueError):   # the ODE fallback keeps the linspace grids
        S.make_compute(S.SweepSpec("x", {**cfg, "Gamma_wash_over_H": 0.1}, AXES, z_rule="continuum"), gpu_engine)
    # every linspace entry point keeps refusing nz < 0
    with pytest.raises(ValueError):
        gpu_engine.aov(cfg, [0.0], nz=-1)
    y = torch.zeros(1, dtype=torch.float64, device=gpu_engine.device)
    a = cfgm.to_ctypes_aov(cfgm.to_aov(cfg))
    assert gpu_engine.lib.lzq_aov_batch(None, ctypes.byref(a), ctypes.c_void_p(y.data_ptr()), 1, -1, Z_MAX,
                                        ctypes.c_void_p(y.data_ptr()), None) == -1
