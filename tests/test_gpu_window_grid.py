"""Window-axis sweeps decoded on the device (lzq_sweep_grid_window and the shared-z-sum twins;
csrc/lzq_window.hip yields_grid_window_kernel / grid_reuse_window_kernel).  Needs an MI355X.

The reference for a grid point is what test_gpu_window.py pins to the reference runs:
lzq_yields_batch_window on the host-decoded records (sweep.grid_records + sweep.window_records).
Everything here is equality of bits against that path, except the one direct check against the
fixtures of tests/golden/golden_window.json, which takes test_gpu_window.py's own tolerance.
n_y = 2000 throughout.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import BASE_CFG, full_cfg, golden, pkg
from test_gpu_window import ZGRIDS, _check, _tables, same

pytestmark = pytest.mark.gpu
QUIET = dict(log=lambda s: None)


def _spec(kind="plateau", axes=None, **extra):
    S = pkg("sweep")
    if kind == "table":
        t = golden("golden_window.json")["tables"]["k1024"]
        axes = axes or [("window_table", np.array([0.0, 1.0])), ("window_scale", np.array([0.5, 1.0, 3.0])),
                        ("delta_LZ", np.logspace(-3, 0, 4))]
        return S.SweepSpec("wt", full_cfg(BASE_CFG), axes, n_y=2000,
                           window=S.WindowSpec({"kind": "table", "y0": 2.0}, t["u"], t["W"]), **extra)
    axes = axes or [("window_y0", np.array([-6.0, 0.0, 8.0])), ("window_sigma", np.array([2.0, 5.0, 9.0, 20.0])),
                    ("delta_LZ", np.logspace(-3, 0, 5))]
    return S.SweepSpec("w345", full_cfg(BASE_CFG), axes, n_y=2000,
                       window=S.WindowSpec({"kind": "plateau", "half_width": 3.0}), **extra)


def _records(eng, spec, start=0, count=None, P=None):
    """The parent's path: explicit records, each with its block, through lzq_yields_batch_window."""
    S = pkg("sweep")
    count = spec.total - start if count is None else count
    pts, _ = S.grid_records(spec, start, count, eng)
    return eng.yields(pts, n_y=spec.n_y, nz=spec.nz, z_max=spec.z_max, P=P, window=S.window_records(spec, start, count),
                      window_tables=spec.window.host_tables())


def _grid(eng, spec, start=0, count=None, reuse=False, axes=None, **kw):
    S = pkg("sweep")
    count = spec.total - start if count is None else count
    return eng.sweep(spec.base, S.grid_axes_for_kernel(spec) if axes is None else axes, start, count, n_y=spec.n_y,
                     reuse=reuse, nz=spec.nz, z_max=spec.z_max, window=spec.window.block,
                     window_tables=spec.window.host_tables(), **kw)


# ---- 1. the batch path, every instantiation ------------------------------------------------------
@pytest.mark.parametrize("exp", ["table", "poly11"])
@pytest.mark.parametrize("nz,z_max", ZGRIDS)
@pytest.mark.parametrize("kind", ["plateau", "table"])
def test_equals_the_batch_path(gpu_engine, kind, nz, z_max, exp):
    spec = _spec(kind)
    spec.nz, spec.z_max = nz, z_max
    prev = gpu_engine.tune_exp(exp)
    try:
        ref = _records(gpu_engine, spec)
        dense = _grid(gpu_engine, spec)
        assert gpu_engine.last_reuse == gpu_engine.last_yields_path == "dense"
        shared = _grid(gpu_engine, spec, reuse=True)
        assert gpu_engine.last_reuse == gpu_engine.last_yields_path == "tables"
    finally:
        gpu_engine.tune_exp(prev)
    if nz == 1200:   # (the coarse grid need not separate every cell)
        assert bool((ref[:, 0] > 0).all()) and len(np.unique(ref[:, 0].cpu().numpy())) == spec.total
    assert same(dense, ref)
    assert same(shared, ref)


# ---- 2. ranges -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plateau_ref(gpu_engine):
    """The 3 x 4 x 5 table by the batch path, computed once."""
    return _records(gpu_engine, _spec())


@pytest.mark.parametrize("reuse", [False, True])
def test_ranges_and_chunks(gpu_engine, plateau_ref, reuse):
    spec = _spec()
    for start, count in ((0, 1), (0, 15), (0, 16), (0, 17), (7, 13), (59, 1), (60, 0), (44, 16)):
        got = _grid(gpu_engine, spec, start, count, reuse=reuse)
        assert got.shape == (count, 6) and same(got, plateau_ref[start:start + count]), (start, count)
    parts = [_grid(gpu_engine, spec, s, min(7, 60 - s), reuse=reuse) for s in range(0, 60, 7)]
    assert same(torch.cat(parts), plateau_ref)
    assert gpu_engine.last_reuse == ("tables" if reuse else "dense")


# ---- 3. z-sum table index with window axes between the table axes -------------------------------
def test_table_index_with_interleaved_axes(gpu_engine):
    n = pkg("_native")
    axes = [("I_p", np.array([0.30, 0.41])), ("window_y0", np.array([-6.0, 0.0, 8.0])),
            ("T_min_over_Tp", np.array([0.001, 0.95])), ("delta_LZ", np.logspace(-3, 0, 4))]
    # (T_min_over_Tp = 0.95 ends the y grid near y = 5, below the clamp at 50: the four tables differ)
    spec = _spec(axes=axes)
    dense = _grid(gpu_engine, spec)
    shared = _grid(gpu_engine, spec, reuse=True)
    assert gpu_engine.last_reuse == "tables"
    assert gpu_engine._zwork.numel() >= 4 * (2000 + n.REUSE_TABLE_HEADER)
    assert same(shared, dense) and same(dense, _records(gpu_engine, spec))
    assert len(np.unique(dense[:, 0].cpu().numpy())) == 48   # every axis moves Y_B: no two cells share a table by luck
    # a range that starts inside the grid, from the tables already built
    assert same(_grid(gpu_engine, spec, 19, 23, reuse=True), dense[19:42])
    # the window axis slowest and fastest
    for order in ([1, 0, 2, 3], [0, 2, 3, 1]):
        s2 = _spec(axes=[axes[i] for i in order])
        assert same(_grid(gpu_engine, s2, reuse=True), _records(gpu_engine, s2)), order


# ---- 4. the per-point P override -----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["crossings", "profile"])
def test_crossing_and_profile_specs_through_the_grid_path(gpu_engine, kind):
    """As test_gpu_window.py::test_crossing_and_profile_specs_carry_a_window: a GAUSS window of the
    base's own sigma_y reproduces the spec without a window, bit for bit."""
    S = pkg("sweep")
    base = full_cfg(BASE_CFG)
    if kind == "crossings":
        axes = [("m_mix", np.logspace(-2, -0.5, 3)), ("dprime", np.logspace(-1, 0.5, 4))]
        extra = dict(crossings=S.CrossingSpec(n_cross=3))
    else:
        axes = [("y_B", np.linspace(0.5, 2.0, 3)), ("lambda_tr_eff", np.logspace(-2, 0, 4))]
        extra = dict(profile=S.ProfileSpec())
    plain = S.run_sweep(S.SweepSpec("p", base, axes, n_y=2000, **extra), gpu_engine, **QUIET)
    sig = np.array([base["source_shape_sigma_y"], 4.0])
    spec = S.SweepSpec("pw", base, axes + [("window_sigma_hi", sig)], n_y=2000, window=S.WindowSpec({"kind": "gauss"}),
                       **extra)
    assert not S.window_axes_collide(spec)
    for chunk, reuse in ((1 << 20, False), (5, True), (5, False)):
        w = S.run_sweep(spec, gpu_engine, chunk=chunk, reuse=reuse, **QUIET)
        assert same(w[0::2], plain), (chunk, reuse)
        assert bool((w[1::2, 0] < w[0::2, 0]).any()) and not bool((w[1::2, 0] > w[0::2, 0]).any())


# ---- 5. a GAUSS block of the point's own sigma_y is lzq_sweep_grid -------------------------------
@pytest.mark.parametrize("nz,z_max", ZGRIDS)
def test_gauss_base_block_without_window_axes_is_the_plain_grid(gpu_engine, nz, z_max):
    base = full_cfg(BASE_CFG)
    axes = [("m_chi_GeV", np.logspace(-1, 3, 5)), ("I_p", np.array([0.3, 0.4])), ("delta_LZ", np.logspace(-3, 0, 3))]
    kw = dict(n_y=2000, nz=nz, z_max=z_max)
    block = {"kind": "gauss", "sigma_hi": base["source_shape_sigma_y"]}
    for reuse in (False, True):
        plain = gpu_engine.sweep(base, axes, 0, 30, reuse=reuse, **kw)
        assert same(gpu_engine.sweep(base, axes, 0, 30, reuse=reuse, window=block, **kw), plain)
        assert same(gpu_engine.sweep(base, axes, 11, 6, reuse=reuse, window=block, **kw), plain[11:17])
    with pytest.raises(ValueError, match="needs a window"):
        gpu_engine.sweep(base, axes + [("window_y0", np.array([0.0]))], 0, 30, **kw)
    with pytest.raises(ValueError, match="window_tables without a window"):
        gpu_engine.sweep(base, axes, 0, 30, window_tables=_tables(golden("golden_window.json")["tables"], "k1024"),
                         **kw)


# ---- 6. a flat index past 2^32 -------------------------------------------------------------------
@pytest.mark.parametrize("reuse", [False, True])
def test_large_flat_index(gpu_engine, reuse):
    n = 70_000
    spec = _spec(axes=[("window_y0", np.linspace(-40.0, 40.0, n)), ("window_sigma", np.linspace(0.5, 30.0, n))])
    assert spec.total == n * n > 1 << 32
    for start in (n * n - 64, (1 << 32) - 32):
        got = _grid(gpu_engine, spec, start, 64, reuse=reuse)
        assert same(got, _records(gpu_engine, spec, start, 64)), start
        assert len(np.unique(got[:, 0].cpu().numpy())) == 64


# ---- 7. values the host check never saw ---------------------------------------------------------
@pytest.mark.parametrize("reuse", [False, True])
def test_bad_values_in_device_memory_give_nan_rows(gpu_engine, plateau_ref, reuse):
    """Axis values handed over as device tensors are not checked on the host: exactly the rows that
    decode a value no block may hold are NaN, the others keep their bits, the run ends normally."""
    S, N = pkg("sweep"), pkg("_native")
    spec = _spec()
    names = [n for n, _ in spec.axes]
    for axis, j, bad in (("window_sigma", 2, float("nan")), ("window_sigma", 1, -1.0), ("window_y0", 0, float("nan")),
                         ("window_sigma", 3, 0.0)):
        vals = {n: np.array(v, dtype=np.float64) for n, v in spec.axes}
        vals[axis][j] = bad
        with pytest.raises(N.LzqError, match=f"axis '{axis}'"):     # host values: refused before any upload
            _grid(gpu_engine, spec, axes=[(n, vals[n]) for n in names], reuse=reuse)
        dev = [(n, torch.from_numpy(vals[n]).to(gpu_engine.device) if n == axis else vals[n]) for n in names]
        got = _grid(gpu_engine, spec, axes=dev, reuse=reuse)
        a = names.index(axis)
        stride = int(np.prod([len(v) for _, v in spec.axes[a + 1:]]))
        hit = torch.as_tensor((np.arange(60) // stride) % len(vals[axis]) == j, device=got.device)
        assert bool(torch.isnan(got[hit][:, 0]).all()) and int(hit.sum()) == 60 // len(vals[axis])
        assert same(got[~hit], plateau_ref[~hit]), (axis, bad)
    # a table axis: 0.5, n_tables, -1 and NaN read no table
    tspec = _spec("table")
    ref = _records(gpu_engine, tspec)
    n_tables = tspec.window.host_tables().n_tables
    for bad in (0.5, float(n_tables), -1.0, float("nan"), 2.0 ** 31, 1e300):
        t = torch.tensor([0.0, bad], dtype=torch.float64, device=gpu_engine.device)
        got = _grid(gpu_engine, tspec, axes=[("window_table", t)] + list(tspec.axes[1:]), reuse=reuse)
        assert same(got[:12], ref[:12]), bad
        assert bool(torch.isnan(got[12:, 0]).all()), bad
    # the raw ABI with a base block that cannot be evaluated: every row NaN, no error
    L = gpu_engine.lib
    base = pkg("config").to_ctypes_point(pkg("config").to_point(spec.base))
    rec = pkg("window").to_window({"kind": "plateau", "sigma_lo": -1.0})
    blk = N.LzqWindow.from_buffer_copy(rec.tobytes())
    d = gpu_engine._f64(np.logspace(-3, 0, 5))
    ax = (N.LzqAxis * 1)()
    ax[0].field, ax[0].n, ax[0].values = N.FIELD["delta_LZ"], 5, d.data_ptr()
    out = torch.zeros((5, 6), dtype=torch.float64, device=gpu_engine.device)
    with torch.cuda.device(gpu_engine.device):
        rc = L.lzq_sweep_grid_window(ctypes.byref(base), ctypes.byref(blk), ax, 1, 0, 5, 2000, 1200, 30.0, None, None,
                                     ctypes.c_void_p(out.data_ptr()), gpu_engine._stream())
    assert rc == 0 and bool(torch.isnan(out[:, 0]).all())


# ---- 8. the sweep driver -------------------------------------------------------------------------
@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("chunk", [1 << 20, 7])
def test_driver(gpu_engine, plateau_ref, chunk, reuse):
    S, F = pkg("sweep"), pkg("fit")
    spec = _spec()
    calls = []
    real = gpu_engine.yields
    gpu_engine.yields = lambda *a, **k: calls.append(1) or real(*a, **k)   # the record path is not taken
    try:
        table = S.run_sweep(spec, gpu_engine, chunk=chunk, reuse=reuse, **QUIET)
        assert same(table, plateau_ref) and not calls
        assert gpu_engine.last_reuse == gpu_engine.last_yields_path == ("tables" if reuse else "dense")
        t = plateau_ref.cpu().numpy()
        yb, dm = np.median(t[:, 0]), np.median(t[:, 4])
        fit = F.FitSpec.from_json({"terms": [{"field": "Y_B", "target": float(yb), "sigma": float(abs(yb))},
                                             {"field": "DM_over_B", "target": float(dm), "sigma": float(abs(dm))}],
                                   "levels": [0.5, 2.0], "maps": [["window_y0", "window_sigma"], ["delta_LZ"]],
                                   "select": {"level": 2.0, "cap": 20}})
        tab2, res = S.run_sweep(spec, gpu_engine, chunk=chunk, reuse=reuse, fit=fit, **QUIET)
        assert same(tab2, plateau_ref)
        h = F.HostFit(fit, fit.resolve(spec))
        h.update(t, 0)
        assert F.differences(res, h.result()) == []
        none, res2 = S.run_sweep(spec, gpu_engine, chunk=chunk, reuse=reuse, fit=fit, keep_table=False, **QUIET)
        assert none is None and F.differences(res2, h.result()) == [] and not calls
    finally:
        del gpu_engine.yields


def test_driver_keeps_the_record_path_for_colliding_axes(gpu_engine):
    """window_sigma next to window_sigma_lo: the entry points refuse the pair, the driver still runs
    it from host records, resolved as sweep.window_records always has."""
    S, N = pkg("sweep"), pkg("_native")
    axes = [("window_sigma", np.array([2.0, 9.0])), ("window_sigma_lo", np.array([1.0, 4.0, 30.0])),
            ("delta_LZ", np.logspace(-2, 0, 3))]
    spec = _spec(axes=axes)
    assert S.window_axes_collide(spec)
    ref = _records(gpu_engine, spec)
    for chunk, reuse in ((1 << 20, False), (5, True)):
        assert same(S.run_sweep(spec, gpu_engine, chunk=chunk, reuse=reuse, **QUIET), ref)
    assert gpu_engine.last_reuse == gpu_engine.last_yields_path == "tables"
    with pytest.raises(N.LzqError, match="writes a window field"):
        _grid(gpu_engine, spec)


# ---- 9. the reference, once, directly ------------------------------------------------------------
def test_fixtures_as_one_point_grids(gpu_engine):
    """The (n_y = 2000, z grid (1200, 30)) fixtures of golden_window.json, each as a one-point grid
    whose only axis holds the block's own y0, dense and from a z-sum table; test_gpu_window.py's
    tolerance (_check: the 1e-8 gate and the 1e-11 guard band, exact zeros)."""
    d = golden("golden_window.json")
    rows = [r for r in d["cases"] if (r["n_y"], r["nz"], r["z_max"]) == (2000, 1200, 30.0)]
    base_rows = [r for r in rows if json.dumps(r["config"], sort_keys=True) == json.dumps(rows[0]["config"],
                                                                                           sort_keys=True)]
    assert len(rows) >= 40 and len(base_rows) >= 15   # the base config under many blocks, and other configs
    worst = 0.0
    for r in rows:
        tabs = _tables(d["tables"], r["tables"])
        block = dict(r["window"])
        axes = [("window_y0", np.array([block.pop("y0")]))]
        for reuse in (False, True):
            got = gpu_engine.sweep(full_cfg(r["config"]), axes, 0, 1, n_y=2000, reuse=reuse, window=block,
                                   window_tables=tabs)
            worst = max(worst, _check(float(got[0, 0]), r["Y_B"], r["window"]))
    print(f"window fixtures as one-point grids vs reference, worst Y_B rel err: {worst:.3e}")
