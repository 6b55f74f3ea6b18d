"""The grid form of the window kernels, host side (no GPU): the decode of a flat grid index into a
window block (csrc/lzq_window.h window_grid_block, built for the host as
lzq_window_grid_blocks_host), its host check, and the argument checks of the *_window grid entry
points that fail before any HIP call.

The reference for a block is sweep.window_records, the numpy decode the host-record path uploads:
equality of bytes.
"""
import ctypes

import numpy as np
import pytest

from conftest import BASE_CFG, full_cfg, golden, pkg

K1024 = golden("golden_window.json")["tables"]["k1024"]


def _spec(axes, block, tables=False):
    S = pkg("sweep")
    w = S.WindowSpec(block, K1024["u"], K1024["W"]) if tables else S.WindowSpec(block)
    return S.SweepSpec("g", full_cfg(BASE_CFG), axes, n_y=2000, window=w)


Y0 = ("window_y0", np.array([-6.0, 0.0, 8.0]))
SIG = ("window_sigma", np.array([2.0, 5.0, 9.0, 20.0]))
DLZ = ("delta_LZ", np.logspace(-3, 0, 5))
PLATEAU = {"kind": "plateau", "half_width": 3.0}

# (axes, base block, tables?): every window axis kind; a window axis slowest, in the middle, fastest
SPECS = {
    "w345": ([Y0, SIG, DLZ], PLATEAU, False),                  # the 3 x 4 x 5 spec of test_gpu_window.py
    "fastest": ([DLZ, SIG, Y0], PLATEAU, False),
    "middle": ([("I_p", np.array([0.3, 0.4])), ("window_half_width", np.array([0.0, 1.5, 7.0])), DLZ], PLATEAU, False),
    "lo_hi": ([("window_sigma_lo", np.array([0.5, 3.0])), ("m_chi_GeV", np.array([1.0, 50.0, 900.0])),
               ("window_sigma_hi", np.array([1e-7, 2.0, 11.0]))], PLATEAU, False),
    "table": ([("window_table", np.array([0.0, 1.0])), ("window_scale", np.array([0.5, 1.0, 3.0])),
               ("delta_LZ", np.logspace(-3, 0, 4))], {"kind": "table", "y0": 2.0}, True),
    "eight": ([("window_y0", np.array([-1.0, 2.5])), ("m_chi_GeV", np.array([1.0, 10.0, 100.0])),
               ("window_half_width", np.array([0.0, 4.0])), ("window_sigma_lo", np.array([1.0, 2.0, 3.0])),
               ("window_table", np.array([1.0, 0.0])), ("window_sigma_hi", np.array([4.0, 5.0])),
               ("delta_LZ", np.array([0.01, 0.1])), ("window_scale", np.array([0.25, 2.0, 8.0]))],
              {"kind": "table", "y0": 2.0}, True),
}


def _ranges(total):
    assert total >= 18
    return [(0, total), (7, 11), (1, 1), (total - 5, 5), (total, 0), (total // 2 - 3, 11)]


@pytest.mark.parametrize("name", sorted(SPECS))
def test_blocks_equal_window_records(name):
    S, W, N = pkg("sweep"), pkg("window"), pkg("_native")
    axes, block, tables = SPECS[name]
    spec = _spec(axes, block, tables)
    assert len(axes) <= N.LZQ_MAX_AXES and (name != "eight" or len(axes) == N.LZQ_MAX_AXES)
    for start, count in _ranges(spec.total):
        got = W.grid_blocks(block, axes, start, count)
        ref = S.window_records(spec, start, count)
        assert got.dtype == ref.dtype == N.WINDOW_DTYPE
        assert got.tobytes() == ref.tobytes(), (name, start, count)
    whole = W.grid_blocks(block, axes, 0, spec.total)
    for f in ("y0", "half_width", "sigma_lo", "sigma_hi", "scale", "table"):
        swept = any(f in S.WINDOW_AXES.get(n, ()) for n, _ in axes)
        assert (len(np.unique(whole[f])) > 1) == swept, (name, f)   # every axis moved its field, and only it


def test_large_flat_index_is_decoded_in_64_bits():
    """4.9e9 points: the index passes 2^32 between the two axes' strides."""
    S, W = pkg("sweep"), pkg("window")
    n = 70_000
    axes = [("window_y0", np.linspace(-40.0, 40.0, n)), ("window_sigma", np.linspace(0.5, 30.0, n))]
    spec = _spec(axes, PLATEAU)
    total = n * n
    assert spec.total == total > 1 << 32
    for start in (total - 64, (1 << 32) - 32):
        got = W.grid_blocks(PLATEAU, axes, start, 64)
        assert got.tobytes() == S.window_records(spec, start, 64).tobytes(), start
        assert len(np.unique(got["sigma_hi"])) == 64
    with pytest.raises(pkg("_native").LzqError, match="outside grid"):
        W.grid_blocks(PLATEAU, axes, total - 63, 64)


def _axes(n, fields, length=3):
    ax = (n.LzqAxis * len(fields))()
    for a, f in enumerate(fields):
        ax[a].field, ax[a].n, ax[a].values = f, length, 8   # values: never read on these paths
    return ax


def test_entry_points_check_arguments_before_any_launch():
    n, cfgm, W = pkg("_native"), pkg("config"), pkg("window")
    L = n.load()
    base = cfgm.to_ctypes_point(cfgm.to_point({**cfgm.default_config(), "P_chi_to_B": 0.1}))
    win = n.LzqWindow.from_buffer_copy(W.to_window(PLATEAU).tobytes())
    b, w = ctypes.byref(base), ctypes.byref(win)
    F, WF = n.FIELD, n.WINDOW_FIELD

    def dense(ax, start=0, count=1, tables=None, w=w):
        return L.lzq_sweep_grid_window(b, w, ax, len(ax), start, count, 2000, 1200, 30.0, None, tables, 8, None)

    def reuse(ax, start=0, count=1, tables=None, work=1 << 20):
        return L.lzq_sweep_grid_reuse_window(b, w, ax, len(ax), start, count, 2000, 1200, 30.0, None, 8, work, tables,
                                             8, None)

    def from_zt(ax, start=0, count=1, tables=None, work=1 << 20):
        return L.lzq_sweep_grid_from_ztables_window(b, w, ax, len(ax), start, count, 2000, 1200, 30.0, None, 8, work,
                                                    tables, 8, None)

    def ztables(ax, start=0, count=1, tables=None):
        return L.lzq_sweep_grid_ztables_window(b, ax, len(ax), 2000, 1200, 30.0, 8, 1 << 20, None)

    bad_tables = n.LzqWindowTables(2, 16, None, None)        # tables without their arrays
    too_many = n.LzqWindowTables(n.WIN_MAX_TABLES + 1, 16, 8, 8)
    for call in (dense, reuse, from_zt, ztables):
        assert call(_axes(n, [99])) == -1 and b"unknown field" in L.lzq_last_error(), call.__name__
        assert call(_axes(n, [WF["window_y0"], F["I_p"], WF["window_y0"]])) == -1
        assert b"writes a window field" in L.lzq_last_error(), call.__name__
        assert call(_axes(n, [WF["window_sigma"], WF["window_sigma_lo"]])) == -1
        assert b"writes a window field" in L.lzq_last_error(), call.__name__
        assert call(_axes(n, [WF["window_sigma_hi"], WF["window_sigma"]])) == -1
        assert call(_axes(n, [WF["window_y0"], F["m_mix"]])) == -1 and b"swept together" in L.lzq_last_error()
        if call is not ztables:
            assert call(_axes(n, [WF["window_y0"], F["I_p"]]), start=5, count=5) == -1
            assert b"outside grid" in L.lzq_last_error(), call.__name__
            for t in (bad_tables, too_many):
                assert call(_axes(n, [WF["window_table"]]), tables=ctypes.byref(t)) == -1, call.__name__
                assert b"n_tables" in L.lzq_last_error() or b"without their" in L.lzq_last_error()
    assert dense(_axes(n, [WF["window_y0"]]), w=None) == -1 and b"bad arguments" in L.lzq_last_error()
    # an empty range is a no-op once the arguments are accepted
    assert dense(_axes(n, [WF["window_y0"], F["I_p"]]), start=9, count=0) == 0
    assert reuse(_axes(n, [WF["window_y0"], F["I_p"]]), start=9, count=0, work=0) == 0
    # a workspace smaller than the grid's tables
    assert from_zt(_axes(n, [F["I_p"], WF["window_y0"], F["T_min_over_Tp"]]), work=9 * 2006 - 1) == -1
    assert b"workspace" in L.lzq_last_error()
    base.regime = n.REGIME_OTHER
    assert dense(_axes(n, [WF["window_y0"]])) == -3
    base.regime = n.THERMAL
    # the entry points without a window keep refusing the window fields, each with its present message
    for f in WF.values():
        ax = _axes(n, [f])
        assert L.lzq_sweep_grid(b, ax, 1, 0, 1, 2000, 1200, 30.0, None, 8, None) == -1
        assert b"unknown field" in L.lzq_last_error()
        assert L.lzq_sweep_grid_reuse(b, ax, 1, 0, 1, 2000, 1200, 30.0, None, 8, 1 << 20, 8, None) == -1
        assert b"unknown field" in L.lzq_last_error()
        assert L.lzq_sweep_grid_ztables(b, ax, 1, 2000, 1200, 30.0, 8, 1 << 20, None) == -1
        assert b"unknown field" in L.lzq_last_error()
        assert L.lzq_sweep_grid_from_ztables(b, ax, 1, 0, 1, 2000, 1200, 30.0, None, 8, 1 << 20, 8, None) == -1
        assert b"unknown field" in L.lzq_last_error()


def test_reuse_workspace_counts_no_table_for_window_axes():
    n = pkg("_native")
    L = n.load()
    F, WF = n.FIELD, n.WINDOW_FIELD
    ax = (n.LzqAxis * 4)()
    for a, (f, k) in enumerate([(F["I_p"], 2), (WF["window_y0"], 3), (F["T_min_over_Tp"], 2), (F["delta_LZ"], 4)]):
        ax[a].field, ax[a].n, ax[a].values = f, k, 8
    assert L.lzq_sweep_grid_reuse_workspace(ax, 4, 2000) == 4 * (2000 + n.REUSE_TABLE_HEADER)
    assert L.lzq_sweep_grid_reuse_workspace(ax, 4, 8000) == 4 * (8000 + n.REUSE_TABLE_HEADER)
    ax[0].field = WF["window_sigma"]
    assert L.lzq_sweep_grid_reuse_workspace(ax, 4, 2000) == 2 * (2000 + n.REUSE_TABLE_HEADER)


def test_host_check_names_the_axis_and_the_value():
    W, N = pkg("window"), pkg("_native")
    tabs = W.WindowTables(K1024["u"], K1024["W"])
    good = [Y0, SIG, DLZ]
    W.grid_check(PLATEAU, good)
    W.grid_check({"kind": "table", "y0": 2.0}, SPECS["table"][0], tabs)
    with pytest.raises(N.LzqError, match=r"axis 'window_sigma'.*value 1 = -2\b.*sigma") as e:
        W.grid_check(PLATEAU, [Y0, ("window_sigma", np.array([2.0, -2.0, 9.0])), DLZ])
    assert e.value.code == -1 and "window axis 1" in str(e.value)
    with pytest.raises(N.LzqError, match=r"axis 'window_sigma_lo'.*sigma"):
        W.grid_check(PLATEAU, [("window_sigma_lo", np.array([0.0]))])
    with pytest.raises(N.LzqError, match=r"axis 'window_y0'.*value 2 = nan.*NaN"):
        W.grid_check(PLATEAU, [DLZ, ("window_y0", np.array([0.0, 1.0, np.nan]))])
    with pytest.raises(N.LzqError, match=r"axis 'window_half_width'.*half_width"):
        W.grid_check(PLATEAU, [("window_half_width", np.array([1.0, -0.5]))])
    with pytest.raises(N.LzqError, match=r"axis 'window_scale'.*scale"):
        W.grid_check({"kind": "table"}, [("window_scale", np.array([1.0, np.inf]))], tabs)
    table = {"kind": "table", "y0": 2.0}
    with pytest.raises(N.LzqError, match=r"axis 'window_table'.*= 0\.5.*integer table index in \[0, 2\)"):
        W.grid_check(table, [("window_table", np.array([0.0, 0.5]))], tabs)
    with pytest.raises(N.LzqError, match=r"axis 'window_table'.*value 1 = 2\b.*\[0, 2\)"):
        W.grid_check(table, [("window_table", np.array([1.0, float(tabs.n_tables)]))], tabs)
    for bad in (-1.0, np.nan, 2.0 ** 31, 1e300):
        with pytest.raises(N.LzqError, match="axis 'window_table'"):
            W.grid_check(table, [("window_table", np.array([bad]))], tabs)
    # a bad base block, whatever the axes
    for block, what in (({"kind": "plateau", "sigma_lo": -1.0}, "sigma"), ({"kind": "gauss", "scale": 0.0}, "scale"),
                        ({"kind": "table", "table": 5}, "table index"), ({"kind": 7}, "kind")):
        with pytest.raises(N.LzqError, match=what):
            W.grid_check(block, good, tabs)
    # and the duplicates the entry points refuse
    with pytest.raises(N.LzqError, match="writes a window field"):
        W.grid_check(PLATEAU, [SIG, ("window_sigma_hi", np.array([1.0]))])
    with pytest.raises(N.LzqError, match="writes a window field"):
        W.grid_blocks(PLATEAU, [Y0, Y0], 0, 1)


def test_table_axis_value_is_tested_before_it_is_converted():
    """A table value that is no integer in [0, 2^31) decodes to table = -1 (refused for a table kind);
    an integer converts exactly."""
    W = pkg("window")
    vals = np.array([0.0, 1.0, 1023.0, 2.0 ** 31 - 1, 0.5, -1.0, -0.0, np.nan, np.inf, 2.0 ** 31, 1e300, -1e300])
    got = W.grid_blocks({"kind": "table"}, [("window_table", vals)], 0, vals.size)["table"]
    assert got.tolist() == [0, 1, 1023, 2 ** 31 - 1, -1, -1, 0, -1, -1, -1, -1, -1]


def test_sweep_driver_picks_the_path():
    """make_compute's choice needs no GPU to be stated: two axes on one block field keep the
    host-record path."""
    S = pkg("sweep")
    assert not S.window_axes_collide(_spec([Y0, SIG, DLZ], PLATEAU))
    assert not S.window_axes_collide(_spec(*SPECS["eight"][:2], tables=True))
    assert S.window_axes_collide(_spec([SIG, ("window_sigma_lo", np.array([1.0, 2.0]))], PLATEAU))
    assert S.window_axes_collide(_spec([("window_sigma_hi", np.array([1.0])), DLZ, SIG], PLATEAU))
    assert S.window_axes_collide(_spec([Y0, DLZ, Y0], PLATEAU))
