"""The y-quadrature and the epilogue of the yields kernels (csrc/lzq_quad.h y_factors, integrand_from,
exp_y, gauss_window, y_triple, the lane sums and the butterfly of yb_wave, epilogue_pre / epilogue_finish;
csrc/lzq_ynode.h) against the mpmath reference of tests/yquad_ref.py.  Needs an MI355X.

Every other GPU comparison of Y_B is FP64 against FP64 at 1e-11 (about 90,000 u), through the whole sum,
under a window that hides the grid's ends, the tail lanes, the clipped nodes and the subnormal band.  Here

* NODE PROBES isolate single nodes with the existing ABI: a LZQ_WIN_PLATEAU block with y0 = y_j,
  half_width = step/4 and both sigmas 1e-6 is 1 at node j and exactly 0 at every other (tests/
  test_yquad_host.py shows it for the host build), so that point's Y_B is fl(w_j I_j).  One batch holds
  one copy of the point per probed node, run dense and from the shared z-sum table;
* SUMS compare the full Y_B under the default Gaussian (sigma_y = 9 and 0.3), under a plateau that is 1
  on the whole grid, and on the default window's own one-node grid (sigma_y = 0);
* the EPILOGUE's four fields are recomputed in mpmath from the device's own Y_B.

F_j are the device's own doubles, read from the table lzq_sweep_grid_ztables builds; the tolerance is the
one derived in yquad_ref.py.  tests/test_yquad_host.py shows on the CPU that correct arithmetic passes
and that six seeded defects do not.

Measured on an MI355X: see README "Parity" (the prints below).
"""
import math

import mpmath as mp
import numpy as np
import pytest
import torch

import yquad_ref as Y
from conftest import pkg
from test_gpu_zsum import HDR, FTable
from test_yquad_host import probe_block

pytestmark = pytest.mark.gpu
SIGMAS = (9.0, 0.3)
FLAT = {"kind": "plateau", "half_width": 200.0}
# (case, (nz, z_max)): every case on the small grid (F is an input), the shipped one on the default grid too
RUNS = [(case, Y.ZGRID) for case in Y.CASES] + [("shipped", (1200, 30.0))]
RUN_IDS = [f"{c}-{g[0]}" for c, g in RUNS]
MORE = [(case, n_y) for case in Y.MULTI_NY for n_y in Y.NYS_MORE]

_cache = {}


def bits(t):
    return t.contiguous().view(torch.int64)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def device_ref(eng, case, grid=Y.ZGRID, n_y=Y.NY, **over):
    """(config, y-grid, the device's F, Nodes) of a case: the table's header is the restatement, and the
    reference is computed once from the table's own F and shared by the tests."""
    key = (case, grid, n_y, tuple(sorted(over.items())))
    if key not in _cache:
        c = Y.cfg_of(case, **over)
        y_lo, y_hi, step, ys = Y.ygrid(c, n_y)
        t = FTable(eng, grid[0], grid[1], cfg=c, axes=[("m_chi_GeV", np.array([c["m_chi_GeV"]]))], n_y=n_y)
        tab = t.table().cpu().numpy()
        assert list(tab[:HDR]) == [y_lo, y_hi, float(n_y), -(c["I_p"] / 6.0), float(grid[0]), grid[1]]
        F = tab[HDR:]
        assert F.size == n_y and np.all(np.isfinite(F)) and np.all(F >= 0.0)
        nd = Y.nodes_ref(c, ys, F)
        assert not nd.undecided, nd.undecided[:4]
        _cache[key] = (c, (y_lo, y_hi, step, ys), F, nd)
    return _cache[key]


def both_paths(eng, pts, **kw):
    """Engine.yields dense and from the shared z-sum table: equal bits; the dense records."""
    dense = eng.yields(pts, **kw)
    assert eng.last_yields_path == "dense"
    reuse = eng.yields(pts, reuse=True, **kw)
    assert eng.last_yields_path == "tables"
    assert same(dense, reuse)
    return dense.cpu().numpy()


def probe(eng, case, grid, n_y):
    cfgm, W = pkg("config"), pkg("window")
    c, (y_lo, y_hi, step, ys), F, nd = device_ref(eng, case, grid, n_y)
    idx = Y.probe_indices(n_y)
    pts = np.repeat(cfgm.to_point(c), idx.size)
    wins = np.concatenate([W.to_window(probe_block(ys[j], step)) for j in idx])
    out = both_paths(eng, pts, window=wins, n_y=n_y, nz=grid[0], z_max=grid[1])
    worst, ratio, bad = Y.compare_nodes(out[:, 0], nd, None, idx=idx, probe=True)
    print(f"node probes [{case}, n_y = {n_y}, z grid {grid}]: {idx.size} of {n_y} nodes, "
          f"{int(np.count_nonzero(out[:, 0]))} non-zero, worst rel err {worst:.3e}, worst err/tol {ratio:.3f}")
    assert not bad, bad[:4]
    assert ratio < 1.0
    return idx, out[:, 0], nd


@pytest.mark.parametrize("case,grid", RUNS, ids=RUN_IDS)
def test_every_node_against_mp(gpu_engine, case, grid):
    """fl(w_j I_j) of EVERY node at n_y = 2000 (31 passes and 16 lanes), dense = reuse."""
    idx, got, nd = probe(gpu_engine, case, grid, Y.NY)
    assert idx.size == Y.NY
    if case == "dead source":
        assert all(Y.is_pos_zero(float(x)) for x in got)
    else:
        assert np.count_nonzero(got) > 64


@pytest.mark.parametrize("case,n_y", MORE, ids=[f"{c}-{n}" for c, n in MORE])
def test_nodes_at_the_pass_boundaries(gpu_engine, case, n_y):
    """The grid's end on a pass boundary (2048), one and two nodes past it (2049, 2050: y_pass_interior's
    base + span + 1 < n), a partial pass after 33 (2113) and an end inside a group of four (4000)."""
    idx, got, nd = probe(gpu_engine, case, Y.ZGRID, n_y)
    assert idx[-130] == n_y - 130 and idx[64] == 64


def sums_of(eng, case, grid, n_y):
    """Y_B under the four windows against the mp sums; dense = reuse = the one-point grid sweep."""
    cfgm = pkg("config")
    c, (y_lo, y_hi, step, ys), F, nd = device_ref(eng, case, grid, n_y)
    kw = dict(n_y=n_y, nz=grid[0], z_max=grid[1])
    axes = [("m_chi_GeV", np.array([c["m_chi_GeV"]]))]
    cfgs = [dict(c, source_shape_sigma_y=s) for s in SIGMAS]
    gauss = both_paths(eng, np.concatenate([cfgm.to_point(x) for x in cfgs]), **kw)
    flat = both_paths(eng, np.repeat(cfgm.to_point(c), 2), window=FLAT, **kw)
    assert np.array_equal(flat[0].view(np.int64), flat[1].view(np.int64))
    rows = [(f"sigma_y = {s}", Y.win_gauss(nd, s), gauss[i], x, None) for i, (s, x) in enumerate(zip(SIGMAS, cfgs))]
    rows.append(("W = 1", Y.win_one(nd), flat[0], c, FLAT))
    worst = 0.0
    for name, win, rec, x, block in rows:
        assert not win.undecided
        one = eng.sweep(x, axes, 0, 1, window=block, **kw)         # lzq_sweep_grid(_window) on a one-point grid
        assert eng.last_yields_path == "dense"
        assert np.array_equal(one.cpu().numpy()[0].view(np.int64), rec.view(np.int64)), (case, name)
        ref = Y.sum_ref(nd, win)
        rel, ratio, bad = Y.compare_sum(rec[0], ref)
        with mp.workdps(Y.DPS):
            acc = float(ref[2] / ref[0]) if ref[0] > 0 else 0.0
        print(f"Y_B [{case}, n_y = {n_y}, z grid {grid}, {name}]: {float(rec[0])!r}, accumulation {acc:.2e}, "
              f"rel err {rel:.3e}, err/tol {ratio:.3f}")
        assert bad is None, (case, name, bad)
        assert not (rec[0] == 0.0 and math.copysign(1.0, rec[0]) < 0)
        worst = max(worst, ratio)
    if case == "dead source":
        assert all(Y.is_pos_zero(float(r[2][0])) for r in rows)
    return worst


@pytest.mark.parametrize("case,grid", RUNS, ids=RUN_IDS)
def test_sums_against_mp(gpu_engine, case, grid):
    assert sums_of(gpu_engine, case, grid, Y.NY) < 1.0


@pytest.mark.parametrize("case,n_y", MORE, ids=[f"{c}-{n}" for c, n in MORE])
def test_sums_at_the_pass_boundaries(gpu_engine, case, n_y):
    assert sums_of(gpu_engine, case, Y.ZGRID, n_y) < 1.0


def test_default_window_single_node(gpu_engine):
    """source_shape_sigma_y = 0 (the 1e-6 floor) and T_max = T_p: y_lo = 0 exactly, W is 1 at node 0 and
    exactly 0 elsewhere, so Y_B is the default window path's own probe of node 0 with its half weight."""
    cfgm = pkg("config")
    over = dict(source_shape_sigma_y=0.0, T_max_over_Tp=1.0)
    c, (y_lo, y_hi, step, ys), F, nd = device_ref(gpu_engine, "shipped", **over)
    assert y_lo == 0.0 and ys[0] == 0.0
    win = Y.win_gauss(nd, 0.0)
    assert not win.zero[0] and all(win.zero[1:]) and not win.undecided
    out = both_paths(gpu_engine, np.repeat(cfgm.to_point(c), 2), n_y=Y.NY, nz=Y.ZGRID[0], z_max=Y.ZGRID[1])
    one = gpu_engine.sweep(c, [("m_chi_GeV", np.array([c["m_chi_GeV"]]))], 0, 1, n_y=Y.NY, nz=Y.ZGRID[0], z_max=Y.ZGRID[1])
    assert np.array_equal(one.cpu().numpy()[0].view(np.int64), out[0].view(np.int64))
    rel, ratio, bad = Y.compare_sum(out[0, 0], Y.sum_ref(nd, win))
    print(f"default window, one node: Y_B = {float(out[0, 0])!r}, rel err {rel:.3e}, err/tol {ratio:.3f}")
    assert bad is None and out[0, 0] > 0.0
    # the same node through the plateau probe: the two window paths agree on fl(w_0 I_0)
    blk = pkg("window").to_window(probe_block(ys[0], step))
    via_probe = gpu_engine.yields(cfgm.to_point(c), window=blk, n_y=Y.NY, nz=Y.ZGRID[0], z_max=Y.ZGRID[1]).cpu().numpy()
    assert via_probe[0, 0] == out[0, 0]


# ---------------------------------------------------------------------------------------------
# the epilogue
# ---------------------------------------------------------------------------------------------
EPILOGUE = {
    "thermal, relativistic": ("shipped", dict(regime="thermal")),
    "thermal, non-relativistic": ("heavy", dict(regime="thermal")),
    # T_hi = 200 = m/3 exactly: the comparison is strict, so the non-relativistic branch
    "thermal, T_hi = m/3 exactly": ("shipped", dict(regime="thermal", T_max_over_Tp=2.0, m_chi_GeV=600.0)),
    "nonthermal, Y_chi_init": ("shipped", {}),
    "nonthermal, n_chi_at_Tp": ("shipped", dict(Y_chi_init=None, n_chi_at_Tp_GeV3=1e-3)),
    "nonthermal, neither": ("shipped", dict(Y_chi_init=None)),
    "Y_B = 0": ("dead source", {}),
    "invalid regime": ("shipped", dict(regime="auto")),
}


def test_epilogue_against_mp(gpu_engine):
    cfgm, nat = pkg("config"), pkg("_native")
    names = list(EPILOGUE)
    cfgs = [Y.cfg_of(case, **over) for case, over in EPILOGUE.values()]
    out = both_paths(gpu_engine, np.concatenate([cfgm.to_point(c) for c in cfgs] * 2), n_y=Y.NY, nz=Y.ZGRID[0],
                     z_max=Y.ZGRID[1])[:len(cfgs)]
    col = {k: i for i, k in enumerate(nat.YIELD_FIELDS)}
    worst = 0.0
    for name, c, rec in zip(names, cfgs, out):
        ref = Y.epilogue_ref(c, rec[col["Y_B"]])
        assert rec[col["P_used"]] == c["P_chi_to_B"]
        if ref is None:
            assert name == "invalid regime"
            assert all(math.isnan(rec[col[k]]) for k in ("Y_B", "rho_B_kg_m3", "rho_DM_kg_m3", "DM_over_B"))
            continue
        for k in Y.EPI_FIELDS:
            val, rel = ref[k]
            got = float(rec[col[k]])
            assert math.isfinite(got) and got >= 0.0, (name, k, got)
            with mp.workdps(Y.DPS):
                if val == 0:
                    assert Y.is_pos_zero(got), (name, k, got)
                    continue
                e = float(abs(mp.mpf(got) - val) / val)
            if rel == 0.0:
                assert e == 0.0, (name, k, got)
            else:
                worst = max(worst, e / rel)
                assert e <= rel, (name, k, got, float(val), e, rel)
        print(f"epilogue [{name}]: Y_B = {float(rec[0])!r}, Y_chi = {float(rec[1])!r}, DM/B = {float(rec[4])!r}")
    # the branch of the exact-equality case, and the Y_B = 0 quotient
    with mp.workdps(Y.DPS):
        i = names.index("thermal, T_hi = m/3 exactly")
        assert cfgs[i]["T_max_over_Tp"] * cfgs[i]["T_p_GeV"] == cfgs[i]["m_chi_GeV"] / 3.0 == 200.0
        assert Y.epilogue_ref(cfgs[i], 0.0)["Y_chi"][1] > 28.0 * Y.U          # the non-relativistic count
        z = out[names.index("Y_B = 0")]
        assert Y.is_pos_zero(float(z[0])) and z[col["DM_over_B"]] == z[col["rho_DM_kg_m3"]] / 1e-300
    print(f"epilogue: worst error / tolerance {worst:.3f}")
    assert worst < 1.0
