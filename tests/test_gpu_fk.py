"""The momentum-averaged LZ probability on the GPU (csrc/lzq_fk.hip): lzq_fk_pbar_batch against the host
build, the R tables, and Y_B = int g(y) P-bar(y) dy from shared z-sum tables against the mpmath reference of
tests/yquad_ref.py (imported unchanged), with the counted P-bar tolerance of tests/fk_ref.py.  Needs an
MI355X.

The yields reference takes two of the device's own arrays as inputs, as yquad_ref takes F_j: the z-sums F_j
(the shared table) and mu_j = m/T(y_j) (lzq_fk_tables' optional output; T comes from rsqrt_pos, whose first
step is the hardware's v_rsq_f64, so no host forms mu_j bit for bit -- mu_j is compared with the exact m/T_j
within its own counted roundings instead).  P-bar_j is then the rule's sum at mu_j in long double, the
per-node window handed to yquad_ref is W_j P-bar_j, and P = 1.

Measured on an MI355X: the prints below.
"""
import ctypes
import math

import mpmath as mp
import numpy as np
import pytest
import torch

import fk_ref as R
import yquad_ref as Y
from conftest import BASE_CFG, full_cfg, pkg
from test_yquad_host import probe_block

pytestmark = pytest.mark.gpu
U = Y.U
HDR = 6
TWO_PI = 2.0 * math.pi
NY = 2000
STATS = {"fermion": 0, "boson": 1}
# three classes; A and B share a z-sum table (m is not in its key), C has its own y-grid
CLASSES = [
    dict(cfg={}, delta=0.0237, block={"p": 1.0, "v_ref": 1.0}),
    dict(cfg={"m_chi_GeV": 600.7}, delta=0.3, block={"p": 2.0, "v_ref": 0.5}),         # T = m/3 at node 214
    dict(cfg={"m_chi_GeV": 30.0, "chi_stats": "boson", "T_max_over_Tp": 3.0}, delta=1e-3,
         block={"p": 3.5, "v_ref": 1.0}),
]
SIGMAS = (9.0, 0.3)
N_POINTS = 130

_cache = {}


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dev_bytes(eng, arr):
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8).copy()).to(eng.device)


def cfg_of(k, **over):
    return full_cfg({**BASE_CFG, **CLASSES[k]["cfg"], **over})


def batch():
    """130 points in 3 classes (44 / 43 / 43), the two sigmas alternating inside a class: more than one
    block of wavefronts and several points per class.  (configs, points, blocks, delta_0)"""
    cfgm, fk = pkg("config"), pkg("fk")
    cfgs = [cfg_of(i % 3, source_shape_sigma_y=SIGMAS[(i // 3) % 2]) for i in range(N_POINTS)]
    pts = np.concatenate([cfgm.to_point(c) for c in cfgs])
    fks = np.concatenate([fk.to_fk(CLASSES[i % 3]["block"]) for i in range(N_POINTS)])
    delta = np.array([CLASSES[i % 3]["delta"] for i in range(N_POINTS)])
    return cfgs, pts, fks, delta


def class_tables(eng, n_y=NY):
    """(R, mu) of the three classes at n_y, one representative point each."""
    cfgm, fk = pkg("config"), pkg("fk")
    pts = np.concatenate([cfgm.to_point(cfg_of(k)) for k in range(3)])
    fks = np.concatenate([fk.to_fk(c["block"]) for c in CLASSES])
    delta = np.array([c["delta"] for c in CLASSES])
    rep = torch.arange(3, dtype=torch.int64, device=eng.device)
    Rt, mu = eng.fk_tables(eng.points_to_device(pts), eng._f64(delta), dev_bytes(eng, fks), rep, n_y, with_mu=True)
    torch.cuda.synchronize()
    return Rt.cpu().numpy(), mu.cpu().numpy()


def pbar_ref(eng, k, n_y=NY):
    """Per class: the device's mu_j, P-bar_j of the rule in long double at them, the counted tolerances."""
    key = ("pbar", k, n_y)
    if key not in _cache:
        _, mu = class_tables(eng, n_y)
        for kk in range(3):
            c, blk = CLASSES[kk], CLASSES[kk]["block"]
            st = STATS[cfg_of(kk)["chi_stats"]]
            g = TWO_PI * c["delta"]
            ld = R.pbar_rule_ld(mu[kk], g, blk["p"], blk["v_ref"], st)
            tol = np.array([R.pbar_tol(m, g, blk["p"], blk["v_ref"], st) for m in mu[kk]])
            _cache[("pbar", kk, n_y)] = (mu[kk], ld, tol)
    return _cache[key]


def mu_check(c, ys, mu):
    """The device's mu_j against the exact m/T_j: the quotient (1), T's product (1), rsqrt_pos (4) and half
    of d's own error u (1 + A), A = |2y/B| / d the cancellation in 1 + 2y/B (yquad_ref's K_X terms)."""
    worst = 0.0
    with mp.workdps(Y.DPS):
        B, Tp, m = mp.mpf(c["beta_over_H"]), mp.mpf(c["T_p_GeV"]), mp.mpf(c["m_chi_GeV"])
        for j in range(0, len(ys), 7):
            y = mp.mpf(float(ys[j]))
            raw = 1 + 2 * y / B
            d = max(raw, mp.mpf(1e-12))
            A = 0.0 if raw <= mp.mpf(1e-12) else float(abs(2 * y / B) / d)
            exact = m * mp.sqrt(d) / Tp
            tol = (6.0 + 0.5 * (1.0 + A)) * U
            worst = max(worst, float(abs(mp.mpf(float(mu[j])) - exact) / exact) / tol)
    return worst


def win_times_pbar(nd, win, ld, tol):
    """yquad_ref's window object for W_j P-bar_j: the product's rounding (1) and P-bar's counted ones."""
    w = Y.Win()
    with mp.workdps(Y.DPS):
        w.W = [W * R.to_mp(p) for W, p in zip(win.W, ld)]
    w.rel = [r + float(t) + U for r, t in zip(win.rel, tol)]
    w.zero, w.exact, w.undecided = list(win.zero), False, list(win.undecided)
    return w


def z_tables_of(eng, n_y):
    """Per point of the engine's last fk batch: its z-sum table row (header + F), from the engine's own
    workspace."""
    _, _, idx = eng._keepalive_fk[:3]
    stride = max(n_y, 2000) + HDR
    tabs = eng._zwork[:(int(idx.max().item()) + 1) * stride].view(-1, stride).cpu().numpy()
    return tabs, idx.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# P-bar alone
# ---------------------------------------------------------------------------------------------
def test_pbar_batch_against_host(gpu_engine):
    fk = pkg("fk")
    rng = np.random.default_rng(7)
    n = 4096
    mu = np.exp(rng.uniform(math.log(1e-3), math.log(849.0), n))
    g = np.exp(rng.uniform(math.log(1e-9), math.log(10.0), n))
    mu[:8] = [0.0, np.nextafter(3.0, 0.0), 3.0, 849.0, 0.0, 3.0, 849.0, 0.3]
    g[8:14] = [0.0, 1e-12, np.inf, 0.0, 1e-12, np.inf]
    mu[8:14] = [0.0, 0.0, 0.0, 849.0, 849.0, 849.0]
    g[14:17], mu[14:17] = [0.0, np.inf, 1e-12], [3.0, 3.0, 42.0]
    delta = g / TWO_PI
    g = TWO_PI * delta                                    # the g both builds form
    blocks = [({"p": 0.0}, 0), ({"p": 1.0, "v_ref": 1.0}, 1), ({"p": 2.0, "v_ref": 0.1}, 0), ({"p": 3.5, "v_ref": 1.0}, 1)]
    worst = 0.0
    for q, (blk, st) in enumerate(blocks):
        sl = slice(q, n, len(blocks)) if q else slice(0, n)   # the first block takes every pair
        m_, d_, g_ = mu[sl], delta[sl], g[sl]
        host = fk.pbar_host(blk, m_, d_, st)
        dev = gpu_engine.pbar(blk, m_, d_, st).cpu().numpy()
        p, v = blk["p"], blk.get("v_ref", 1.0)
        for i in range(m_.size):
            if g_[i] == 0.0:
                assert Y.is_pos_zero(float(dev[i])) and Y.is_pos_zero(float(host[i]))
            elif math.isinf(g_[i]):
                assert dev[i] == 1.0 and host[i] == 1.0
            else:
                # each build is within the counted tolerance of the rule's exact sum
                tol = 2.0 * R.pbar_tol(m_[i], g_[i], p, v, st)
                assert tol < 2e-12
                e = abs(dev[i] - host[i]) / host[i]
                worst = max(worst, e / tol)
                assert e <= tol, (blk, st, m_[i], g_[i], dev[i], host[i], e, tol)
    print(f"lzq_fk_pbar_batch vs lzq_fk_pbar_host, {n} pairs: worst error / counted tolerance {worst:.3f}")
    # refused values in device memory: NaN
    bad = gpu_engine.pbar({"p": 1.0}, [1.0, -1.0, float("nan"), 1.0], [-0.5, 0.1, 0.1, float("nan")]).cpu().numpy()
    assert np.all(np.isnan(bad))


@pytest.mark.parametrize("n_y", [2000, 2049])
def test_r_tables(gpu_engine, n_y):
    """Every node of the R tables equals lzq_fk_pbar_batch at the mu_j the table kernel formed, bit for
    bit; the last slot is P-bar(m/T_p); mu_j is the exact m/T_j within its counted roundings."""
    Rt, mu = class_tables(gpu_engine, n_y)
    assert Rt.shape == (3, n_y + 1 + HDR) and mu.shape == (3, n_y + 1)
    for k, c in enumerate(CLASSES):
        cfg = cfg_of(k)
        st = STATS[cfg["chi_stats"]]
        y_lo, y_hi, step, ys = Y.ygrid(cfg, n_y)
        assert list(Rt[k, :2]) == [y_lo, y_hi] and Rt[k, 3] == cfg["m_chi_GeV"] and Rt[k, 4] == TWO_PI * c["delta"]
        assert Rt[k, 2] == n_y + 2.0 ** 32 * st
        alone = gpu_engine.pbar(c["block"], mu[k], c["delta"], st).cpu().numpy()
        assert np.array_equal(alone.view(np.int64), Rt[k, HDR:].view(np.int64))
        assert mu[k, n_y] == cfg["m_chi_GeV"] / cfg["T_p_GeV"]
        assert np.all((Rt[k, HDR:] > 0.0) & (Rt[k, HDR:] <= 1.0))
        worst = mu_check(cfg, ys, mu[k, :n_y])
        print(f"R table class {k}, n_y = {n_y}: mu in [{mu[k].min():.3g}, {mu[k].max():.3g}], "
              f"R in [{Rt[k, HDR:].min():.3e}, {Rt[k, HDR:].max():.3e}], mu_j error / tolerance {worst:.3f}")
        assert worst < 1.0


# ---------------------------------------------------------------------------------------------
# yields
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("continuum", [False, True], ids=["linspace", "continuum"])
def test_yields_against_mp(gpu_engine, continuum):
    eng = gpu_engine
    cfgs, pts, fks, delta = batch()
    out = eng.yields(pts, n_y=NY, fk=fks, fk_delta=delta, continuum=continuum).cpu().numpy()
    assert eng.last_yields_path == "tables" and eng.last_fk_classes == 3
    tabs, idx = z_tables_of(eng, NY)
    assert tabs.shape[0] == 2 and idx[0] == idx[1] != idx[2]          # A and B share a z-sum table
    assert tabs[0, 4] == (-1.0 if continuum else 1200.0)
    worst = 0.0
    for k in range(3):
        mu, ld, tol = pbar_ref(eng, k)
        c = cfg_of(k)
        y_lo, y_hi, step, ys = Y.ygrid(c, NY)
        F = tabs[idx[k], HDR:]
        assert list(tabs[idx[k], :3]) == [y_lo, y_hi, float(NY)]
        nd = Y.nodes_ref(dict(c, P_chi_to_B=1.0), ys, F)
        assert not nd.undecided
        if k == 1:   # T = m/3 inside one wavefront's 64 nodes
            j = int(np.argmax(~nd.relativistic))
            assert nd.relativistic[j - 1] and not nd.relativistic[j] and 0 < j % 64 < 63, j
        for s, sigma in enumerate(SIGMAS):
            rows = [i for i in range(N_POINTS) if i % 3 == k and (i // 3) % 2 == s]
            assert len(rows) >= 21
            assert all(np.array_equal(out[i].view(np.int64), out[rows[0]].view(np.int64)) for i in rows)
            win = win_times_pbar(nd, Y.win_gauss(nd, sigma), ld[:NY], tol[:NY])
            assert not win.undecided
            rec = out[rows[0]]
            rel, ratio, bad = Y.compare_sum(rec[0], Y.sum_ref(nd, win))
            print(f"Y_B [class {k}, sigma_y = {sigma}, {'continuum' if continuum else 'linspace'}]: {float(rec[0])!r}, "
                  f"P_used = {float(rec[5])!r}, rel err {rel:.3e}, err/tol {ratio:.3f}")
            assert bad is None, (k, sigma, bad)
            worst = max(worst, ratio)
            # P_used is the table's last slot: P-bar(m/T_p) within its count; the epilogue from the device's Y_B
            assert abs(np.longdouble(rec[5]) - ld[NY]) <= tol[NY] * ld[NY]
            epi = Y.epilogue_ref(c, rec[0])
            for f, col in (("rho_B_kg_m3", 2), ("DM_over_B", 4)):
                val, r = epi[f]
                with mp.workdps(Y.DPS):
                    assert abs(mp.mpf(float(rec[col])) - val) <= r * val
    assert worst < 1.0


def test_p0_is_the_constant_P(gpu_engine):
    """p = 0 against Engine.yields(reuse=True) with P = 1 - e^(-2 pi delta_0)."""
    cfgm = pkg("config")
    for delta in (1e-3, 0.0237, 1.0):
        P = -math.expm1(-TWO_PI * delta)
        for k in range(3):
            pts = np.repeat(cfgm.to_point(cfg_of(k, P_chi_to_B=P)), 4)
            ref = gpu_engine.yields(pts, n_y=NY, reuse=True).cpu().numpy()
            assert gpu_engine.last_yields_path == "tables"
            got = gpu_engine.yields(pts, n_y=NY, fk={"p": 0.0}, fk_delta=delta).cpu().numpy()
            e = abs(got[:, 0] - ref[:, 0]) / ref[:, 0]
            print(f"p = 0, delta_0 = {delta}, class {k}: Y_B = {got[0, 0]!r} vs {ref[0, 0]!r}, rel {e.max():.3e}")
            assert np.all(e <= 1e-11) and np.all(abs(got[:, 5] - P) <= 1e-11 * P)
            assert np.array_equal(got[:, 1].view(np.int64), ref[:, 1].view(np.int64))      # Y_chi: untouched


def test_node_probes(gpu_engine):
    """A plateau window that is 1 at one node and exactly 0 elsewhere: Y_B = fl(w_j I_j R_j)."""
    eng, cfgm, W, fk = gpu_engine, pkg("config"), pkg("window"), pkg("fk")
    k = 1
    c, blk = cfg_of(k), CLASSES[k]["block"]
    mu, ld, tol = pbar_ref(eng, k)
    y_lo, y_hi, step, ys = Y.ygrid(c, NY)
    js = [0, 1, 63, 64, 213, 214, 215, 1000, NY - 2, NY - 1]
    pts = np.repeat(cfgm.to_point(c), len(js))
    wins = np.concatenate([W.to_window(probe_block(ys[j], step)) for j in js])
    out = eng.yields(pts, n_y=NY, fk=blk, fk_delta=CLASSES[k]["delta"], window=wins).cpu().numpy()
    tabs, idx = z_tables_of(eng, NY)
    nd = Y.nodes_ref(dict(c, P_chi_to_B=1.0), ys, tabs[idx[0], HDR:])
    one = Y.win_one(nd)
    worst, nonzero = 0.0, 0
    with mp.workdps(Y.DPS):
        for j, rec in zip(js, out):
            term, t = Y.node_tol(nd, one, j)
            if t is None:
                assert Y.is_pos_zero(float(rec[0])), j
                continue
            want = term * R.to_mp(ld[j])
            t = t * R.to_mp(ld[j]) + (float(tol[j]) + U) * want
            worst = max(worst, float(abs(mp.mpf(float(rec[0])) - want) / t))
            nonzero += 1
    print(f"node probes with P-bar: {nonzero} of {len(js)} non-zero, worst error / tolerance {worst:.3f}")
    assert nonzero >= 5 and worst < 1.0


def raw_fk(eng, pts, fks, delta, tidx, cidx, work, Rt, n_y=NY, nz=1200, z_max=30.0):
    """lzq_yields_batch_reuse_fk through the raw ABI on given tables."""
    n = pts.size
    out = torch.full((n, 6), -7.0, dtype=torch.float64, device=eng.device)
    d_pts, d_fk, d_delta = eng.points_to_device(pts), dev_bytes(eng, fks), eng._f64(delta)
    d_t = torch.as_tensor(np.asarray(tidx, dtype=np.int32), device=eng.device)
    d_c = torch.as_tensor(np.asarray(cidx, dtype=np.int32), device=eng.device)
    eng._check(eng.lib.lzq_yields_batch_reuse_fk(vp(d_pts), n, n_y, nz, z_max, vp(d_delta), vp(d_fk), vp(d_t), vp(work),
                                                 work.numel(), vp(d_c), vp(Rt), Rt.numel(), None, None, vp(out),
                                                 eng._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_headers_refusals_and_dead_source(gpu_engine):
    eng, cfgm, fk = gpu_engine, pkg("config"), pkg("fk")
    c = cfg_of(0)
    blk, delta = fk.to_fk(CLASSES[0]["block"]), CLASSES[0]["delta"]
    pt = cfgm.to_point(c)
    good = eng.yields(pt, n_y=NY, fk=blk, fk_delta=delta).cpu().numpy()[0]
    assert np.all(np.isfinite(good)) and good[0] > 0.0
    stride = NY + HDR
    work = eng._zwork[:stride].clone()
    Rt = eng._keepalive_fk[7].clone()
    again = raw_fk(eng, pt, blk, [delta], [0], [0], work, Rt)[0]
    assert np.array_equal(again.view(np.int64), good.view(np.int64))
    # a wrong key in either header: NaN yields, Y_chi and rho_DM untouched
    for slot in range(HDR):
        bad = Rt.clone()
        bad.view(torch.int64)[0, slot] ^= 1            # one bit of the key (its last slot is a bit pattern)
        o = raw_fk(eng, pt, blk, [delta], [0], [0], work, bad)[0]
        assert all(math.isnan(o[i]) for i in (0, 2, 4, 5)) and o[1] == good[1] and o[3] == good[3], (slot, o)
    for slot in (0, 3, 4, 5):
        bad = work.clone()
        bad.view(torch.int64)[slot] ^= 1
        o = raw_fk(eng, pt, blk, [delta], [0], [0], bad, Rt)[0]
        assert all(math.isnan(o[i]) for i in (0, 2, 4)), (slot, o)
    # another point's class table: the key differs in m
    other = cfgm.to_point(cfg_of(0, m_chi_GeV=0.96))
    assert math.isnan(raw_fk(eng, other, blk, [delta], [0], [0], work, Rt)[0, 0])
    # a continuum key against a linspace table
    assert math.isnan(raw_fk(eng, pt, blk, [delta], [0], [0], work, Rt, nz=-1)[0, 0])
    # refused blocks and delta_0 in device memory, and indices outside the tables: NaN, no table read
    blocks = np.concatenate([fk.to_fk({"p": 9.0}), fk.to_fk({"v_ref": 0.0}), fk.to_fk({"kind": 3}), blk, blk, blk, blk])
    deltas = [delta, delta, delta, -1.0, float("nan"), delta, delta]
    tix = [-1, -1, -1, -1, -1, 1, 0]
    cix = [-1, -1, -1, -1, -1, 0, 1]
    o = raw_fk(eng, np.repeat(pt, 7), blocks, deltas, tix, cix, work, Rt)
    assert np.all(np.isnan(o[:, [0, 2, 4]])) and np.all(o[:, 1] == good[1])
    # a dead source (exp(-m/T) underflows at every node): exactly +0
    dead = cfgm.to_point(cfg_of(0, m_chi_GeV=1e6))
    z = eng.yields(np.repeat(dead, 2), n_y=NY, fk=blk, fk_delta=delta).cpu().numpy()
    assert all(Y.is_pos_zero(float(x)) for x in z[:, 0]) and np.all(np.isfinite(z[:, 5]))
    # host-side refusals of Engine.yields
    nat = pkg("_native")
    with pytest.raises(nat.LzqError):
        eng.yields(pt, n_y=NY, fk={"p": 9.0})
    with pytest.raises(nat.LzqError):
        eng.yields(pt, n_y=NY, fk=blk, fk_delta=-1.0)
    with pytest.raises(ValueError):
        eng.yields(pt, n_y=NY, fk=blk, aov=c)


def test_sweep_spec_with_fk_axes(gpu_engine):
    """An "fk" section with an fk_p axis of 3 x a delta_LZ axis of 4: the table equals Engine.yields(fk=)
    on the expanded points, bit for bit, for two chunkings."""
    eng, sw, fk = gpu_engine, pkg("sweep"), pkg("fk")
    spec = sw.spec_from_json({"name": "fk", "base": dict(BASE_CFG), "n_y": NY, "fk": {"p": 1.0, "v_ref": 0.5},
                              "axes": [{"field": "fk_p", "values": [0.0, 1.0, 3.5]},
                                       {"field": "delta_LZ", "values": [1e-3, 0.0237, 0.3, 1.0]}]})
    assert spec.total == 12 and sw.spec_from_json(spec.to_json()).to_json() == spec.to_json()
    compute = sw.make_compute(spec, eng)
    tables = []
    for chunks in ([(0, 12)], [(0, 5), (5, 5), (10, 2)]):
        tab = torch.empty((12, 6), dtype=torch.float64, device=eng.device)
        for s, n in chunks:
            compute(s, n, tab[s:s + n])
        tables.append(tab.cpu().numpy())
    pts, _ = sw.grid_records(spec, 0, 12, eng)
    fks, delta = sw.fk_records(spec, 0, 12, pts)
    assert list(fks["p"]) == [0.0] * 4 + [1.0] * 4 + [3.5] * 4 and list(delta[:4]) == [1e-3, 0.0237, 0.3, 1.0]
    assert np.all(fks["v_ref"] == 0.5)
    direct = eng.yields(pts, n_y=NY, fk=fks, fk_delta=delta).cpu().numpy()
    assert eng.last_fk_classes == 12
    for t in tables:
        assert np.array_equal(t.view(np.int64), direct.view(np.int64))
    assert np.all(np.isfinite(direct)) and np.all(np.diff(direct[:4, 0]) > 0)       # Y_B rises with delta_0
    with pytest.raises(ValueError):
        sw.spec_from_json({"axes": [{"field": "fk_p", "values": [1.0]}]})
