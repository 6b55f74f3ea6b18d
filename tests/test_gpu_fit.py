"""Sweep fits on the device (lzq_fit_*, csrc/lzq_fit.hip) against the numpy implementation
(fit.HostFit, itself pinned to literal values by tests/test_fit_host.py): bit-identical chi2, indices
and counts for every row count around the wave and block sizes, every chunking, every map shape and
both map paths (block-private LDS, straight to global memory), 64-bit flat indices, the selection
list, the real engine through run_sweep, and the sweep CLI as child processes (one rank, and two
gloo ranks on the one GPU)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import BASE_CFG, PKG_NAME, ROOT, full_cfg, pkg

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
F = pkg("fit")
FIELDS = pkg("_native").YIELD_FIELDS


def wide_table(n, seed):
    """Magnitudes from 1e-300 to 1e300 in both signs, planted NaN / inf / overflowing rows, and pairs
    of identical rows that are the minimum of their cell of a 16-cell fastest-axis map: inside a
    wave (3, 35), across a wave boundary (60, 76) and across a block boundary (250, 266)."""
    rng = np.random.default_rng(seed)
    t = rng.choice([-1.0, 1.0], (n, 6)) * 10.0 ** rng.uniform(-300, 300, (n, 6))
    t[rng.random((n, 6)) < 0.3] = 0.0
    t[:, 0] = 10.0 ** rng.uniform(-3, 3, n)       # a well-scaled column, so most rows are valid
    for k, (a, b) in enumerate(((3, 35), (60, 76), (250, 266))):
        for r in (a, b):
            if r < n:
                t[r] = 0.0
                t[r, 0] = 1.0 + (k + 1) * 2.0 ** -30
    if n > 8:
        bad = rng.choice(np.arange(n)[np.isin(np.arange(n), (3, 35, 60, 76, 250, 266), invert=True)], max(3, n // 40),
                         replace=False)
        t[bad[0::3], 0] = NAN
        t[bad[1::3], 0] = INF
        t[bad[2::3], 0] = 1e300      # (x - 1) / 0.5 squared overflows
    return t


def coarse_table(n, seed):
    """Quarter-integer values: exact ties everywhere."""
    rng = np.random.default_rng(seed)
    t = rng.integers(-6, 7, (n, 6)).astype(np.float64) / 4.0
    bad = rng.choice(n, max(1, n // 50), replace=False)
    t[bad[0::2], 4] = NAN
    t[bad[1::2], 0] = -INF
    return t


TERMS = [{"field": "Y_B", "target": 1.0, "sigma": 0.5}, {"field": "DM_over_B", "target": -0.5, "sigma": 0.25},
         {"field": "P_used", "target": 0.0, "sigma": 1e3}, {"field": "Y_chi", "target": 0.25, "sigma": 3.0}]


def make_fit(n_terms=2, levels=(1.0, 4.0, 9.0, 1e6), select=(9.0, 1000)):
    return F.FitSpec.from_json({"terms": TERMS[:n_terms], "levels": list(levels),
                                "select": None if select is None else {"level": select[0], "cap": select[1]}})


def fmap(*axes):
    """A map from (stride, len) pairs."""
    return F.FitMap(tuple(f"a{k}" for k in range(len(axes))), tuple(a[0] for a in axes), tuple(a[1] for a in axes))


def host_result(fit, maps, table, start=0):
    h = F.HostFit(fit, maps)
    h.update(table, start)
    return h.result()


def device_result(eng, fit, maps, table, start=0, chunk=None, unaligned=False):
    n = table.shape[0]
    if unaligned:   # records on an 8-byte but not 16-byte aligned base
        buf = torch.empty(n * 6 + 1, dtype=torch.float64, device=eng.device)
        d = buf[1:].view(n, 6)
        d.copy_(torch.from_numpy(table))
        assert d.data_ptr() % 16 == 8
    else:
        d = torch.from_numpy(table).to(eng.device)
    st = eng.fit_state(fit, maps)
    for a in range(0, n, chunk or max(n, 1)):
        b = min(n, a + (chunk or n))
        eng.fit_update(st, d[a:b], start + a)
        if fit.select is not None:
            eng.fit_select(st, d[a:b], start + a)
    return eng.fit_result(st)


SIZES = [1, 63, 64, 65, 255, 257, 1000, 70_001]
SMALL_MAPS = [fmap((1, 16)), fmap((64, 5), (1, 16)), fmap((4096, 1000))]


@pytest.fixture(scope="module")
def tables():
    return {(kind, n): (wide_table if kind == "wide" else coarse_table)(n, 7 + n) for n in SIZES
            for kind in ("wide", "coarse")}


@pytest.mark.parametrize("n", SIZES)
def test_row_counts_terms_and_ties(gpu_engine, tables, n):
    for kind in ("wide", "coarse"):
        t = tables[(kind, n)]
        for n_terms in ((1, 2, 3, 4) if n <= 1000 else (2, 4)):
            fit = make_fit(n_terms)
            ref = host_result(fit, SMALL_MAPS, t, 5)
            got = device_result(gpu_engine, fit, SMALL_MAPS, t, 5)
            assert F.differences(got, ref) == [], (kind, n, n_terms)
        if kind == "wide" and n > 266:   # the planted pairs are their cells' minima, at the lower index
            ref = host_result(make_fit(1), [fmap((1, 16))], t, 0)
            assert ref["n_invalid"] > 0
            assert [int(ref["maps"][0]["argmin"][c]) for c in (3, 60 % 16, 250 % 16)] == [3, 60, 250]
    got = device_result(gpu_engine, make_fit(3), SMALL_MAPS, tables[("wide", n)], 5, unaligned=True)
    assert F.differences(got, host_result(make_fit(3), SMALL_MAPS, tables[("wide", n)], 5)) == []


@pytest.mark.parametrize("chunk", [1, 7, 64, 1000])
def test_chunking_is_invisible(gpu_engine, tables, chunk):
    t = tables[("coarse", 70_001)]
    start = 12_345_677
    fit = make_fit(2, select=None if chunk == 1 else (4.0, 500))
    ref = host_result(fit, SMALL_MAPS, t, start)
    assert ref["n_selected"] is None or ref["n_selected"] > 500
    assert F.differences(device_result(gpu_engine, fit, SMALL_MAPS, t, start, chunk), ref) == []


def test_merge_of_disjoint_ranges(gpu_engine, tables):
    eng, t, fit = gpu_engine, tables[("coarse", 70_001)], make_fit(2, select=None)
    ref = host_result(fit, SMALL_MAPS, t, 0)
    d = torch.from_numpy(t).to(eng.device)
    parts = []
    for a, b in ((40_000, 70_001), (0, 1), (1, 40_000)):
        st = eng.fit_state(fit, SMALL_MAPS)
        eng.fit_update(st, d[a:b], a)
        parts.append(st)
    tot = eng.fit_state(fit, SMALL_MAPS)
    for st in parts:
        eng.fit_merge(tot, st.words)
    assert F.differences(eng.fit_result(tot), ref) == []


GRID = (3, 5, 7, 11)
GRID_STRIDE = (385, 77, 11, 1)
ax = lambda k: (GRID_STRIDE[k], GRID[k])


def test_map_shapes_on_a_small_grid(gpu_engine):
    t = coarse_table(1155, 3)
    shapes = [[fmap(ax(0), ax(1))], [fmap(ax(2), ax(3))], [fmap(ax(1), ax(3))], [fmap(ax(3), ax(1))], [fmap(ax(0))],
              [fmap(ax(3))], [fmap(ax(2))], [fmap(ax(0), ax(1)), fmap(ax(3), ax(1)), fmap(ax(2)), fmap(ax(2), ax(3))]]
    fit = make_fit(2, select=None)
    for maps in shapes:
        ref = host_result(fit, maps, t)
        assert ref["maps"][0]["chi2_min"].shape == tuple(m for m in maps[0].len)
        assert F.differences(device_result(gpu_engine, fit, maps, t, chunk=400), ref) == [], maps


def test_global_path_and_mixed_paths(gpu_engine):
    """300 x 300: the 90,000-cell map cannot be block-private in LDS; with four maps at once two
    take LDS and two go straight to global memory, and each is what it is alone."""
    n = 90_000
    t = coarse_table(n, 4)
    fit = make_fit(2, select=None)
    both, a0, a1, rev = fmap((300, 300), (1, 300)), fmap((300, 300)), fmap((1, 300)), fmap((1, 300), (300, 300))
    ref = host_result(fit, [both, a0, a1, rev], t)
    assert (ref["maps"][0]["argmin"] >= -1).all() and ref["maps"][0]["chi2_min"].shape == (300, 300)
    assert np.array_equal(ref["maps"][3]["argmin"], ref["maps"][0]["argmin"].T)
    got = device_result(gpu_engine, fit, [both, a0, a1, rev], t, chunk=33_333)
    assert F.differences(got, ref) == []
    for k, m in enumerate((both, a0, a1, rev)):
        alone = device_result(gpu_engine, fit, [m], t)
        assert np.array_equal(alone["maps"][0]["argmin"], ref["maps"][k]["argmin"]), k
        assert np.array_equal(alone["maps"][0]["chi2_min"].view(np.int64), ref["maps"][k]["chi2_min"].view(np.int64)), k
    # every row its own cell: ties impossible, argmin is the identity where the row is valid
    assert np.array_equal(got["maps"][0]["argmin"].ravel() >= 0, np.isfinite(F.chi2_rows(fit, t)))


def test_int64_flat_indices(gpu_engine):
    """Virtual axes 70,001 x 70,001 (4.9e9 points), rows of the flat range [2^32 - 100, 2^32 + 100)."""
    L = 70_001
    start = (1 << 32) - 100
    t = coarse_table(200, 5)
    fit = make_fit(2, select=(1e9, 300))
    maps = [fmap((L, L)), fmap((1, L))]
    ref = host_result(fit, maps, t, start)
    assert ref["best"]["index"] >= start and ref["selected"].max() > 1 << 32
    touched = np.flatnonzero(ref["maps"][1]["argmin"] >= 0)
    assert touched.size > 100 and set(np.flatnonzero(ref["maps"][0]["argmin"] >= 0)) == {start // L, (start + 199) // L}
    assert F.differences(device_result(gpu_engine, fit, maps, t, start, chunk=64), ref) == []


def test_grid_stride_walk(gpu_engine):
    """More rows than one launch has threads (512 blocks of 256): a thread then walks several rows,
    advancing its cell indices by carries instead of dividing again; here across 2^32, with strides
    that do and do not divide the step."""
    n, L = 300_007, 70_001
    start = (1 << 32) - 150_000
    t = coarse_table(n, 6)
    fit = make_fit(2, select=(2.0, 5000))
    maps = [fmap((L, 1000), (1, 1000)), fmap((64, 5), (1, 16)), fmap((4096, 1000)), fmap((7, 3), (100_003, 1 << 20))]
    ref = host_result(fit, maps, t, start)
    assert ref["n_selected"] > 5000 and (ref["maps"][0]["argmin"].max(axis=1) >= 0).sum() > 3
    for chunk in (None, 200_000):
        assert F.differences(device_result(gpu_engine, fit, maps, t, start, chunk), ref) == [], chunk


def test_selection(gpu_engine, tables):
    t = tables[("coarse", 70_001)]
    for level, cap in ((4.0, 1 << 20), (4.0, 777), (4.0, 0), (-1.0, 100)):
        fit = make_fit(2, select=(level, cap))
        ref = host_result(fit, [], t, 3)
        for chunk in (None, 5000, 2049):
            got = device_result(gpu_engine, fit, [], t, 3, chunk)
            assert F.differences(got, ref) == [], (level, cap, chunk)
            assert np.all(np.diff(got["selected"]) > 0) and got["selected"].size == min(cap, ref["n_selected"])
    assert host_result(make_fit(2, select=(4.0, 777)), [], t, 3)["n_selected"] > 777
    assert host_result(make_fit(2, select=(-1.0, 100)), [], t, 3)["n_selected"] == 0


# ---- one accumulator, two backends -------------------------------------------------------------
ACC_START, ACC_GRID = 5, (7, 112)       # flat indices 5 .. 781 of a 7 x 112 grid: the last grid row is partial
ACC_MAPS = [fmap((112, 7), (1, 112)), fmap((1, 112))]


def acc_table():
    """777 quarter-integer rows with two copies of the best row (chi2 0) in different chunks and one
    row so far out that it weighs nothing at either offset."""
    t = coarse_table(777, 11)
    t[[100, 500]] = 0.0
    t[[100, 500], 0], t[[100, 500], 4] = 1.0, -0.5
    t[700, 0], t[700, 4] = 1.0, 3.0      # chi2 196: exp(-97) is below 2^-62
    return t


def acc_fit(offset):
    return F.FitSpec.from_json({
        "terms": TERMS[:2], "levels": [1.0, 9.0], "select": {"level": 9.0, "cap": 5}, "posterior": {"offset": offset},
        "observables": [{"axes": [{"field": FIELDS[1], "lo": -1.0, "hi": 1.0, "bins": 16}]},
                        {"axes": [{"field": FIELDS[2], "lo": 0.3, "hi": 1.2, "per_octave": 4},
                                  {"field": FIELDS[3], "lo": -2.0, "hi": 1.0, "bins": 6}]}]})


def acc_fold(fit, engine, rows, bounds):
    acc = F.make_accumulator(fit, ACC_MAPS, engine, {"a0": np.linspace(0.0, 1.0, 112)})
    for a, b in bounds:
        acc.update(rows[a:b], ACC_START + a)
    return acc


def all_differences(a, b):
    return (F.differences(a, b) + F.post_differences(a["posterior"], b["posterior"]) +
            F.obs_differences(a["observables"], b["observables"]))


@pytest.mark.parametrize("offset", [2.0, "best"])
def test_host_and_device_are_one_accumulator(gpu_engine, offset):
    """The same chunks (300, 300, 177 rows, records on a base that is only 8-byte aligned) through
    make_accumulator's numpy states and its device states: one combined result, bit for bit, in one
    pass and as two ranks' words merged by the functions combine() calls behind its gather."""
    t, fit = acc_table(), acc_fit(offset)
    buf = torch.empty(t.size + 1, dtype=torch.float64, device=gpu_engine.device)
    d = buf[1:].view(777, 6)
    d.copy_(torch.from_numpy(t))
    assert d.data_ptr() % 16 == 8
    chunks = ((0, 300), (300, 600), (600, 777))
    ref = F.combine(acc_fold(fit, None, t, chunks), local=t, start=ACC_START)
    c = F.chi2_rows(fit, t)
    post = ref["posterior"]
    assert ref["n_valid"] > 0 and ref["n_invalid"] > 0 and ref["n_selected"] > 5 == len(ref["selected"])
    assert (c == np.nanmin(c)).sum() >= 2 and ref["best"]["index"] == ACC_START + int(np.flatnonzero(c == np.nanmin(c))[0])
    assert post["n_used"] > 0 and (post["n_zero"] > 0 or post["n_above"] > 0)
    assert all(o["n_in"] > 0 and o["n_out"] > 0 for o in ref["observables"])
    got = F.combine(acc_fold(fit, gpu_engine, d, chunks), local=d, start=ACC_START)
    assert all_differences(got, ref) == []
    for engine, rows in ((None, t), (gpu_engine, d)):
        parts = [acc_fold(fit, engine, rows, [ab]) for ab in ((0, 400), (400, 777))]
        for (a, b), acc in zip(((0, 400), (400, 777)), parts):
            if offset == "best":      # the second pass combine_posterior runs, at the whole table's best chi2
                acc.post_begin(ref["best"]["chi2"])
                acc.post_update(rows[a:b], ACC_START + a)
        stack = lambda get: torch.stack([get(acc) for acc in parts])
        res = F.merged_fit(parts[0], stack(lambda acc: acc.state.words),
                           torch.cat([acc.state.kept() for acc in parts])[:5])
        res["posterior"] = F.merged_posterior(parts[0], stack(lambda acc: acc.post.words))
        res["observables"] = F.merged_observables(parts[0], stack(lambda acc: acc.obs.words), int(post["Z_units"]))
        assert all_differences(res, ref) == [], engine


# ---- the real engine ---------------------------------------------------------------------------
def engine_spec():
    sw = pkg("sweep")
    return sw.SweepSpec("grid60", full_cfg(BASE_CFG), [("m_chi_GeV", np.logspace(0, 3.5, 5)),
                                                       ("I_p", np.linspace(0.05, 1, 3)),
                                                       ("delta_LZ", np.logspace(-4, 0, 4))])


def engine_fit(table):
    """Targets inside the 60-point table's own range, so levels and the selection split the grid."""
    yb, dm = np.median(table[:, 0]), np.median(table[:, 4])
    return F.FitSpec.from_json({"terms": [{"field": "Y_B", "target": float(yb), "sigma": float(abs(yb))},
                                          {"field": "DM_over_B", "target": float(dm), "sigma": float(abs(dm))}],
                                "levels": [0.5, 2.0], "maps": [["m_chi_GeV", "I_p"], ["delta_LZ"], ["delta_LZ", "m_chi_GeV"]],
                                "select": {"level": 2.0, "cap": 20}})


@pytest.mark.parametrize("reuse", [False, True])
def test_run_sweep_with_fit_on_the_engine(gpu_engine, reuse):
    sw = pkg("sweep")
    spec = engine_spec()
    plain = sw.run_sweep(spec, gpu_engine, chunk=16, log=lambda s: None, reuse=reuse)
    fit = engine_fit(plain.cpu().numpy())
    table, res = sw.run_sweep(spec, gpu_engine, chunk=16, log=lambda s: None, reuse=reuse, fit=fit)
    assert torch.equal(table, plain)
    ref = host_result(fit, fit.resolve(spec), table.cpu().numpy())
    assert ref["n_within"][0] <= ref["n_within"][1] and ref["n_valid"] == 60 and ref["best"]["index"] >= 0
    assert F.differences(res, ref) == []
    none, only = sw.run_sweep(spec, gpu_engine, chunk=16, log=lambda s: None, reuse=reuse, fit=fit, keep_table=False)
    assert none is None and F.differences(only, ref) == []
    # the best point evaluated again through the sweep's compute function is the table's row
    compute = sw.make_compute(spec, gpu_engine, reuse=reuse)
    mk = lambda n: torch.empty((n, 6), dtype=torch.float64, device=gpu_engine.device)
    again = F.best_point_yields(compute, res["best"]["index"], mk, gpu_engine)
    assert np.array_equal(again.view(np.int64), table[res["best"]["index"]].cpu().numpy().view(np.int64))


# ---- the CLI as child processes ----------------------------------------------------------------
def run(cmd, timeout=300, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, (cmd, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """One plain run, one --fit run, one --fit --no-table run, one two-rank gloo --fit run and one
    one-rank RCCL --fit run (the device-side all-gather and merge of the states) of the same small spec."""
    d = tmp_path_factory.mktemp("fitcli")
    spec = engine_spec()
    with open(d / "spec.json", "w") as f:
        json.dump(spec.to_json(), f)
    base = [sys.executable, "-m", PKG_NAME + ".sweep", "--spec", str(d / "spec.json"), "--chunk", "16"]
    run(base + ["--out", str(d / "plain")])
    fit = engine_fit(np.load(d / "plain" / "table.npy"))
    with open(d / "fit.json", "w") as f:
        json.dump(fit.to_json(), f)
    run(base + ["--out", str(d / "fit"), "--fit", str(d / "fit.json")])
    run(base + ["--out", str(d / "only"), "--fit", str(d / "fit.json"), "--no-table"])
    torchrun = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "2",
                "--master-addr", "127.0.0.1", "--master-port", str(free_port())]
    run(torchrun + base[1:] + ["--out", str(d / "two"), "--fit", str(d / "fit.json"), "--dist-backend", "gloo"])
    torchrun[torchrun.index("--nproc-per-node") + 1], torchrun[-1] = "1", str(free_port())
    run(torchrun + base[1:] + ["--out", str(d / "rccl"), "--fit", str(d / "fit.json"), "--dist-backend", "nccl"])
    return d, spec, fit


def load_fit_files(path):
    with open(path / "fit.json") as f:
        rep = json.load(f)
    return rep, dict(np.load(path / "fit_maps.npz")), np.load(path / "selected.npy")


def test_cli_fit_files(cli_runs):
    d, spec, fit = cli_runs
    table = np.load(d / "fit" / "table.npy")
    assert np.array_equal(table, np.load(d / "plain" / "table.npy"))
    ref = host_result(fit, fit.resolve(spec), table)
    rep, maps, sel = load_fit_files(d / "fit")
    assert rep["spec"] == fit.to_json() and rep["n_points"] == 60
    assert (rep["n_valid"], rep["n_invalid"], rep["n_within"]) == (ref["n_valid"], ref["n_invalid"], ref["n_within"])
    assert rep["columns"] == ref["columns"] and rep["n_selected"] == ref["n_selected"]
    best = rep["best"]
    assert best["index"] == ref["best"]["index"] and best["chi2"] == ref["best"]["chi2"]
    assert best["params"] == spec.point_params(best["index"])
    assert [best["final"][k] for k in FIELDS] == table[best["index"]].tolist()       # bitwise: floats round-trip
    assert sel.dtype == np.int64 and np.array_equal(sel, ref["selected"])
    for k, m in enumerate(ref["maps"]):
        assert maps[f"map{k}_chi2_min"].shape == m["chi2_min"].shape == tuple(rep["maps"][k]["shape"])
        assert np.array_equal(maps[f"map{k}_chi2_min"].view(np.int64), m["chi2_min"].view(np.int64))
        assert np.array_equal(maps[f"map{k}_argmin"], m["argmin"]) and maps[f"map{k}_argmin"].dtype == np.int64
    with open(d / "fit" / "summary.json") as f:
        summ = json.load(f)
    assert summ["fit"] == rep and "closest_to_planck_ratio" in summ
    # fit only: the same fit, no table, no checkpoints; the column extrema stand in for the statistics
    rep2, maps2, sel2 = load_fit_files(d / "only")
    assert rep2 == rep and np.array_equal(sel2, sel)
    assert all(np.array_equal(maps2[k].view(np.int64), maps[k].view(np.int64)) for k in maps)
    names = set(os.listdir(d / "only"))
    assert names == {"manifest.json", "summary.json", "fit.json", "fit_maps.npz", "selected.npy"}
    with open(d / "only" / "summary.json") as f:
        s2 = json.load(f)
    assert s2["fit"] == rep and s2["final"] == rep["columns"] and s2["n_points"] == 60
    for k in FIELDS:   # the same extrema summarize reduces on the host
        assert (summ["final"][k]["min"], summ["final"][k]["max"], summ["final"][k]["n_nonfinite"]) == \
            (s2["final"][k]["min"], s2["final"][k]["max"], s2["final"][k]["n_nonfinite"])


def test_cli_without_fit_is_unchanged(cli_runs):
    d, _, _ = cli_runs
    names = set(os.listdir(d / "plain"))
    assert {n for n in names if not n.startswith("shard_")} == {"manifest.json", "summary.json", "table.npy"}
    assert len([n for n in names if n.startswith("shard_")]) == 4
    with open(d / "plain" / "summary.json") as f:
        assert set(json.load(f)) == {"spec", "n_points", "fields", "final", "closest_to_planck_ratio", "elapsed_s",
                                     "points_per_s", "n_gpus", "spec_def"}


def test_cli_two_gloo_ranks_same_fit(cli_runs):
    d, _, _ = cli_runs
    rep, maps, sel = load_fit_files(d / "fit")
    rep2, maps2, sel2 = load_fit_files(d / "two")
    assert rep2 == rep and np.array_equal(sel2, sel)
    assert all(np.array_equal(maps2[k].view(np.int64), maps[k].view(np.int64)) for k in maps)
    assert np.array_equal(np.load(d / "two" / "table.npy"), np.load(d / "fit" / "table.npy"))


def test_cli_rccl_one_rank_same_fit(cli_runs):
    d, _, _ = cli_runs
    rep, maps, sel = load_fit_files(d / "fit")
    rep2, maps2, sel2 = load_fit_files(d / "rccl")
    assert rep2 == rep and np.array_equal(sel2, sel)
    assert all(np.array_equal(maps2[k].view(np.int64), maps[k].view(np.int64)) for k in maps)


def test_cli_refuses_no_table_resume(cli_runs, tmp_path):
    d, _, _ = cli_runs
    base = [sys.executable, "-m", PKG_NAME + ".sweep", "--spec", str(d / "spec.json"), "--out", str(tmp_path / "x")]
    r = run(base + ["--fit", str(d / "fit.json"), "--no-table", "--resume"], ok=False)
    assert "--no-table --resume" in r.stderr
    r = run(base + ["--no-table"], ok=False)
    assert "--no-table needs --fit" in r.stderr
