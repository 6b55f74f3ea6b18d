"""Sweep posteriors on the device (lzq_post_*, csrc/lzq_post.hip) against the numpy implementation
(fit.HostPosterior, itself pinned to literal values by tests/test_post_host.py): the device state
equals the host's words exactly for every row count around the wave and block sizes, every chunking,
every map shape and both map paths (block-private LDS, straight to global memory), an unaligned
record base, 64-bit flat indices and merges; then the real engine through run_sweep and the sweep
CLI as child processes (one rank, two gloo ranks on the one GPU, one RCCL rank)."""
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
PAIRS = ((3, 35), (60, 76), (250, 266))


def post_table(n, seed, coarse=False):
    """Records in the style of the fit tests' tables (wide magnitudes, or quarter integers), column
    0 redrawn as 1 + sqrt(s) / 2 with s uniform in [0, 200): under the single term (target 1, sigma
    0.5) chi2 ~ s.  Planted NaN / inf / overflowing rows, and pairs of identical rows inside a wave
    (3, 35), across a wave boundary (60, 76) and across a block boundary (250, 266)."""
    rng = np.random.default_rng(seed)
    if coarse:
        t = rng.integers(-6, 7, (n, 6)).astype(np.float64) / 4.0
    else:
        t = rng.choice([-1.0, 1.0], (n, 6)) * 10.0 ** rng.uniform(-300, 300, (n, 6))
    t[:, 0] = 1.0 + 0.5 * np.sqrt(rng.uniform(0.0, 200.0, n))
    for k, (a, b) in enumerate(PAIRS):
        for r in (a, b):
            if r < n:
                t[r] = 0.0
                t[r, 0] = 1.0 + 0.5 * np.sqrt(51.0 + k)
    if n > 8:
        free = np.arange(n)[np.isin(np.arange(n), np.ravel(PAIRS), invert=True)]
        bad = rng.choice(free, max(3, n // 40), replace=False)
        t[bad[0::3], 0] = NAN
        t[bad[1::3], 0] = INF
        t[bad[2::3], 0] = 1e300      # (x - 1) / 0.5 squared overflows
    return t


def make_fit(levels=(20.0, 60.0, 70.0, 1e6)):
    return F.FitSpec.from_json({"terms": [{"field": "Y_B", "target": 1.0, "sigma": 0.5}], "levels": list(levels),
                                "posterior": {}})


def fmap(*axes):
    """A map from (stride, len) pairs."""
    return F.FitMap(tuple(f"a{k}" for k in range(len(axes))), tuple(a[0] for a in axes), tuple(a[1] for a in axes))


def host_words(fit, maps, offset, table, start=0):
    h = F.HostPosterior(fit, maps, offset)
    h.update(table, start)
    return h.to_words()


def to_device(eng, table, unaligned=False):
    n = table.shape[0]
    if not unaligned:
        return torch.from_numpy(table).to(eng.device)
    buf = torch.empty(n * 6 + 1, dtype=torch.float64, device=eng.device)   # an 8-byte, not 16-byte aligned base
    d = buf[1:].view(n, 6)
    d.copy_(torch.from_numpy(table))
    assert d.data_ptr() % 16 == 8
    return d


def device_words(eng, fit, maps, offset, table, start=0, chunk=None, unaligned=False):
    d = to_device(eng, table, unaligned)
    n = table.shape[0]
    st = eng.post_state(fit, maps, offset)
    for a in range(0, n, chunk or max(n, 1)):
        eng.post_update(st, d[a:min(n, a + (chunk or n))], start + a)
    assert st.rows == n
    return st.words.cpu().numpy()


def classes(words):
    return [int(x) for x in words[:4]]      # used, zero, above, invalid


def same(got, ref):
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, f"{bad.size} words differ, the first at {bad[:8].tolist()}"


SIZES = [1, 63, 64, 65, 255, 257, 1000, 70_001]
# 16 + 80 cells are block-private in LDS; with them the 1000-cell map no longer fits the 1024 cells
# of a block and goes straight to global memory; alone it is block-private too
SMALL_MAPS = [fmap((1, 16)), fmap((64, 5), (1, 16)), fmap((4096, 1000))]
OFFSETS = (0.0, 50.0)


@pytest.fixture(scope="module")
def tables():
    return {n: post_table(n, 11 + n) for n in SIZES + [140_000]}


@pytest.fixture(scope="module")
def refs(tables):
    """HostPosterior's words of the 70,001-row table with SMALL_MAPS at start 5, per offset."""
    return {off: host_words(make_fit(), SMALL_MAPS, off, tables[70_001], 5) for off in OFFSETS}


def test_the_reference_has_every_class(refs):
    n = 70_001
    used, zero, above, invalid = classes(refs[0.0])
    assert above == 0 and abs(used / n - 0.43 * 0.975) < 0.02 and zero > 0.5 * n and invalid == n // 40
    used, zero, above, invalid = classes(refs[50.0])
    assert abs(above / n - 0.25 * 0.975) < 0.02 and used > 0.3 * n and zero > 0.2 * n and invalid == n // 40
    for off in OFFSETS:
        assert sum(classes(refs[off])) == n and int(refs[off][F.PW_Z]) > 0


@pytest.mark.parametrize("n", SIZES)
def test_row_counts(gpu_engine, tables, refs, n):
    fit, t = make_fit(), tables[n]
    for off in OFFSETS:
        ref = refs[off] if n == 70_001 else host_words(fit, SMALL_MAPS, off, t, 5)
        if n >= 1000:
            assert all(c > 0 for c in classes(ref)) == (off > 0) and classes(ref)[0] > 0 and classes(ref)[3] > 0
        same(device_words(gpu_engine, fit, SMALL_MAPS, off, t, 5), ref)
        same(device_words(gpu_engine, fit, SMALL_MAPS, off, t, 5, unaligned=True), ref)
    if n > 266:     # the planted pairs: identical rows, both weighted at both offsets
        q = F.post_weights(fit, 50.0, t[np.ravel(PAIRS)])
        assert q[0] == q[1] and q[2] == q[3] and q[4] == q[5] and q[0] > q[2] > q[4] > 0


def test_grid_stride_walk(gpu_engine, tables):
    """140,000 rows, more than one launch has threads (512 blocks of 256): a thread walks a second
    row, advancing its cell indices by carries."""
    fit, t = make_fit(), tables[140_000]
    maps = SMALL_MAPS + [fmap((7, 3), (100_003, 1 << 20))]
    start = (1 << 32) - 70_000
    for off in OFFSETS:
        ref = host_words(fit, maps, off, t, start)
        assert classes(ref)[0] > 40_000
        same(device_words(gpu_engine, fit, maps, off, t, start), ref)


@pytest.mark.parametrize("chunk", [1, 64, 1000, 4097])
def test_chunking_is_invisible(gpu_engine, tables, refs, chunk):
    n = 1000 if chunk == 1 else 70_001
    t = tables[n]
    for off in OFFSETS if chunk != 1 else (50.0,):
        ref = refs[off] if n == 70_001 else host_words(make_fit(), SMALL_MAPS, off, t, 5)
        same(device_words(gpu_engine, make_fit(), SMALL_MAPS, off, t, 5, chunk), ref)


def test_map_shapes_and_paths(gpu_engine, tables):
    """Each map alone and all together, no map at all, a 300 x 300 map that only global memory
    holds, and coarse records (exact ties in chi2: whole runs of rows in one histogram bin)."""
    fit = make_fit()
    t = tables[70_001]
    big, rev = fmap((300, 300), (1, 300)), fmap((1, 300), (300, 300))
    for maps in ([], [SMALL_MAPS[0]], [SMALL_MAPS[1]], [SMALL_MAPS[2]], SMALL_MAPS[:2], [big, SMALL_MAPS[0], rev, SMALL_MAPS[2]]):
        ref = host_words(fit, maps, 50.0, t, 0)
        got = device_words(gpu_engine, fit, maps, 50.0, t, 0, chunk=33_333)
        same(got, ref)
        assert got.size == 32 + 4096 + 2 * sum(m.cells for m in maps)
    # every map's cells sum to Z, and the transposed map is the transpose
    res = F.HostPosterior.from_words(fit, [big, SMALL_MAPS[0], rev, SMALL_MAPS[2]], 50.0, got).result()
    Z = int(res["Z_units"])
    total = lambda p: (int(p[:, 0].sum()) << 31) + int(p[:, 1].sum())
    assert Z > 0 and all(total(m["weight"]) == Z for m in res["maps"]) and total(res["hist"]) == Z
    assert np.array_equal(res["maps"][2]["weight"].reshape(300, 300, 2),
                          res["maps"][0]["weight"].reshape(300, 300, 2).transpose(1, 0, 2))
    c = post_table(5000, 3, coarse=True)
    c[:, 0] = 1.0 + np.round(c[:, 1] * 2.0) / 2.0       # chi2 in {0, 1, 4, 9}: whole runs of rows in one bin
    levels = (0.0, 1.0, 4.0, 9.0)
    for off in (0.0, 4.0):
        ref = host_words(make_fit(levels), SMALL_MAPS, off, c, 7)
        assert classes(ref)[0] > 1000 and (classes(ref)[2] > 0) == (off > 0)
        same(device_words(gpu_engine, make_fit(levels), SMALL_MAPS, off, c, 7, chunk=999), ref)


def test_int64_flat_indices(gpu_engine, tables):
    """start = 2^40 + 3 on virtual axes of 70,001 x 70,001 x 300 points (the middle axis mapped modulo 1000)."""
    L = 70_001
    start = (1 << 40) + 3
    t = tables[1000]
    maps = [fmap((300 * L, L)), fmap((300, 1000), (1, 300)), fmap((1, 300))]
    ref = host_words(make_fit(), maps, 50.0, t, start)
    res = F.HostPosterior.from_words(make_fit(), maps, 50.0, ref).result()
    assert set(np.flatnonzero(res["maps"][0]["weight"].any(axis=1))) == {start // (300 * L) % L}
    same(device_words(gpu_engine, make_fit(), maps, 50.0, t, start, chunk=64), ref)


def test_merge_of_disjoint_ranges(gpu_engine, tables, refs):
    eng, t, fit = gpu_engine, tables[70_001], make_fit()
    d = torch.from_numpy(t).to(eng.device)
    tot = eng.post_state(fit, SMALL_MAPS, 50.0)
    for a, b in ((40_000, 70_001), (0, 1), (1, 40_000)):
        st = eng.post_state(fit, SMALL_MAPS, 50.0)
        eng.post_update(st, d[a:b], 5 + a)
        eng.post_merge(tot, st.words)
    same(tot.words.cpu().numpy(), refs[50.0])
    assert tot.rows == 70_001
    res = eng.post_result(tot)
    assert F.post_differences(res, F.HostPosterior.from_words(fit, SMALL_MAPS, 50.0, refs[50.0]).result()) == []
    tot.rows = (1 << 32) - 10
    with pytest.raises(ValueError, match="2\\^32 rows"):
        eng.post_update(tot, d[:11], 0)
    with pytest.raises(ValueError, match="finite"):
        eng.post_state(fit, SMALL_MAPS, -1.0)


# ---- the real engine ---------------------------------------------------------------------------
def engine_spec():
    sw = pkg("sweep")
    return sw.SweepSpec("grid60", full_cfg(BASE_CFG), [("m_chi_GeV", np.logspace(0, 3.5, 5)),
                                                       ("I_p", np.linspace(0.05, 1, 3)),
                                                       ("delta_LZ", np.logspace(-4, 0, 4))])


def engine_fit(table, offset):
    """Targets inside the 60-point table's own range; sigmas small enough that the weights spread
    over many histogram bins."""
    yb, dm = np.median(table[:, 0]), np.median(table[:, 4])
    d = {"terms": [{"field": "Y_B", "target": float(yb), "sigma": float(abs(yb)) / 4},
                   {"field": "DM_over_B", "target": float(dm), "sigma": float(abs(dm)) / 4}],
         "levels": [0.5, 8.0], "maps": [["m_chi_GeV", "I_p"], ["delta_LZ"], ["delta_LZ", "m_chi_GeV"]],
         "select": {"level": 2.0, "cap": 20}}
    if offset is not None:
        d["posterior"] = {"offset": offset, "credible": [0.5, 0.9]}
    return F.FitSpec.from_json(d)


def host_posterior(fit, spec, table):
    """The posterior the host computes from the plain table."""
    maps = fit.resolve(spec)
    off = fit.posterior["offset"]
    if off == "best":
        h = F.HostFit(fit, maps)
        h.update(table, 0)
        off = h.result()["best"]["chi2"]
    p = F.HostPosterior(fit, maps, off, fit.axis_values(spec))
    p.update(table, 0)
    return p.result()


@pytest.mark.parametrize("offset", [0.125, "best"])
def test_run_sweep_with_posterior_on_the_engine(gpu_engine, offset):
    sw = pkg("sweep")
    spec = engine_spec()
    plain = sw.run_sweep(spec, gpu_engine, chunk=16, log=lambda s: None)
    fit = engine_fit(plain.cpu().numpy(), offset)
    ref = host_posterior(fit, spec, plain.cpu().numpy())
    assert ref["n_used"] > 5 and ref["n_used"] + ref["n_zero"] + ref["n_above"] + ref["n_invalid"] == 60
    table, res = sw.run_sweep(spec, gpu_engine, chunk=16, log=lambda s: None, fit=fit)
    assert torch.equal(table, plain) and F.post_differences(res["posterior"], ref) == []
    assert res["posterior"]["maps"][1]["mean"] is not None
    if offset == "best":
        assert ref["n_above"] == 0 and ref["offset"] == res["best"]["chi2"]
        with pytest.raises(ValueError, match="give a number"):
            sw.run_sweep(spec, gpu_engine, chunk=16, log=lambda s: None, fit=fit, keep_table=False)
    else:
        none, only = sw.run_sweep(spec, gpu_engine, chunk=16, log=lambda s: None, fit=fit, keep_table=False)
        assert none is None and F.post_differences(only["posterior"], ref) == []


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
    """One plain run; then with a numeric offset a table run, a --no-table run, a two-rank gloo run
    and a one-rank RCCL run; with "best" a table run and a two-rank gloo run; and a run of the
    same fit without the key."""
    d = tmp_path_factory.mktemp("postcli")
    spec = engine_spec()
    with open(d / "spec.json", "w") as f:
        json.dump(spec.to_json(), f)
    base = [sys.executable, "-m", PKG_NAME + ".sweep", "--spec", str(d / "spec.json"), "--chunk", "16"]
    run(base + ["--out", str(d / "plain")])
    table = np.load(d / "plain" / "table.npy")
    fits = {"num": engine_fit(table, 0.125), "best": engine_fit(table, "best"), "nokey": engine_fit(table, None)}
    for k, fit in fits.items():
        with open(d / f"{k}.json", "w") as f:
            json.dump(fit.to_json(), f)
    torchrun = lambda nproc: [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node",
                              str(nproc), "--master-addr", "127.0.0.1", "--master-port", str(free_port())]
    run(base + ["--out", str(d / "num"), "--fit", str(d / "num.json")])
    run(base + ["--out", str(d / "num_only"), "--fit", str(d / "num.json"), "--no-table"])
    run(torchrun(2) + base[1:] + ["--out", str(d / "num_two"), "--fit", str(d / "num.json"), "--dist-backend", "gloo"])
    run(torchrun(1) + base[1:] + ["--out", str(d / "num_rccl"), "--fit", str(d / "num.json"), "--dist-backend", "nccl"])
    run(base + ["--out", str(d / "best"), "--fit", str(d / "best.json")])
    run(torchrun(2) + base[1:] + ["--out", str(d / "best_two"), "--fit", str(d / "best.json"), "--dist-backend", "gloo"])
    run(base + ["--out", str(d / "nokey"), "--fit", str(d / "nokey.json")])
    return d, spec, fits, table


def load_fit_files(path):
    with open(path / "fit.json") as f:
        rep = json.load(f)
    return rep, dict(np.load(path / "fit_maps.npz"))


@pytest.mark.parametrize("name", ["num", "num_only", "num_two", "num_rccl", "best", "best_two"])
def test_cli_posterior_files(cli_runs, name):
    d, spec, fits, table = cli_runs
    fit = fits[name.split("_")[0]]
    ref = host_posterior(fit, spec, table)
    assert ref["n_used"] > 5 and (name[:4] != "best" or ref["n_above"] == 0)
    rep, maps = load_fit_files(d / name)
    assert rep["spec"] == fit.to_json() and rep["spec"]["posterior"]["credible"] == [0.5, 0.9]
    want = {**{k: ref[k] for k in ("offset", "n_used", "n_zero", "n_above", "n_invalid", "Z", "Z_units", "mass_within",
                                   "credible")},
            "maps": [{"axes": m["axes"], "mean": m["mean"], "std": m["std"]} for m in ref["maps"]]}
    assert rep["posterior"] == want                 # floats round-trip through JSON bit for bit
    assert set(maps) == {f"map{k}_{s}" for k in range(3) for s in ("chi2_min", "argmin", "posterior", "weight")}
    for k, m in enumerate(ref["maps"]):
        assert maps[f"map{k}_weight"].dtype == np.uint64 and np.array_equal(maps[f"map{k}_weight"], m["weight"])
        assert maps[f"map{k}_weight"].shape == (m["posterior"].size, 2)
        assert maps[f"map{k}_posterior"].shape == m["posterior"].shape
        assert np.array_equal(maps[f"map{k}_posterior"].view(np.int64), m["posterior"].view(np.int64))
    with open(d / name / "summary.json") as f:
        assert json.load(f)["fit"] == rep


def test_cli_without_the_key_is_unchanged(cli_runs):
    """The same fit without the key: fit.json and the arrays are what HostFit alone gives."""
    d, spec, fits, table = cli_runs
    fit = fits["nokey"]
    assert "posterior" not in fit.to_json()
    h = F.HostFit(fit, fit.resolve(spec))
    h.update(table, 0)
    res = h.result()
    rep, maps = load_fit_files(d / "nokey")
    want = F.report(fit, res, spec, 60, table[res["best"]["index"]])
    assert rep == json.loads(json.dumps(want)) and "posterior" not in rep
    assert set(maps) == {f"map{k}_{s}" for k in range(3) for s in ("chi2_min", "argmin")}
    assert set(os.listdir(d / "nokey")) - {n for n in os.listdir(d / "nokey") if n.startswith("shard_")} == \
        {"manifest.json", "summary.json", "table.npy", "fit.json", "fit_maps.npz", "selected.npy"}
    # and with the key, the fit's own part of the report is the same
    with_key, _ = load_fit_files(d / "num")
    assert {k: v for k, v in with_key.items() if k not in ("spec", "posterior")} == \
        {k: v for k, v in rep.items() if k != "spec"}


def test_cli_refuses_no_table_with_best(cli_runs, tmp_path):
    d, _, _, _ = cli_runs
    base = [sys.executable, "-m", PKG_NAME + ".sweep", "--spec", str(d / "spec.json"), "--out", str(tmp_path / "x")]
    r = run(base + ["--fit", str(d / "best.json"), "--no-table"], ok=False)
    assert "--no-table" in r.stderr and "give a number" in r.stderr
    assert not (tmp_path / "x").exists()
