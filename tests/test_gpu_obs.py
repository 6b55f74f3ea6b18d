"""Sweep observables on the device (lzq_obs_*, csrc/lzq_obs.hip) against the numpy implementation
(fit.HostObservables, itself pinned to literal values by tests/test_obs_host.py): whole device
states equal the host's words exactly -- for the special values, past one full grid of threads and
in every chunking, from an unaligned record base, on both sides of the block-private limit and on
the global-memory path, with a whole wave in one cell and with lanes alternating between two, and
after merges; then the sweep CLI with the key, with --no-table and without the key."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import pkg
from obs_tables import SALTED_OBS, TERM, lin, log, salted_table

pytestmark = pytest.mark.gpu

F = pkg("fit")
LDS = F.OBS_LDS_CELLS
OFFSETS = (None, 40.0)          # unweighted; weighted with rows above, with weight and with none
FULL_GRID = 512 * 256


def make_fit(*axes_lists):
    return F.FitSpec.from_json({"terms": [TERM], "observables": [{"axes": list(a)} for a in axes_lists]})


def host_words(fit, offset, table):
    h = F.HostObservables(fit, fit.observables, offset)
    h.update(table)
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


def device_words(eng, fit, offset, table, chunk=None, order=1, unaligned=False):
    d = to_device(eng, table, unaligned)
    n = table.shape[0]
    st = eng.obs_state(fit, fit.observables, offset)
    assert st.words.numel() == F.obs_state_words(fit.observables)
    for a in list(range(0, n, chunk or max(n, 1)))[::order]:
        eng.obs_update(st, d[a:min(n, a + (chunk or n))])
    assert st.rows == n
    return st.words.cpu().numpy()


def same(got, ref):
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, f"{bad.size} words differ, the first at {bad[:8].tolist()}"


@pytest.fixture(scope="module")
def big():
    """One row more than a full grid of threads and a ragged tail, with the host's words per offset."""
    t = salted_table(FULL_GRID + 300, 9)
    fit = make_fit(*SALTED_OBS)
    return t, fit, {off: host_words(fit, off, t) for off in OFFSETS}


def test_an_empty_state(gpu_engine):
    fit = make_fit(*SALTED_OBS)
    for off in OFFSETS:
        same(gpu_engine.obs_state(fit, fit.observables, off).words.cpu().numpy(),
             F.HostObservables(fit, fit.observables, off).to_words())


@pytest.mark.parametrize("offset", OFFSETS)
def test_special_values(gpu_engine, offset):
    """The salted table of the host tests: range ends and the values just below them, zeros of both
    signs, subnormals, non-finite values, invalid rows; two observables block-private, one in global
    memory, one two-dimensional."""
    t = salted_table()
    fit = make_fit(*SALTED_OBS)
    ref = host_words(fit, offset, t)
    res = F.HostObservables.from_words(fit, fit.observables, offset, ref).result()
    for r in res:
        assert r["n_in"] > 500 and r["n_out"] > 100 and r["n_nonfinite"] > 100
        assert (int(r["total_units"]) > 0) == (offset is not None)
    same(device_words(gpu_engine, fit, offset, t), ref)
    assert F.obs_differences(gpu_engine.obs_result(gpu_engine.obs_state(fit, fit.observables, offset)),
                             F.HostObservables(fit, fit.observables, offset).result()) == []


@pytest.mark.parametrize("how", ["whole", "chunks", "reversed"])
def test_past_a_full_grid_and_chunking(gpu_engine, big, how):
    """131,072 + 300 rows: some threads walk a second row and the last block is ragged; whole, in
    chunks of 4,099 rows, and with the chunks in reversed order."""
    t, fit, refs = big
    chunk, order = {"whole": (None, 1), "chunks": (4099, 1), "reversed": (4099, -1)}[how]
    for off in OFFSETS:
        assert int(refs[off][0]) > 30_000
        same(device_words(gpu_engine, fit, off, t, chunk, order), refs[off])


def test_unaligned_base(gpu_engine, big):
    t, fit, _ = big
    t = t[:70_001]
    for off in OFFSETS:
        same(device_words(gpu_engine, fit, off, t, unaligned=True), host_words(fit, off, t))


@pytest.mark.parametrize("shapes", [[LDS], [LDS + 1], [1000, LDS - 1000], [1000, LDS - 999], [LDS - 999, 1000, 7],
                                    [(256, 256), 16]])
def test_block_private_limit_and_global_path(gpu_engine, big, shapes):
    """Observables of LZQ_OBS_LDS_CELLS cells in all stay block-private; with one cell more the one
    that no longer fits goes straight to global memory (and a later, smaller one may still fit); a
    256 x 256 observable on the global path next to a small block-private one."""
    t = big[0][:40_000]
    fields = ("DM_over_B", "Y_chi", "rho_B_kg_m3")
    ranges = {"DM_over_B": (0.0, 10.0), "Y_chi": (0.0, 2e-10), "rho_B_kg_m3": (-1e3, 1e3)}
    axes = []
    for k, s in enumerate(shapes):
        if isinstance(s, tuple):
            axes.append([lin("Y_chi", 0.0, 2e-10, s[0]), lin("DM_over_B", 0.0, 10.0, s[1])])
        else:
            axes.append([lin(fields[k], *ranges[fields[k]], s)])
    fit = make_fit(*axes)
    assert [o.cells for o in fit.observables] == [s[0] * s[1] if isinstance(s, tuple) else s for s in shapes]
    for off in OFFSETS:
        ref = host_words(fit, off, t)
        res = F.HostObservables.from_words(fit, fit.observables, off, ref).result()
        assert all((r["count"] > 0).sum() > min(0.3 * r["count"].size, 2000) for r in res)   # the cells are really used
        same(device_words(gpu_engine, fit, off, t, chunk=15_000), ref)


def test_one_cell_for_a_whole_wave_and_two_alternating(gpu_engine):
    """Every row identical: each wave combines into one atomic per word.  Then two cells alternating
    lane by lane, in runs of 64 and of 100 rows: waves with one destination and with two."""
    fit = make_fit([log("DM_over_B", 0.01, 1000.0, 8)], [lin("Y_chi", 0.0, 2e-10, 200), lin("DM_over_B", 0.0, 10.0, 100)])
    n = 5000
    t = np.ones((n, 6))
    t[:, 0], t[:, 1], t[:, 4] = 2.0, 1e-10, 5.357
    alt = t.copy()
    alt[1::2, 4], alt[1::2, 0] = 7.5, 2.5
    runs = t.copy()
    runs[(np.arange(n) // 64) % 2 == 1, 4] = 7.5
    runs100 = t.copy()
    runs100[(np.arange(n) // 100) % 2 == 1, 4] = 7.5
    runs100[::7, 0] = 1.0 + 0.5 * np.sqrt(np.arange(n)[::7] % 90)      # chi2 varies inside a cell
    for table in (t, alt, runs, runs100):
        for off in (None, 0.0, 4.0):
            ref = host_words(fit, off, table)
            got = device_words(gpu_engine, fit, off, table)
            same(got, ref)
            assert int(got[0]) == n and int(got[1]) == 0
    res = F.HostObservables.from_words(fit, fit.observables, 4.0, host_words(fit, 4.0, t)).result()
    assert (res[0]["count"] > 0).sum() == 1 and res[0]["count"].max() == n and res[0]["total_units"] == str(n << 62)


def test_merge_of_disjoint_ranges(gpu_engine, big):
    eng = gpu_engine
    t, fit, refs = big
    d = torch.from_numpy(t).to(eng.device)
    n = t.shape[0]
    for off in OFFSETS:
        tot = eng.obs_state(fit, fit.observables, off)
        for a, b in ((90_000, n), (0, 90_000)):
            st = eng.obs_state(fit, fit.observables, off)
            eng.obs_update(st, d[a:b])
            eng.obs_merge(tot, st.words)
        same(tot.words.cpu().numpy(), refs[off])
        valid = int(np.isfinite(F.chi2_rows(fit, t)).sum())
        assert tot.rows == valid       # a merged state is counted by the valid rows its words hold
        ref = F.HostObservables.from_words(fit, fit.observables, off, refs[off]).result()
        assert F.obs_differences(eng.obs_result(tot), ref) == []
    with pytest.raises(ValueError, match="layouts"):
        eng.obs_merge(tot, tot.words[:-1])


def test_row_limit_raises_on_the_host(gpu_engine, big):
    t, fit, _ = big
    d = torch.from_numpy(t[:11]).to(gpu_engine.device)
    st = gpu_engine.obs_state(fit, fit.observables, 0.0)
    before = st.words.clone()
    st.rows = (1 << 32) - 10
    with pytest.raises(ValueError, match="2\\^32 rows"):
        gpu_engine.obs_update(st, d)
    other = gpu_engine.obs_state(fit, fit.observables, 0.0)
    with pytest.raises(ValueError, match="2\\^32 rows"):
        gpu_engine.obs_merge(st, other.words, rows=11)
    assert torch.equal(st.words, before)        # nothing was launched
    with pytest.raises(ValueError, match="finite"):
        gpu_engine.obs_state(fit, fit.observables, -1.0)


# ---- the sweep CLI ---------------------------------------------------------------------------------
CLI = ["--spec", "C4", "--limit", "3000", "--chunk", "1024", "--reuse-zsums"]
TODAY = {"manifest.json", "summary.json", "table.npy", "fit.json", "fit_maps.npz", "selected.npy"}


def files(path):
    return {n for n in os.listdir(path) if not n.startswith("shard_")}


@pytest.fixture(scope="module")
def cli_runs(gpu_engine, tmp_path_factory):
    """A fit without the key (its table gives targets inside the slice's own range), then the same
    fit with observables and a numeric offset: with the table and with --no-table."""
    sw = pkg("sweep")
    d = tmp_path_factory.mktemp("obscli")
    plain = {"terms": [{"field": "Y_B", "target": 8.72e-11, "sigma": 8.72e-13}], "levels": [2.3], "maps": [["I_p"]]}
    with open(d / "plain.json", "w") as f:
        json.dump(plain, f)
    sw.main(CLI + ["--out", str(d / "plain"), "--fit", str(d / "plain.json")])
    table = np.load(d / "plain" / "table.npy")
    yb, dm = table[:, 0], table[:, 4]
    fin = np.isfinite(yb) & np.isfinite(dm) & (yb > 0) & (dm > 0)
    assert fin.sum() > 1000
    mid = float(np.median(yb[fin]))
    spec = {"terms": [{"field": "Y_B", "target": mid, "sigma": mid / 4}], "levels": [2.3], "maps": [["I_p"]],
            "posterior": {"offset": 0.0},
            "observables": [{"axes": [log("DM_over_B", float(dm[fin].min()) * 1.5, float(dm[fin].max()) / 1.5, 8)]},
                            {"axes": [lin("Y_B", 0.0, 2.0 * mid, 50), log("DM_over_B", 1e-30, 1e30, 1)],
                             "quantiles": [0.16, 0.5, 0.84]}]}
    with open(d / "obs.json", "w") as f:
        json.dump(spec, f)
    sw.main(CLI + ["--out", str(d / "with"), "--fit", str(d / "obs.json")])
    sw.main(CLI + ["--out", str(d / "only"), "--fit", str(d / "obs.json"), "--no-table"])
    return d, F.FitSpec.from_json(spec), table


def test_cli_observables_with_and_without_the_table(cli_runs):
    d, fit, table = cli_runs
    assert np.array_equal(np.load(d / "with" / "table.npy"), table, equal_nan=True)
    reps, arrays = {}, {}
    for name in ("with", "only"):
        with open(d / name / "fit.json") as f:
            reps[name] = json.load(f)
        arrays[name] = dict(np.load(d / name / "fit_obs.npz"))
        with open(d / name / "summary.json") as f:
            assert json.load(f)["fit"]["observables"] == reps[name]["observables"]
    assert reps["with"]["observables"] == reps["only"]["observables"]
    assert set(arrays["with"]) == set(arrays["only"])
    for k, v in arrays["with"].items():
        assert v.dtype == arrays["only"][k].dtype and np.array_equal(v.view(np.uint64), arrays["only"][k].view(np.uint64)), k
    assert files(d / "with") == TODAY | {"fit_obs.npz"}
    assert files(d / "only") == (TODAY | {"fit_obs.npz"}) - {"table.npy"}
    # and both are what the host computes from the table
    post = F.HostPosterior(fit, fit.resolve(pkg("sweep").builtin_specs()["C4"]), 0.0)
    post.update(table, 0)
    h = F.HostObservables(fit, fit.observables, 0.0)
    h.update(table)
    ref = h.result(int(post.result()["Z_units"]))
    assert ref[0]["n_in"] > 500 and ref[0]["n_out"] > 0 and int(ref[0]["total_units"]) > 0 and ref[1]["n_in"] > 500
    assert ref[0]["quantiles"][2]["bin"] is not None and 0.0 < ref[0]["in_range_share"] <= 1.0
    want = json.loads(json.dumps(F.report(fit, {**_fit_result(fit, table), "observables": ref},
                                          pkg("sweep").builtin_specs()["C4"], 3000, None)["observables"]))
    assert reps["with"]["observables"] == want
    for k, o in enumerate(ref):
        assert np.array_equal(arrays["with"][f"obs{k}_weight"], o["weight"])
        assert np.array_equal(arrays["with"][f"obs{k}_count"], o["count"])
        assert np.array_equal(arrays["with"][f"obs{k}_chi2_min"].view(np.int64), o["chi2_min"].view(np.int64))
        assert np.array_equal(arrays["with"][f"obs{k}_posterior"].view(np.int64), o["posterior"].view(np.int64))
        for a, e in enumerate(o["edges"]):
            assert np.array_equal(arrays["with"][f"obs{k}_edges{a}"], e)


def _fit_result(fit, table):
    h = F.HostFit(fit, fit.resolve(pkg("sweep").builtin_specs()["C4"]))
    h.update(table, 0)
    return h.result()


def test_cli_without_the_key_lists_todays_files(cli_runs):
    d, _, _ = cli_runs
    assert files(d / "plain") == TODAY
    with open(d / "plain" / "fit.json") as f:
        rep = json.load(f)
    assert "observables" not in rep and "observables" not in rep["spec"]
