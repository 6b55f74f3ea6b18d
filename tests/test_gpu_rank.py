"""Ranked points on the device (lzq_rank_*, csrc/lzq_rank.hip) against the numpy implementation
(fit.HostRanked, itself pinned to literal values by tests/test_rank_host.py): whole device states
equal the host's words exactly -- for capacities around the wave size and the largest, for every
chunking in ascending and shuffled order, with exact ties inside a chunk, across a chunk boundary
and across the list's last entry, when every chunk replaces the whole list and when none adds a
row, with more keys than one block sorts at once (the radix select, through the index word), with
flat indices beyond 2^32 and next to 2^62, after merges in different orders and from a record base
that is only 8-byte aligned; then the real engine through run_sweep and the sweep CLI as child
processes (one rank, --no-table, two gloo ranks on the one GPU, one RCCL rank)."""
import itertools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import BASE_CFG, PKG_NAME, ROOT, full_cfg, pkg
from obs_tables import TERM, salted_table

pytestmark = pytest.mark.gpu

F = pkg("fit")
FIELDS = pkg("_native").YIELD_FIELDS
NAN = float("nan")
FIT = F.FitSpec.from_json({"terms": [TERM]})
ROWS = 3000
SORT_CAP = 4096                 # the keys one block sorts at once: more take the select first


def rank_table(n=ROWS, seed=21):
    """The salted table of the observable tests (chi2 spread over [0, 150), NaN / inf / overflowing
    rows planted) with every fourth row on a quarter integer: exact ties all through the ranking."""
    t = salted_table(n, seed)
    rng = np.random.default_rng(seed + 1)
    keep = np.isfinite(t[1::4, 0]) & (t[1::4, 0] < 1e299)
    t[1::4, 0] = np.where(keep, rng.integers(5, 30, keep.size) / 4.0, t[1::4, 0])
    return t


def host_words(n, table, start=0, fit=FIT):
    h = F.HostRanked(fit, n)
    h.update(table, start)
    return h.to_words()


def to_device(eng, table, unaligned=False):
    rows = table.shape[0]
    if not unaligned:
        return torch.from_numpy(table).to(eng.device)
    buf = torch.empty(rows * 6 + 1, dtype=torch.float64, device=eng.device)   # an 8-byte, not 16-byte aligned base
    d = buf[1:].view(rows, 6)
    d.copy_(torch.from_numpy(table))
    assert d.data_ptr() % 16 == 8
    return d


def feed(eng, st, d, bounds, start=0):
    for a, b in bounds:
        eng.rank_update(st, d[a:b], start + a)
    return st.words.cpu().numpy()


def chunks(rows, chunk):
    return [(a, min(rows, a + chunk)) for a in range(0, rows, chunk)]


def same(got, ref, what=None):
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, f"{what}: {bad.size} words differ, the first at {bad[:8].tolist()}"


@pytest.fixture(scope="module")
def salted(gpu_engine):
    t = rank_table()
    c = F.chi2_rows(FIT, t)
    assert 50 < (~np.isfinite(c)).sum() < 300 and np.unique(c[np.isfinite(c)]).size < np.isfinite(c).sum() - 300
    return t, to_device(gpu_engine, t)


def test_an_empty_state_and_an_empty_chunk(gpu_engine):
    for n in (1, 64, 4096):
        st = gpu_engine.rank_state(FIT, n)
        assert st.words.numel() == F.rank_state_words(n)
        ref = F.HostRanked(FIT, n)
        same(st.words.cpu().numpy(), ref.to_words(), n)
        gpu_engine.rank_update(st, torch.empty((0, 6), dtype=torch.float64, device=gpu_engine.device), 5)
        same(st.words.cpu().numpy(), ref.to_words(), n)
        assert F.rank_differences(gpu_engine.rank_result(st), ref.result()) == []


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4096])
def test_capacities_and_chunkings(gpu_engine, salted, n):
    """3000 salted rows whole and in chunks of 1, 7, 64, 65, 257 and 1000, in ascending and in
    shuffled order of `start`: one list."""
    t, d = salted
    ref = host_words(n, t, 11)
    r = F.HostRanked.from_words(FIT, n, ref).result()
    assert r["count"] == min(n, r["n_valid"]) and r["n_invalid"] > 50 and r["n_valid"] + r["n_invalid"] == ROWS
    for chunk in (ROWS, 1, 7, 64, 65, 257, 1000):
        bounds = chunks(ROWS, chunk)
        shuffled = [bounds[k] for k in np.random.default_rng(chunk).permutation(len(bounds))]
        for order in ((bounds,) if chunk == ROWS else (bounds, shuffled)):
            same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), d, order, 11), ref, (n, chunk))
    assert F.rank_differences(gpu_engine.rank_result(_fed(gpu_engine, n, d, 11)), r) == []


def _fed(eng, n, d, start=0):
    st = eng.rank_state(FIT, n)
    eng.rank_update(st, d, start)
    return st


@pytest.mark.parametrize("n", [1, 64, 4096])
def test_more_keys_than_one_block_sorts(gpu_engine, n):
    """A cold state takes every valid row of a chunk as a candidate: 6000 rows whole and in chunks
    of 4500 go through the select, 131,372 rows also through the grid-stride walk."""
    t = rank_table(6000, 22)
    d = to_device(gpu_engine, t)
    ref = host_words(n, t, 3)
    assert int(ref[2]) > SORT_CAP
    same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), d, [(0, 6000)], 3), ref, n)
    same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), d, [(1500, 6000), (0, 1500)], 3), ref, n)
    big = rank_table(512 * 256 + 300, 23)
    same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), to_device(gpu_engine, big), [(0, big.shape[0])], 3),
         host_words(n, big, 3), n)


def constant_rows(rows, yb=2.0):
    t = np.arange(rows * 6, dtype=np.float64).reshape(rows, 6)      # records tell the rows apart
    t[:, 0] = yb
    return t


@pytest.mark.parametrize("n", [1, 64, 4096])
def test_all_rows_tie(gpu_engine, n):
    """A constant field: the list is the n lowest indices, whichever chunk they arrive in.  Whole,
    5000 tied keys go through the select, which has to tell them apart by the index word."""
    rows = 5000
    t = constant_rows(rows)
    d = to_device(gpu_engine, t)
    ref = host_words(n, t, 9)
    r = F.HostRanked.from_words(FIT, n, ref).result()
    assert r["index"].tolist() == list(range(9, 9 + min(n, rows))) and set(r["chi2"].tolist()) == {4.0}
    same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), d, [(0, rows)], 9), ref, n)
    same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), d, chunks(rows, 1000)[::-1], 9), ref, n)
    same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), d, chunks(rows, 333)[::-1], 9), ref, n)


def test_ties_across_a_chunk_boundary_and_across_the_last_entry(gpu_engine):
    # 21 rows tie at the minimum across the boundary between two chunks of 1000; the list holds 10
    t = rank_table(2000, 24)
    t[990:1011, 0] = 1.0
    d = to_device(gpu_engine, t)
    for n in (10, 21, 30):
        ref = host_words(n, t)
        first = F.HostRanked.from_words(FIT, n, ref).result()["index"][:min(n, 21)]
        assert first.tolist() == list(range(990, 990 + min(n, 21)))
        for order in (1, -1):
            same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), d, chunks(2000, 1000)[::order]), ref, (n, order))
    # 59 better rows, then tied rows for the 5 free places: 50 of them (sorted in one go) and 6000
    # (selected first), arriving behind the better rows and ahead of them
    for tied in (50, 6000):
        t = constant_rows(59 + tied, 2.0)
        t[:59, 0] = 1.0 + np.arange(59) / 128.0
        d = to_device(gpu_engine, t)
        ref = host_words(64, t, 100)
        r = F.HostRanked.from_words(FIT, 64, ref).result()
        assert r["index"].tolist() == list(range(100, 164)) and r["chi2"][58:].tolist() == [0.8212890625] + [4.0] * 5
        same(feed(gpu_engine, gpu_engine.rank_state(FIT, 64), d, [(0, 59), (59, 59 + tied)], 100), ref, tied)
        same(feed(gpu_engine, gpu_engine.rank_state(FIT, 64), d, [(59, 59 + tied), (0, 59)], 100), ref, tied)
        swapped = np.concatenate([t[59:], t[:59]])                   # the better rows at the higher indices
        ref = host_words(64, swapped, 100)
        assert F.HostRanked.from_words(FIT, 64, ref).result()["index"][59:].tolist() == list(range(100, 105))
        ds = to_device(gpu_engine, swapped)
        same(feed(gpu_engine, gpu_engine.rank_state(FIT, 64), ds, [(0, tied), (tied, tied + 59)], 100), ref, tied)
        same(feed(gpu_engine, gpu_engine.rank_state(FIT, 64), ds, [(tied, tied + 59), (0, tied)], 100), ref, tied)


@pytest.mark.parametrize("n", [64, 256])
def test_every_chunk_replaces_the_list_and_no_chunk_adds_to_it(gpu_engine, salted, n):
    t, _ = salted
    c = F.chi2_rows(FIT, t)
    c = np.where(np.isfinite(c), c, -1.0)                           # the invalid rows first / last
    down = t[np.argsort(-c, kind="stable")]
    valid = int((c >= 0).sum())
    for table, name in ((down, "descending"), (down[::-1].copy(), "ascending")):
        d = to_device(gpu_engine, table)
        st = gpu_engine.rank_state(FIT, n)
        h = F.HostRanked(FIT, n)
        before = None
        for a, b in chunks(ROWS, 500):
            gpu_engine.rank_update(st, d[a:b], a)
            h.update(table[a:b], a)
            got = st.words.cpu().numpy()
            same(got, h.to_words(), (name, a))
            if name == "ascending" and before is not None and a >= 1000:
                assert np.array_equal(got[8:], before[8:]) and got[1] == before[1]     # no row was a candidate
            if name == "descending" and before is not None and b <= valid:
                assert not np.intersect1d(got[9::8], before[9::8]).size               # every entry is new
            before = got
    # a chunk of invalid rows only counts
    st = _fed(gpu_engine, n, to_device(gpu_engine, down))
    bad = np.full((700, 6), 1.0)
    bad[::2, 0], bad[1::2, 0] = NAN, 1e300
    h = F.HostRanked(FIT, n)
    h.update(down, 0)
    h.update(bad, ROWS)
    gpu_engine.rank_update(st, to_device(gpu_engine, bad), ROWS)
    same(st.words.cpu().numpy(), h.to_words())
    only_bad = gpu_engine.rank_state(FIT, n)
    gpu_engine.rank_update(only_bad, to_device(gpu_engine, bad), 0)
    assert only_bad.words[:4].tolist() == [n, 0, 0, 700]
    same(only_bad.words.cpu().numpy(), host_words(n, bad))


@pytest.mark.parametrize("start", [(1 << 40) + 3, (1 << 62) - ROWS, (1 << 32) - 1500])
def test_wide_flat_indices(gpu_engine, salted, start):
    t, d = salted
    for n in (65, 4096):
        ref = host_words(n, t, start)
        idx = F.HostRanked.from_words(FIT, n, ref).result()["index"]
        assert idx.min() >= start and idx.max() < start + ROWS and (idx.max() > 1 << 32)
        same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), d, [(0, ROWS)], start), ref, n)
        same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), d, chunks(ROWS, 257)[::-1], start), ref, n)


def test_unaligned_record_base(gpu_engine, salted):
    t, _ = salted
    d = to_device(gpu_engine, t, unaligned=True)
    for n in (64, 4096):
        same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), d, [(0, ROWS)], 5), host_words(n, t, 5), n)
        same(feed(gpu_engine, gpu_engine.rank_state(FIT, n), d, chunks(ROWS, 999), 5), host_words(n, t, 5), n)


@pytest.mark.parametrize("n", [1, 64, 4096])
def test_merges(gpu_engine, n):
    """Two and three device states over disjoint rows in every order (with n = 4096 two full lists:
    more keys than one block sorts), an empty state either way round, and a state from the host."""
    eng = gpu_engine
    t = rank_table(9000, 25)
    d = to_device(eng, t)
    ref = host_words(n, t, 2)
    parts = ((0, 4400), (4400, 4600), (4600, 9000))

    def part(a, b):
        st = eng.rank_state(FIT, n)
        eng.rank_update(st, d[a:b], 2 + a)
        return st
    for perm in itertools.permutations(range(3)):
        tot = eng.rank_state(FIT, n)
        for k in perm:
            eng.rank_merge(tot, part(*parts[k]).words)
        same(tot.words.cpu().numpy(), ref, (n, perm))
    two = part(0, 4400)
    eng.rank_merge(two, part(4400, 9000).words)
    same(two.words.cpu().numpy(), ref, n)
    assert F.rank_differences(eng.rank_result(two), F.HostRanked.from_words(FIT, n, ref).result()) == []
    eng.rank_merge(two, eng.rank_state(FIT, n).words)               # an empty state changes nothing
    same(two.words.cpu().numpy(), ref, n)
    empty = eng.rank_state(FIT, n)
    eng.rank_merge(empty, two.words)                                # and takes everything
    same(empty.words.cpu().numpy(), ref, n)
    host = F.HostRanked(FIT, n)
    host.update(t[4400:], 2 + 4400)
    from_host = part(0, 4400)
    eng.rank_merge(from_host, host.words)                           # CPU words, as gloo delivers them
    same(from_host.words.cpu().numpy(), ref, n)
    with pytest.raises(ValueError, match="layouts"):
        eng.rank_merge(two, two.words[:-8])


# ---- the real engine ---------------------------------------------------------------------------
def engine_spec():
    sw = pkg("sweep")
    return sw.SweepSpec("grid60", full_cfg(BASE_CFG), [("m_chi_GeV", np.logspace(0, 3.5, 5)),
                                                       ("I_p", np.linspace(0.05, 1, 3)),
                                                       ("delta_LZ", np.logspace(-4, 0, 4))])


def engine_fit(table, n, ranked=True):
    """Targets inside the 60-point table's own range (tests/test_gpu_fit.py's)."""
    yb, dm = np.median(table[:, 0]), np.median(table[:, 4])
    d = {"terms": [{"field": "Y_B", "target": float(yb), "sigma": float(abs(yb))},
                   {"field": "DM_over_B", "target": float(dm), "sigma": float(abs(dm))}],
         "levels": [0.5, 2.0], "maps": [["delta_LZ"]], "select": {"level": 2.0, "cap": 20}}
    if ranked:
        d["ranked"] = {"n": n}
    return F.FitSpec.from_json(d)


def host_ranked(fit, table):
    h = F.HostRanked(fit, fit.ranked)
    h.update(table, 0)
    return h.result()


@pytest.mark.parametrize("n", [7, 100])
def test_run_sweep_with_ranked_on_the_engine(gpu_engine, n):
    sw = pkg("sweep")
    spec = engine_spec()
    plain = sw.run_sweep(spec, gpu_engine, chunk=16, log=lambda s: None, reuse=True)
    fit = engine_fit(plain.cpu().numpy(), n)
    table, res = sw.run_sweep(spec, gpu_engine, chunk=16, log=lambda s: None, reuse=True, fit=fit)
    assert torch.equal(table, plain)
    ref = host_ranked(fit, table.cpu().numpy())
    assert ref["count"] == min(n, 60) and ref["n_valid"] == 60
    assert F.rank_differences(res["ranked"], ref) == []
    first = res["ranked"]
    assert int(first["index"][0]) == res["best"]["index"] and float(first["chi2"][0]) == res["best"]["chi2"]
    none, only = sw.run_sweep(spec, gpu_engine, chunk=16, log=lambda s: None, reuse=True, fit=fit, keep_table=False)
    assert none is None and F.rank_differences(only["ranked"], ref) == []


# ---- the CLI as child processes ----------------------------------------------------------------
def run(cmd, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (cmd, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


N_CLI = 25
TODAY = {"manifest.json", "summary.json", "table.npy", "fit.json", "fit_maps.npz", "selected.npy"}


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """One --fit run without the key (its table gives the targets), then with the key: one rank,
    --no-table, two gloo ranks on the one GPU and one RCCL rank, all of the same small spec."""
    d = tmp_path_factory.mktemp("rankcli")
    spec = engine_spec()
    with open(d / "spec.json", "w") as f:
        json.dump(spec.to_json(), f)
    base = [sys.executable, "-m", PKG_NAME + ".sweep", "--spec", str(d / "spec.json"), "--chunk", "16"]
    run(base + ["--out", str(d / "seed")])
    table = np.load(d / "seed" / "table.npy")
    for name, ranked in (("plain", False), ("ranked", True)):
        with open(d / f"{name}.json", "w") as f:
            json.dump(engine_fit(table, N_CLI, ranked).to_json(), f)
    run(base + ["--out", str(d / "plain"), "--fit", str(d / "plain.json")])
    fit = ["--fit", str(d / "ranked.json")]
    run(base + ["--out", str(d / "one")] + fit)
    run(base + ["--out", str(d / "only"), "--no-table"] + fit)
    torchrun = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "2",
                "--master-addr", "127.0.0.1", "--master-port", str(free_port())]
    run(torchrun + base[1:] + ["--out", str(d / "two"), "--dist-backend", "gloo"] + fit)
    torchrun[torchrun.index("--nproc-per-node") + 1], torchrun[-1] = "1", str(free_port())
    run(torchrun + base[1:] + ["--out", str(d / "rccl"), "--dist-backend", "nccl"] + fit)
    return d, spec, engine_fit(table, N_CLI), table


def files(path):
    return {n for n in os.listdir(path) if not n.startswith("shard_")}


def test_cli_ranked_files(cli_runs):
    d, spec, fit, table = cli_runs
    assert np.array_equal(np.load(d / "one" / "table.npy"), table)
    ref = host_ranked(fit, table)
    assert ref["count"] == N_CLI
    with open(d / "one" / "fit.json") as f:
        rep = json.load(f)
    assert rep["spec"] == fit.to_json() and rep["spec"]["ranked"] == {"n": N_CLI}
    assert rep["ranked"] == {"n": N_CLI, "count": N_CLI, "chi2_first": float(ref["chi2"][0]),
                             "chi2_last": float(ref["chi2"][-1]), "axes": ["m_chi_GeV", "I_p", "delta_LZ"]}
    z = dict(np.load(d / "one" / "fit_ranked.npz"))
    assert set(z) == {"index", "chi2", "records", "params"}
    assert z["index"].dtype == np.int64 and np.array_equal(z["index"], ref["index"])
    assert np.array_equal(z["chi2"].view(np.int64), ref["chi2"].view(np.int64))
    assert np.array_equal(z["records"].view(np.int64), table[z["index"]].view(np.int64))
    assert [rep["best"]["final"][k] for k in FIELDS] == z["records"][0].tolist()
    assert rep["best"]["index"] == int(z["index"][0]) and rep["best"]["chi2"] == float(z["chi2"][0])
    for j in range(N_CLI):
        assert dict(zip(rep["ranked"]["axes"], z["params"][j].tolist())) == spec.point_params(int(z["index"][j]))
    with open(d / "one" / "summary.json") as f:
        assert json.load(f)["fit"] == rep
    assert files(d / "one") == TODAY | {"fit_ranked.npz"}
    assert files(d / "only") == (TODAY | {"fit_ranked.npz"}) - {"table.npy"}


@pytest.mark.parametrize("other", ["only", "two", "rccl"])
def test_cli_every_run_gives_the_same_list(cli_runs, other):
    d = cli_runs[0]
    with open(d / "one" / "fit.json") as f:
        rep = json.load(f)
    with open(d / other / "fit.json") as f:
        rep2 = json.load(f)
    assert rep2["ranked"] == rep["ranked"] and rep2 == rep
    z, z2 = dict(np.load(d / "one" / "fit_ranked.npz")), dict(np.load(d / other / "fit_ranked.npz"))
    assert set(z) == set(z2)
    for k in z:
        assert z[k].dtype == z2[k].dtype and z[k].shape == z2[k].shape
        assert np.array_equal(z[k].view(np.int64), z2[k].view(np.int64)), k


def test_cli_without_the_key_writes_todays_files(cli_runs):
    d = cli_runs[0]
    assert files(d / "plain") == TODAY
    with open(d / "plain" / "fit.json") as f:
        rep = json.load(f)
    assert "ranked" not in rep and "ranked" not in rep["spec"]
    with open(d / "one" / "fit.json") as f:
        assert set(json.load(f)) == set(rep) | {"ranked"}
