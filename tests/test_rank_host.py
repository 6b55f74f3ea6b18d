"""Ranked points on the host: the numpy state (fit.HostRanked) against literal values on a dozen
hand-made rows (exact ties, invalid rows, a capacity larger than the valid rows), its independence
of chunking, chunk order and merge order word for word, the "ranked" key of the fit spec, the sweep
driver on CPU tensors (one process: plain, resumed, fit only; three gloo ranks), the report and
fit_ranked.npz, the list against the selection, and the C ABI's argument validation (which returns
before any GPU work)."""
import itertools
import json
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import pkg

F = pkg("fit")
INF, NAN = float("inf"), float("nan")
TERM = {"field": "Y_B", "target": 1.0, "sigma": 0.5}
INF_BITS, NONE = 0x7FF0000000000000, (1 << 64) - 1
FIT_JSON_KEYS = {"spec", "sweep", "n_points", "n_valid", "n_invalid", "levels", "n_within", "columns", "best", "maps",
                 "n_selected", "n_selected_kept"}


def make_fit(n=None, **more):
    d = {"terms": [TERM], **more}
    if n is not None:
        d["ranked"] = {"n": n}
    return F.FitSpec.from_json(d)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- literal values ----------------------------------------------------------------------------------
#         chi2:  1    1    -    4    1/16   -    0    1/16  16    -     9     9
LITERAL_YB = [1.5, 0.5, NAN, 2.0, 0.875, INF, 1.0, 1.125, 3.0, 1e300, -0.5, 2.5]
START = 10
ORDER = [6, 4, 7, 0, 1, 3, 10, 11, 8]            # by chi2, exact ties by index: d = -+0.25, -+1, -+3
CHI2 = [0.0, 0.0625, 0.0625, 1.0, 1.0, 4.0, 9.0, 9.0, 16.0]


def literal():
    t = np.arange(12, dtype=np.float64)[:, None] * 10.0 + np.arange(6, dtype=np.float64)[None, :]
    t[:, 0] = LITERAL_YB
    t[3, 5], t[0, 2] = NAN, -INF                # non-finite values outside the terms do not matter
    return t


def test_literal_rows():
    t = literal()
    h = F.HostRanked(make_fit(4), 4)
    h.update(t, START)
    r = h.result()
    assert (r["n"], r["count"], r["n_valid"], r["n_invalid"]) == (4, 4, 9, 3)
    assert r["index"].tolist() == [16, 14, 17, 10] and r["index"].dtype == np.int64
    assert r["chi2"].tolist() == [0.0, 0.0625, 0.0625, 1.0]
    assert np.array_equal(bits(r["records"]), bits(t[[6, 4, 7, 0]]))
    w = h.to_words()
    assert w.dtype == np.int64 and w.size == F.rank_state_words(4) == 8 + 32
    assert w[:8].tolist() == [4, 4, 9, 3, 0, 0, 0, 0]
    assert w[8:16].view(np.uint64).tolist() == [0, 16] + bits(t[6]).tolist()
    assert w[16:18].view(np.uint64).tolist() == [bits([0.0625])[0], 14]


def test_capacity_above_the_valid_rows():
    t = literal()
    h = F.HostRanked(make_fit(12), 12)
    h.update(t, START)
    r = h.result()
    assert (r["count"], r["n_valid"], r["n_invalid"]) == (9, 9, 3)
    assert r["index"].tolist() == [START + k for k in ORDER] and r["chi2"].tolist() == CHI2
    assert np.array_equal(bits(r["records"]), bits(t[ORDER]))
    w = h.to_words().view(np.uint64)
    assert w[:4].tolist() == [12, 9, 9, 3]
    assert w[8 + 8 * 9:].reshape(3, 8).tolist() == [[INF_BITS, NONE, 0, 0, 0, 0, 0, 0]] * 3
    # an empty state, an empty chunk and a chunk of invalid rows only
    e = F.HostRanked(make_fit(3), 3)
    empty = [3, 0, 0, 0, 0, 0, 0, 0] + [INF_BITS, NONE, 0, 0, 0, 0, 0, 0] * 3
    assert e.to_words().view(np.uint64).tolist() == empty
    e.update(np.empty((0, 6)), 5)
    assert e.to_words().view(np.uint64).tolist() == empty
    e.update(t[[2, 5, 9]], 0)
    assert e.result()["count"] == 0 and e.result()["n_invalid"] == 3 and e.result()["index"].size == 0
    assert F.rank_differences(F.HostRanked.from_words(make_fit(12), 12, h.to_words()).result(), r) == []
    assert F.rank_differences(h.result(), e.like().result()) != []
    with pytest.raises(ValueError, match="words"):
        F.HostRanked(make_fit(3), 3).load(h.to_words())


# ---- invariance ----------------------------------------------------------------------------------------
def tied_table(n=1001, seed=4):
    """Quarter-integer Y_B (exact ties everywhere) with NaN, inf and overflowing rows planted."""
    rng = np.random.default_rng(seed)
    t = rng.normal(size=(n, 6))
    t[:, 0] = rng.integers(-40, 41, n) / 4.0
    bad = rng.choice(n, n // 20, replace=False)
    t[bad[0::3], 0], t[bad[1::3], 0], t[bad[2::3], 0] = NAN, INF, 1e300
    return t


@pytest.mark.parametrize("n", [1, 50, 2000])
def test_chunking_and_chunk_order_are_invisible(n):
    t, fit = tied_table(), make_fit(n)
    one = F.HostRanked(fit, n)
    one.update(t, 7)
    ref = one.to_words()
    r = one.result()
    assert r["n_valid"] + r["n_invalid"] == 1001 and r["n_invalid"] > 10 and r["count"] == min(n, r["n_valid"])
    c = F.chi2_rows(fit, t)
    valid = np.flatnonzero(np.isfinite(c))
    want = valid[np.lexsort((valid, c[valid]))][:n]
    assert r["index"].tolist() == (7 + want).tolist() and np.array_equal(bits(r["records"]), bits(t[want]))
    if n == 50:
        assert len(set(r["chi2"].tolist())) < 25          # the list is full of ties
    for chunk in (1, 97, 1001):
        starts = list(range(0, 1001, chunk))
        for order in (starts, list(np.random.default_rng(chunk).permutation(starts))):
            h = F.HostRanked(fit, n)
            for a in order:
                h.update(t[a:a + chunk], 7 + int(a))
            assert np.array_equal(h.to_words(), ref), (chunk, order[:3])


@pytest.mark.parametrize("n", [1, 50, 2000])
def test_three_shards_merge_in_every_order(n):
    t, fit = tied_table(), make_fit(n)
    one = F.HostRanked(fit, n)
    one.update(t, 0)
    bounds = ((0, 120), (120, 800), (800, 1001))
    for perm in itertools.permutations(range(3)):
        tot = F.HostRanked(fit, n)
        for k in perm:
            a, b = bounds[k]
            s = F.HostRanked(fit, n)
            s.update(t[a:b], a)
            tot.merge_words(s.words)
        assert np.array_equal(tot.to_words(), one.to_words()), perm
    with pytest.raises(ValueError, match="capacities"):
        one.merge(F.HostRanked(fit, n + 1))


# ---- the spec ------------------------------------------------------------------------------------------
def test_ranked_spec_parsing_and_round_trip():
    fit = make_fit(1000, levels=[1.0])
    assert fit.ranked == 1000 and fit.to_json()["ranked"] == {"n": 1000}
    assert F.FitSpec.from_json(fit.to_json()).to_json() == fit.to_json()
    assert F.FitSpec([F.FitTerm("Y_B", 1.0, 0.5)], ranked={"n": 4096}).ranked == 4096
    assert make_fit(1).ranked == 1
    assert make_fit().ranked is None and "ranked" not in make_fit().to_json()
    for bad in ({"n": 0}, {"n": 4097}, {"n": 2.5}, {"n": True}, {"n": "12"}, {"n": 5, "cap": 3}, [5], 5, {}, {"n": -1}):
        with pytest.raises(ValueError, match="ranked"):
            make_fit(levels=[1.0], ranked=bad)
    for bad in (0, 4097, 2.5, True, "7"):
        with pytest.raises(ValueError, match="ranked"):
            F.HostRanked(make_fit(), bad)


# ---- the sweep driver on CPU tensors -------------------------------------------------------------------
def fake_compute(start, n, out):
    idx = torch.arange(start, start + n, dtype=torch.float64)
    out.copy_(torch.stack([idx * k * 0.015625 + 0.25 for k in range(1, 7)], dim=1))


TOTAL, CHUNK, N_RANKED = 1001, 97, 100     # 7 x 11 x 13 grid; three uneven shards
MK = lambda n: torch.empty((n, 6), dtype=torch.float64)


def spec_of(lens, names=("beta_over_H", "I_p", "v_w")):
    sw = pkg("sweep")
    return sw.SweepSpec("t", dict(sw.EQUAL_MASS), [(n, np.linspace(0.1, 0.9, k)) for n, k in zip(names, lens)])


def driver(n=N_RANKED):
    """Y_B = idx / 64 + 0.25, target 5.5, sigma 0.5: chi2 = ((idx - 336) / 32)^2, so rows 336 -+ k tie
    exactly (from k = 3 on across the first two of three shards); the level 1.0 holds 65 rows."""
    fit = F.FitSpec.from_json({"terms": [{"field": "Y_B", "target": 5.5, "sigma": 0.5}], "levels": [1.0, 30.0],
                               "maps": [["v_w"]], "select": {"level": 1.0, "cap": 1000}, "ranked": {"n": n}})
    spec = spec_of((7, 11, 13))
    table = MK(TOTAL)
    fake_compute(0, TOTAL, table)
    h = F.HostRanked(fit, n)
    h.update(table.numpy(), 0)
    return fit, spec, table.numpy(), h.result()


def accumulator(fit, spec):
    return F.make_accumulator(fit, fit.resolve(spec), None, fit.axis_values(spec))


def test_run_local_with_ranked_single_process(tmp_path):
    sw = pkg("sweep")
    fit, spec, table, ref = driver()
    assert ref["count"] == N_RANKED and ref["index"][:5].tolist() == [336, 335, 337, 334, 338]
    acc = accumulator(fit, spec)
    local = sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, str(tmp_path), fit=acc)
    res = F.combine(acc, local=local, start=0)
    assert F.rank_differences(res["ranked"], ref) == []
    # resumed chunks pass through the same call
    acc = accumulator(fit, spec)
    again = sw.run_local(lambda *a: 1 / 0, 0, TOTAL, MK, CHUNK, str(tmp_path), resume=True, fit=acc)
    assert F.rank_differences(F.combine(acc, local=again, start=0)["ranked"], ref) == []
    # fit only: no table is needed
    acc = accumulator(fit, spec)
    assert sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, fit=acc, keep_table=False) is None
    assert F.rank_differences(F.combine(acc)["ranked"], ref) == []
    # the first entry is the fit's best point
    r = res["ranked"]
    assert int(r["index"][0]) == res["best"]["index"] == 336 and float(r["chi2"][0]) == res["best"]["chi2"] == 0.0
    # against the selection: the level holds no more than n rows
    level = fit.select[0]
    assert res["n_selected"] == len(res["selected"]) == 65 <= N_RANKED
    assert np.array_equal(np.sort(r["index"][r["chi2"] <= level]), res["selected"])
    # the report and the files
    rep = F.report(fit, res, spec, TOTAL, None)
    json.dumps(rep)
    assert rep["spec"]["ranked"] == {"n": N_RANKED}
    assert rep["ranked"] == {"n": N_RANKED, "count": N_RANKED, "chi2_first": 0.0, "chi2_last": float(ref["chi2"][-1]),
                             "axes": ["beta_over_H", "I_p", "v_w"]}
    assert set(rep) == FIT_JSON_KEYS | {"ranked"}
    out = tmp_path / "files"
    out.mkdir()
    F.write_files(str(out), rep, res)
    assert sorted(os.listdir(out)) == ["fit.json", "fit_maps.npz", "fit_ranked.npz", "selected.npy"]
    z = np.load(out / "fit_ranked.npz")
    assert set(z.files) == {"index", "chi2", "records", "params"}
    assert z["index"].dtype == np.int64 and z["index"].tolist() == ref["index"].tolist()
    assert z["chi2"].dtype == np.float64 and np.array_equal(bits(z["chi2"]), bits(ref["chi2"]))
    assert z["records"].shape == (N_RANKED, 6) and np.array_equal(bits(z["records"]), bits(table[z["index"]]))
    assert z["params"].shape == (N_RANKED, 3) and z["params"].dtype == np.float64
    for j in range(N_RANKED):
        assert z["params"][j].tolist() == list(spec.point_params(int(z["index"][j])).values())[::-1]
        assert dict(zip(rep["ranked"]["axes"], z["params"][j].tolist())) == spec.point_params(int(z["index"][j]))
    with open(out / "fit.json") as f:
        assert json.load(f)["ranked"] == rep["ranked"]


def test_a_capacity_above_the_grid_and_an_empty_list(tmp_path):
    sw = pkg("sweep")
    fit, spec, table, ref = driver(4096)
    assert ref["count"] == TOTAL
    acc = accumulator(fit, spec)
    sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, fit=acc, keep_table=False)
    res = F.combine(acc)
    assert F.rank_differences(res["ranked"], ref) == []
    assert np.array_equal(np.sort(res["ranked"]["index"]), np.arange(TOTAL))
    none = accumulator(fit, spec)
    res = F.combine(none)
    rep = F.report(fit, res, spec, TOTAL, None)
    assert rep["ranked"] == {"n": 4096, "count": 0, "chi2_first": None, "chi2_last": None,
                             "axes": ["beta_over_H", "I_p", "v_w"]}
    F.write_files(str(tmp_path), rep, res)
    z = np.load(tmp_path / "fit_ranked.npz")
    assert z["index"].shape == (0,) and z["records"].shape == (0, 6) and z["params"].shape == (0, 3)


def test_without_the_key_nothing_changes(tmp_path):
    sw = pkg("sweep")
    fit, spec, _, _ = driver()
    plain = F.FitSpec.from_json({k: v for k, v in fit.to_json().items() if k != "ranked"})
    acc = accumulator(plain, spec)
    table = sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, fit=acc)
    res = F.combine(acc, local=table, start=0)
    assert "ranked" not in res and acc.rank is None
    rep = F.report(plain, res, spec, TOTAL, None)
    assert set(rep) == FIT_JSON_KEYS and "ranked" not in rep["spec"]
    F.write_files(str(tmp_path), rep, res)
    assert sorted(os.listdir(tmp_path)) == ["fit.json", "fit_maps.npz", "selected.npy"]


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sw = pkg("sweep")
    fit, spec, _, ref = driver()
    s, e = sw.shard_range(TOTAL, rank, world)
    acc = accumulator(fit, spec)
    local = sw.run_local(fake_compute, s, e, MK, CHUNK, fit=acc)
    res = F.combine(acc, world, local=local, start=s)
    own = acc.rank.result()
    with open(os.path.join(out_dir, f"diff.{rank}.json"), "w") as f:
        json.dump({"diff": F.rank_differences(res["ranked"], ref), "own": own["n_valid"],
                   "best": [res["best"]["index"], int(res["ranked"]["index"][0])]}, f)
    dist.destroy_process_group()


def test_three_gloo_ranks_combine_to_the_one_pass_list():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(3, free_port(), d), nprocs=3, join=True)
        own = []
        for r in range(3):
            with open(os.path.join(d, f"diff.{r}.json")) as f:
                got = json.load(f)
            assert got["diff"] == [] and got["best"] == [336, 336], r
            own.append(got["own"])
        assert sum(own) == TOTAL and min(own) > 300       # every rank held a shard of its own


# ---- C ABI: every validation error is LZQ_EINVAL with a message, before any GPU work -------------------
def test_capi_rank_validation():
    n = pkg("_native")
    L = n.load()

    def terms(*ts):
        arr = (n.LzqFitTerm * max(1, len(ts)))()
        for k, (f, t, s) in enumerate(ts):
            arr[k].field, arr[k].target, arr[k].sigma = f, t, s
        return arr

    good = terms((0, 1.0, 1.0))

    def update(t=good, nt=1, cap=8, y=8, start=0, count=1, st=8):
        return L.lzq_rank_update(t, nt, cap, y, start, count, st, None)

    def expect(rc, msg):
        assert rc == -1 and msg in L.lzq_last_error(), (rc, msg, L.lzq_last_error())
    for bad in (0, -1, 4097, 1 << 30):
        expect(update(cap=bad), b"n = ")
        expect(L.lzq_rank_state_bytes(bad), b"(1..4096)")
        expect(L.lzq_rank_reset(bad, 8, None), b"n = ")
        expect(L.lzq_rank_merge(bad, 8, 16, None), b"n = ")
    expect(update(t=None), b"null terms")
    expect(update(nt=0), b"0 terms")
    expect(update(t=terms(*[(0, 1.0, 1.0)] * 4), nt=5), b"5 terms")
    expect(update(t=terms((6, 1.0, 1.0))), b"unknown field")
    expect(update(t=terms((-1, 1.0, 1.0))), b"unknown field")
    for sigma in (0.0, -1.0, NAN, INF):
        expect(update(t=terms((0, 1.0, sigma))), b"sigma")
    for target in (NAN, INF, -INF):
        expect(update(t=terms((0, target, 1.0))), b"target")
    expect(update(count=-1), b"bad arguments")
    expect(update(start=-1), b"bad arguments")
    expect(update(start=(1 << 62) - 4, count=5), b"bad arguments")
    expect(update(start=1 << 62, count=1), b"bad arguments")
    expect(update(y=None), b"bad arguments")
    expect(update(st=None), b"bad arguments")
    expect(L.lzq_rank_reset(8, None, None), b"null state")
    expect(L.lzq_rank_merge(8, 8, 8, None), b"distinct")
    expect(L.lzq_rank_merge(8, None, 8, None), b"distinct")
    expect(L.lzq_rank_merge(8, 8, None, None), b"distinct")
    # count == 0 is a no-op that still validates; the state's size
    assert update(y=None, count=0) == 0 and update(start=1 << 62, count=0) == 0
    expect(update(cap=0, count=0), b"n = ")
    for cap in (1, 2, 1000, 4096):
        assert L.lzq_rank_state_bytes(cap) == 8 * (8 + 8 * cap) == 8 * F.rank_state_words(cap)
    assert n.ABI_VERSION == 3 and L.lzq_abi_version() == 3     # additive entry points
    assert (n.RANK_MAX_N, n.RANK_HEADER_WORDS) == (4096, 8) == (F.RANK_MAX_N, F.RANK_HEADER_WORDS)
