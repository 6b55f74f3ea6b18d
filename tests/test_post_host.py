"""Sweep posteriors on the host: the one definition of a row's weight (csrc/lzq_post.h, through the
library's host function lzq_post_weights_host) against numpy's exp and at its edges, the numpy
implementation (fit.HostPosterior) against literal values on a hand-written table, its independence
of chunking and merging word for word, the "posterior" key of the fit spec, the sweep driver's
posterior on CPU tensors (one process, three gloo ranks; a numeric offset and "best"), and the C
ABI's argument validation (which returns before any GPU work)."""
import ctypes
import json
import math
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import pkg

INF, NAN = float("inf"), float("nan")
F = pkg("fit")
ONE = 1 << 62
TERM = {"field": "Y_B", "target": 1.0, "sigma": 0.5}


def one_term(**kw):
    return F.FitSpec.from_json({"terms": [TERM], **kw})


def rows_of_a(a):
    """Records whose chi2 under TERM is exactly the non-negative doubles `a` where sqrt(a) / 2 is exact,
    and within an ulp or two otherwise: Y_B = 1 + sqrt(a) / 2."""
    t = np.zeros((len(a), 6))
    t[:, 0] = 1.0 + 0.5 * np.sqrt(np.asarray(a, dtype=np.float64))
    return t


def spec_of(lens, names=("beta_over_H", "I_p", "v_w")):
    sw = pkg("sweep")
    return sw.SweepSpec("t", dict(sw.EQUAL_MASS), [(n, np.linspace(0.1, 0.9, k)) for n, k in zip(names, lens)])


# ---- the weight --------------------------------------------------------------------------------
def test_weight_against_numpy_exp():
    """q 2^-62 against exp(-a/2) on 10^4 values of a in [0, 86): relative difference at most
    2^-46 plus one unit of 2^-62 (the truncation).  The bound is derived: the polynomial is within
    0.63 ulp, the rounding of u = a K costs |u| 2^-53 with |u| <= 62, numpy's exp is within 1 ulp;
    (62 + 2) 2^-53 = 2^-47, doubled."""
    fit = one_term()
    rows = rows_of_a(np.random.default_rng(1).uniform(0.0, 86.0, 10_000))
    a = F.chi2_rows(fit, rows)          # the a the function sees (offset 0)
    assert a.min() >= 0.0 and a.max() < 86.0 + 1e-9 and a.size == 10_000
    q = F.post_weights(fit, 0.0, rows)
    assert q.dtype == np.uint64 and (q <= np.uint64(ONE)).all()
    ref = np.exp(-a / 2.0)
    err = np.abs(q.astype(np.float64) * 2.0 ** -62 - ref)
    worst = float(np.max((err - 2.0 ** -62) / ref))
    print(f"worst relative difference beyond one unit: {worst:.3e} (bound {2.0 ** -46:.3e})")
    assert worst <= 2.0 ** -46


def test_weight_edges():
    fit = one_term()
    # a = 0 is exactly one
    assert F.post_weights(fit, 0.0, rows_of_a([0.0])).tolist() == [ONE]
    assert F.post_weights(fit, 4.0, rows_of_a([4.0])).tolist() == [ONE]      # chi2 4 at offset 4
    # above the offset's floor, and rows whose chi2 is not finite
    t = rows_of_a([1.0, 0.0, 0.0, 0.0, 0.0])
    t[1:, 0] = [NAN, INF, -INF, 1e200]
    assert F.post_weights(fit, 4.0, t).tolist() == [F.Q_ABOVE] + [F.Q_INVALID] * 4
    assert (F.Q_INVALID, F.Q_ABOVE) == (2 ** 64 - 1, 2 ** 64 - 2)
    # q = 0 from the first a past 124 ln 2 = 85.95: w < 2^-62 truncates to nothing
    a = np.arange(85.0, 87.0, 1.0 / 1024)                   # chi2 of these rows is within 2 ulp of a
    q = F.post_weights(fit, 0.0, rows_of_a(a))
    c = F.chi2_rows(fit, rows_of_a(a))
    assert np.all(np.diff(q.astype(np.int64)) <= 0)         # monotone
    cross = float(c[np.flatnonzero(q == 0)[0]])
    assert 85.9 <= cross <= 86.0 and abs(cross - 124 * math.log(2.0)) < 2.0 / 1024
    assert q[c < 85.9].min() >= 1 and q[c > 86.0].max() == 0
    # far beyond: still zero, never a sentinel
    assert F.post_weights(fit, 0.0, rows_of_a([1e3, 1e10, 1e300])).tolist() == [0, 0, 0]


# ---- literal values on a hand-written 2 x 2 x 2 grid --------------------------------------------
# chi2 = ((Y_B - 1) / 0.5)^2, offset 1:
#   row   Y_B     chi2   a     class
#   0     1.5     1      0     weight 2^62
#   1     1.0     0      -1    above
#   2     nan                  invalid
#   3     2.0     4      3     weight trunc(exp(-1.5) 2^62)
#   4     0.5     1      0     weight 2^62
#   5     6.0     100    99    zero
#   6     1e200   inf          invalid (overflow)
#   7     1.5     1      0     weight 2^62
LIT_YB = [1.5, 1.0, NAN, 2.0, 0.5, 6.0, 1e200, 1.5]
E15 = 1029006239845977778          # floor(exp(-3/2) * 2^62) to 60 digits


def literal():
    t = np.zeros((8, 6))
    t[:, 0] = LIT_YB
    fit = one_term(levels=[1.0, 4.0], maps=[["v_w"], ["beta_over_H", "I_p"]],
                   posterior={"offset": 1.0, "credible": [0.683, 0.954, 0.997]})
    spec = spec_of((2, 2, 2))
    return t, fit, fit.resolve(spec), fit.axis_values(spec)


def check_literal(res):
    assert (res["n_used"], res["n_zero"], res["n_above"], res["n_invalid"]) == (4, 1, 1, 2)
    assert res["offset"] == 1.0
    Z = int(res["Z_units"])
    q3 = Z - 3 * ONE
    assert abs(q3 - E15) <= E15 * 2.0 ** -46 + 1
    assert res["Z"] == Z / ONE and abs(res["Z"] - (3 + math.exp(-1.5))) < 1e-13
    assert res["mass_within"] == [3 * ONE / Z, 1.0]
    # a = 0 sits in bin 0 (93% of the mass), a = 3 in bin 48: upper edges 1/16 and 49/16
    assert res["credible"] == [{"p": 0.683, "delta_chi2": 0.0625}, {"p": 0.954, "delta_chi2": 3.0625},
                               {"p": 0.997, "delta_chi2": 3.0625}]
    pair = lambda v: [v >> 31, v & 0x7FFFFFFF]
    hist = res["hist"]
    assert hist.shape == (2048, 2) and hist.dtype == np.uint64
    assert hist[0].tolist() == pair(3 * ONE) and hist[48].tolist() == pair(q3)
    assert int(hist.sum()) == sum(pair(3 * ONE)) + sum(pair(q3))
    m0, m1 = res["maps"]
    # v_w (the fastest axis): even rows 0, 4 / odd rows 3, 7
    assert m0["axes"] == ["v_w"] and m0["weight"].tolist() == [pair(2 * ONE), pair(ONE + q3)]
    assert m0["weight"].dtype == np.uint64 and m0["posterior"].dtype == np.float64
    assert m0["posterior"].tolist() == [float(2 * ONE) / float(Z), float(ONE + q3) / float(Z)]
    e = math.exp(-1.5)
    mean = (0.1 * 2 + 0.9 * (1 + e)) / (3 + e)
    assert abs(m0["mean"] - mean) < 1e-13
    assert abs(m0["std"] - math.sqrt((0.1 - mean) ** 2 * 2 / (3 + e) + (0.9 - mean) ** 2 * (1 + e) / (3 + e))) < 1e-13
    # (beta_over_H, I_p): rows (0, 1), (2, 3), (4, 5), (6, 7)
    assert m1["weight"].tolist() == [pair(ONE), pair(q3), pair(ONE), pair(ONE)]
    assert m1["posterior"].shape == (2, 2) and m1["mean"] is None and m1["std"] is None
    assert abs(float(m1["posterior"].sum()) - 1.0) < 1e-15


def test_literal_values():
    t, fit, maps, ax = literal()
    h = F.HostPosterior(fit, maps, 1.0, ax)
    h.update(t, 0)
    check_literal(h.result())
    assert h.to_words().dtype == np.int64 and h.to_words().size == 32 + 2 * 2048 + 2 * (2 + 4)
    again = F.HostPosterior.from_words(fit, maps, 1.0, h.to_words(), ax)
    assert again.rows == 8 and F.post_differences(again.result(), h.result()) == []
    # an empty state: nothing to normalise by
    res = F.HostPosterior(fit, maps, 1.0, ax).result()
    assert res["Z"] == 0.0 and res["Z_units"] == "0" and res["mass_within"] == [None, None]
    assert [c["delta_chi2"] for c in res["credible"]] == [None] * 3 and res["maps"][0]["mean"] is None
    # mass in the overflow bin: its upper edge is not a threshold
    far = one_term(posterior={"offset": 0.0, "credible": [0.5]})
    h = F.HostPosterior(far, [], 0.0)
    h.w[F.PW_HIST + 2 * 2047] = 5
    assert h.result()["credible"] == [{"p": 0.5, "delta_chi2": None}]


def test_row_limit():
    t, fit, maps, ax = literal()
    h = F.HostPosterior(fit, maps, 1.0, ax)
    h.rows = (1 << 32) - 7
    with pytest.raises(ValueError, match="2\\^32 rows"):
        h.update(t, 0)
    other = F.HostPosterior(fit, maps, 1.0, ax)
    other.update(t, 0)
    with pytest.raises(ValueError, match="2\\^32 rows"):
        h.merge(other)
    with pytest.raises(ValueError, match="offsets"):
        F.HostPosterior(fit, maps, 2.0, ax).merge(other)
    with pytest.raises(ValueError, match="finite"):
        F.HostPosterior(fit, maps, -1.0)


# ---- chunking and merging ------------------------------------------------------------------------
def random_table(n, seed):
    rng = np.random.default_rng(seed)
    t = rng.normal(size=(n, 6))
    t[:, 0] = 1.0 + 0.5 * np.sqrt(rng.uniform(0.0, 200.0, n))
    bad = rng.choice(n, n // 20, replace=False)
    t[bad[0::3], 0], t[bad[1::3], 0], t[bad[2::3], 0] = NAN, INF, 1e300
    return t


def test_chunking_and_merging_are_bitwise_invisible():
    n, start = 3001, 10 ** 12 + 5
    t = random_table(n, 2)
    fit = one_term(levels=[20.0, 60.0, 90.0], maps=[["v_w"], ["beta_over_H", "v_w"], ["I_p"]], posterior={})
    maps = [F.FitMap(("v_w",), (1,), (16,)), F.FitMap(("beta_over_H", "v_w"), (64, 1), (5, 16)),
            F.FitMap(("I_p",), (4096,), (1000,))]
    for offset in (0.0, 50.0):
        one = F.HostPosterior(fit, maps, offset)
        one.update(t, start)
        c = (one.w[:4]).tolist()
        assert all(x > 0 for x in c) == (offset > 0) and c[0] > 500 and c[1] > 500 and c[3] > 100 and sum(c) == n
        for chunk in (1, 7, 1000):
            for order in (1, -1):
                h = F.HostPosterior(fit, maps, offset)
                for a in list(range(0, n, chunk))[::order]:
                    h.update(t[a:a + chunk], start + a)
                assert np.array_equal(h.to_words(), one.to_words()), (offset, chunk, order)
        tot = F.HostPosterior(fit, maps, offset)
        for a, b in ((2000, n), (0, 1), (1, 2000)):
            part = F.HostPosterior(fit, maps, offset)
            part.update(t[a:b], start + a)
            tot.merge(F.HostPosterior.from_words(fit, maps, offset, part.to_words()))
        assert np.array_equal(tot.to_words(), one.to_words()) and tot.rows == n
        # the histogram and every map hold the whole weight
        res = one.result()
        Z = int(res["Z_units"])
        total = lambda p: (int(p[:, 0].sum()) << 31) + int(p[:, 1].sum())
        assert total(res["hist"]) == Z and all(total(m["weight"]) == Z for m in res["maps"])
        assert res["mass_within"][0] < res["mass_within"][1] <= 1.0


# ---- the spec key --------------------------------------------------------------------------------
def test_posterior_spec_parsing_and_round_trip():
    base = {"terms": [TERM], "levels": [1.0], "maps": [["v_w"]]}
    plain = F.FitSpec.from_json(base)
    assert plain.posterior is None and "posterior" not in plain.to_json()
    assert plain.to_json() == {"terms": [TERM], "levels": [1.0], "maps": [["v_w"]]}
    d = F.FitSpec.from_json({**base, "posterior": {}})
    assert d.posterior == {"offset": "best", "credible": [0.683, 0.954, 0.997]}
    assert d.to_json()["posterior"] == {"offset": "best", "credible": [0.683, 0.954, 0.997]}
    s = F.FitSpec.from_json({**base, "posterior": {"offset": 3, "credible": [0.5, 0.9]}})
    assert s.posterior == {"offset": 3.0, "credible": [0.5, 0.9]}
    for spec in (plain, d, s):
        again = F.FitSpec.from_json(json.loads(json.dumps(spec.to_json())))
        assert again.to_json() == spec.to_json() and again.posterior == spec.posterior
    bad = [{"offset": -1.0}, {"offset": NAN}, {"offset": INF}, {"offset": "worst"}, {"offset": None}, {"offset": True},
           {"offset": [1.0]}, {"credible": [0.9, 0.5]}, {"credible": [0.5, 0.5]}, {"credible": [0.0]}, {"credible": [1.0]},
           {"credible": [NAN]}, {"credible": 0.5}, {"credible": ["x"]}, {"level": 1.0}, [1.0], "best", 3.0]
    for p in bad:
        with pytest.raises(ValueError, match="posterior"):
            F.FitSpec.from_json({**base, "posterior": p})
    assert F.FitSpec.from_json({**base, "posterior": {"credible": []}}).posterior["credible"] == []
    ax = d.axis_values(spec_of((2, 3, 4)))
    assert list(ax) == ["v_w"] and ax["v_w"].tolist() == np.linspace(0.1, 0.9, 4).tolist()


# ---- the sweep driver with a posterior, on CPU tensors -------------------------------------------
def fake_compute(start, n, out):
    idx = torch.arange(start, start + n, dtype=torch.float64)
    out.copy_(torch.stack([idx * k * 0.015625 + 0.25 for k in range(1, 7)], dim=1))


TOTAL, CHUNK = 1001, 97     # 7 x 11 x 13 grid; three uneven shards
MK = lambda n: torch.empty((n, 6), dtype=torch.float64)


def driver(offset):
    """Y_B = idx / 64 + 0.25, target 5.5, sigma 0.5: chi2 = ((idx - 336) / 32)^2, from 0 at row 336 (rank 1 of three)
    to 432 at row 1000."""
    fit = F.FitSpec.from_json({"terms": [{"field": "Y_B", "target": 5.5, "sigma": 0.5}], "levels": [1.0, 30.0],
                               "maps": [["beta_over_H", "I_p"], ["v_w"]], "posterior": {"offset": offset}})
    spec = spec_of((7, 11, 13))
    table = MK(TOTAL)
    fake_compute(0, TOTAL, table)
    h = F.HostFit(fit, fit.resolve(spec))
    h.update(table.numpy(), 0)
    off = h.result()["best"]["chi2"] if offset == "best" else offset
    p = F.HostPosterior(fit, fit.resolve(spec), off, fit.axis_values(spec))
    p.update(table.numpy(), 0)
    return fit, spec, h.result(), p.result()


@pytest.mark.parametrize("offset", [2.0, "best"])
def test_run_local_with_posterior_single_process(tmp_path, offset):
    sw = pkg("sweep")
    fit, spec, ref, pref = driver(offset)
    assert pref["offset"] == (0.0 if offset == "best" else 2.0) and ref["best"] == {"chi2": 0.0, "index": 336}
    assert pref["n_used"] > 100 and pref["n_zero"] > 100 and (pref["n_above"] > 0) == (offset == 2.0)
    acc = F.make_accumulator(fit, fit.resolve(spec), None, fit.axis_values(spec))
    table = sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, str(tmp_path), fit=acc)
    res = F.combine(acc, local=table, start=0)
    assert F.differences(res, ref) == [] and F.post_differences(res["posterior"], pref) == []
    assert res["posterior"]["maps"][1]["mean"] is not None and res["posterior"]["maps"][0]["mean"] is None
    # resumed chunks are folded too
    acc = F.make_accumulator(fit, fit.resolve(spec), None, fit.axis_values(spec))
    again = sw.run_local(lambda *a: 1 / 0, 0, TOTAL, MK, CHUNK, str(tmp_path), resume=True, fit=acc)
    assert F.post_differences(F.combine(acc, local=again, start=0)["posterior"], pref) == []
    # fit only: a numeric offset needs no table, "best" is refused with the way out
    acc = F.make_accumulator(fit, fit.resolve(spec), None, fit.axis_values(spec))
    assert sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, fit=acc, keep_table=False) is None
    if offset == "best":
        with pytest.raises(ValueError, match="give a number"):
            F.combine(acc)
    else:
        assert F.post_differences(F.combine(acc)["posterior"], pref) == []
    # the report and the files
    rep = F.report(fit, res, spec, TOTAL, None)
    json.dumps(rep)
    assert rep["spec"]["posterior"]["offset"] == offset and rep["posterior"]["Z_units"] == pref["Z_units"]
    assert set(rep["posterior"]) == {"offset", "n_used", "n_zero", "n_above", "n_invalid", "Z", "Z_units", "mass_within",
                                     "credible", "maps"}
    assert rep["posterior"]["maps"][1] == {"axes": ["v_w"], "mean": pref["maps"][1]["mean"], "std": pref["maps"][1]["std"]}
    F.write_files(str(tmp_path), rep, res)
    z = np.load(tmp_path / "fit_maps.npz")
    assert set(z.files) == {f"map{k}_{s}" for k in (0, 1) for s in ("chi2_min", "argmin", "posterior", "weight")}
    assert z["map0_weight"].shape == (77, 2) and z["map0_weight"].dtype == np.uint64
    assert z["map0_posterior"].shape == (7, 11) and np.array_equal(z["map1_weight"], pref["maps"][1]["weight"])


def test_without_the_key_nothing_changes(tmp_path):
    sw = pkg("sweep")
    fit, spec, ref, _ = driver(2.0)
    plain = F.FitSpec.from_json({k: v for k, v in fit.to_json().items() if k != "posterior"})
    acc = F.make_accumulator(plain, plain.resolve(spec))
    sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, fit=acc)
    res = F.combine(acc)
    assert "posterior" not in res and F.differences(res, ref) == [] and acc.post is None
    rep = F.report(plain, res, spec, TOTAL, None)
    assert "posterior" not in rep and "posterior" not in rep["spec"]
    F.write_files(str(tmp_path), rep, res)
    assert set(np.load(tmp_path / "fit_maps.npz").files) == {f"map{k}_{s}" for k in (0, 1) for s in ("chi2_min", "argmin")}


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, offset):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sw = pkg("sweep")
    fit, spec, ref, pref = driver(offset)
    s, e = sw.shard_range(TOTAL, rank, world)
    acc = F.make_accumulator(fit, fit.resolve(spec), None, fit.axis_values(spec))
    local = sw.run_local(fake_compute, s, e, MK, CHUNK, fit=acc)
    res = F.combine(acc, world, local=local, start=s)
    diff = F.differences(res, ref) + F.post_differences(res["posterior"], pref)
    with open(os.path.join(out_dir, f"diff.{rank}.json"), "w") as f:
        json.dump(diff, f)
    dist.destroy_process_group()


@pytest.mark.parametrize("offset", [2.0, "best"])
def test_three_gloo_ranks_combine_to_the_one_pass_posterior(offset):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(3, free_port(), d, offset), nprocs=3, join=True)
        for r in range(3):
            with open(os.path.join(d, f"diff.{r}.json")) as f:
                assert json.load(f) == [], r


# ---- C ABI: every validation error is LZQ_EINVAL with a message, before any GPU work ------------
def test_capi_post_validation():
    n = pkg("_native")
    L = n.load()

    def terms(*ts):
        arr = (n.LzqFitTerm * max(1, len(ts)))()
        for k, (f, t, s) in enumerate(ts):
            arr[k].field, arr[k].target, arr[k].sigma = f, t, s
        return arr

    def maps(*ms):
        arr = (n.LzqFitMap * max(1, len(ms)))()
        for k, m in enumerate(ms):
            arr[k].n_axes = len(m)
            for a, (stride, ln) in enumerate(m):
                arr[k].stride[a], arr[k].len[a] = stride, ln
        return arr

    def levels(*ls):
        return (ctypes.c_double * max(1, len(ls)))(*ls)

    good_t, good_m = terms((0, 1.0, 1.0)), maps([(1, 4)])

    def update(t, nt, lv, nl, m, nm, offset=0.0):
        return L.lzq_post_update(t, nt, lv, nl, m, nm, offset, 8, 0, 1, 8, None)

    def expect(rc, msg):
        assert rc == -1 and msg in L.lzq_last_error(), (rc, msg, L.lzq_last_error())
    expect(update(terms(*[(0, 1.0, 1.0)] * 4), 5, levels(), 0, good_m, 0), b"5 terms")
    expect(update(good_t, 0, levels(), 0, good_m, 0), b"0 terms")
    expect(update(good_t, 1, levels(1, 2, 3, 4), 5, good_m, 0), b"5 levels")
    expect(update(good_t, 1, levels(), 0, maps(*[[(1, 4)]] * 4), 5), b"5 maps")
    expect(update(terms((6, 1.0, 1.0)), 1, levels(), 0, good_m, 0), b"unknown field")
    expect(update(terms((0, 1.0, 0.0)), 1, levels(), 0, good_m, 0), b"sigma")
    expect(update(terms((0, NAN, 1.0)), 1, levels(), 0, good_m, 0), b"target")
    expect(update(good_t, 1, levels(2.0, 1.0), 2, good_m, 0), b"ascending")
    expect(update(good_t, 1, levels(), 0, maps([(1, (1 << 24) + 1)]), 1), b"2^24 cells")
    for off in (-1.0, -1e-300, NAN, INF, -INF):
        expect(update(good_t, 1, levels(), 0, good_m, 1, off), b"offset must be finite and >= 0")
        expect(L.lzq_post_weights_host(good_t, 1, off, None, 0, None), b"offset")
    expect(update(None, 1, levels(), 0, good_m, 1), b"null terms")
    expect(L.lzq_post_update(good_t, 1, levels(), 0, good_m, 1, 0.0, 8, -1, 1, 8, None), b"bad arguments")
    expect(L.lzq_post_update(good_t, 1, levels(), 0, good_m, 1, 0.0, 8, 0, 1, None, None), b"bad arguments")
    expect(L.lzq_post_update(good_t, 1, levels(), 0, good_m, 1, 0.0, None, 0, 1, 8, None), b"bad arguments")
    expect(L.lzq_post_update(good_t, 1, levels(), 0, good_m, 1, 0.0, 8, (1 << 62) - 1, 2, 8, None), b"bad arguments")
    expect(L.lzq_post_update(good_t, 1, levels(), 0, good_m, 1, 0.0, 8, 0, (1 << 32) + 1, 8, None), b"2^32 rows")
    expect(L.lzq_post_weights_host(good_t, 1, 0.0, None, 1, None), b"bad arguments")
    expect(L.lzq_post_weights_host(good_t, 1, 0.0, None, -1, None), b"bad arguments")
    expect(L.lzq_post_weights_host(terms((0, 1.0, -1.0)), 1, 0.0, None, 0, None), b"sigma")
    expect(L.lzq_post_reset(good_m, 1, None, None), b"null state")
    expect(L.lzq_post_merge(good_m, 1, 8, 8, None), b"distinct")
    expect(L.lzq_post_merge(good_m, 1, None, 8, None), b"distinct")
    expect(L.lzq_post_merge(maps([(1, 1 << 25)]), 1, 8, 16, None), b"2^24 cells")
    assert L.lzq_post_state_bytes(maps([(1, 1 << 25)]), 1) == -1 and b"2^24 cells" in L.lzq_last_error()
    # sizes: 32 header words, 2048 histogram pairs, a pair per cell; empty chunks are no-ops that still validate
    assert L.lzq_post_state_bytes(None, 0) == (32 + 4096) * 8
    assert L.lzq_post_state_bytes(maps([(77, 5), (1, 11)], [(385, 3)]), 2) == (32 + 4096 + 2 * 55 + 2 * 3) * 8
    assert L.lzq_post_update(good_t, 1, levels(), 0, good_m, 1, 0.0, None, 0, 0, 8, None) == 0
    assert L.lzq_post_weights_host(good_t, 1, 0.0, None, 0, None) == 0
    assert n.ABI_VERSION == 3 and L.lzq_abi_version() == 3     # additive entry points
    assert (n.POST_HEADER_WORDS, n.POST_BINS, n.POST_MAX_ROWS) == (32, 2048, 1 << 32)
