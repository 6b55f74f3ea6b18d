"""Sweep fits on the host: the numpy implementation (fit.HostFit) against literal expected values
on a hand-written table (this pins the specification: chi2 term by term, validity, ties to the lower
index, empty cells, `<=` at the levels, the selection cap), its independence of chunking and
merging, FitSpec parsing and map resolution, the sweep driver's fit on CPU tensors (one process,
three gloo ranks, a resumed run), and the C ABI's argument validation (which returns before any GPU
work)."""
import ctypes
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

INF, NAN = float("inf"), float("nan")
F = pkg("fit")


def spec_of(lens, names=("beta_over_H", "I_p", "v_w", "delta_LZ")):
    sw = pkg("sweep")
    return sw.SweepSpec("t", dict(sw.EQUAL_MASS), [(n, np.linspace(0.1, 0.9, k)) for n, k in zip(names, lens)])


# ---- the specification on a hand-written 2 x 3 x 2 grid of 12 rows -------------------------------
# (Y_B, DM_over_B) per row; chi2 = ((Y_B - 1) / 0.5)^2 + ((DM_over_B - 2) / 1)^2
YB = [1.5, 1.0, 2.0, NAN, 1.25, INF, 1e200, 1.0, 1.0, 0.0, 3.0, 1.0]
DM = [2.0, 3.0, NAN, 2.0, 2.0, 2.0, 2.0, 2.5, 4.0, 2.0, 2.0, 5.0]
# chi2:  1    1   nan  nan  .25  inf  inf(overflow) .25  4    4    16   9


def literal_table():
    t = np.empty((12, 6))
    i = np.arange(12.0)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4], t[:, 5] = YB, -i, 0.5, NAN, DM, i * 0.125
    return t


def literal_fit():
    return F.FitSpec.from_json({
        "terms": [{"field": "Y_B", "target": 1.0, "sigma": 0.5}, {"field": "DM_over_B", "target": 2.0, "sigma": 1.0}],
        "levels": [0.25, 1.0, 4.0], "maps": [["beta_over_H", "I_p"], ["v_w"], ["v_w", "beta_over_H"]],
        "select": {"level": 4.0, "cap": 4}})


def check_literal(res):
    assert res["n_valid"] == 8 and res["n_invalid"] == 4           # NaN, NaN, inf and the overflow row
    assert res["n_within"] == [2, 4, 6]                             # <= at 0.25, 1.0 and 4.0
    assert res["best"] == {"chi2": 0.25, "index": 4}                # rows 4 and 7 tie: the lower index
    c = res["columns"]
    assert c["Y_B"] == {"min": 0.0, "max": 1e200, "n_nonfinite": 2}
    assert c["Y_chi"] == {"min": -11.0, "max": 0.0, "n_nonfinite": 0}
    assert c["rho_B_kg_m3"] == {"min": 0.5, "max": 0.5, "n_nonfinite": 0}
    assert c["rho_DM_kg_m3"] == {"min": None, "max": None, "n_nonfinite": 12}
    assert c["DM_over_B"] == {"min": 2.0, "max": 5.0, "n_nonfinite": 1}
    assert c["P_used"] == {"min": 0.0, "max": 1.375, "n_nonfinite": 0}
    m0, m1, m2 = res["maps"]
    # (beta_over_H, I_p): cell (0, 0) ties rows 0 and 1; (0, 1) holds only invalid rows: empty
    assert m0["chi2_min"].tolist() == [[1.0, INF, 0.25], [0.25, 4.0, 9.0]]
    assert m0["argmin"].tolist() == [[0, -1, 4], [7, 8, 11]]
    assert m1["chi2_min"].tolist() == [0.25, 0.25] and m1["argmin"].tolist() == [4, 7]
    # (v_w, beta_over_H): the fastest axis first
    assert m2["chi2_min"].tolist() == [[0.25, 4.0], [1.0, 0.25]] and m2["argmin"].tolist() == [[4, 8], [1, 7]]
    assert res["n_selected"] == 6 and res["selected"].tolist() == [0, 1, 4, 7]   # of [0, 1, 4, 7, 8, 9]
    assert res["selected"].dtype == np.int64 and m0["argmin"].dtype == np.int64


def test_numpy_fit_literal_values():
    fit = literal_fit()
    maps = fit.resolve(spec_of((2, 3, 2), ("beta_over_H", "I_p", "v_w")))
    assert [(m.stride, m.len) for m in maps] == [((6, 2), (2, 3)), ((1,), (2,)), ((1, 6), (2, 2))]
    chi2 = F.chi2_rows(fit, literal_table())
    assert chi2[[0, 1, 4, 7, 8, 9, 10, 11]].tolist() == [1.0, 1.0, 0.25, 0.25, 4.0, 4.0, 16.0, 9.0]
    assert np.isnan(chi2[[2, 3]]).all() and np.isposinf(chi2[[5, 6]]).all()
    h = F.HostFit(fit, maps)
    h.update(literal_table(), 0)
    check_literal(h.result())
    # chunked (an empty chunk, a single row), and through the 64-bit words of the state
    h2 = F.HostFit(fit, maps)
    for a, b in ((0, 5), (5, 5), (5, 6), (6, 12)):
        h2.update(literal_table()[a:b], a)
    check_literal(h2.result())
    check_literal(F.HostFit.from_words(fit, maps, h2.to_words(), h2.sel).result())
    # merged from disjoint ranges, the later rows first in the state
    lo, hi = F.HostFit(fit, maps), F.HostFit(fit, maps)
    lo.update(literal_table()[:7], 0)
    hi.update(literal_table()[7:], 7)
    tot = F.HostFit(fit, maps)
    tot.merge(lo)
    tot.merge(hi)
    check_literal(tot.result())


def test_numpy_fit_no_valid_row():
    fit = F.FitSpec.from_json({"terms": [{"field": "Y_B", "target": 0.0, "sigma": 1.0}], "levels": [1.0],
                               "maps": [["I_p"]], "select": {"level": 1.0, "cap": 0}})
    h = F.HostFit(fit, fit.resolve(spec_of((3,), ("I_p",))))
    res = h.result()
    assert res["best"]["index"] == -1 and res["best"]["chi2"] == INF and res["n_within"] == [0]
    h.update(np.full((3, 6), NAN), 0)
    res = h.result()
    assert res["n_valid"] == 0 and res["n_invalid"] == 3 and res["best"] == {"chi2": INF, "index": -1}
    assert res["maps"][0]["argmin"].tolist() == [-1, -1, -1] and np.isposinf(res["maps"][0]["chi2_min"]).all()
    assert res["selected"].size == 0 and res["n_selected"] == 0
    assert res["columns"]["Y_B"] == {"min": None, "max": None, "n_nonfinite": 3}


def random_table(n, seed):
    """Coarse values (so exact ties abound), both signs, planted NaN / inf / overflow rows."""
    rng = np.random.default_rng(seed)
    t = rng.integers(-6, 7, (n, 6)).astype(np.float64) / 4.0
    t[:, 5] = rng.uniform(-1, 1, n)
    bad = rng.choice(n, max(3, n // 50), replace=False)
    t[bad[0::3], 0] = NAN
    t[bad[1::3], 4] = INF
    t[bad[2::3], 0] = 1e300
    return t


def random_fit():
    return F.FitSpec.from_json({
        "terms": [{"field": "Y_B", "target": 0.25, "sigma": 0.5}, {"field": "DM_over_B", "target": -0.5, "sigma": 0.25},
                  {"field": "P_used", "target": 0.0, "sigma": 1e3}],
        "levels": [1.0, 4.0, 9.0, 100.0], "maps": [["beta_over_H", "I_p"], ["v_w", "delta_LZ"], ["delta_LZ", "I_p"],
                                                   ["v_w"]],
        "select": {"level": 4.0, "cap": 300}})


def test_chunking_and_merging_are_bitwise_invisible():
    n = 5000
    t, fit = random_table(n, 1), random_fit()
    maps = fit.resolve(spec_of((3, 5, 7, 50)))     # 5250 cells of grid: the last 250 stay empty
    one = F.HostFit(fit, maps)
    one.update(t, 0)
    ref = one.result()
    assert ref["n_invalid"] > 0 and ref["n_selected"] > 300 and (ref["maps"][0]["argmin"] >= 0).all()
    rng = np.random.default_rng(2)
    for trial in range(3):
        cuts = np.sort(rng.integers(0, n + 1, 40))
        cuts = np.concatenate([[0], cuts, cuts[5:8], cuts[9:10] + 1, [n]])   # empty and single-row chunks
        cuts = np.sort(np.clip(cuts, 0, n))
        h = F.HostFit(fit, maps)
        for a, b in zip(cuts[:-1], cuts[1:]):
            h.update(t[a:b], int(a))
        assert F.differences(h.result(), ref) == []
        # disjoint ranges as separate states, merged in order; and through the state's words
        parts = []
        for a, b in zip(cuts[:-1:7], list(cuts[7:-1:7]) + [n]):
            p = F.HostFit(fit, maps)
            p.update(t[a:b], int(a))
            parts.append(F.HostFit.from_words(fit, maps, p.to_words(), p.sel))
        tot = F.HostFit(fit, maps)
        for p in parts:
            tot.merge(p)
        assert F.differences(tot.result(), ref) == []
    # chunks in any order: everything but the selection list's order is the same
    h = F.HostFit(fit, maps)
    for a, b in ((3000, 5000), (0, 1), (1, 3000)):
        h.update(t[a:b], a)
    r = h.result()
    r["selected"] = ref["selected"]
    assert F.differences(r, ref) == []


def test_fitspec_parsing_errors_and_map_resolution():
    term = {"field": "Y_B", "target": 1.0, "sigma": 1.0}
    ok = F.FitSpec.from_json({"terms": [term], "maps": ["I_p", ["v_w", "I_p"]]})
    assert ok.maps == [("I_p",), ("v_w", "I_p")] and ok.levels == [] and ok.select is None
    assert F.FitSpec.from_json(ok.to_json()).to_json() == ok.to_json()
    paper = F.load("paper")
    assert [(t.field, t.target, t.sigma) for t in paper.terms] == [("Y_B", 8.72e-11, 8.72e-13),
                                                                   ("DM_over_B", 5.357, 0.05357)]
    bad = [{"terms": []}, {"terms": [term] * 5}, {"terms": [{**term, "field": "nope"}]},
           {"terms": [{**term, "sigma": 0.0}]}, {"terms": [{**term, "sigma": -1.0}]},
           {"terms": [{**term, "sigma": INF}]}, {"terms": [{**term, "sigma": NAN}]},
           {"terms": [{**term, "target": INF}]}, {"terms": [{**term, "target": NAN}]},
           {"terms": [{"field": "Y_B"}]},
           {"terms": [term], "levels": [1, 2, 3, 4, 5]}, {"terms": [term], "levels": [2.0, 1.0]},
           {"terms": [term], "levels": [1.0, 1.0]}, {"terms": [term], "maps": [["I_p"]] * 5},
           {"terms": [term], "maps": [["I_p", "v_w", "delta_LZ"]]}, {"terms": [term], "maps": [[]]},
           {"terms": [term], "select": {"level": 1.0, "cap": -1}}, {"terms": [term], "nonsense": 1}]
    for d in bad:
        with pytest.raises(ValueError):
            F.FitSpec.from_json(d)
    spec = spec_of((3, 5, 7, 11))
    with pytest.raises(ValueError, match="not an axis"):
        F.FitSpec.from_json({"terms": [term], "maps": [["m_mix"]]}).resolve(spec)
    with pytest.raises(ValueError, match="2\\^24"):
        F.FitSpec.from_json({"terms": [term], "maps": [["I_p", "v_w"]]}).resolve(
            spec_of((2, 5000, 5000), ("beta_over_H", "I_p", "v_w")))
    want = {("beta_over_H", "I_p"): ((385, 77), (3, 5)), ("v_w", "delta_LZ"): ((11, 1), (7, 11)),
            ("I_p", "delta_LZ"): ((77, 1), (5, 11)), ("delta_LZ", "I_p"): ((1, 77), (11, 5)),
            ("beta_over_H",): ((385,), (3,)), ("delta_LZ",): ((1,), (11,)), ("v_w",): ((11,), (7,))}
    for axes, (stride, ln) in want.items():
        m, = F.FitSpec.from_json({"terms": [term], "maps": [list(axes)]}).resolve(spec)
        assert (m.axes, m.stride, m.len) == (axes, stride, ln)
        idx = np.arange(1155)
        ijkl = np.unravel_index(idx, (3, 5, 7, 11))
        pos = [("beta_over_H", "I_p", "v_w", "delta_LZ").index(a) for a in axes]
        cell = ijkl[pos[0]] if len(axes) == 1 else ijkl[pos[0]] * ln[1] + ijkl[pos[1]]
        assert np.array_equal(m.cell(idx), cell)


# ---- the sweep driver with a fit, on CPU tensors ------------------------------------------------
def fake_compute(start, n, out):
    idx = torch.arange(start, start + n, dtype=torch.float64)
    out.copy_(torch.stack([idx * k + 0.25 for k in range(1, 7)], dim=1))


TOTAL, CHUNK = 1001, 97     # 7 x 11 x 13 grid; three uneven shards [0, 333), [333, 667), [667, 1001)
MK = lambda n: torch.empty((n, 6), dtype=torch.float64)


def driver_fit():
    # Y_B = idx + 0.25: rows 332 (rank 0) and 333 (rank 1) tie exactly at d = -+0.25
    return F.FitSpec.from_json({"terms": [{"field": "Y_B", "target": 332.75, "sigma": 2.0}],
                                "levels": [0.0625, 100.0], "maps": [["beta_over_H", "I_p"], ["v_w"], ["v_w", "I_p"]],
                                "select": {"level": 900.0, "cap": 50}})


def driver_reference():
    fit = driver_fit()
    maps = fit.resolve(spec_of((7, 11, 13), ("beta_over_H", "I_p", "v_w")))
    table = MK(TOTAL)
    fake_compute(0, TOTAL, table)
    h = F.HostFit(fit, maps)
    h.update(table.numpy(), 0)
    return fit, maps, h.result()


def test_run_local_with_fit_single_process_and_resumed(tmp_path):
    sw = pkg("sweep")
    fit, maps, ref = driver_reference()
    assert ref["best"] == {"chi2": 0.0625, "index": 332} and ref["n_within"][0] == 2
    assert ref["n_selected"] == 120 and ref["selected"].tolist() == list(range(273, 323))
    acc = F.make_accumulator(fit, maps)
    table = sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, str(tmp_path), fit=acc)
    assert table.shape == (TOTAL, 6) and F.differences(F.combine(acc), ref) == []

    def boom(*a):
        raise AssertionError("recomputed a checkpointed chunk")
    acc = F.make_accumulator(fit, maps)
    again = sw.run_local(boom, 0, TOTAL, MK, CHUNK, str(tmp_path), resume=True, fit=acc)
    assert torch.equal(again, table) and F.differences(acc.result(), ref) == []
    # fit only: two chunk-sized buffers, nothing returned, nothing written
    acc = F.make_accumulator(fit, maps)
    made = []
    out = tmp_path / "none"
    assert sw.run_local(fake_compute, 0, TOTAL, lambda n: (made.append(n), MK(n))[1], CHUNK, str(out), fit=acc,
                        keep_table=False) is None
    assert made == [2 * CHUNK] and not out.exists() and F.differences(acc.result(), ref) == []
    with pytest.raises(ValueError, match="resume"):
        sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, str(out), resume=True, fit=acc, keep_table=False)
    with pytest.raises(ValueError, match="needs a fit"):
        sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, keep_table=False)
    # the report: best point's axis values and its yields evaluated again through compute
    spec = spec_of((7, 11, 13), ("beta_over_H", "I_p", "v_w"))
    rep = F.report(fit, ref, spec, TOTAL, F.best_point_yields(fake_compute, 332, MK))
    assert rep["best"]["index"] == 332 and rep["best"]["params"] == spec.point_params(332)
    assert list(rep["best"]["final"].values()) == table[332].tolist()
    json.dumps(rep)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, keep_table):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sw = pkg("sweep")
    fit, maps, ref = driver_reference()
    s, e = sw.shard_range(TOTAL, rank, world)
    acc = F.make_accumulator(fit, maps)
    sw.run_local(fake_compute, s, e, MK, CHUNK, fit=acc, keep_table=keep_table)
    diff = F.differences(F.combine(acc, world), ref)
    with open(os.path.join(out_dir, f"diff.{rank}.json"), "w") as f:
        json.dump(diff, f)
    dist.destroy_process_group()


@pytest.mark.parametrize("keep_table", [True, False])
def test_three_gloo_ranks_combine_to_the_one_pass_fit(keep_table):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(3, free_port(), d, keep_table), nprocs=3, join=True)
        for r in range(3):
            with open(os.path.join(d, f"diff.{r}.json")) as f:
                assert json.load(f) == [], r


# ---- C ABI: every validation error is LZQ_EINVAL with a message, before any GPU work ------------
def test_capi_fit_validation():
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

    def update(t, nt, lv, nl, m, nm):
        return L.lzq_fit_update(t, nt, lv, nl, m, nm, 8, 0, 1, 8, None)

    def expect(rc, msg):
        assert rc == -1 and msg in L.lzq_last_error(), (rc, msg, L.lzq_last_error())
    expect(update(terms(*[(0, 1.0, 1.0)] * 4), 5, levels(), 0, good_m, 0), b"5 terms")
    expect(update(good_t, 0, levels(), 0, good_m, 0), b"0 terms")
    expect(update(good_t, 1, levels(1, 2, 3, 4), 5, good_m, 0), b"5 levels")
    expect(update(good_t, 1, levels(), 0, maps(*[[(1, 4)]] * 4), 5), b"5 maps")
    expect(update(terms((6, 1.0, 1.0)), 1, levels(), 0, good_m, 0), b"unknown field")
    for s in (0.0, -2.0, INF, NAN):
        expect(update(terms((0, 1.0, s)), 1, levels(), 0, good_m, 0), b"sigma")
    for t in (NAN, INF, -INF):
        expect(update(terms((0, t, 1.0)), 1, levels(), 0, good_m, 0), b"target")
    expect(update(good_t, 1, levels(2.0, 1.0), 2, good_m, 0), b"ascending")
    expect(update(good_t, 1, levels(1.0, NAN), 2, good_m, 0), b"ascending")
    expect(update(good_t, 1, levels(), 0, maps([(1, 4097), (4097, 4096)]), 1), b"2^24 cells")
    expect(update(good_t, 1, levels(), 0, maps([(1, (1 << 24) + 1)]), 1), b"2^24 cells")
    three = maps([(1, 3), (3, 3)])
    three[0].n_axes = 3
    expect(update(good_t, 1, levels(), 0, three, 1), b"axes")
    expect(update(good_t, 1, levels(), 0, maps([(0, 3)]), 1), b">= 1")
    expect(L.lzq_fit_update(good_t, 1, levels(), 0, good_m, 1, 8, -1, 1, 8, None), b"bad arguments")
    expect(L.lzq_fit_update(good_t, 1, levels(), 0, good_m, 1, 8, 0, 1, None, None), b"bad arguments")
    expect(L.lzq_fit_select(good_t, 1, NAN, 8, 0, 1, 8, 8, 4, None), b"NaN")
    expect(L.lzq_fit_select(good_t, 1, 1.0, 8, 0, 1, 8, 8, -1, None), b"bad arguments")
    expect(L.lzq_fit_select(terms((0, 1.0, 0.0)), 1, 1.0, 8, 0, 1, 8, 8, 4, None), b"sigma")
    expect(L.lzq_fit_reset(good_m, 1, None, None), b"null state")
    expect(L.lzq_fit_merge(good_m, 1, 8, 8, None), b"distinct")
    expect(L.lzq_fit_merge(maps([(1, 1 << 25)]), 1, 8, 16, None), b"2^24 cells")
    assert L.lzq_fit_state_bytes(maps([(1, 1 << 25)]), 1) == -1 and b"2^24 cells" in L.lzq_last_error()
    # sizes: 32 header words + 2 per cell; empty chunks are no-ops that still validate
    assert L.lzq_fit_state_bytes(None, 0) == 32 * 8
    assert L.lzq_fit_state_bytes(maps([(77, 5), (1, 11)], [(385, 3)]), 2) == (32 + 2 * 55 + 2 * 3) * 8
    assert L.lzq_fit_state_bytes(maps([(1, 1 << 24)]), 1) == (32 + (2 << 24)) * 8
    assert L.lzq_fit_update(good_t, 1, levels(), 0, good_m, 1, None, 0, 0, 8, None) == 0
    assert L.lzq_fit_select(good_t, 1, 1.0, None, 0, 0, 8, None, 0, None) == 0
    assert n.ABI_VERSION == 3 and L.lzq_abi_version() == 3     # the new entry points are additive
