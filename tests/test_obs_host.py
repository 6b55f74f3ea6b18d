"""Sweep observables on the host: the one definition of a row's cell (csrc/lzq_obs.h, through the
library's host function lzq_obs_cells_host) and its numpy twin (fit.Observable.cell) against
literal values and against each other, the numpy state (fit.HostObservables) against literal words
on a hand-written table, its independence of chunking and merging word for word, the
"observables" key of the fit spec, quantiles and the mode, the sweep driver on CPU tensors (one
process and three gloo ranks; a numeric offset, "best" and no posterior), and the C ABI's argument
validation (which returns before any GPU work)."""
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
from obs_tables import DOWN, INF, NAN, SALTED_OBS, TERM, lin, log, salted_table

F = pkg("fit")
ONE = 1 << 62


def observables(*axes_lists):
    return F.FitSpec.from_json({"terms": [TERM], "observables": [{"axes": list(a)} for a in axes_lists]}).observables


def rows_with(**cols):
    n = len(next(iter(cols.values())))
    t = np.ones((n, 6))
    for f, v in cols.items():
        t[:, F.YIELD_FIELDS.index(f)] = v
    return t


def both(obs, k, rows):
    """The cells by numpy and by the library; they must agree before either is compared with literals."""
    a, b = obs[k].cell(rows), F.obs_cells_host(obs, k, rows)
    assert a.dtype == np.int64 and b.dtype == np.int32 and np.array_equal(a, b)
    return a.tolist()


# ---- (a) the cell against literals ---------------------------------------------------------------
def test_linear_axis_literals():
    obs = observables([lin("DM_over_B", 0.0, 8.0, 8)], [lin("DM_over_B", 0.0, 0.9, 9)], [lin("Y_chi", -2.0, 2.0, 4)])
    x = [0.0, 8.0, DOWN(8.0), 3.0, DOWN(3.0), -0.0, 5e-324, DOWN(0.0), NAN, INF, -INF, 1e300]
    assert both(obs, 0, rows_with(DM_over_B=x)) == [0, -1, 7, 3, 2, 0, 0, -1, -2, -2, -2, -1]
    # just under hi the product rounds up to bins: the clamp keeps the row in the last bin
    top = DOWN(0.9)
    assert (np.float64(top) - 0.0) * obs[1].axes[0].inv >= 9.0 and top < 0.9
    assert both(obs, 1, rows_with(DM_over_B=[top, 0.9, 0.85])) == [8, -1, 8]
    assert both(obs, 2, rows_with(Y_chi=[-2.0, DOWN(-2.0), -1.0, DOWN(-1.0), -0.0, 0.0, 1.999, 2.0])) == \
        [0, -1, 1, 0, 2, 2, 3, -1]
    assert obs[0].axes[0].edges().tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    assert obs[1].axes[0].edges()[-1] == 0.9 and obs[1].shape == (9,) and obs[1].cells == 9


def test_log_axis_literals():
    obs = observables([log("DM_over_B", 1.0, 16.0, 1)], [log("DM_over_B", 1.0, 2.0, 256)],
                      [log("DM_over_B", 1.3, 5.0, 4)], [log("DM_over_B", 5e-324, 1e-300, 1)])
    # s = 0: one bin an octave, the exponent alone
    x = [1.0, 2.0, DOWN(2.0), 15.99, 16.0, DOWN(1.0), 0.5, 0.0, -0.0, -1.0, 5e-324, NAN, INF, -INF, 4.0, 8.0]
    assert both(obs, 0, rows_with(DM_over_B=x)) == [0, 1, 0, 3, -1, -1, -1, -1, -1, -1, -1, -2, -2, -2, 2, 3]
    assert obs[0].axes[0].edges().tolist() == [1.0, 2.0, 4.0, 8.0, 16.0] and obs[0].cells == 4
    # s = 8: 256 sub-bins an octave, linear inside it
    assert obs[1].cells == 256
    x = [1.0, 1.0 + 7 / 256, DOWN(1.0 + 7 / 256), 1.0 + 255 / 256, DOWN(2.0), 2.0, 1.5]
    assert both(obs, 1, rows_with(DM_over_B=x)) == [0, 7, 6, 255, 255, -1, 128]
    # lo = 1.3 is no sub-bin edge: the range really starts at 1.25, and is reported so
    e = obs[2].axes[0].edges()
    assert e.tolist() == [1.25, 1.5, 1.75, 2.0, 2.5, 3.0, 3.5, 4.0, 5.0] and obs[2].cells == 8
    x = [1.3, 1.25, DOWN(1.25), 1.5, 3.99, 4.0, 4.99, 5.0, 2.0]
    assert both(obs, 2, rows_with(DM_over_B=x)) == [0, 0, -1, 1, 6, 7, 7, -1, 3]
    # subnormals have keys too (exponent field 0)
    assert both(obs, 3, rows_with(DM_over_B=[5e-324, 1e-310, 2.3e-308, 0.0]))[:2] == [0, 0]


def test_two_axes_and_row_classes():
    obs = observables([lin("DM_over_B", 0.0, 4.0, 4), log("Y_chi", 1.0, 4.0, 1)])
    assert obs[0].shape == (4, 2) and obs[0].cells == 8
    t = rows_with(DM_over_B=[0.5, 3.5, 3.5, 4.0, 0.5, NAN, 4.0, NAN], Y_chi=[1.0, 2.0, 3.99, 1.0, 4.0, 1.0, INF, 9.0])
    #                         (0,0) (3,1) (3,1) out  out  nonfinite: nonfinite beats out
    assert both(obs, 0, t) == [0, 7, 7, -1, -1, -2, -2, -2]


# ---- (b) numpy equals the library on many rows -----------------------------------------------------
def test_numpy_cells_equal_the_library():
    t = salted_table()
    obs = observables(*SALTED_OBS)
    assert [o.cells for o in obs] == [133, 200, 20000, obs[3].shape[0] * 9]
    for k in range(4):
        cells = np.asarray(both(obs, k, t))
        # every class occurs, and many cells
        assert (cells == -1).sum() > 100 and (cells == -2).sum() > 100 and np.unique(cells[cells >= 0]).size > 50, k
        assert cells.max() < obs[k].cells


# ---- (c) the state on a hand-written table ---------------------------------------------------------
# chi2 = ((Y_B - 1) / 0.5)^2; observable 0: DM_over_B in 4 bins of [0, 4); observable 1: that times Y_chi in
# the octaves [1, 2), [2, 4).  At offset 1:
#   row  Y_B    DM_over_B  Y_chi  chi2   obs 0          obs 1
#   0    1.5    0.5        1.0    1      cell 0, 2^62   cell 0
#   1    1.0    0.5        2.0    0      cell 0, above  cell 1
#   2    nan    0.5        1.0           invalid
#   3    2.0    1.5        3.0    4      cell 1, q3     cell 3
#   4    0.5    3.99       1.5    1      cell 3, 2^62   cell 6
#   5    6.0    2.0        1.0    100    cell 2, zero   cell 4
#   6    1e200  1.0        1.0    inf    invalid
#   7    1.5    4.0        1.0    1      out            out
#   8    1.5    -1.0       1.0    1      out            out
#   9    1.5    nan        1.0    1      nonfinite      nonfinite
#   10   1.5    inf        1.0    1      nonfinite      nonfinite
#   11   1.5    1.0        8.0    1      cell 1, 2^62   out
def literal():
    t = rows_with(Y_B=[1.5, 1.0, NAN, 2.0, 0.5, 6.0, 1e200, 1.5, 1.5, 1.5, 1.5, 1.5],
                  DM_over_B=[0.5, 0.5, 0.5, 1.5, 3.99, 2.0, 1.0, 4.0, -1.0, NAN, INF, 1.0],
                  Y_chi=[1.0, 2.0, 1.0, 3.0, 1.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 8.0])
    fit = F.FitSpec.from_json({"terms": [TERM], "observables": [
        {"axes": [lin("DM_over_B", 0.0, 4.0, 4)]},
        {"axes": [lin("DM_over_B", 0.0, 4.0, 4), log("Y_chi", 1.0, 4.0, 1)]}]})
    return t, fit


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("weighted", [True, False])
def test_state_literals(weighted):
    t, fit = literal()
    h = F.HostObservables(fit, fit.observables, 1.0 if weighted else None)
    h.update(t)
    q3 = int(F.post_weights(fit, 1.0, t[3:4])[0])
    assert abs(q3 - 1029006239845977778) <= 2 ** 16          # floor(exp(-3/2) 2^62), to the weight's accuracy
    pair = lambda v: [v >> 31, v & 0x7FFFFFFF]
    zero = [0, 0]
    w = h.w.tolist()
    assert len(w) == F.obs_state_words(fit.observables) == (4 + 16) + (4 + 32) and h.rows == 12
    # observable 0: header, 4 pairs, 4 counts, 4 chi2
    assert w[0:4] == [6, 2, 2, 0]
    w0 = [pair(ONE), pair(q3 + ONE), zero, pair(ONE)] if weighted else [zero] * 4
    assert w[4:12] == sum(w0, [])
    assert w[12:16] == [2, 2, 1, 1]
    assert w[16:20] == bits([0.0, 1.0, 100.0, 1.0])
    # observable 1: 8 cells
    assert w[20:24] == [5, 3, 2, 0]
    w1 = [zero] * 8
    if weighted:
        w1 = [pair(ONE), zero, zero, pair(q3), zero, zero, pair(ONE), zero]
    assert w[24:40] == sum(w1, [])
    assert w[40:48] == [1, 1, 0, 1, 1, 0, 1, 0]
    assert w[48:56] == bits([1.0, 0.0, INF, 4.0, 100.0, INF, 1.0, INF])
    res = h.result()
    assert [r["n_in"] for r in res] == [6, 5] and res[0]["count"].tolist() == [2, 2, 1, 1]
    assert res[1]["count"].shape == (4, 2) and res[1]["chi2_min"][1].tolist() == [INF, 4.0]
    assert res[0]["weighted"] is weighted and res[0]["offset"] == (1.0 if weighted else None)
    if weighted:
        tot = 3 * ONE + q3
        assert res[0]["total_units"] == str(tot) and res[1]["total_units"] == str(2 * ONE + q3)
        assert res[0]["posterior"].tolist() == [float(ONE) / float(tot), float(ONE + q3) / float(tot), 0.0,
                                                float(ONE) / float(tot)]
        assert res[0]["mode"] == {"bin": 1, "lo": 1.0, "hi": 2.0}
        assert res[0]["in_range_share"] is None and h.result(2 * tot)[0]["in_range_share"] == 0.5
        assert res[1]["quantiles"] is None and res[1]["mode"] is None
    else:
        assert res[0]["total_units"] == "0" and np.isnan(res[0]["posterior"]).all()
        assert res[0]["quantiles"] is None and res[0]["mode"] is None
    again = F.HostObservables.from_words(fit, fit.observables, h.offset, h.to_words())
    assert again.rows == 10 and F.obs_differences(again.result(), res) == []    # the valid rows
    assert h.to_words().dtype == np.int64


def test_row_limit_and_merge_refusals():
    t, fit = literal()
    h = F.HostObservables(fit, fit.observables, 1.0)
    h.rows = (1 << 32) - 7
    with pytest.raises(ValueError, match="2\\^32 rows"):
        h.update(t)
    other = F.HostObservables(fit, fit.observables, 1.0)
    other.update(t)
    with pytest.raises(ValueError, match="2\\^32 rows"):
        h.merge(other)
    with pytest.raises(ValueError, match="offsets"):
        F.HostObservables(fit, fit.observables, None).merge(other)
    with pytest.raises(ValueError, match="finite"):
        F.HostObservables(fit, fit.observables, -1.0)
    with pytest.raises(ValueError, match="words"):
        F.HostObservables.from_words(fit, fit.observables, 1.0, np.zeros(5, dtype=np.int64))


# ---- (d) chunking and merging ----------------------------------------------------------------------
@pytest.mark.parametrize("offset", [None, 0.0, 40.0])
def test_chunking_and_merging_are_bitwise_invisible(offset):
    n = 1001
    t = salted_table(n, 5)
    fit = F.FitSpec.from_json({"terms": [TERM], "observables": [{"axes": list(a)} for a in SALTED_OBS]})
    obs = fit.observables
    one = F.HostObservables(fit, obs, offset)
    one.update(t)
    assert one.w[0] > 100 and one.w[1] > 50 and one.w[2] > 10
    for order in (1, -1):
        h = F.HostObservables(fit, obs, offset)
        for a in list(range(0, n, 97))[::order]:
            h.update(t[a:a + 97])
        assert np.array_equal(h.to_words(), one.to_words()), order
    tot = F.HostObservables(fit, obs, offset)
    for a, b in ((700, n), (0, 1), (1, 700)):
        part = F.HostObservables(fit, obs, offset)
        part.update(t[a:b])
        tot.merge(F.HostObservables.from_words(fit, obs, offset, part.to_words()))
    assert np.array_equal(tot.to_words(), one.to_words())
    res = one.result()
    for r in res:       # the counts hold every in-range row; with weight, the cells hold the whole of it
        assert int(r["count"].sum()) == r["n_in"]
        assert (int(r["total_units"]) > 0) == (offset is not None)
        assert np.array_equal(np.isfinite(r["chi2_min"]), r["count"] > 0)


# ---- (e) the spec key --------------------------------------------------------------------------------
def test_observables_spec_parsing_and_round_trip():
    base = {"terms": [TERM], "levels": [1.0], "maps": [["v_w"]]}
    plain = F.FitSpec.from_json(base)
    assert plain.observables == [] and plain.to_json() == {"terms": [TERM], "levels": [1.0], "maps": [["v_w"]]}
    assert "observables" not in F.FitSpec.from_json({**base, "observables": []}).to_json()
    issue = [{"axes": [log("DM_over_B", 0.01, 1000.0, 8)]},
             {"axes": [lin("Y_B", 0.0, 2e-10, 200), lin("DM_over_B", 0.0, 10.0, 100)], "quantiles": [0.16, 0.5, 0.84]}]
    s = F.FitSpec.from_json({**base, "observables": issue, "posterior": {"offset": 3}})
    assert [o.cells for o in s.observables] == [133, 20000]
    assert s.observables[0].quantiles == (0.025, 0.16, 0.5, 0.84, 0.975) and s.observables[1].quantiles == (0.16, 0.5, 0.84)
    j = s.to_json()
    assert j["observables"][0] == {"axes": [log("DM_over_B", 0.01, 1000.0, 8)], "quantiles": [0.025, 0.16, 0.5, 0.84, 0.975]}
    assert j["observables"][1] == issue[1] and list(j)[-1] == "observables"
    again = F.FitSpec.from_json(json.loads(json.dumps(j)))
    assert again.to_json() == j and again.observables == s.observables
    a = lin("Y_B", 0.0, 1.0, 4)
    bad = [3, "x", {"axes": [a]}, [3], [{"axes": a}], [{"axes": []}], [{"axes": [a, a, a]}], [{"axes": [a, a]}],
           [{"axes": [a], "bins": 3}], [{"axes": ["Y_B"]}], [{"axes": [{"field": "Y_B", "lo": 0.0, "hi": 1.0}]}],
           [{"axes": [{**a, "per_octave": 2}]}], [{"axes": [{**a, "field": "nope"}]}], [{"axes": [{**a, "field": 3}]}],
           [{"axes": [{**a, "extra": 1}]}], [{"axes": [{"lo": 0.0, "hi": 1.0, "bins": 2}]}],
           [{"axes": [lin("Y_B", 1.0, 1.0, 4)]}], [{"axes": [lin("Y_B", 2.0, 1.0, 4)]}], [{"axes": [lin("Y_B", NAN, 1.0, 4)]}],
           [{"axes": [lin("Y_B", 0.0, INF, 4)]}], [{"axes": [lin("Y_B", "0", 1.0, 4)]}], [{"axes": [lin("Y_B", True, 2.0, 4)]}],
           [{"axes": [lin("Y_B", -1e308, 1e308, 4)]}], [{"axes": [lin("Y_B", 0.0, 5e-324, 4)]}],
           [{"axes": [lin("Y_B", 0.0, 1.0, 0)]}], [{"axes": [lin("Y_B", 0.0, 1.0, 2.5)]}], [{"axes": [lin("Y_B", 0.0, 1.0, True)]}],
           [{"axes": [lin("Y_B", 0.0, 1.0, (1 << 20) + 1)]}],
           [{"axes": [lin("Y_B", 0.0, 1.0, 1025), lin("Y_chi", 0.0, 1.0, 1024)]}],
           [{"axes": [log("Y_B", 0.0, 1.0, 2)]}], [{"axes": [log("Y_B", -1.0, 1.0, 2)]}], [{"axes": [log("Y_B", 1.0, 2.0, 3)]}],
           [{"axes": [log("Y_B", 1.0, 2.0, 512)]}], [{"axes": [log("Y_B", 1.0, 2.0, 0)]}], [{"axes": [log("Y_B", 1.0, 2.0, 2.0)]}],
           [{"axes": [log("Y_B", 1.0, 1.5, 1)]}],
           [{"axes": [a], "quantiles": [0.5, 0.4]}], [{"axes": [a], "quantiles": [0.0]}], [{"axes": [a], "quantiles": [1.0]}],
           [{"axes": [a], "quantiles": [NAN]}], [{"axes": [a], "quantiles": 0.5}], [{"axes": [a], "quantiles": ["x"]}],
           [{"axes": [a]}] * 5]
    for o in bad:
        with pytest.raises(ValueError, match="observables"):
            F.FitSpec.from_json({**base, "observables": o})
    # the limits themselves are fine
    ok = F.FitSpec.from_json({**base, "observables": [{"axes": [lin("Y_B", 0.0, 1.0, 1024), lin("Y_chi", 0.0, 1.0, 1024)],
                                                       "quantiles": []}] * 4})
    assert ok.observables[3].cells == 1 << 20 and F.obs_state_words(ok.observables) == 4 * (4 + (4 << 20))
    with pytest.raises(ValueError, match="unknown fit-spec keys"):
        F.FitSpec.from_json({**base, "observable": []})
    # "observables" does not go inside "posterior"
    with pytest.raises(ValueError, match="posterior"):
        F.FitSpec.from_json({**base, "posterior": {"observables": issue}})


# ---- (f) quantiles, the mode, an empty state ---------------------------------------------------------
def test_quantiles_mode_and_empty_state():
    fit = F.FitSpec.from_json({"terms": [TERM], "observables": [
        {"axes": [lin("DM_over_B", 0.0, 8.0, 4)], "quantiles": [0.0625, 0.1, 0.125, 0.25, 0.5, 0.999]}]})
    h = F.HostObservables(fit, fit.observables, 0.0)
    empty = h.result()[0]
    assert empty["quantiles"] == [{"p": p, "bin": None, "lo": None, "hi": None} for p in fit.observables[0].quantiles]
    assert empty["mode"] is None and np.isnan(empty["posterior"]).all() and empty["total_units"] == "0"
    assert np.isinf(empty["chi2_min"]).all() and (empty["n_in"], empty["n_out"], empty["n_nonfinite"]) == (0, 0, 0)
    json.dumps(F.report(fit, {**F.HostFit(fit, []).result(), "observables": h.result()},
                        pkg("sweep").SweepSpec("t", {}, []), 0, None)["observables"])
    # weights 1, 2, 3, 4 (in units of 2^62, split over hi and lo words as a sum of many rows would)
    for b, v in enumerate([1, 2, 3, 4]):
        h.w[4 + 2 * b], h.w[4 + 2 * b + 1] = (v * ONE >> 31) - 1, 1 << 31
    r = h.result()[0]
    assert r["total_units"] == str(10 * ONE) and r["posterior"].tolist() == [0.1, 0.2, 0.3, 0.4]
    # cumulated 1, 3, 6, 10 of 10: the first bin with cum >= p * 10, exactly (0.1 as a double is above 1/10)
    assert [q["bin"] for q in r["quantiles"]] == [0, 1, 1, 1, 2, 3]
    assert r["quantiles"][4] == {"p": 0.5, "bin": 2, "lo": 4.0, "hi": 6.0} and r["mode"] == {"bin": 3, "lo": 6.0, "hi": 8.0}
    # a tie: the lowest bin of greatest weight
    h.w[4:12] = [4, 0, 1, 0, 4, 0, 0, 0]
    assert h.result()[0]["mode"]["bin"] == 0


# ---- (g), (h) the sweep driver on CPU tensors ---------------------------------------------------------
def fake_compute(start, n, out):
    idx = torch.arange(start, start + n, dtype=torch.float64)
    out.copy_(torch.stack([idx * k * 0.015625 + 0.25 for k in range(1, 7)], dim=1))


TOTAL, CHUNK = 1001, 97     # 7 x 11 x 13 grid; three uneven shards
MK = lambda n: torch.empty((n, 6), dtype=torch.float64)
DRIVER_OBS = [{"axes": [log("DM_over_B", 0.5, 64.0, 4)], "quantiles": [0.16, 0.5, 0.84]},
              {"axes": [lin("Y_B", 0.0, 10.0, 20), lin("Y_chi", 0.0, 16.0, 8)]}]


def spec_of(lens, names=("beta_over_H", "I_p", "v_w")):
    sw = pkg("sweep")
    return sw.SweepSpec("t", dict(sw.EQUAL_MASS), [(n, np.linspace(0.1, 0.9, k)) for n, k in zip(names, lens)])


def driver(offset):
    """Y_B = idx / 64 + 0.25, target 5.5, sigma 0.5: chi2 = ((idx - 336) / 32)^2; offset None: no posterior."""
    d = {"terms": [{"field": "Y_B", "target": 5.5, "sigma": 0.5}], "levels": [1.0, 30.0], "maps": [["v_w"]],
         "observables": DRIVER_OBS}
    if offset is not None:
        d["posterior"] = {"offset": offset}
    fit = F.FitSpec.from_json(d)
    spec = spec_of((7, 11, 13))
    table = MK(TOTAL)
    fake_compute(0, TOTAL, table)
    off = {None: None, "best": 0.0}.get(offset, offset)
    z = None
    if off is not None:
        p = F.HostPosterior(fit, fit.resolve(spec), off, fit.axis_values(spec))
        p.update(table.numpy(), 0)
        z = int(p.result()["Z_units"])
    o = F.HostObservables(fit, fit.observables, off)
    o.update(table.numpy())
    return fit, spec, o.result(z)


@pytest.mark.parametrize("offset", [2.0, "best", None])
def test_run_local_with_observables_single_process(tmp_path, offset):
    sw = pkg("sweep")
    fit, spec, oref = driver(offset)
    assert oref[0]["n_in"] > 500 and oref[0]["n_out"] > 10 and oref[1]["n_out"] > 100
    assert oref[0]["weighted"] == (offset is not None)
    if offset is not None:
        assert 0.5 < oref[1]["in_range_share"] <= 1.0 and oref[0]["quantiles"][1]["bin"] is not None
    acc = F.make_accumulator(fit, fit.resolve(spec), None, fit.axis_values(spec))
    table = sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, str(tmp_path), fit=acc)
    res = F.combine(acc, local=table, start=0)
    assert F.obs_differences(res["observables"], oref) == []
    # resumed chunks are folded too
    acc = F.make_accumulator(fit, fit.resolve(spec), None, fit.axis_values(spec))
    again = sw.run_local(lambda *a: 1 / 0, 0, TOTAL, MK, CHUNK, str(tmp_path), resume=True, fit=acc)
    assert F.obs_differences(F.combine(acc, local=again, start=0)["observables"], oref) == []
    # fit only: no table is needed, except by "best" (the existing refusal)
    acc = F.make_accumulator(fit, fit.resolve(spec), None, fit.axis_values(spec))
    assert sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, fit=acc, keep_table=False) is None
    if offset == "best":
        with pytest.raises(ValueError, match="give a number"):
            F.combine(acc)
    else:
        assert F.obs_differences(F.combine(acc)["observables"], oref) == []
    # the report and the files
    rep = F.report(fit, res, spec, TOTAL, None)
    json.dumps(rep)
    assert [o["axes"] for o in rep["spec"]["observables"]] == [o["axes"] for o in DRIVER_OBS]
    assert len(rep["observables"]) == 2 and rep["observables"][1]["shape"] == [20, 8]
    assert rep["observables"][0]["n_in"] == oref[0]["n_in"] and rep["observables"][0]["quantiles"] == oref[0]["quantiles"]
    assert rep["observables"][0]["range"] == [[0.5, 64.0]] and rep["observables"][0]["total_units"] == oref[0]["total_units"]
    if offset is not None:
        assert "observables" not in rep["posterior"]
    out = tmp_path / "files"
    out.mkdir()
    F.write_files(str(out), rep, res)
    assert sorted(os.listdir(out)) == ["fit.json", "fit_maps.npz", "fit_obs.npz", "selected.npy"]
    z = np.load(out / "fit_obs.npz")
    assert set(z.files) == {f"obs{k}_{s}" for k in (0, 1) for s in ("weight", "count", "chi2_min", "posterior", "edges0")} | \
        {"obs1_edges1"}
    assert z["obs1_count"].shape == (20, 8) and z["obs1_weight"].shape == (160, 2) and z["obs1_weight"].dtype == np.uint64
    assert np.array_equal(z["obs0_weight"], oref[0]["weight"]) and np.array_equal(z["obs0_count"], oref[0]["count"])
    assert np.array_equal(z["obs0_edges0"], fit.observables[0].axes[0].edges()) and z["obs1_edges1"].size == 9
    with open(out / "fit.json") as f:
        assert json.load(f)["observables"][0]["n_in"] == oref[0]["n_in"]


def test_without_the_key_nothing_changes(tmp_path):
    sw = pkg("sweep")
    fit, spec, _ = driver(2.0)
    plain = F.FitSpec.from_json({k: v for k, v in fit.to_json().items() if k != "observables"})
    acc = F.make_accumulator(plain, plain.resolve(spec), None, plain.axis_values(spec))
    table = sw.run_local(fake_compute, 0, TOTAL, MK, CHUNK, fit=acc)
    res = F.combine(acc, local=table, start=0)
    assert "observables" not in res and acc.obs is None
    rep = F.report(plain, res, spec, TOTAL, None)
    assert "observables" not in rep and "observables" not in rep["spec"]
    F.write_files(str(tmp_path), rep, res)
    assert sorted(os.listdir(tmp_path)) == ["fit.json", "fit_maps.npz", "selected.npy"]


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
    fit, spec, oref = driver(offset)
    s, e = sw.shard_range(TOTAL, rank, world)
    acc = F.make_accumulator(fit, fit.resolve(spec), None, fit.axis_values(spec))
    local = sw.run_local(fake_compute, s, e, MK, CHUNK, fit=acc)
    res = F.combine(acc, world, local=local, start=s)
    with open(os.path.join(out_dir, f"diff.{rank}.json"), "w") as f:
        json.dump(F.obs_differences(res["observables"], oref), f)
    dist.destroy_process_group()


@pytest.mark.parametrize("offset", [2.0, "best", None])
def test_three_gloo_ranks_combine_to_the_one_pass_observables(offset):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(3, free_port(), d, offset), nprocs=3, join=True)
        for r in range(3):
            with open(os.path.join(d, f"diff.{r}.json")) as f:
                assert json.load(f) == [], r


# ---- (i) C ABI: every validation error is LZQ_EINVAL with a message, before any GPU work ------------
def test_capi_obs_validation():
    n = pkg("_native")
    L = n.load()

    def terms(*ts):
        arr = (n.LzqFitTerm * max(1, len(ts)))()
        for k, (f, t, s) in enumerate(ts):
            arr[k].field, arr[k].target, arr[k].sigma = f, t, s
        return arr

    def obs(*os_):
        """each observable a list of axes (field, kind, lo, hi, bins, log2_sub)"""
        arr = (n.LzqObs * max(1, len(os_)))()
        for k, axes in enumerate(os_):
            arr[k].n_axes = len(axes)
            for a, v in enumerate(axes[:2]):
                c = arr[k].axes[a]
                c.field, c.kind, c.lo, c.hi, c.bins, c.log2_sub = v
        return arr

    good_t = terms((0, 1.0, 1.0))
    LIN, LOG = (4, 0, 0.0, 4.0, 4, 0), (1, 1, 1.0, 4.0, 0, 0)
    good_o = obs([LIN])

    def update(t, nt, o, no, weighted=0, offset=0.0, y=8, count=1, st=8):
        return L.lzq_obs_update(t, nt, o, no, weighted, offset, y, count, st, None)

    def expect(rc, msg):
        assert rc == -1 and msg in L.lzq_last_error(), (rc, msg, L.lzq_last_error())
    expect(update(None, 1, good_o, 1), b"null terms")
    expect(update(good_t, 0, good_o, 1), b"0 terms")
    expect(update(terms((6, 1.0, 1.0)), 1, good_o, 1), b"unknown field")
    expect(update(good_t, 1, None, 1), b"null observables")
    expect(update(good_t, 1, obs(*[[LIN]] * 4), 5), b"5 observables")
    expect(update(good_t, 1, good_o, -1), b"-1 observables")
    expect(update(good_t, 1, obs([]), 1), b"1 or 2 axes")
    expect(update(good_t, 1, obs([LIN, LOG, LOG]), 1), b"1 or 2 axes")
    expect(update(good_t, 1, obs([LIN, LIN]), 1), b"two axes over one field")
    expect(update(good_t, 1, obs([(6, 0, 0.0, 4.0, 4, 0)]), 1), b"unknown field")
    expect(update(good_t, 1, obs([(-1, 0, 0.0, 4.0, 4, 0)]), 1), b"unknown field")
    expect(update(good_t, 1, obs([(4, 2, 0.0, 4.0, 4, 0)]), 1), b"unknown kind")
    for lo, hi in ((4.0, 4.0), (5.0, 4.0), (NAN, 4.0), (0.0, INF), (-INF, 0.0)):
        expect(update(good_t, 1, obs([(4, 0, lo, hi, 4, 0)]), 1), b"lo < hi")
        expect(update(good_t, 1, obs([(4, 1, lo, hi, 0, 2)]), 1), b"lo < hi")
    expect(update(good_t, 1, obs([(4, 0, 0.0, 4.0, 0, 0)]), 1), b"bins")
    expect(update(good_t, 1, obs([(4, 0, -1e308, 1e308, 4, 0)]), 1), b"finite and > 0")
    expect(update(good_t, 1, obs([(4, 0, 0.0, 5e-324, 4, 0)]), 1), b"finite and > 0")
    expect(update(good_t, 1, obs([(4, 1, 0.0, 4.0, 0, 2)]), 1), b"lo > 0")
    expect(update(good_t, 1, obs([(4, 1, -1.0, 4.0, 0, 2)]), 1), b"lo > 0")
    expect(update(good_t, 1, obs([(4, 1, 1.0, 4.0, 0, 9)]), 1), b"log2_sub")
    expect(update(good_t, 1, obs([(4, 1, 1.0, 4.0, 0, -1)]), 1), b"log2_sub")
    expect(update(good_t, 1, obs([(4, 1, 1.0, 1.5, 0, 0)]), 1), b"at least one sub-bin")
    expect(update(good_t, 1, obs([(4, 0, 0.0, 1.0, (1 << 20) + 1, 0)]), 1), b"2^20 cells")
    expect(update(good_t, 1, obs([(4, 0, 0.0, 1.0, 1025, 0), (1, 0, 0.0, 1.0, 1024, 0)]), 1), b"2^20 cells")
    for off in (-1.0, NAN, INF):
        expect(update(good_t, 1, good_o, 1, 1, off), b"offset must be finite and >= 0")
        assert update(good_t, 1, good_o, 1, 0, off, None, 0) == 0        # unweighted: the offset is not looked at
    expect(update(good_t, 1, good_o, 1, y=None), b"bad arguments")
    expect(update(good_t, 1, good_o, 1, st=None), b"bad arguments")
    expect(update(good_t, 1, good_o, 1, count=-1), b"bad arguments")
    expect(update(good_t, 1, good_o, 1, count=(1 << 32) + 1), b"2^32 rows")
    expect(L.lzq_obs_reset(good_o, 1, None, None), b"null state")
    expect(L.lzq_obs_reset(obs([LIN, LIN]), 1, 8, None), b"two axes")
    expect(L.lzq_obs_merge(good_o, 1, 8, 8, None), b"distinct")
    expect(L.lzq_obs_merge(good_o, 1, None, 8, None), b"distinct")
    expect(L.lzq_obs_cells_host(good_o, 1, 1, None, 0, None), b"bad arguments")
    expect(L.lzq_obs_cells_host(good_o, 1, 0, None, 1, None), b"bad arguments")
    expect(L.lzq_obs_cells_host(obs([(4, 1, 0.0, 4.0, 0, 2)]), 1, 0, None, 0, None), b"lo > 0")
    assert L.lzq_obs_state_bytes(obs([(4, 0, 0.0, 1.0, (1 << 20) + 1, 0)]), 1) == -1 and b"2^20 cells" in L.lzq_last_error()
    # sizes: 4 header words and 4 words a cell per observable; empty calls are no-ops that still validate
    assert L.lzq_obs_state_bytes(None, 0) == 0
    assert L.lzq_obs_state_bytes(good_o, 1) == (4 + 16) * 8
    assert L.lzq_obs_state_bytes(obs([LIN, LOG], [(4, 1, 0.01, 1000.0, 0, 3)]), 2) == (4 + 4 * 8 + 4 + 4 * 133) * 8
    assert L.lzq_obs_state_bytes(obs([(4, 0, 0.0, 1.0, 1024, 0), (1, 0, 0.0, 1.0, 1024, 0)]), 1) == (4 + (4 << 20)) * 8
    assert update(good_t, 1, good_o, 1, y=None, count=0) == 0
    assert update(good_t, 1, None, 0, y=8, count=1) == 0
    assert L.lzq_obs_cells_host(good_o, 1, 0, None, 0, None) == 0
    assert n.ABI_VERSION == 3 and L.lzq_abi_version() == 3     # additive entry points
    assert (n.OBS_MAX, n.OBS_MAX_CELLS, n.OBS_HEADER_WORDS) == (4, 1 << 20, 4) and 1 <= n.OBS_LDS_CELLS <= 2040
    assert F.obs_state_words(observables([lin("DM_over_B", 0.0, 4.0, 4)])) * 8 == (4 + 16) * 8
