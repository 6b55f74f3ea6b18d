"""The source activity window W(y) on the host (include/lzq.h lzq_window, csrc/lzq_window.h): the
library's host build against a numpy statement of the definition, operation for operation; every
refusal; and the headline kernels' machine code, which the window must not move.  No GPU.

The exponential's bound is libm's: glibc documents exp within 1 ulp, so W is held to 1 ulp of
mpmath's exp at the host's own q (the ulp of the exact value; the subnormal spacing below 2^-1022).
"""
import json
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

NEUTRAL = {"y0": 0.0, "half_width": 0.0, "sigma_lo": 1.0, "sigma_hi": 1.0, "scale": 1.0, "table": 0}


def win(kind, **kw):
    return dict(NEUTRAL, kind=kind, **kw)


def around(x, k=1):
    """x and its k neighbours on either side."""
    out = [float(x)]
    lo = hi = float(x)
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [float(lo), float(hi)]
    return out


def q_numpy(w, y):
    """q of the Gaussian kinds, one numpy operation per IEEE operation of the definition."""
    y = np.asarray(y, dtype=np.float64)
    if w["kind"] == "gauss":
        return y * (1.0 / max(w["sigma_hi"], 1e-6))
    u = y - w["y0"]
    d = np.maximum(np.abs(u) - w["half_width"], 0.0)
    return d * np.where(u < 0.0, 1.0 / max(w["sigma_lo"], 1e-6), 1.0 / max(w["sigma_hi"], 1e-6))


def table_numpy(w, u, W, y):
    """(v, W(v)) of the table kind: linear on [u_k, u_{k+1}), the end values outside."""
    u, W = np.asarray(u, dtype=np.float64), np.asarray(W, dtype=np.float64)
    v = (np.asarray(y, dtype=np.float64) - w["y0"]) / w["scale"]
    k = np.clip(np.searchsorted(u, v, side="right") - 1, 0, u.size - 2)
    lin = W[k] + (v - u[k]) * ((W[k + 1] - W[k]) / (u[k + 1] - u[k]))
    return v, np.where(v < u[0], W[0], np.where(v >= u[-1], W[-1], lin))


def exp_ulps(got, q):
    """|got - exp(-q^2/2)| in ulps of the exact value, by mpmath at 60 digits."""
    import mpmath
    mpmath.mp.dps = 60
    x = -0.5 * (q * q)                       # the library's argument, one rounding per operation
    exact = mpmath.exp(mpmath.mpf(float(x)))
    ulp = math.ulp(max(float(exact), 2.0 ** -1022))
    return float(abs(mpmath.mpf(float(got)) - exact) / ulp)


GAUSS_KINDS = [
    win("gauss", sigma_hi=9.0),
    win("gauss", sigma_hi=1e-9),                       # the 1e-6 clamp
    win("plateau", sigma_lo=7.0, sigma_hi=7.0),
    win("plateau", y0=2.0, half_width=10.0, sigma_lo=1e-3, sigma_hi=1e-3),
    win("plateau", y0=-10.0, half_width=4.0, sigma_lo=3.0, sigma_hi=12.0),
    win("plateau", y0=70.0, half_width=0.5, sigma_lo=15.0, sigma_hi=2.0),
    win("plateau", half_width=200.0),
]


def edge_ys(w):
    """The y range of the shipped config, coarse, plus an ulp either side of u = 0 and |u| = half_width."""
    ys = list(np.linspace(-80.0, 50.0, 261))
    for c in (w["y0"], w["y0"] - w["half_width"], w["y0"] + w["half_width"]):
        ys += around(c, 2)
        ys += [c - 1e-3, c + 1e-3, c - 4e-2, c + 4e-2]
    return np.array(ys)


@pytest.mark.parametrize("w", GAUSS_KINDS, ids=lambda w: f"{w['kind']}-{w['y0']}-{w['half_width']}-{w['sigma_hi']}")
def test_gauss_kinds_q_bit_equal_and_W_within_libm(w):
    ys = edge_ys(w)
    q, W = pkg("window").eval_host(w, ys)
    ref = q_numpy(w, ys)
    assert np.array_equal(q, ref), (ys[q != ref], q[q != ref], ref[q != ref])
    worst = max(exp_ulps(Wi, qi) for Wi, qi in zip(W, q))
    print(f"{w}: worst W error {worst:.3f} ulp of mpmath's exp")
    assert worst <= 1.0
    if w["half_width"] >= 200.0:
        assert np.all(W[np.abs(ys) <= 200.0] == 1.0)   # the whole y range of any point ([-80, 50]) and beyond


def table_cases():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "golden_window.json")))["tables"]
    return [("two", d["two"], win("table", table=1)), ("two", d["two"], win("table", table=0, y0=3.0, scale=0.5)),
            ("ends0", d["ends0"], win("table")), ("ends0", d["ends0"], win("table", y0=-3.0, scale=0.25)),
            ("node", d["node"], win("table")), ("k1024", d["k1024"], win("table", table=1)),
            ("k1024", d["k1024"], win("table", table=0, y0=5.0, scale=3.0))]


@pytest.mark.parametrize("name,t,w", table_cases(), ids=lambda x: x if isinstance(x, str) else None)
def test_table_kind_bit_equal(name, t, w):
    u = np.array(t["u"])
    # every knot and both ends, an ulp either side, mapped back through y = y0 + scale v (and so a
    # value or two off the knot: the neighbours of y cover it)
    ys = list(np.linspace(-80.0, 50.0, 523))
    for uk in u:
        ys += around(w["y0"] + w["scale"] * uk, 3)
    ys = np.array(ys)
    tabs = pkg("window").WindowTables(t["u"], t["W"])
    v, W = pkg("window").eval_host(w, ys, tabs)
    v_ref, W_ref = table_numpy(w, t["u"], t["W"][w["table"]], ys)
    assert np.array_equal(v, v_ref)
    assert np.array_equal(W, W_ref), (ys[W != W_ref], W[W != W_ref], W_ref[W != W_ref])
    row = np.array(t["W"][w["table"]])
    assert np.all(W[v < u[0]] == row[0]) and np.all(W[v >= u[-1]] == row[-1])
    on_knot = np.isin(v, u)
    assert on_knot.sum() >= (u.size if (w["y0"], w["scale"]) == (0.0, 1.0) else 1)
    assert np.array_equal(W[on_knot], row[np.searchsorted(u, v[on_knot])])   # a knot returns its own value


BAD_BLOCKS = [
    (win("gauss", y0=float("nan")), "NaN"), (win("plateau", half_width=float("nan")), "NaN"),
    (win("gauss", sigma_lo=float("nan")), "NaN"), (win("gauss", sigma_hi=float("nan")), "NaN"),
    (win("table", scale=float("nan")), "NaN"),
    (win("gauss", sigma_hi=0.0), "sigma"), (win("plateau", sigma_lo=-1.0), "sigma"),
    (win("plateau", sigma_hi=float("inf")), "sigma"), (win("table", scale=0.0), "scale"),
    (win("table", scale=float("inf")), "scale"), (win("plateau", scale=-2.0), "scale"),
    (win("plateau", half_width=-1e-300), "half_width"),
    (dict(NEUTRAL, kind=3), "kind"), (dict(NEUTRAL, kind=-1), "kind"),
    (win("table", table=2), "table index"), (win("table", table=-1), "table index"),
]


@pytest.mark.parametrize("w,what", BAD_BLOCKS, ids=[f"{i}-{b[1]}" for i, b in enumerate(BAD_BLOCKS)])
def test_bad_block_is_refused_with_a_message(w, what):
    W, N = pkg("window"), pkg("_native")
    tabs = W.WindowTables([0.0, 1.0], [[1.0, 0.5], [0.0, 1.0]])
    with pytest.raises(N.LzqError) as e:
        W.eval_host(w, [0.0, 1.0], tabs)
    assert e.value.code == -1 and what in str(e.value)
    recs = np.concatenate([W.to_window(win("gauss")), W.to_window(w)])
    with pytest.raises(N.LzqError) as e:
        W.check(recs, tabs)
    assert e.value.code == -1 and "window 1" in str(e.value)   # names the offending record
    W.check(recs[:1], tabs)


def test_table_kind_without_tables_is_refused():
    W, N = pkg("window"), pkg("_native")
    with pytest.raises(N.LzqError, match="table index"):
        W.eval_host(win("table"), [0.0])


@pytest.mark.parametrize("u,Wt,what", [
    ([0.0, 0.0], [1.0, 1.0], "ascending"), ([0.0, 1.0, 0.5], [1.0, 1.0, 1.0], "ascending"),
    ([0.0, float("nan")], [1.0, 1.0], "finite"), ([0.0, float("inf")], [1.0, 1.0], "finite"),
    ([0.0, 1.0], [1.0, -1e-300], "W["), ([0.0, 1.0], [float("nan"), 1.0], "W["),
    ([0.0, 1.0], [1.0, float("inf")], "W["), ([0.0], [1.0], "n_knots"),
    (list(range(4097)), [1.0] * 4097, "n_knots"),
])
def test_bad_tables_are_refused_with_a_message(u, Wt, what):
    with pytest.raises(pkg("_native").LzqError) as e:
        pkg("window").WindowTables(u, Wt)
    assert e.value.code == -1 and what in str(e.value)


def test_too_many_tables_are_refused():
    with pytest.raises(pkg("_native").LzqError, match="n_tables"):
        pkg("window").WindowTables([0.0, 1.0], np.ones((1025, 2)))
    pkg("window").WindowTables([0.0, 1.0], np.ones((1024, 2)))
    pkg("window").WindowTables(np.arange(4096.0), np.ones(4096))


def test_to_window_mapping():
    W, N = pkg("window"), pkg("_native")
    r = W.to_window({"kind": "plateau", "sigma": 3.0, "y0": 2.0})[0]
    assert (r["kind"], r["sigma_lo"], r["sigma_hi"], r["y0"], r["scale"], r["half_width"]) == (1, 3.0, 3.0, 2.0, 1.0, 0.0)
    assert N.WINDOW_DTYPE.itemsize == 48
    with pytest.raises(ValueError):
        W.to_window({"kind": "plateau", "sigma": 3.0, "sigma_lo": 1.0})
    with pytest.raises(ValueError):
        W.to_window({"kind": "tophat"})
    with pytest.raises(ValueError):
        W.to_window({"kind": "gauss", "width": 1.0})
    assert W.to_windows({"kind": "gauss"}, 5).size == 5
    with pytest.raises(ValueError):
        W.to_windows(np.zeros(3, dtype=N.WINDOW_DTYPE), 5)


def test_csv_tables(tmp_path):
    p = tmp_path / "w.csv"
    p.write_text("# activity profile\nu,W\n-1.0,0.0\n0.5,1.0\n2.0,0.25\n")
    t = pkg("window").WindowTables.from_csv(str(p))
    assert t.u.tolist() == [-1.0, 0.5, 2.0] and t.W.tolist() == [[0.0, 1.0, 0.25]]


def test_headline_machine_code_is_the_profiled_one():
    """The window is a parameter of lzq_quad.h's y_factors / yb_wave; the headline kernels' ISA (the
    identity the bench's roofline profile is tied to) must not have moved."""
    lib = pkg("build").LIB_PATH
    if not os.path.exists(lib):
        pytest.fail(f"{lib} not built; run __graft_entry__.build()", pytrace=False)
    got = pkg("codeobj").kernel_isa_sha256(lib)
    assert got is not None, "llvm-objdump (ROCm) is needed to disassemble the code object"
    with open(os.path.join(ROOT, "profiles", "round6", "pmc_summary.json")) as f:
        assert got == json.load(f)["kernel_isa_sha256"]


def test_window_quadrature_kernels_keep_occupancy_without_scratch():
    """tools/kernel_resources.py on lzq_window.hip: both quadrature kernels at the 8 waves/SIMD of
    their __launch_bounds__, no scratch, and the dense one's LDS lets two blocks share a CU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    rows = [r for r in kr.resources("lzq_window.hip", []) if "window_kernel" in r["kernel"]]
    names = " ".join(r["kernel"] for r in rows)
    assert "yields_points_window_kernel" in names and "points_reuse_window_kernel" in names
    for r in rows:
        assert int(r["ScratchSize [bytes/lane]"]) == 0, r
        assert int(r["Occupancy [waves/SIMD]"]) == 8, r
        assert 2 * int(r["LDS Size [bytes/block]"]) <= 160 * 1024, r
