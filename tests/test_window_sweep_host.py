"""Sweep specs with a source activity window (sweep.WindowSpec, the window_* axes): parsing, the
to_json round trip, checkpoint keys and the C-order decode of the window blocks.  No GPU."""
import json

import numpy as np
import pytest

from conftest import pkg

SPEC = {"name": "w", "n_y": 2000,
        "axes": [{"field": "window_y0", "values": [-5, 0, 5]}, {"field": "window_sigma", "linspace": [3, 12, 4]},
                 {"field": "delta_LZ", "logspace": [-3, 0, 5]}],
        "window": {"kind": "plateau", "half_width": 2.0}}


def test_round_trip_and_keys():
    S = pkg("sweep")
    sp = S.spec_from_json(SPEC)
    j = sp.to_json()
    assert j["window"] == {"kind": "plateau", "half_width": 2.0}
    again = S.spec_from_json(json.loads(json.dumps(j)))
    assert again.to_json() == j and S.spec_key(again) == S.spec_key(sp)
    other = S.spec_from_json(dict(SPEC, window={"kind": "plateau", "half_width": 2.5}))
    gauss = S.spec_from_json(dict(SPEC, window={"kind": "gauss"}))
    assert len({S.spec_key(sp), S.spec_key(other), S.spec_key(gauss)}) == 3


def test_specs_without_a_window_keep_their_json_and_key():
    S = pkg("sweep")
    for name, sp in S.builtin_specs().items():
        assert "window" not in sp.to_json(), name
    plain = {k: v for k, v in SPEC.items() if k != "window"}
    plain["axes"] = [a for a in SPEC["axes"] if not a["field"].startswith("window_")]
    sp = S.spec_from_json(plain)
    assert sp.window is None and "window" not in sp.to_json()
    # the key is a hash of to_json() and the library: the definition part is what it was before
    assert sorted(sp.to_json()) == ["axes", "base", "n_y", "name", "notes"]


def test_window_blocks_decode_in_c_order():
    S, N = pkg("sweep"), pkg("_native")
    sp = S.spec_from_json(SPEC)
    assert sp.total == 60
    rec = S.window_records(sp, 0, 60)
    assert rec.dtype == N.WINDOW_DTYPE and rec.size == 60
    y0, sig = [-5.0, 0.0, 5.0], np.linspace(3, 12, 4)
    for i in range(60):
        a, b = i // 20, (i // 5) % 4          # the last axis (delta_LZ, 5 values) is the fastest
        r = rec[i]
        assert (r["kind"], r["y0"], r["half_width"], r["sigma_lo"], r["sigma_hi"], r["scale"]) == \
            (N.WIN_PLATEAU, y0[a], 2.0, sig[b], sig[b], 1.0), i
        assert sp.point_params(i)["window_y0"] == y0[a] and sp.point_params(i)["window_sigma"] == sig[b]
    assert np.array_equal(S.window_records(sp, 13, 9), rec[13:22])


def test_table_axis_and_inline_tables(tmp_path):
    S, N = pkg("sweep"), pkg("_native")
    d = {"axes": [{"field": "window_table", "values": [0, 1]}, {"field": "window_scale", "values": [1.0, 2.0, 4.0]}],
         "window": {"kind": "table", "y0": 1.0, "u": [-1.0, 0.0, 3.0], "tables": [[0.0, 1.0, 0.0], [1.0, 1.0, 0.5]]}}
    sp = S.spec_from_json(d)
    rec = S.window_records(sp, 0, 6)
    assert rec["table"].tolist() == [0, 0, 0, 1, 1, 1] and rec["scale"].tolist() == [1.0, 2.0, 4.0] * 2
    assert (rec["kind"] == N.WIN_TABLE).all() and (rec["y0"] == 1.0).all()
    assert S.spec_from_json(sp.to_json()).to_json() == sp.to_json()
    # a csv is read once and carried inline: the key follows the file's contents
    p = tmp_path / "w.csv"
    p.write_text("u,W\n-1,0\n0,1\n3,0\n")
    c = S.spec_from_json({"axes": [{"field": "window_scale", "values": [1.0]}],
                          "window": {"kind": "table", "csv": str(p)}})
    assert c.to_json()["window"]["u"] == [-1.0, 0.0, 3.0] and c.to_json()["window"]["tables"] == [[0.0, 1.0, 0.0]]
    p.write_text("u,W\n-1,0\n0,1\n3,0.5\n")
    c2 = S.spec_from_json({"axes": [{"field": "window_scale", "values": [1.0]}],
                           "window": {"kind": "table", "csv": str(p)}})
    assert S.spec_key(c) != S.spec_key(c2)
    with pytest.raises(ValueError, match="integers"):
        S.spec_from_json(dict(d, axes=[{"field": "window_table", "values": [0.5]}]))


def test_usage_errors():
    S, N = pkg("sweep"), pkg("_native")
    no_section = {k: v for k, v in SPEC.items() if k != "window"}
    with pytest.raises(ValueError, match="need a 'window' section"):
        S.spec_from_json(no_section)
    with pytest.raises(ValueError, match="ODE"):       # a window on an ODE spec
        S.spec_from_json(dict(SPEC, base={"Gamma_wash_over_H": 0.5}))
    with pytest.raises(ValueError, match="ODE"):
        S.spec_from_json(dict(SPEC, axes=SPEC["axes"] + [{"field": "Gamma_wash_over_H", "values": [0.0, 0.5]}]))
    with pytest.raises(ValueError, match="table"):
        S.spec_from_json(dict(SPEC, window={"kind": "table"}))
    with pytest.raises(ValueError, match="unknown"):
        S.spec_from_json(dict(SPEC, window={"kind": "gauss", "width": 3.0}))
    with pytest.raises(N.LzqError, match="sigma"):
        S.spec_from_json(dict(SPEC, window={"kind": "gauss", "sigma_hi": -1.0}))
    # crossings and profile specs may carry one
    S.spec_from_json(dict(SPEC, axes=[{"field": "m_mix", "values": [0.1]}, {"field": "dprime", "values": [1.0]},
                                      {"field": "window_y0", "values": [0.0, 1.0]}], crossings={"n_cross": 2}))
    S.spec_from_json(dict(SPEC, axes=[{"field": "y_B", "values": [1.0]}, {"field": "window_y0", "values": [0.0]}],
                          profile={"synthetic": 12}))
