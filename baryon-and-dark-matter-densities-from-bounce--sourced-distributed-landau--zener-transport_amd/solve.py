"""The solve spec of an inverse sweep (include/lzq.h lzq_solve): for every grid point, the value of one
parameter in [lo, hi] at which a yield field takes a target value.  No GPU here: the mapping form, its
checks through the library's host-side lzq_solve_check_host, the CLI form and the summary block.

A spec is a mapping
    {"field": NAME, "lo": LO, "hi": HI, "target": {"field": YIELD_FIELD, "value": V}, "xtol": 1e-12,
     "max_evals": 64}
NAME: an lzq_point double field that contributes no z-sum table, 'delta_LZ' / 'm_mix' / 'dprime', or
with a window one of the window axis names but 'window_table'.  The target defaults to the Planck
ratio DM_over_B = 5.357 (PAPER eq.(22)).
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional, Sequence

import numpy as np

from . import _native

DEFAULT_TARGET = {"field": "DM_over_B", "value": 5.357}
DEFAULT_XTOL = 1e-12
DEFAULT_MAX_EVALS = 64
_KEYS = {"field", "lo", "hi", "target", "xtol", "max_evals"}


def normalize(solve: Mapping) -> dict:
    """The spec with every default filled in and every value of its JSON type (ValueError on a
    malformed one); what SweepSpec.to_json carries, so the checkpoint key changes with it."""
    if not isinstance(solve, Mapping):
        raise ValueError("solve: expected a mapping {field, lo, hi, target, xtol, max_evals}")
    extra = set(solve) - _KEYS
    if extra:
        raise ValueError(f"solve: unknown keys {sorted(extra)}")
    for k in ("field", "lo", "hi"):
        if k not in solve:
            raise ValueError(f"solve: missing {k!r}")
    name = str(solve["field"])
    if name not in _native.FIELD and name not in _native.WINDOW_FIELD and name not in _native.WASH_FIELD:
        raise ValueError(f"solve: unknown field {name!r}")
    target = dict(DEFAULT_TARGET, **dict(solve.get("target") or {}))
    if set(target) != {"field", "value"}:
        raise ValueError("solve: target is {field, value}")
    if target["field"] not in _native.YIELD_FIELDS:
        raise ValueError(f"solve: target field {target['field']!r} is not one of {_native.YIELD_FIELDS}")
    max_evals = solve.get("max_evals", DEFAULT_MAX_EVALS)
    if int(max_evals) != max_evals:
        raise ValueError("solve: max_evals must be an integer")
    max_evals = min(max(int(max_evals), _native.SOLVE_MIN_EVALS), _native.SOLVE_MAX_EVALS_CAP)
    return {"field": name, "lo": float(solve["lo"]), "hi": float(solve["hi"]),
            "target": {"field": str(target["field"]), "value": float(target["value"])},
            "xtol": float(solve.get("xtol", DEFAULT_XTOL)), "max_evals": max_evals}


def to_ctypes(solve: Mapping) -> "_native.LzqSolve":
    s = normalize(solve)
    field = _native.FIELD.get(s["field"], _native.WINDOW_FIELD.get(s["field"], _native.WASH_FIELD.get(s["field"])))
    return _native.LzqSolve(field, _native.YIELD_FIELDS.index(s["target"]["field"]), s["lo"], s["hi"],
                            s["target"]["value"], s["xtol"], s["max_evals"])


def check(solve: Mapping, axis_names: Sequence[str], window_block=None, lib=None, wash=None) -> dict:
    """Every host-side refusal of the solve (include/lzq.h), before anything is uploaded: raises
    ValueError with the library's message.  axis_names: the grid's axes; window_block: the base window
    (anything but None counts as "the sweep has a window"); wash: the base wash block of a sweep through
    the wash-out quadrature (wash.py), where Gamma_wash_over_H is a solve field too.  Returns the
    normalized spec."""
    s = normalize(solve)
    if s["field"] in _native.WINDOW_FIELD and window_block is None:
        raise ValueError(f"solve: window field {s['field']!r} needs a window")
    if wash is not None:
        from . import wash as _wash
        _wash.solve_check(to_ctypes(s), axis_names, wash, window_block, lib)
        return s
    if s["field"] in _native.WASH_FIELD:
        raise ValueError(f"solve: field {s['field']!r} needs the wash-out quadrature (wash=...)")
    L = lib or _native.load()
    n = len(axis_names)
    if n > _native.LZQ_MAX_AXES:
        raise ValueError(f"at most {_native.LZQ_MAX_AXES} sweep axes")
    arr = (_native.LzqAxis * max(1, n))()
    for a, name in enumerate(axis_names):
        f = _native.FIELD.get(name, _native.WINDOW_FIELD.get(name))
        if f is None:
            raise ValueError(f"unknown sweep field {name!r}")
        arr[a].field, arr[a].n, arr[a].values = f, 1, None
    win = _native.LzqWindow() if window_block is not None else None
    rc = L.lzq_solve_check_host(ctypes.byref(to_ctypes(s)), ctypes.byref(win) if win is not None else None, arr, n)
    if rc:
        raise ValueError("solve: " + (L.lzq_last_error() or b"").decode())
    return s


def parse_cli(text: str) -> dict:
    """FIELD:LO:HI[:TARGETFIELD=VALUE], the sweep CLI's --solve."""
    parts = text.split(":")
    if len(parts) not in (3, 4):
        raise ValueError(f"--solve {text!r}: expected FIELD:LO:HI[:TARGETFIELD=VALUE]")
    try:
        out = {"field": parts[0], "lo": float(parts[1]), "hi": float(parts[2])}
        if len(parts) == 4:
            tf, _, tv = parts[3].partition("=")
            if not tf or not tv:
                raise ValueError
            out["target"] = {"field": tf, "value": float(tv)}
    except ValueError:
        raise ValueError(f"--solve {text!r}: expected FIELD:LO:HI[:TARGETFIELD=VALUE]") from None
    return normalize(out)


def summary_from_parts(solve: Mapping, x_solved, status_counts, evals_sum: int, evals_max: int, n: int) -> dict:
    """The "solve" block from what a sweep can keep without the result table: x of the solved rows
    (status ok or max_evals; NaN entries are dropped), the row counts per status, and the sum and
    maximum of the evaluations over all n rows (integers: exact in any order)."""
    s = normalize(solve)
    out = {"field": s["field"], "lo": s["lo"], "hi": s["hi"], "target": s["target"], "xtol": s["xtol"],
           "max_evals": s["max_evals"]}
    x = np.asarray(x_solved, dtype=np.float64).reshape(-1)
    x = x[~np.isnan(x)]
    out["status"] = {name: int(status_counts[code]) for code, name in _native.SOLVE_STATUS.items()}
    out["x"] = {"min": float(x.min()), "median": float(np.median(x)), "max": float(x.max())} if x.size else None
    out["evals"] = {"mean": float(int(evals_sum) / n), "max": int(evals_max)} if n else None
    return out


def summary(solve: Mapping, results: Optional[np.ndarray]) -> dict:
    """The "solve" block of summary.json from the (total, 6) result table: field and target, counts
    per status, min / median / max of x over the solved rows (status ok or max_evals), mean and max
    evaluations."""
    s = normalize(solve)
    if results is None:
        return {"field": s["field"], "lo": s["lo"], "hi": s["hi"], "target": s["target"], "xtol": s["xtol"],
                "max_evals": s["max_evals"]}
    r = np.asarray(results, dtype=np.float64).reshape(-1, 6)
    status = r[:, 5].astype(np.int64)
    solved = (status == _native.SOLVE_OK) | (status == _native.SOLVE_MAX_EVALS)
    return summary_from_parts(s, r[solved, 0], np.bincount(status, minlength=5), int(r[:, 4].sum()),
                              int(r[:, 4].max()) if len(r) else 0, len(r))
