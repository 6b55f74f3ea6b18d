"""The source activity window W(y) of a point (include/lzq.h lzq_window; PAPER §10 step 4).

Host side: window blocks as WINDOW_DTYPE records, tabulated profiles, and the library's host build
of the window (lzq_window_check_host / lzq_window_eval_host: no GPU).  The kernels are reached
through engine.Engine.yields(window=...) and Engine.window.
"""
from __future__ import annotations

import ctypes
import re
from typing import Optional

import numpy as np

from . import _native

# the neutral block: a field a kind does not read still has to be valid (include/lzq.h)
DEFAULTS = {"y0": 0.0, "half_width": 0.0, "sigma_lo": 1.0, "sigma_hi": 1.0, "scale": 1.0}
KEYS = ("kind", "table", "sigma") + _native.WINDOW_FIELDS


def to_window(obj) -> np.ndarray:
    """One WINDOW_DTYPE record from a record or a mapping {"kind": "gauss" | "plateau" | "table" (or
    its code), "y0", "half_width", "sigma_lo", "sigma_hi", "sigma" (both sigmas), "scale", "table"};
    fields left out take DEFAULTS.  Values are not judged here (check does that)."""
    if isinstance(obj, np.ndarray) and obj.dtype == _native.WINDOW_DTYPE:
        if obj.size != 1:
            raise ValueError(f"window: expected one record, got {obj.size}")
        return np.ascontiguousarray(obj).reshape(1).copy()
    d = dict(obj)
    unknown = sorted(set(d) - set(KEYS))
    if unknown:
        raise ValueError(f"window: unknown field(s) {unknown}")
    if "kind" not in d:
        raise ValueError("window: 'kind' is required")
    kind = d["kind"]
    if isinstance(kind, str):
        if kind not in _native.WINDOW_KINDS:
            raise ValueError(f"window: unknown kind {kind!r} (one of {sorted(_native.WINDOW_KINDS)})")
        kind = _native.WINDOW_KINDS[kind]
    rec = np.zeros(1, dtype=_native.WINDOW_DTYPE)
    rec["kind"] = int(kind)
    rec["table"] = int(d.get("table", 0))
    for k, v in DEFAULTS.items():
        rec[k] = float(d.get(k, v))
    if "sigma" in d:
        if "sigma_lo" in d or "sigma_hi" in d:
            raise ValueError("window: give 'sigma' or 'sigma_lo' / 'sigma_hi', not both")
        rec["sigma_lo"] = rec["sigma_hi"] = float(d["sigma"])
    return rec


def to_windows(window, n: int) -> np.ndarray:
    """n WINDOW_DTYPE records from one block for all points (a mapping or a 1-record array) or n
    records."""
    if isinstance(window, np.ndarray) and window.dtype == _native.WINDOW_DTYPE:
        rec = np.ascontiguousarray(window).reshape(-1)
    else:
        rec = to_window(window)
    if rec.size == 1 and n != 1:
        rec = np.repeat(rec, n)
    if rec.size != n:
        raise ValueError(f"window: {rec.size} records for {n} points")
    return rec


class WindowTables:
    """Tabulated profiles shared by a batch (lzq_window_tables): u (n_knots,) strictly ascending,
    W (n_tables, n_knots) finite and >= 0; a 1-D W is one table."""

    def __init__(self, u, W):
        self.u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        W = np.asarray(W, dtype=np.float64)
        self.W = np.ascontiguousarray(W.reshape(1, -1) if W.ndim == 1 else W)
        if self.W.ndim != 2 or self.W.shape[1] != self.u.size:
            raise ValueError(f"window tables: W of shape {W.shape} for {self.u.size} knots")
        check(None, self)

    @property
    def n_tables(self) -> int:
        return self.W.shape[0]

    @property
    def n_knots(self) -> int:
        return self.u.size

    def ctypes_host(self) -> "_native.LzqWindowTables":
        return _native.LzqWindowTables(self.n_tables, self.n_knots, self.u.ctypes.data, self.W.ctypes.data)

    def to_json(self) -> dict:
        return {"u": self.u.tolist(), "tables": self.W.tolist()}

    @classmethod
    def from_csv(cls, path: str) -> "WindowTables":
        """One table from a two-column `u,W` file (lines starting with # and a header line of
        names are skipped)."""
        rows = []
        with open(path) as f:
            for line in f:
                t = line.strip()
                if not t or t.startswith("#"):
                    continue
                parts = t.replace(";", ",").split(",") if "," in t or ";" in t else t.split()
                try:
                    rows.append((float(parts[0]), float(parts[1])))
                except (ValueError, IndexError):
                    if rows:
                        raise ValueError(f"{path}: cannot read {t!r} as `u,W`")
        if not rows:
            raise ValueError(f"{path}: no `u,W` rows")
        a = np.asarray(rows)
        return cls(a[:, 0], a[:, 1])


def as_tables(tables) -> Optional[WindowTables]:
    """None, a WindowTables, or (u, W)."""
    if tables is None or isinstance(tables, WindowTables):
        return tables
    u, W = tables
    return WindowTables(u, W)


def check(windows: Optional[np.ndarray], tables: Optional[WindowTables] = None) -> None:
    """Every refusal of include/lzq.h for these blocks and tables (lzq_window_check_host): raises
    _native.LzqError (LZQ_EINVAL) with the library's message."""
    lib = _native.load()
    n = 0 if windows is None else int(windows.size)
    w = None if windows is None else np.ascontiguousarray(windows, dtype=_native.WINDOW_DTYPE)
    t = None if tables is None else tables.ctypes_host()
    _native.check(lib.lzq_window_check_host(None if w is None else w.ctypes.data, n,
                                            None if t is None else ctypes.byref(t)), lib)


def eval_host(window, ys, tables=None) -> tuple:
    """The library's host build of one block at ys: (q, W), q the v of a table kind and W its
    interpolated value, else W = libm exp(-q^2 / 2) (lzq_window_eval_host)."""
    lib = _native.load()
    rec = to_window(window)
    tables = as_tables(tables)
    y = np.ascontiguousarray(ys, dtype=np.float64).reshape(-1)
    q, W = np.empty_like(y), np.empty_like(y)
    blk = _native.LzqWindow.from_buffer_copy(rec.tobytes())
    t = None if tables is None else tables.ctypes_host()
    _native.check(lib.lzq_window_eval_host(ctypes.byref(blk), None if t is None else ctypes.byref(t), y.ctypes.data,
                                           y.size, q.ctypes.data, W.ctypes.data), lib)
    return q, W


def _host_axes(axes):
    """(lzq_axis array, keep-alive list) for (name, values) axes with HOST values: the window axes
    (_native.WINDOW_FIELD; sweep.WINDOW_AXES) carry their values, the others only their length."""
    arr = (_native.LzqAxis * max(1, len(axes)))()
    keep = []
    for a, (name, vals) in enumerate(axes):
        if name in _native.WINDOW_FIELD:
            v = np.ascontiguousarray(vals, dtype=np.float64).reshape(-1)
            keep.append(v)
            arr[a].field, arr[a].n, arr[a].values = _native.WINDOW_FIELD[name], v.size, v.ctypes.data
        else:
            field = name if isinstance(name, int) else _native.FIELD.get(name)
            if field is None:
                raise ValueError(f"unknown sweep field {name!r}")
            arr[a].field, arr[a].n, arr[a].values = field, len(vals), None
    return arr, keep


def grid_blocks(base, axes, start: int, count: int) -> np.ndarray:
    """The window blocks (WINDOW_DTYPE) of flat grid indices [start, start + count) of base x axes
    (C order, last axis fastest): the library's host build of the decode the grid kernels run
    (lzq_window_grid_blocks_host; csrc/lzq_window.h window_grid_block).  No GPU."""
    lib = _native.load()
    blk = _native.LzqWindow.from_buffer_copy(to_window(base).tobytes())
    arr, keep = _host_axes(axes)
    out = np.zeros(int(count), dtype=_native.WINDOW_DTYPE)
    _native.check(lib.lzq_window_grid_blocks_host(ctypes.byref(blk), arr, len(axes), int(start), int(count),
                                                  out.ctypes.data), lib)
    return out


def grid_check(base, axes, tables: Optional[WindowTables] = None) -> None:
    """Every refusal of include/lzq.h for the blocks of the grid base x axes, from the base block and
    each window axis's values on their own (lzq_window_grid_check_host): raises _native.LzqError
    naming the axis and the value.  No GPU."""
    lib = _native.load()
    blk = _native.LzqWindow.from_buffer_copy(to_window(base).tobytes())
    arr, keep = _host_axes(axes)
    t = None if tables is None else tables.ctypes_host()
    rc = lib.lzq_window_grid_check_host(ctypes.byref(blk), arr, len(axes), None if t is None else ctypes.byref(t))
    if rc:
        msg = (lib.lzq_last_error() or b"").decode()
        m = re.match(r"window axis (\d+) ", msg)
        if m:
            msg = f"axis {axes[int(m.group(1))][0]!r}: {msg}"
        raise _native.LzqError(rc, msg)
