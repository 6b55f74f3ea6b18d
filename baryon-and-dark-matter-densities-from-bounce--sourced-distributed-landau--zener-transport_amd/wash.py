"""Wash-out and source depletion on the y-grid quadrature (include/lzq.h "wash-out and source
depletion"; PAPER §10 step 5).

Host side: a point's block as an ODE_DTYPE record (the reference's sigma_v_chi_GeV_m2,
Gamma_wash_over_H, deplete_DM_from_source), the library's host-side refusals (lzq_wash_check_host,
lzq_solve_check_host_wash) and its host build of the wash-out factor omega (lzq_wash_factor_host): no
GPU.  The kernels are reached through engine.Engine.yields / sweep / solve_point (wash=...).
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Sequence

import numpy as np

from . import _native

KEYS = ("sigma_v_chi_GeV_m2", "Gamma_wash_over_H", "deplete_DM_from_source")
AXES = tuple(_native.WASH_FIELD)  # the sweep axes over a block's fields


def to_wash(obj) -> np.ndarray:
    """One ODE_DTYPE record from a record or a mapping of KEYS (fields left out are 0 / False).  Values
    are not judged here (check does that)."""
    if isinstance(obj, np.ndarray) and obj.dtype == _native.ODE_DTYPE:
        if obj.size != 1:
            raise ValueError(f"wash: expected one record, got {obj.size}")
        return np.ascontiguousarray(obj).reshape(1).copy()
    d = dict(obj)
    unknown = sorted(set(d) - set(KEYS))
    if unknown:
        raise ValueError(f"wash: unknown field(s) {unknown}")
    rec = np.zeros(1, dtype=_native.ODE_DTYPE)
    rec["sigma_v_chi_GeV_m2"] = float(d.get("sigma_v_chi_GeV_m2", 0.0))
    rec["Gamma_wash_over_H"] = float(d.get("Gamma_wash_over_H", 0.0))
    rec["deplete_DM_from_source"] = 1 if d.get("deplete_DM_from_source", False) else 0
    return rec


def to_washes(wash, n: int) -> np.ndarray:
    """n ODE_DTYPE records from one block for all points (a mapping or a 1-record array) or n records."""
    if isinstance(wash, np.ndarray) and wash.dtype == _native.ODE_DTYPE:
        rec = np.ascontiguousarray(wash).reshape(-1)
    else:
        rec = to_wash(wash)
    if rec.size == 1 and n != 1:
        rec = np.repeat(rec, n)
    if rec.size != n:
        raise ValueError(f"wash: {rec.size} records for {n} points")
    return rec


def from_config(cfg) -> np.ndarray:
    """The block of a Config (or a mapping with its three fields)."""
    get = cfg.get if isinstance(cfg, Mapping) else lambda k, d=None: getattr(cfg, k, d)
    return to_wash({k: get(k, 0) or 0 for k in KEYS})


def check(rec: np.ndarray, lib=None) -> np.ndarray:
    """Every refusal of include/lzq.h for the records (sigma_v > 0, a NaN in sigma_v or Gamma): raises
    ValueError with the library's message, which names the field."""
    L = lib or _native.load()
    rec = np.ascontiguousarray(rec).reshape(-1)
    if L.lzq_wash_check_host(rec.ctypes.data, rec.size):
        raise ValueError("wash: " + (L.lzq_last_error() or b"").decode())
    return rec


def to_ctypes(rec: np.ndarray) -> "_native.LzqOdeParams":
    return _native.LzqOdeParams.from_buffer_copy(to_wash(rec).tobytes())


def factor_host(point, wash, ys, lib=None) -> np.ndarray:
    """omega(T(y)) of include/lzq.h from its host build (libm's log and exp; no GPU).  point: a
    1-record POINT_DTYPE array."""
    L = lib or _native.load()
    pt = _native.LzqPoint.from_buffer_copy(np.ascontiguousarray(point).reshape(1).tobytes())
    o = to_ctypes(wash)
    y = np.ascontiguousarray(ys, dtype=np.float64).reshape(-1)
    out = np.empty_like(y)
    _native.check(L.lzq_wash_factor_host(ctypes.byref(pt), ctypes.byref(o), y.ctypes.data, y.size, out.ctypes.data), L)
    return out


def field_code(name: str):
    """The lzq_field of an axis or solve field name of a wash sweep (None: unknown)."""
    for table in (_native.FIELD, _native.WINDOW_FIELD, _native.WASH_FIELD):
        if name in table:
            return table[name]
    return None


def solve_check(sv: "_native.LzqSolve", axis_names: Sequence[str], wash, window_block=None, lib=None) -> None:
    """The solve's host-side refusals on a wash sweep (lzq_solve_check_host_wash): ValueError with the
    library's message."""
    L = lib or _native.load()
    n = len(axis_names)
    if n > _native.LZQ_MAX_AXES:
        raise ValueError(f"at most {_native.LZQ_MAX_AXES} sweep axes")
    arr = (_native.LzqAxis * max(1, n))()
    for a, name in enumerate(axis_names):
        f = field_code(name)
        if f is None:
            raise ValueError(f"unknown sweep field {name!r}")
        arr[a].field, arr[a].n, arr[a].values = f, 1, None
    win = _native.LzqWindow() if window_block is not None else None
    o = to_ctypes(wash) if wash is not None else None
    rc = L.lzq_solve_check_host_wash(ctypes.byref(sv), ctypes.byref(win) if win is not None else None,
                                     ctypes.byref(o) if o is not None else None, arr, n)
    if rc:
        raise ValueError("solve: " + (L.lzq_last_error() or b"").decode())
