"""The momentum-averaged Landau-Zener probability P-bar(T) from a momentum kernel F(k) (include/lzq.h
lzq_fk; PAPER §10 step 1; csrc/lzq_fk.h).

Host side: kernel blocks as FK_DTYPE records, the library's host checks and host build of P-bar
(lzq_fk_check_host / lzq_fk_pbar_host: no GPU), delta_0 of a point, and the grouping of points into
classes that share one R table.  The kernels are reached through engine.Engine.yields(fk=...) and
Engine.pbar.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _native

DEFAULTS = {"p": 0.0, "v_ref": 1.0}
KEYS = ("kind",) + tuple(DEFAULTS)
# what an R table depends on besides delta_0 and the block: the y-grid and T(y) of quad_setup /
# y_factors (csrc/lzq_quad.h), m and the statistics
CLASS_POINT_FIELDS = ("T_p_GeV", "beta_over_H", "T_min_over_Tp", "T_max_over_Tp", "m_chi_GeV", "stats")


def to_fk(obj) -> np.ndarray:
    """One FK_DTYPE record from a record or a mapping {"kind": "power" (or its code, the default),
    "p", "v_ref"}; fields left out take DEFAULTS (p = 0: the paper's F = 1).  Values are not judged
    here (check does that)."""
    if isinstance(obj, np.ndarray) and obj.dtype == _native.FK_DTYPE:
        if obj.size != 1:
            raise ValueError(f"fk: expected one record, got {obj.size}")
        return np.ascontiguousarray(obj).reshape(1).copy()
    d = dict(obj)
    unknown = sorted(set(d) - set(KEYS))
    if unknown:
        raise ValueError(f"fk: unknown field(s) {unknown}")
    kind = d.get("kind", "power")
    if isinstance(kind, str):
        if kind not in _native.FK_KINDS:
            raise ValueError(f"fk: unknown kind {kind!r} (one of {sorted(_native.FK_KINDS)})")
        kind = _native.FK_KINDS[kind]
    rec = np.zeros(1, dtype=_native.FK_DTYPE)
    rec["kind"] = int(kind)
    for k, v in DEFAULTS.items():
        rec[k] = float(d.get(k, v))
    return rec


def to_fks(fk, n: int) -> np.ndarray:
    """n FK_DTYPE records from one block for all points (a mapping or a 1-record array) or n records."""
    if isinstance(fk, np.ndarray) and fk.dtype == _native.FK_DTYPE:
        rec = np.ascontiguousarray(fk).reshape(-1)
    else:
        rec = to_fk(fk)
    if rec.size == 1 and n != 1:
        rec = np.repeat(rec, n)
    if rec.size != n:
        raise ValueError(f"fk: {rec.size} records for {n} points")
    return rec


def check(fks: np.ndarray, delta0=None) -> None:
    """Every refusal of include/lzq.h for these blocks and (if given) their points' delta_0
    (lzq_fk_check_host): raises _native.LzqError (LZQ_EINVAL) with the library's message."""
    lib = _native.load()
    f = np.ascontiguousarray(fks, dtype=_native.FK_DTYPE).reshape(-1)
    d = None if delta0 is None else np.ascontiguousarray(delta0, dtype=np.float64).reshape(-1)
    if d is not None and d.size != f.size:
        raise ValueError(f"fk: {d.size} values of delta0 for {f.size} blocks")
    _native.check(lib.lzq_fk_check_host(f.ctypes.data, None if d is None else d.ctypes.data, f.size), lib)


def nodes() -> tuple:
    """Host copies of the t-rule's node table (lzq_fk_nodes): t, W e^-t, e^-t.  No GPU."""
    lib = _native.load()
    n = ctypes.c_int32(0)
    dp = ctypes.POINTER(ctypes.c_double)
    _native.check(lib.lzq_fk_nodes(None, None, None, ctypes.byref(n)), lib)
    t, we, e = (np.empty(n.value) for _ in range(3))
    _native.check(lib.lzq_fk_nodes(t.ctypes.data_as(dp), we.ctypes.data_as(dp), e.ctypes.data_as(dp), ctypes.byref(n)),
                  lib)
    return t, we, e


def stats_code(stats) -> int:
    if isinstance(stats, str):
        return _native.FERMION if stats.lower().startswith("ferm") else _native.BOSON
    return int(stats)


def pbar_host(block, mu, delta0, stats=_native.FERMION) -> np.ndarray:
    """P-bar(mu) at delta_0 from the library's host build (lzq_fk_pbar_host: libm, no GPU).  mu and
    delta0 broadcast against each other."""
    lib = _native.load()
    rec = to_fk(block)
    m, d = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(delta0, dtype=np.float64))
    m, d = np.ascontiguousarray(m).reshape(-1), np.ascontiguousarray(d).reshape(-1)
    out = np.empty_like(m)
    blk = _native.LzqFk.from_buffer_copy(rec.tobytes())
    _native.check(lib.lzq_fk_pbar_host(ctypes.byref(blk), stats_code(stats), m.ctypes.data, d.ctypes.data, m.size,
                                       out.ctypes.data), lib)
    return out


def delta_from_P(P) -> np.ndarray:
    """delta_0 of a point given as its F = 1 probability P = 1 - exp(-2 pi delta_0):
    -log1p(-P) / (2 pi); P = 1 is +inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.log1p(-np.asarray(P, dtype=np.float64)) / (2.0 * math.pi)


def point_delta(points: np.ndarray, delta=None) -> np.ndarray:
    """delta_0 per point: `delta` (one value or one per point) if given, else from each point's
    P_chi_to_B (delta_from_P)."""
    n = points.size
    if delta is None:
        return np.ascontiguousarray(delta_from_P(points["P_chi_to_B"]))
    d = np.asarray(delta, dtype=np.float64).reshape(-1)
    if d.size == 1 and n != 1:
        d = np.repeat(d, n)
    if d.size != n:
        raise ValueError(f"fk: {d.size} values of delta for {n} points")
    return np.ascontiguousarray(d)


def class_groups(points: np.ndarray, delta0: np.ndarray, fks: np.ndarray) -> tuple:
    """(rep, cls): the classes of points that share one R table -- equal, bit for bit, in
    CLASS_POINT_FIELDS, delta_0 and the block (kind, p, v_ref) -- by numpy.unique over the key's
    words.  rep[c] (int64) is the first point of class c, cls[i] (int32) point i's class."""
    n = points.size
    key = np.empty((n, len(CLASS_POINT_FIELDS) + 4), dtype=np.uint64)
    for k, f in enumerate(CLASS_POINT_FIELDS):
        col = points[f]
        key[:, k] = col.astype(np.float64).view(np.uint64) if col.dtype.kind == "f" else col.astype(np.uint64)
    k = len(CLASS_POINT_FIELDS)
    key[:, k] = np.ascontiguousarray(delta0, dtype=np.float64).view(np.uint64)
    key[:, k + 1] = fks["kind"].astype(np.int64).astype(np.uint64)
    key[:, k + 2] = np.ascontiguousarray(fks["p"]).view(np.uint64)
    key[:, k + 3] = np.ascontiguousarray(fks["v_ref"]).view(np.uint64)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return first.astype(np.int64), np.asarray(inv).reshape(-1).astype(np.int32)
