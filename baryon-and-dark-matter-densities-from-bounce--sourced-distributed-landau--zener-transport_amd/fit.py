"""Fit of a sweep's yield records to targets: chi2, best point, profile maps, selection.

A fit spec (JSON):

    {"terms":  [{"field": "Y_B", "target": 8.72e-11, "sigma": 8.72e-13}, ...],      # 1..4
     "levels": [2.30, 6.18],                                                         # 0..4, ascending
     "maps":   [["m_mix", "dprime"], ["m_mix"]],                                     # 0..4, 1 or 2 sweep axes
     "select": {"level": 6.18, "cap": 100000}}                                       # optional

chi2 of a row: for each term in order d = (x - target) / sigma, q = d * d, summed left to right in
float64, each operation rounded on its own.  A row is valid iff its chi2 is finite.  The state
accumulated over rows (include/lzq.h, "fit state") is independent of the order rows arrive in, so
it is the same bit for bit however a sweep is cut into chunks, shards or ranks.

HostFit is the plain numpy implementation (update, merge, result): the sweep driver uses it when
the records are CPU tensors, and the GPU tests compare the HIP kernels (lzq_fit_*, through
Engine.fit_*) against it.

The optional key "posterior": {"offset": 12.5 | "best", "credible": [0.683, 0.954, 0.997]} adds
the likelihood-weighted half: a valid row weighs exp(-(chi2 - offset)/2), kept as an integer in
units of 2^-62 by one definition shared by host and device (csrc/lzq_post.h); the evidence Z, the
mass within each level, a histogram of weight by chi2 - offset (the Delta chi2 enclosing each
credible fraction is read from it) and a marginal weight per map cell are sums of such integers,
held as (hi, lo) pairs of 64-bit words (include/lzq.h, "posterior state"), so they too are the
same bit for bit for every chunking, sharding and world size, up to 2^32 rows a state.  A numeric
offset is folded chunk by chunk behind the fit; "best" (the default) is the combined fit's best
chi2 and takes a second pass over the rank's shard, so it needs the table.  HostPosterior is the
numpy implementation (weights from the library's host function lzq_post_weights_host, integer
sums in numpy); Engine.post_* drive the HIP kernel (lzq_post_update).
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native

YIELD_FIELDS = _native.YIELD_FIELDS
MAX_TERMS, MAX_LEVELS, MAX_MAPS = _native.FIT_MAX_TERMS, _native.FIT_MAX_LEVELS, _native.FIT_MAX_MAPS
MAX_CELLS = _native.FIT_MAX_CELLS
HEADER_WORDS = _native.FIT_HEADER_WORDS
POST_HEADER_WORDS, POST_BINS, POST_MAX_ROWS = _native.POST_HEADER_WORDS, _native.POST_BINS, _native.POST_MAX_ROWS
# word offsets of the posterior state (include/lzq.h); pairs are (hi, lo), value hi * 2^31 + lo
PW_NUSED, PW_NZERO, PW_NABOVE, PW_NINVALID, PW_Z, PW_LEVEL, PW_HIST = 0, 1, 2, 3, 4, 6, POST_HEADER_WORDS
PW_MAPS = POST_HEADER_WORDS + 2 * POST_BINS
POST_UNIT = 1 << 62                      # the weight of a row at the offset
Q_INVALID, Q_ABOVE = (1 << 64) - 1, (1 << 64) - 2   # lzq_post_weights_host's sentinels
DEFAULT_CREDIBLE = (0.683, 0.954, 0.997)
NO_TABLE_BEST = ('a posterior with offset "best" takes a second pass over the table, which --no-table does not '
                 'keep: give a number as "offset"')
# word offsets of the state (include/lzq.h)
W_NVALID, W_NINVALID, W_WITHIN, W_BEST_CHI2, W_BEST_IDX, W_COLMIN, W_COLMAX, W_COLBAD, W_SEL_TOTAL = \
    0, 1, 2, 6, 7, 8, 14, 20, 26

# --fit paper: the project's baryon yield and the DM/baryon ratio summarize() already uses; the 1%
# sigmas are nominal tolerances, not measurement errors.  Levels: delta chi2 of 68.3 / 95.4 / 99.7%
# for two parameters.
PAPER = {"terms": [{"field": "Y_B", "target": 8.72e-11, "sigma": 8.72e-13},
                   {"field": "DM_over_B", "target": 5.357, "sigma": 0.05357}],
         "levels": [2.30, 6.18, 11.83], "maps": [], "select": {"level": 11.83, "cap": 1 << 20}}


@dataclass(frozen=True)
class FitTerm:
    field: str
    target: float
    sigma: float


@dataclass(frozen=True)
class FitMap:
    """A map resolved against a sweep's axes: cell (i_0[, i_1]) of flat index i has
    i_a = (i // stride[a]) % len[a] (the C-order decode of lzq_sweep_grid)."""
    axes: Tuple[str, ...]
    stride: Tuple[int, ...]
    len: Tuple[int, ...]

    @property
    def cells(self) -> int:
        return int(np.prod(self.len, dtype=np.int64))

    def cell(self, idx: np.ndarray) -> np.ndarray:
        c = (idx // self.stride[0]) % self.len[0]
        if len(self.axes) == 2:
            c = c * self.len[1] + (idx // self.stride[1]) % self.len[1]
        return c


class FitSpec:
    def __init__(self, terms: Sequence[FitTerm], levels: Sequence[float] = (), maps: Sequence[Sequence[str]] = (),
                 select: Optional[Tuple[float, int]] = None, posterior: Optional[dict] = None):
        self.posterior = self._posterior(posterior)
        self.terms = [t if isinstance(t, FitTerm) else FitTerm(*t) for t in terms]
        self.levels = [float(x) for x in levels]
        self.maps = [tuple(m) for m in maps]
        self.select = None if select is None else (float(select[0]), int(select[1]))
        if not 1 <= len(self.terms) <= MAX_TERMS:
            raise ValueError(f"a fit takes 1..{MAX_TERMS} terms, got {len(self.terms)}")
        for t in self.terms:
            if t.field not in YIELD_FIELDS:
                raise ValueError(f"unknown fit field {t.field!r} (one of {YIELD_FIELDS})")
            if not (math.isfinite(t.sigma) and t.sigma > 0):
                raise ValueError(f"fit term {t.field}: sigma must be finite and > 0, got {t.sigma!r}")
            if not math.isfinite(t.target):
                raise ValueError(f"fit term {t.field}: target must be finite, got {t.target!r}")
        if len(self.levels) > MAX_LEVELS:
            raise ValueError(f"a fit takes at most {MAX_LEVELS} levels, got {len(self.levels)}")
        if any(math.isnan(x) for x in self.levels) or any(b <= a for a, b in zip(self.levels, self.levels[1:])):
            raise ValueError(f"fit levels must be ascending, got {self.levels}")
        if len(self.maps) > MAX_MAPS:
            raise ValueError(f"a fit takes at most {MAX_MAPS} maps, got {len(self.maps)}")
        for m in self.maps:
            if not 1 <= len(m) <= 2 or len(set(m)) != len(m) or not all(isinstance(a, str) for a in m):
                raise ValueError(f"a fit map names one or two different sweep axes, got {list(m)!r}")
        if self.select is not None:
            if math.isnan(self.select[0]) or self.select[1] < 0:
                raise ValueError("fit select: level must be a number and cap >= 0")

    @staticmethod
    def _posterior(p) -> Optional[dict]:
        """{"offset": number >= 0 | "best", "credible": ascending fractions in (0, 1)}, defaults filled."""
        if p is None:
            return None
        if not isinstance(p, dict) or set(p) - {"offset", "credible"}:
            raise ValueError(f'fit posterior: an object with the keys "offset" and "credible", got {p!r}')
        off = p.get("offset", "best")
        if off != "best":
            if isinstance(off, (bool, str)) or not isinstance(off, (int, float)) or not (math.isfinite(off) and off >= 0):
                raise ValueError(f'fit posterior: offset must be a number >= 0 or "best", got {off!r}')
            off = float(off)
        cred = p.get("credible", DEFAULT_CREDIBLE)
        try:
            cred = [float(x) for x in cred]
        except (TypeError, ValueError):
            raise ValueError(f"fit posterior: credible must be a list of fractions, got {cred!r}") from None
        if any(not 0.0 < x < 1.0 for x in cred) or any(b <= a for a, b in zip(cred, cred[1:])):
            raise ValueError(f"fit posterior: credible fractions must be ascending and inside (0, 1), got {cred}")
        return {"offset": off, "credible": cred}

    @classmethod
    def from_json(cls, d: dict) -> "FitSpec":
        unknown = set(d) - {"terms", "levels", "maps", "select", "posterior"}
        if unknown:
            raise ValueError(f"unknown fit-spec keys {sorted(unknown)}")
        try:
            terms = [FitTerm(str(t["field"]), float(t["target"]), float(t["sigma"])) for t in d.get("terms", [])]
            sel = d.get("select")
            select = None if sel is None else (float(sel["level"]), int(sel["cap"]))
            maps = [[m] if isinstance(m, str) else list(m) for m in d.get("maps", [])]
        except (KeyError, TypeError) as e:
            raise ValueError(f"malformed fit spec: {e!r}") from None
        return cls(terms, d.get("levels", []), maps, select, d.get("posterior"))

    def to_json(self) -> dict:
        d = {"terms": [{"field": t.field, "target": t.target, "sigma": t.sigma} for t in self.terms],
             "levels": list(self.levels), "maps": [list(m) for m in self.maps]}
        if self.select is not None:
            d["select"] = {"level": self.select[0], "cap": self.select[1]}
        if self.posterior is not None:
            d["posterior"] = {"offset": self.posterior["offset"], "credible": list(self.posterior["credible"])}
        return d

    def axis_values(self, sweep_spec) -> dict:
        """The values of the sweep axes the maps name (the posterior's means and deviations)."""
        vals = {n: np.asarray(v, dtype=np.float64) for n, v in sweep_spec.axes}
        return {a: vals[a] for m in self.maps for a in m if a in vals}

    def resolve(self, sweep_spec) -> List[FitMap]:
        """The maps' axis names -> strides and lengths of `sweep_spec`'s grid (C order)."""
        names = [n for n, _ in sweep_spec.axes]
        lens = [len(v) for _, v in sweep_spec.axes]
        strides = [int(np.prod(lens[k + 1:], dtype=np.int64)) for k in range(len(lens))]
        out = []
        for m in self.maps:
            for a in m:
                if a not in names:
                    raise ValueError(f"fit map axis {a!r} is not an axis of sweep {sweep_spec.name!r} ({names})")
            fm = FitMap(tuple(m), tuple(strides[names.index(a)] for a in m), tuple(lens[names.index(a)] for a in m))
            if fm.cells > MAX_CELLS:
                raise ValueError(f"fit map {list(m)} has {fm.cells} cells (at most 2^24)")
            out.append(fm)
        return out


def load(arg: str) -> FitSpec:
    """--fit's argument: `paper` (the built-in preset) or the path of a fit-spec JSON."""
    if arg == "paper":
        return FitSpec.from_json(PAPER)
    with open(arg) as f:
        return FitSpec.from_json(json.load(f))


def state_words(maps: Sequence[FitMap]) -> int:
    return HEADER_WORDS + 2 * sum(m.cells for m in maps)


_TOP = np.uint64(1 << 63)
_ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def _key(x: np.ndarray) -> np.ndarray:
    """The order-preserving uint64 key of float64 values (include/lzq.h, words 8..19)."""
    b = np.asarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | _TOP)


def _unkey(k: np.ndarray) -> np.ndarray:
    k = np.asarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k ^ _TOP, ~k).view(np.float64)


def chi2_rows(fit: FitSpec, rows: np.ndarray) -> np.ndarray:
    """chi2 of (n, 6) float64 records, by the specification's expression."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    with np.errstate(all="ignore"):
        c = None
        for t in fit.terms:
            d = (rows[:, YIELD_FIELDS.index(t.field)] - np.float64(t.target)) / np.float64(t.sigma)
            q = d * d
            c = q if c is None else c + q
    return c


class HostFit:
    """The fit state in numpy: update (rows of flat indices [start, start + n)), merge, result."""

    def __init__(self, fit: FitSpec, maps: Sequence[FitMap]):
        self.fit, self.maps = fit, list(maps)
        if any(m.cells > MAX_CELLS for m in self.maps):
            raise ValueError("a fit map has at most 2^24 cells")
        self.n_valid = self.n_invalid = 0
        self.n_within = np.zeros(MAX_LEVELS, dtype=np.int64)
        self.best_chi2, self.best_idx = np.float64(np.inf), -1
        self.col_min = np.full(6, np.inf)      # +inf / -inf: no finite value yet
        self.col_max = np.full(6, -np.inf)
        self.col_bad = np.zeros(6, dtype=np.int64)
        self.map_chi2 = [np.full(m.cells, np.inf) for m in self.maps]
        self.map_idx = [np.full(m.cells, -1, dtype=np.int64) for m in self.maps]
        self.sel = np.empty(0, dtype=np.int64)
        self.sel_total = 0

    def update(self, rows, start: int) -> None:
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
        n = rows.shape[0]
        if n == 0:
            return
        c = chi2_rows(self.fit, rows)
        valid = np.isfinite(c)
        idx = np.arange(start, start + n, dtype=np.int64)
        self.n_valid += int(valid.sum())
        self.n_invalid += int(n - valid.sum())
        fin = np.isfinite(rows)
        for j in range(6):
            col = rows[fin[:, j], j]
            if col.size:
                self.col_min[j] = min(self.col_min[j], col.min())
                self.col_max[j] = max(self.col_max[j], col.max())
            self.col_bad[j] += n - col.size
        cv, iv = c[valid], idx[valid]
        if cv.size == 0:
            return
        for l, lev in enumerate(self.fit.levels):
            self.n_within[l] += int((cv <= lev).sum())
        m = cv.min()
        i = int(iv[cv == m].min())
        if m < self.best_chi2 or (m == self.best_chi2 and i < self.best_idx):
            self.best_chi2, self.best_idx = np.float64(m), i
        for k, fm in enumerate(self.maps):
            cells, inv = np.unique(fm.cell(iv), return_inverse=True)
            inv = inv.reshape(-1)
            cm = np.full(cells.size, np.inf)
            np.minimum.at(cm, inv, cv)
            eq = cv == cm[inv]
            im = np.full(cells.size, np.iinfo(np.int64).max, dtype=np.int64)
            np.minimum.at(im, inv[eq], iv[eq])
            self._take(k, cells, cm, im)
        if self.fit.select is not None:
            level, cap = self.fit.select
            s = iv[cv <= level]
            self.sel = np.concatenate([self.sel, s[:max(0, cap - self.sel.size)]])
            self.sel_total += int(s.size)

    def _take(self, k: int, cells, chi2, idx) -> None:
        """Cells `cells` of map k <- the smaller chi2, on a tie the lower index (-1 = empty loses)."""
        cc, ci = self.map_chi2[k][cells], self.map_idx[k][cells]
        take = (chi2 < cc) | ((chi2 == cc) & (idx.view(np.uint64) < ci.view(np.uint64)))
        self.map_chi2[k][cells] = np.where(take, chi2, cc)
        self.map_idx[k][cells] = np.where(take, idx, ci)

    def merge(self, o: "HostFit") -> None:
        """Fold in the state of other (disjoint) rows; selections concatenate in call order."""
        self.n_valid += o.n_valid
        self.n_invalid += o.n_invalid
        self.n_within += o.n_within
        if o.best_chi2 < self.best_chi2 or (o.best_chi2 == self.best_chi2 and
                                            np.uint64(o.best_idx & 0xFFFFFFFFFFFFFFFF) <
                                            np.uint64(self.best_idx & 0xFFFFFFFFFFFFFFFF)):
            self.best_chi2, self.best_idx = o.best_chi2, o.best_idx
        self.col_min = np.minimum(self.col_min, o.col_min)
        self.col_max = np.maximum(self.col_max, o.col_max)
        self.col_bad += o.col_bad
        for k in range(len(self.maps)):
            self._take(k, np.arange(self.maps[k].cells), o.map_chi2[k], o.map_idx[k])
        if self.fit.select is not None:
            self.sel = np.concatenate([self.sel, o.sel])[:self.fit.select[1]]
        self.sel_total += o.sel_total

    # -- the state as 64-bit words (include/lzq.h): what the ranks of a sharded sweep exchange ----
    def to_words(self) -> np.ndarray:
        w = np.zeros(state_words(self.maps), dtype=np.int64)
        w[W_NVALID], w[W_NINVALID] = self.n_valid, self.n_invalid
        w[W_WITHIN:W_WITHIN + MAX_LEVELS] = self.n_within
        w[W_BEST_CHI2] = np.float64(self.best_chi2).view(np.int64)
        w[W_BEST_IDX] = self.best_idx
        w[W_COLMIN:W_COLMIN + 6] = np.where(np.isfinite(self.col_min), _key(self.col_min), _ALL).view(np.int64)
        w[W_COLMAX:W_COLMAX + 6] = np.where(np.isfinite(self.col_max), _key(self.col_max), np.uint64(0)).view(np.int64)
        w[W_COLBAD:W_COLBAD + 6] = self.col_bad
        w[W_SEL_TOTAL] = self.sel_total
        off = HEADER_WORDS
        for k, m in enumerate(self.maps):
            w[off:off + m.cells] = self.map_chi2[k].view(np.int64)
            w[off + m.cells:off + 2 * m.cells] = self.map_idx[k]
            off += 2 * m.cells
        return w

    @classmethod
    def from_words(cls, fit: FitSpec, maps: Sequence[FitMap], words, selected=None) -> "HostFit":
        w = np.ascontiguousarray(np.asarray(words), dtype=np.int64).reshape(-1)
        if w.size != state_words(maps):
            raise ValueError(f"fit state of {w.size} words, expected {state_words(maps)} for these maps")
        s = cls(fit, maps)
        s.n_valid, s.n_invalid = int(w[W_NVALID]), int(w[W_NINVALID])
        s.n_within = w[W_WITHIN:W_WITHIN + MAX_LEVELS].copy()
        s.best_chi2, s.best_idx = w[W_BEST_CHI2:W_BEST_CHI2 + 1].view(np.float64)[0], int(w[W_BEST_IDX])
        kmin, kmax = w[W_COLMIN:W_COLMIN + 6].view(np.uint64), w[W_COLMAX:W_COLMAX + 6].view(np.uint64)
        s.col_min = np.where(kmin == _ALL, np.inf, _unkey(np.where(kmin == _ALL, _TOP, kmin)))
        s.col_max = np.where(kmax == 0, -np.inf, _unkey(np.where(kmax == 0, _TOP, kmax)))
        s.col_bad = w[W_COLBAD:W_COLBAD + 6].copy()
        s.sel_total = int(w[W_SEL_TOTAL])
        off = HEADER_WORDS
        for k, m in enumerate(maps):
            s.map_chi2[k] = w[off:off + m.cells].view(np.float64).copy()
            s.map_idx[k] = w[off + m.cells:off + 2 * m.cells].copy()
            off += 2 * m.cells
        if selected is not None:
            s.sel = np.asarray(selected, dtype=np.int64).reshape(-1)
        return s

    def result(self) -> dict:
        cols = {}
        for j, f in enumerate(YIELD_FIELDS):
            any_fin = np.isfinite(self.col_min[j])
            cols[f] = {"min": float(self.col_min[j]) if any_fin else None,
                       "max": float(self.col_max[j]) if any_fin else None, "n_nonfinite": int(self.col_bad[j])}
        res = {"n_valid": int(self.n_valid), "n_invalid": int(self.n_invalid),
               "n_within": [int(x) for x in self.n_within[:len(self.fit.levels)]],
               "best": {"chi2": float(self.best_chi2), "index": int(self.best_idx)}, "columns": cols,
               "maps": [{"axes": list(m.axes), "chi2_min": self.map_chi2[k].reshape(m.len).copy(),
                         "argmin": self.map_idx[k].reshape(m.len).copy()} for k, m in enumerate(self.maps)],
               "selected": None, "n_selected": None}
        if self.fit.select is not None:
            res["selected"], res["n_selected"] = self.sel.copy(), int(self.sel_total)
        return res


def differences(a: dict, b: dict) -> List[str]:
    """Where two fit results differ: chi2 by bits, indices and counts exactly, the column extrema
    as values.  Empty when they are the same fit."""
    out = []
    for k in ("n_valid", "n_invalid", "n_within", "n_selected"):
        if a[k] != b[k]:
            out.append(f"{k}: {a[k]} != {b[k]}")
    bits = lambda x: np.asarray(x, dtype=np.float64).view(np.int64)
    if bits(a["best"]["chi2"]) != bits(b["best"]["chi2"]) or a["best"]["index"] != b["best"]["index"]:
        out.append(f"best: {a['best']} != {b['best']}")
    if a["columns"] != b["columns"]:
        out.append(f"columns: {a['columns']} != {b['columns']}")
    if len(a["maps"]) != len(b["maps"]):
        out.append("number of maps")
    for k, (ma, mb) in enumerate(zip(a["maps"], b["maps"])):
        if ma["axes"] != mb["axes"] or ma["chi2_min"].shape != mb["chi2_min"].shape:
            out.append(f"map {k}: axes / shape")
        elif not np.array_equal(bits(ma["chi2_min"]), bits(mb["chi2_min"])):
            out.append(f"map {k}: chi2_min differs in {int((bits(ma['chi2_min']) != bits(mb['chi2_min'])).sum())} cells")
        elif not np.array_equal(ma["argmin"], mb["argmin"]):
            out.append(f"map {k}: argmin differs in {int((ma['argmin'] != mb['argmin']).sum())} cells")
    if (a["selected"] is None) != (b["selected"] is None) or \
            (a["selected"] is not None and not np.array_equal(a["selected"], b["selected"])):
        out.append("selected indices differ")
    return out


# ---- posterior: likelihood-weighted sums as exact integers -------------------------------------
def post_state_words(maps: Sequence[FitMap]) -> int:
    return PW_MAPS + 2 * sum(m.cells for m in maps)


def post_weights(fit: FitSpec, offset: float, rows) -> np.ndarray:
    """q of (n, 6) float64 records (uint64; Q_INVALID / Q_ABOVE for rows without weight), from the
    library's host build of the one definition (lzq_post_weights_host; no GPU is touched)."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, 6))
    terms = (_native.LzqFitTerm * len(fit.terms))()
    for k, t in enumerate(fit.terms):
        terms[k].field, terms[k].target, terms[k].sigma = YIELD_FIELDS.index(t.field), t.target, t.sigma
    q = np.empty(rows.shape[0], dtype=np.uint64)
    lib = _native.load()
    _native.check(lib.lzq_post_weights_host(terms, len(fit.terms), float(offset), rows.ctypes.data, rows.shape[0],
                                            q.ctypes.data), lib)
    return q


def _pair(w: np.ndarray, k: int) -> int:
    return (int(w[k]) << 31) + int(w[k + 1])


class HostPosterior:
    """The posterior state in numpy: `w`, the uint64 words of include/lzq.h's "posterior state".
    update (rows of flat indices [start, start + n)), merge, result."""

    def __init__(self, fit: FitSpec, maps: Sequence[FitMap], offset: float, axis_values: Optional[dict] = None):
        self.fit, self.maps, self.offset = fit, list(maps), float(offset)
        if not (math.isfinite(self.offset) and self.offset >= 0):
            raise ValueError(f"posterior offset must be finite and >= 0, got {offset!r}")
        if any(m.cells > MAX_CELLS for m in self.maps):
            raise ValueError("a fit map has at most 2^24 cells")
        self.axis_values = dict(axis_values or {})
        self.w = np.zeros(post_state_words(self.maps), dtype=np.uint64)
        self.rows = 0    # rows folded in, merges included: the exact sums hold up to POST_MAX_ROWS

    def _count(self, n: int) -> None:
        if self.rows + n > POST_MAX_ROWS:
            raise ValueError(f"a posterior state takes at most 2^32 rows (exact 64-bit sums), got {self.rows + n}")
        self.rows += n

    def update(self, rows, start: int) -> None:
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
        n = rows.shape[0]
        if n == 0:
            return
        self._count(n)
        q = post_weights(self.fit, self.offset, rows)
        inv, above, zero = q == np.uint64(Q_INVALID), q == np.uint64(Q_ABOVE), q == np.uint64(0)
        used = ~(inv | above | zero)
        w = self.w
        for k, mask in ((PW_NUSED, used), (PW_NZERO, zero), (PW_NABOVE, above), (PW_NINVALID, inv)):
            w[k] += np.uint64(int(mask.sum()))
        if not used.any():
            return
        qu = q[used]
        hi, lo = qu >> np.uint64(31), qu & np.uint64(0x7FFFFFFF)
        c = chi2_rows(self.fit, rows)[used]
        idx = np.arange(start, start + n, dtype=np.int64)[used]

        def add(word, mask=None):
            w[word] += hi.sum(dtype=np.uint64) if mask is None else hi[mask].sum(dtype=np.uint64)
            w[word + 1] += lo.sum(dtype=np.uint64) if mask is None else lo[mask].sum(dtype=np.uint64)
        add(PW_Z)
        for l, lev in enumerate(self.fit.levels):
            add(PW_LEVEL + 2 * l, c <= lev)
        b = np.minimum(POST_BINS - 1, ((c - self.offset) * 16.0).astype(np.int64))
        np.add.at(w, PW_HIST + 2 * b, hi)
        np.add.at(w, PW_HIST + 2 * b + 1, lo)
        off = PW_MAPS
        for fm in self.maps:
            cell = fm.cell(idx)
            np.add.at(w, off + 2 * cell, hi)
            np.add.at(w, off + 2 * cell + 1, lo)
            off += 2 * fm.cells

    def merge(self, o: "HostPosterior") -> None:
        """Fold in the state of other (disjoint) rows at the same offset: word-wise addition."""
        if o.offset != self.offset or o.w.size != self.w.size:
            raise ValueError("posterior merge: states of different offsets or layouts")
        self._count(o.rows)
        self.w += o.w

    def to_words(self) -> np.ndarray:
        return self.w.view(np.int64).copy()

    @classmethod
    def from_words(cls, fit: FitSpec, maps: Sequence[FitMap], offset: float, words,
                   axis_values: Optional[dict] = None) -> "HostPosterior":
        w = np.ascontiguousarray(np.asarray(words), dtype=np.int64).reshape(-1)
        s = cls(fit, maps, offset, axis_values)
        if w.size != s.w.size:
            raise ValueError(f"posterior state of {w.size} words, expected {s.w.size} for these maps")
        s.w = w.view(np.uint64).copy()
        s.rows = int(sum(int(x) for x in s.w[:4]))
        return s

    def result(self) -> dict:
        """Host values of the state.  Everything is computed from the exact integers in a fixed
        order (integer arithmetic, correctly rounded int / int divisions, math.fsum), so every rank
        that holds the same words gets the same floats."""
        w = self.w
        Z = _pair(w, PW_Z)
        hist = w[PW_HIST:PW_MAPS].reshape(POST_BINS, 2).copy()
        cum, binned, edges = [], 0, []
        for b in range(POST_BINS):
            binned += (int(hist[b, 0]) << 31) + int(hist[b, 1])
            cum.append(binned)
        for p in self.fit.posterior["credible"] if self.fit.posterior else DEFAULT_CREDIBLE:
            edge = None
            if binned > 0:
                fp = Fraction(p)    # exact: the first bin with cum >= p * binned, in integers
                b = next(b for b in range(POST_BINS) if cum[b] * fp.denominator >= fp.numerator * binned)
                edge = None if b == POST_BINS - 1 else (b + 1) / 16.0
            edges.append({"p": p, "delta_chi2": edge})
        res = {"offset": self.offset, "n_used": int(w[PW_NUSED]), "n_zero": int(w[PW_NZERO]),
               "n_above": int(w[PW_NABOVE]), "n_invalid": int(w[PW_NINVALID]),
               "Z": Z / POST_UNIT, "Z_units": str(Z),
               "mass_within": [(_pair(w, PW_LEVEL + 2 * l) / Z if Z else None) for l in range(len(self.fit.levels))],
               "credible": edges, "hist": hist, "maps": []}
        off = PW_MAPS
        for m in self.maps:
            pairs = w[off:off + 2 * m.cells].reshape(m.cells, 2).copy()
            off += 2 * m.cells
            # a cell's weight as a float: hi * 2^31 is exact below 2^84, the sum rounds once
            wf = pairs[:, 0].astype(np.float64) * 2.0 ** 31 + pairs[:, 1].astype(np.float64)
            post = (wf / np.float64(Z) if Z else np.full(m.cells, np.nan)).reshape(m.len)
            mean = std = None
            x = self.axis_values.get(m.axes[0]) if len(m.axes) == 1 else None
            if x is not None and Z and len(x) == m.cells:
                x = [float(v) for v in x]
                pl = [float(v) for v in post]
                mean = math.fsum(p * v for p, v in zip(pl, x))
                std = math.sqrt(max(0.0, math.fsum(p * (v - mean) ** 2 for p, v in zip(pl, x))))
            res["maps"].append({"axes": list(m.axes), "weight": pairs, "posterior": post, "mean": mean, "std": std})
        return res


def post_differences(a: dict, b: dict) -> List[str]:
    """Where two posterior results differ (exact integers, floats by bits); empty when equal."""
    out = []
    bits = lambda x: np.asarray(x, dtype=np.float64).view(np.int64)
    for k in ("offset", "n_used", "n_zero", "n_above", "n_invalid", "Z_units", "Z", "mass_within", "credible"):
        if a[k] != b[k]:
            out.append(f"{k}: {a[k]} != {b[k]}")
    if not np.array_equal(a["hist"], b["hist"]):
        out.append(f"hist differs in {int((a['hist'] != b['hist']).any(axis=1).sum())} bins")
    if len(a["maps"]) != len(b["maps"]):
        out.append("number of maps")
    for k, (ma, mb) in enumerate(zip(a["maps"], b["maps"])):
        if ma["axes"] != mb["axes"] or ma["weight"].shape != mb["weight"].shape:
            out.append(f"map {k}: axes / shape")
        elif not np.array_equal(ma["weight"], mb["weight"]):
            out.append(f"map {k}: weight differs in {int((ma['weight'] != mb['weight']).any(axis=1).sum())} cells")
        elif not np.array_equal(bits(ma["posterior"]), bits(mb["posterior"])) or \
                (ma["mean"], ma["std"]) != (mb["mean"], mb["std"]):
            out.append(f"map {k}: posterior / mean / std")
    return out


# ---- accumulators: what the sweep driver folds chunks into -----------------------------------
class HostAccumulator:
    """Chunks of CPU records (the gloo tests, any host table) into a HostFit."""

    def __init__(self, fit: FitSpec, maps: Sequence[FitMap], axis_values: Optional[dict] = None):
        self.fit, self.maps, self.axis_values = fit, list(maps), axis_values
        self.host = HostFit(fit, maps)
        self.post = None    # a numeric posterior offset is folded chunk by chunk; "best" after the combine
        if fit.posterior is not None and fit.posterior["offset"] != "best":
            self.post_begin(fit.posterior["offset"])

    def update(self, rows, start: int) -> None:
        rows = rows.detach().numpy() if hasattr(rows, "detach") else rows
        self.host.update(rows, start)
        if self.post is not None:
            self.post.update(rows, start)

    def post_begin(self, offset: float) -> None:
        self.post = HostPosterior(self.fit, self.maps, offset, self.axis_values)

    def post_update(self, rows, start: int) -> None:
        self.post.update(rows.detach().cpu().numpy() if hasattr(rows, "detach") else rows, start)

    def post_words(self):
        import torch
        return torch.from_numpy(self.post.to_words())

    def post_result(self) -> dict:
        return self.post.result()

    def post_merged(self, words) -> dict:
        """The result of the ranks' posterior states `words` [world, n] summed."""
        import torch
        tot = HostPosterior(self.fit, self.maps, self.post.offset, self.axis_values)
        for w in torch.as_tensor(words).cpu().numpy():
            tot.merge(HostPosterior.from_words(self.fit, self.maps, self.post.offset, w))
        return tot.result()

    def words(self):
        import torch
        return torch.from_numpy(self.host.to_words())

    def selected(self):
        import torch
        return torch.from_numpy(self.host.sel.copy())

    def result(self) -> dict:
        return self.host.result()

    def merged(self, words, selected) -> dict:
        """The result of the ranks' states `words` [world, n] merged in rank order."""
        import torch
        tot = HostFit(self.fit, self.maps)
        for w in torch.as_tensor(words).cpu().numpy():
            tot.merge(HostFit.from_words(self.fit, self.maps, w))
        if selected is not None:
            tot.sel = selected.cpu().numpy()
        return tot.result()


class DeviceAccumulator:
    """Chunks of device records into a device-resident state (lzq_fit_update / lzq_fit_select on the
    current stream, behind the chunk's own kernels)."""

    def __init__(self, fit: FitSpec, maps: Sequence[FitMap], engine, axis_values: Optional[dict] = None):
        self.fit, self.maps, self.engine, self.axis_values = fit, list(maps), engine, axis_values
        self.state = engine.fit_state(fit, maps)
        self.post = None
        if fit.posterior is not None and fit.posterior["offset"] != "best":
            self.post_begin(fit.posterior["offset"])

    def update(self, rows, start: int) -> None:
        self.engine.fit_update(self.state, rows, start)
        if self.fit.select is not None:
            self.engine.fit_select(self.state, rows, start)
        if self.post is not None:   # right behind the fit, on the same stream
            self.engine.post_update(self.post, rows, start)

    def post_begin(self, offset: float) -> None:
        self.post = self.engine.post_state(self.fit, self.maps, offset)

    def post_update(self, rows, start: int) -> None:
        self.engine.post_update(self.post, rows, start)

    def post_words(self):
        return self.post.words

    def post_result(self) -> dict:
        return self.engine.post_result(self.post, self.axis_values)

    def post_merged(self, words) -> dict:
        tot = self.engine.post_state(self.fit, self.maps, self.post.offset)
        for w in words:
            self.engine.post_merge(tot, w)
        return self.engine.post_result(tot, self.axis_values)

    def words(self):
        return self.state.words

    def selected(self):
        kept = min(int(self.state.words[W_SEL_TOTAL]), self.fit.select[1])
        return self.state.sel[:kept]

    def result(self) -> dict:
        return self.engine.fit_result(self.state)

    def merged(self, words, selected) -> dict:
        tot = self.engine.fit_state(self.fit, self.maps, select=False)
        for w in words:
            self.engine.fit_merge(tot, w)
        return self.engine.fit_result(tot, selected=selected)


def make_accumulator(fit: FitSpec, maps: Sequence[FitMap], engine=None, axis_values: Optional[dict] = None):
    """engine None: records are CPU tensors / arrays (numpy); else the engine's device.
    axis_values (FitSpec.axis_values): the sweep axes' values, for the posterior's means."""
    if engine is None:
        return HostAccumulator(fit, maps, axis_values)
    return DeviceAccumulator(fit, maps, engine, axis_values)


def _gather_words(src, world: int, group):
    import torch
    import torch.distributed as dist
    flat = torch.empty(world * src.numel(), dtype=torch.int64, device=src.device)   # (gloo takes a flat output)
    dist.all_gather_into_tensor(flat, src, group=group)
    return flat.view(world, src.numel())


def combine_posterior(acc, res: dict, local=None, start: int = 0, group=None) -> dict:
    """The posterior of the whole grid on every rank.  A numeric offset was folded chunk by chunk;
    "best" is the combined fit's best chi2 (`res`, identical on every rank; 0 when no row is valid)
    and is applied now, in a second pass over the rank's own shard `local` (rows of flat indices
    from `start`).  The ranks' states are all-gathered and summed."""
    import torch.distributed as dist
    if acc.fit.posterior["offset"] == "best":
        if local is None:
            raise ValueError(NO_TABLE_BEST)
        acc.post_begin(float(res["best"]["chi2"]) if res["best"]["index"] >= 0 else 0.0)
        acc.post_update(local, start)
    if not (dist.is_available() and dist.is_initialized()):
        return acc.post_result()
    w = acc.post_words()
    src = (w if dist.get_backend(group) == "nccl" else w.cpu()).contiguous()
    return acc.post_merged(_gather_words(src, dist.get_world_size(group), group))


def combine(acc, world: int = 1, group=None, local=None, start: int = 0) -> dict:
    """The fit of the whole grid on every rank: the ranks' fixed-size states all-gathered and
    merged in rank order, their selection lists concatenated in rank order and cut to `cap`
    (shards are contiguous and ascending, so the list stays ascending).  Without a process group
    the rank's own result.  A fit with a "posterior" key gets result["posterior"]
    (combine_posterior; `local`, `start`: the rank's shard, for the offset "best")."""
    res = _combine_fit(acc, group)
    if acc.fit.posterior is not None:
        res["posterior"] = combine_posterior(acc, res, local, start, group)
    return res


def _combine_fit(acc, group=None) -> dict:
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return acc.result()
    world = dist.get_world_size(group)
    nccl = dist.get_backend(group) == "nccl"
    w = acc.words()
    src = (w if nccl else w.cpu()).contiguous()
    flat = torch.empty(world * src.numel(), dtype=torch.int64, device=src.device)   # (gloo takes a flat output)
    dist.all_gather_into_tensor(flat, src, group=group)
    allw = flat.view(world, src.numel())
    selected = None
    if acc.fit.select is not None:
        cap = acc.fit.select[1]
        kept = [min(int(t), cap) for t in allw[:, W_SEL_TOTAL].cpu()]
        m = max(kept + [1])
        mine = acc.selected()
        pad = torch.zeros(m, dtype=torch.int64, device=src.device)
        pad[:mine.numel()] = mine.to(src.device)
        alls = torch.empty(world * m, dtype=torch.int64, device=src.device)
        dist.all_gather_into_tensor(alls, pad, group=group)
        alls = alls.view(world, m)
        selected = torch.cat([alls[r, :kept[r]] for r in range(world)])[:cap]
    return acc.merged(allw, selected)


def best_point_yields(compute, best: int, make_out, engine=None) -> Optional[np.ndarray]:
    """The six yields of grid index `best`, evaluated again through the sweep's own compute function
    (the shard invariant makes them the table's row bit for bit).  The compute function's run
    statistics (ODE status counts, reuse mode) are left as the sweep set them."""
    if best < 0:
        return None
    st, tb = getattr(compute, "ode_status", None), getattr(compute, "ode_tables", None)
    keep = (None if st is None else st.copy(), None if tb is None else dict(tb), getattr(engine, "last_reuse", None))
    out = make_out(1)
    compute(int(best), 1, out)
    if st is not None:
        st[:] = keep[0]
    if tb is not None:
        tb.update(keep[1])
    if engine is not None:
        engine.last_reuse = keep[2]
    return out.detach().cpu().numpy().reshape(6).copy()


def report(fit: FitSpec, result: dict, sweep_spec, n_points: int, best_yields: Optional[np.ndarray]) -> dict:
    """fit.json / summary.json's "fit" block: the spec, the counts, the column extrema and the best
    point (index, axis values, yields); the maps and the selection go to their own files."""
    b = result["best"]
    best = {"chi2": b["chi2"] if b["index"] >= 0 else None, "index": b["index"], "params": None, "final": None}
    if b["index"] >= 0:
        best["params"] = sweep_spec.point_params(b["index"])
        if best_yields is not None:
            best["final"] = dict(zip(YIELD_FIELDS, map(float, best_yields)))
    rep = {"spec": fit.to_json(), "sweep": sweep_spec.name, "n_points": int(n_points),
            "n_valid": result["n_valid"], "n_invalid": result["n_invalid"], "levels": list(fit.levels),
            "n_within": result["n_within"], "columns": result["columns"], "best": best,
            "maps": [{"axes": m["axes"], "shape": list(m["chi2_min"].shape)} for m in result["maps"]],
            "n_selected": result["n_selected"],
            "n_selected_kept": None if result["selected"] is None else int(len(result["selected"]))}
    if result.get("posterior") is not None:
        p = result["posterior"]
        rep["posterior"] = {**{k: p[k] for k in ("offset", "n_used", "n_zero", "n_above", "n_invalid", "Z", "Z_units",
                                                 "mass_within", "credible")},
                            "maps": [{"axes": m["axes"], "mean": m["mean"], "std": m["std"]} for m in p["maps"]]}
    return rep


def write_files(out_dir: str, rep: dict, result: dict) -> None:
    """fit.json, fit_maps.npz (map<k>_chi2_min / map<k>_argmin; with a posterior map<k>_posterior and
    map<k>_weight, the (cells, 2) uint64 pairs) and selected.npy in `out_dir`."""
    import os
    with open(os.path.join(out_dir, "fit.json"), "w") as f:
        json.dump(rep, f, indent=2)
    arrays = {}
    for k, m in enumerate(result["maps"]):
        arrays[f"map{k}_chi2_min"], arrays[f"map{k}_argmin"] = m["chi2_min"], m["argmin"]
    if result.get("posterior") is not None:
        for k, m in enumerate(result["posterior"]["maps"]):
            arrays[f"map{k}_posterior"], arrays[f"map{k}_weight"] = m["posterior"], m["weight"]
    np.savez(os.path.join(out_dir, "fit_maps.npz"), **arrays)
    sel = result["selected"] if result["selected"] is not None else np.empty(0, dtype=np.int64)
    np.save(os.path.join(out_dir, "selected.npy"), np.asarray(sel, dtype=np.int64), allow_pickle=False)
