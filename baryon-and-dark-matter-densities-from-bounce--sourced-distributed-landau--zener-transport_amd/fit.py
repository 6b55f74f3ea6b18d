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
Engine.fit_*) against it.  The three numpy states here and the three device states of engine.py
follow one protocol -- update(rows, start), words, like(), merge_words(words), result(...) -- so
one Accumulator and one combine() serve both.

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

The optional top-level key "observables" describes the OUTPUTS: a list of 0..4 histograms over one
or two yield fields,

    "observables": [{"axes": [{"field": "DM_over_B", "lo": 0.01, "hi": 1000.0, "per_octave": 8}]},
                    {"axes": [{"field": "Y_B", "lo": 0.0, "hi": 2e-10, "bins": 200},
                              {"field": "DM_over_B", "lo": 0.0, "hi": 10.0, "bins": 100}],
                     "quantiles": [0.16, 0.5, 0.84]}]

"bins" makes an axis linear, "per_octave" (1, 2, .. 256) binary-logarithmic: its bins are the
exponent and the leading mantissa bits of the value, so sub-bins are linear inside an octave and
no logarithm is taken.  Per cell the state (include/lzq.h, "sweep observables") holds the number
of valid rows, their smallest chi2 (the profile likelihood of the field) and, with a posterior,
their weight: a third device-resident state, folded behind the fit's (and with the offset "best"
in the posterior's second pass), with the same independence of chunking, sharding and world
size.  HostObservables is the numpy implementation, written from the definition;
Engine.obs_* drive the HIP kernel (lzq_obs_update).  "quantiles" (1-D observables with weight;
default 0.025, 0.16, 0.5, 0.84, 0.975) are read from the cumulated weights in exact integers.

The optional key "ranked": {"n": 1000} (n in 1..4096) keeps the n rows of smallest chi2 themselves,
in order, each with its flat index and its record: a fourth state (include/lzq.h, "ranked points"),
folded behind the fit's and independent of the posterior, so it works with --no-table.  Rows are
ordered by (chi2 bits, flat index) -- a strict total order, since indices are distinct -- so the list
is one fixed list for every chunking, sharding, world size and merge order.  HostRanked is the numpy
implementation (a lexsort over the old entries and the chunk); Engine.rank_* drive the HIP kernels
(lzq_rank_update).  The result goes to fit.json's "ranked" block and to fit_ranked.npz (index, chi2,
records and params, the sweep axes' values of each point).
"""
from __future__ import annotations

import ctypes
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
OBS_MAX, OBS_MAX_CELLS = _native.OBS_MAX, _native.OBS_MAX_CELLS
OBS_LDS_CELLS, OBS_HEADER_WORDS = _native.OBS_LDS_CELLS, _native.OBS_HEADER_WORDS
OBS_OUT, OBS_NONFINITE = -1, -2          # lzq_obs_cells_host's classes of a row without a cell
DEFAULT_QUANTILES = (0.025, 0.16, 0.5, 0.84, 0.975)
RANK_MAX_N, RANK_HEADER_WORDS = _native.RANK_MAX_N, _native.RANK_HEADER_WORDS
RW_N, RW_FILLED, RW_NVALID, RW_NINVALID = 0, 1, 2, 3     # word offsets of the ranked state (include/lzq.h)
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


def _obs_number(x, what: str) -> float:
    if isinstance(x, (bool, str)) or not isinstance(x, (int, float)) or not math.isfinite(x):
        raise ValueError(f"fit observables: {what} must be a finite number, got {x!r}")
    return float(x)


@dataclass(frozen=True)
class ObsAxis:
    """One axis of an observable over a yield field: linear (`bins`) or binary-logarithmic
    (`per_octave` = 2^s sub-bins per octave).  The bin of a value is include/lzq.h's definition."""
    field: str
    lo: float
    hi: float
    bins: Optional[int] = None
    per_octave: Optional[int] = None

    def __post_init__(self):
        if self.field not in YIELD_FIELDS:
            raise ValueError(f"fit observables: unknown field {self.field!r} (one of {YIELD_FIELDS})")
        lo, hi = _obs_number(self.lo, "lo"), _obs_number(self.hi, "hi")
        if not lo < hi:
            raise ValueError(f"fit observables: axis {self.field} needs lo < hi, got {lo!r}, {hi!r}")
        if (self.bins is None) == (self.per_octave is None):
            raise ValueError(f'fit observables: axis {self.field} takes exactly one of "bins" and "per_octave"')
        if self.bins is not None:
            if isinstance(self.bins, bool) or not isinstance(self.bins, int) or not 1 <= self.bins <= OBS_MAX_CELLS:
                raise ValueError(f"fit observables: axis {self.field}: bins is an integer in 1..2^20, "
                                 f"got {self.bins!r}")
            with np.errstate(all="ignore"):
                inv = np.float64(self.bins) / (np.float64(hi) - np.float64(lo))
            if not (np.isfinite(inv) and inv > 0):
                raise ValueError(f"fit observables: axis {self.field}: bins / (hi - lo) must be finite and > 0")
        else:
            po = self.per_octave
            if isinstance(po, bool) or not isinstance(po, int) or po not in (1, 2, 4, 8, 16, 32, 64, 128, 256):
                raise ValueError(f"fit observables: axis {self.field}: per_octave is a power of two in 1..256, "
                                 f"got {po!r}")
            if not lo > 0:
                raise ValueError(f"fit observables: a logarithmic axis ({self.field}) needs lo > 0, got {lo!r}")
            if self.n_bins < 1:
                raise ValueError(f"fit observables: axis {self.field}: no sub-bin edge between lo and hi")
        object.__setattr__(self, "lo", lo)
        object.__setattr__(self, "hi", hi)

    @property
    def log(self) -> bool:
        return self.per_octave is not None

    @property
    def log2_sub(self) -> int:
        return int(self.per_octave).bit_length() - 1

    def _key(self, x) -> np.ndarray:
        """bits(x) >> (52 - s) of positive doubles."""
        return (np.asarray(x, dtype=np.float64).view(np.uint64) >> np.uint64(52 - self.log2_sub)).astype(np.int64)

    @property
    def n_bins(self) -> int:
        if not self.log:
            return int(self.bins)
        return int(self._key([self.hi])[0] - self._key([self.lo])[0])

    @property
    def inv(self) -> np.float64:
        return np.float64(self.bins) / (np.float64(self.hi) - np.float64(self.lo))

    def bin(self, x: np.ndarray) -> np.ndarray:
        """The bin of each value (int64), OBS_OUT below or above the range; non-finite values are
        the caller's (Observable.cell)."""
        x = np.asarray(x, dtype=np.float64)
        b = np.full(x.shape, OBS_OUT, dtype=np.int64)
        fin = np.isfinite(x)
        if self.log:
            m = fin & (x > 0.0)
            k = self._key(x[m]) - self._key([self.lo])[0]
            b[m] = np.where((k >= 0) & (k < self.n_bins), k, OBS_OUT)
        else:
            m = fin & (x >= self.lo) & (x < self.hi)
            t = (x[m] - np.float64(self.lo)) * self.inv        # two roundings, as the kernel's
            b[m] = np.minimum(self.bins - 1, t.astype(np.int64))
        return b

    def edges(self) -> np.ndarray:
        """The n_bins + 1 bin edges.  A logarithmic axis starts at lo rounded DOWN to a sub-bin edge
        (and ends at hi rounded down to one): the edges the bins really have."""
        e = np.arange(self.n_bins + 1, dtype=np.int64)
        if self.log:
            return ((self._key([self.lo])[0] + e).astype(np.uint64) << np.uint64(52 - self.log2_sub)).view(np.float64)
        out = np.float64(self.lo) + e * ((np.float64(self.hi) - np.float64(self.lo)) / np.float64(self.bins))
        out[-1] = self.hi
        return out

    def to_json(self) -> dict:
        d = {"field": self.field, "lo": self.lo, "hi": self.hi}
        d.update({"per_octave": self.per_octave} if self.log else {"bins": self.bins})
        return d


@dataclass(frozen=True)
class Observable:
    """A histogram over one or two different yield fields; cell b0, or b0 * bins1 + b1."""
    axes: Tuple[ObsAxis, ...]
    quantiles: Tuple[float, ...] = DEFAULT_QUANTILES

    def __post_init__(self):
        if not 1 <= len(self.axes) <= 2 or len({a.field for a in self.axes}) != len(self.axes):
            raise ValueError("fit observables: an observable has one or two axes over different fields")
        if self.cells > OBS_MAX_CELLS:
            raise ValueError(f"fit observables: {self.cells} cells (at most 2^20 an observable)")
        q = self.quantiles
        if any(not 0.0 < x < 1.0 for x in q) or any(b <= a for a, b in zip(q, q[1:])):
            raise ValueError(f"fit observables: quantiles must be ascending and inside (0, 1), got {list(q)}")

    @property
    def shape(self) -> Tuple[int, ...]:
        return tuple(a.n_bins for a in self.axes)

    @property
    def cells(self) -> int:
        return int(np.prod(self.shape, dtype=np.int64))

    def cell(self, rows: np.ndarray) -> np.ndarray:
        """The class of (n, 6) records: the cell, OBS_OUT or OBS_NONFINITE (int64)."""
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
        cols = [rows[:, YIELD_FIELDS.index(a.field)] for a in self.axes]
        bins = [a.bin(x) for a, x in zip(self.axes, cols)]
        cell = bins[0] if len(bins) == 1 else bins[0] * self.shape[1] + bins[1]
        cell = np.where(np.logical_and.reduce([b >= 0 for b in bins]), cell, OBS_OUT)
        return np.where(np.logical_and.reduce([np.isfinite(x) for x in cols]), cell, OBS_NONFINITE)

    def to_json(self) -> dict:
        return {"axes": [a.to_json() for a in self.axes], "quantiles": list(self.quantiles)}

    @classmethod
    def from_json(cls, d) -> "Observable":
        if not isinstance(d, dict) or set(d) - {"axes", "quantiles"} or not isinstance(d.get("axes"), (list, tuple)):
            raise ValueError(f'fit observables: an object with the keys "axes" (a list) and "quantiles", got {d!r}')
        axes = []
        for a in d["axes"]:
            if not isinstance(a, dict) or set(a) - {"field", "lo", "hi", "bins", "per_octave"} or \
                    not {"field", "lo", "hi"} <= set(a) or not isinstance(a["field"], str):
                raise ValueError('fit observables: an axis is an object with "field", "lo", "hi" and one of "bins" and '
                                 f'"per_octave", got {a!r}')
            axes.append(ObsAxis(a["field"], a["lo"], a["hi"], a.get("bins"), a.get("per_octave")))
        q = d.get("quantiles", DEFAULT_QUANTILES)
        try:
            q = tuple(float(x) for x in q)
        except (TypeError, ValueError):
            raise ValueError(f"fit observables: quantiles must be a list of fractions, got {q!r}") from None
        return cls(tuple(axes), q)


class FitSpec:
    def __init__(self, terms: Sequence[FitTerm], levels: Sequence[float] = (), maps: Sequence[Sequence[str]] = (),
                 select: Optional[Tuple[float, int]] = None, posterior: Optional[dict] = None,
                 observables: Optional[Sequence] = None, ranked: Optional[dict] = None):
        self.posterior = self._posterior(posterior)
        self.ranked = self._ranked(ranked)
        self.observables = self._observables(observables)
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

    @staticmethod
    def _ranked(r) -> Optional[int]:
        """{"n": integer in 1..RANK_MAX_N} -> n."""
        if r is None:
            return None
        if not isinstance(r, dict) or set(r) != {"n"}:
            raise ValueError(f'fit ranked: an object with exactly the key "n", got {r!r}')
        n = r["n"]
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= RANK_MAX_N:
            raise ValueError(f"fit ranked: n is an integer in 1..{RANK_MAX_N}, got {n!r}")
        return int(n)

    @staticmethod
    def _observables(obs) -> List[Observable]:
        if obs is None:
            return []
        if not isinstance(obs, (list, tuple)):
            raise ValueError(f"fit observables: a list of at most {OBS_MAX} observables, got {obs!r}")
        if len(obs) > OBS_MAX:
            raise ValueError(f"fit observables: at most {OBS_MAX} observables, got {len(obs)}")
        return [o if isinstance(o, Observable) else Observable.from_json(o) for o in obs]

    @classmethod
    def from_json(cls, d: dict) -> "FitSpec":
        unknown = set(d) - {"terms", "levels", "maps", "select", "posterior", "observables", "ranked"}
        if unknown:
            raise ValueError(f"unknown fit-spec keys {sorted(unknown)}")
        try:
            terms = [FitTerm(str(t["field"]), float(t["target"]), float(t["sigma"])) for t in d.get("terms", [])]
            sel = d.get("select")
            select = None if sel is None else (float(sel["level"]), int(sel["cap"]))
            maps = [[m] if isinstance(m, str) else list(m) for m in d.get("maps", [])]
        except (KeyError, TypeError) as e:
            raise ValueError(f"malformed fit spec: {e!r}") from None
        return cls(terms, d.get("levels", []), maps, select, d.get("posterior"), d.get("observables"),
                   d.get("ranked"))

    def to_json(self) -> dict:
        d = {"terms": [{"field": t.field, "target": t.target, "sigma": t.sigma} for t in self.terms],
             "levels": list(self.levels), "maps": [list(m) for m in self.maps]}
        if self.select is not None:
            d["select"] = {"level": self.select[0], "cap": self.select[1]}
        if self.posterior is not None:
            d["posterior"] = {"offset": self.posterior["offset"], "credible": list(self.posterior["credible"])}
        if self.observables:
            d["observables"] = [o.to_json() for o in self.observables]
        if self.ranked is not None:
            d["ranked"] = {"n": self.ranked}
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


def _records(rows) -> np.ndarray:
    """(n, 6) float64 records of an array or a tensor (a device tensor is read back)."""
    if hasattr(rows, "detach"):
        rows = rows.detach().cpu().numpy()
    return np.asarray(rows, dtype=np.float64).reshape(-1, 6)


def _indices(selected) -> np.ndarray:
    """A selection list (an array or a tensor on any device) as an int64 array."""
    return np.asarray(selected.cpu() if hasattr(selected, "cpu") else selected, dtype=np.int64).reshape(-1)


def check_offset(offset, what: str, optional: bool = False) -> Optional[float]:
    """The offset of a weighted state as a float: finite and >= 0, or None where the state may be
    unweighted."""
    if offset is None and optional:
        return None
    offset = float(offset)
    if not (math.isfinite(offset) and offset >= 0):
        raise ValueError(f"{what}: the offset must be finite and >= 0, got {offset!r}")
    return offset


def count_rows(state, n: int, what: str) -> None:
    """state.rows += n, the rows folded into a state of exact sums (merges included): they hold up
    to POST_MAX_ROWS."""
    if state.rows + n > POST_MAX_ROWS:
        raise ValueError(f"{what} state takes at most 2^32 rows (exact 64-bit sums), got {state.rows + n}")
    state.rows += n


# ---- the specs as the C ABI's arrays (include/lzq.h); at least one element each, so none is NULL
def term_structs(fit: FitSpec):
    arr = (_native.LzqFitTerm * len(fit.terms))()
    for k, t in enumerate(fit.terms):
        arr[k].field, arr[k].target, arr[k].sigma = YIELD_FIELDS.index(t.field), t.target, t.sigma
    return arr


def level_array(fit: FitSpec):
    return (ctypes.c_double * max(1, len(fit.levels)))(*fit.levels)


def map_structs(maps: Sequence[FitMap]):
    arr = (_native.LzqFitMap * max(1, len(maps)))()
    for k, m in enumerate(maps):
        arr[k].n_axes = len(m.axes)
        for a in range(len(m.axes)):
            arr[k].stride[a], arr[k].len[a] = m.stride[a], m.len[a]
    return arr


def obs_structs(observables: Sequence["Observable"]):
    arr = (_native.LzqObs * max(1, len(observables)))()
    for k, o in enumerate(observables):
        arr[k].n_axes = len(o.axes)
        for a, ax in enumerate(o.axes):
            c = arr[k].axes[a]
            c.field, c.kind, c.lo, c.hi = YIELD_FIELDS.index(ax.field), int(ax.log), ax.lo, ax.hi
            c.bins, c.log2_sub = (0, ax.log2_sub) if ax.log else (ax.bins, 0)
    return arr


class _HostState:
    """What the three numpy states share with each other and with the device states of engine.py:
    `words` (the state as an int64 tensor, what ranks exchange), like() (an empty state of the same
    layout and offset), merge_words(words); update(rows, start) and result(...) are each kind's.
    to_words and load are those of a state kept as its words `w` (HostFit has its own)."""
    COUNT_WORDS = 0     # the leading words that count the rows of a state of exact sums (count_rows)

    @property
    def words(self):
        import torch
        return torch.from_numpy(self.to_words())

    def merge_words(self, words) -> None:
        self.merge(self.like().load(words))

    def to_words(self) -> np.ndarray:
        return self.w.view(np.int64).copy()

    def load(self, words) -> "_HostState":
        """self.w <- the words of a state of exact sums; its rows are the counts it starts with."""
        w = np.ascontiguousarray(np.asarray(words), dtype=np.int64).reshape(-1)
        if w.size != self.w.size:
            raise ValueError(f"{self.WHAT} state of {w.size} words, expected {self.w.size} for this layout")
        self.w = w.view(np.uint64).copy()
        self.rows = int(sum(int(x) for x in self.w[:self.COUNT_WORDS]))
        return self


class HostFit(_HostState):
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

    def like(self) -> "HostFit":
        return HostFit(self.fit, self.maps)

    def kept(self):
        """The selection list (what a rank contributes to the combined one), an int64 tensor."""
        import torch
        return torch.from_numpy(self.sel.copy())

    def update(self, rows, start: int) -> None:
        rows = _records(rows)
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
        s = cls(fit, maps).load(words)
        if selected is not None:
            s.sel = _indices(selected)
        return s

    def load(self, words) -> "HostFit":
        w = np.ascontiguousarray(np.asarray(words), dtype=np.int64).reshape(-1)
        if w.size != state_words(self.maps):
            raise ValueError(f"fit state of {w.size} words, expected {state_words(self.maps)} for these maps")
        self.n_valid, self.n_invalid = int(w[W_NVALID]), int(w[W_NINVALID])
        self.n_within = w[W_WITHIN:W_WITHIN + MAX_LEVELS].copy()
        self.best_chi2, self.best_idx = w[W_BEST_CHI2:W_BEST_CHI2 + 1].view(np.float64)[0], int(w[W_BEST_IDX])
        kmin, kmax = w[W_COLMIN:W_COLMIN + 6].view(np.uint64), w[W_COLMAX:W_COLMAX + 6].view(np.uint64)
        self.col_min = np.where(kmin == _ALL, np.inf, _unkey(np.where(kmin == _ALL, _TOP, kmin)))
        self.col_max = np.where(kmax == 0, -np.inf, _unkey(np.where(kmax == 0, _TOP, kmax)))
        self.col_bad = w[W_COLBAD:W_COLBAD + 6].copy()
        self.sel_total = int(w[W_SEL_TOTAL])
        off = HEADER_WORDS
        for k, m in enumerate(self.maps):
            self.map_chi2[k] = w[off:off + m.cells].view(np.float64).copy()
            self.map_idx[k] = w[off + m.cells:off + 2 * m.cells].copy()
            off += 2 * m.cells
        return self

    def result(self, selected=None) -> dict:
        """selected: a selection list assembled elsewhere (the ranks' lists combined), in place of
        the state's own."""
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
            res["selected"] = self.sel.copy() if selected is None else _indices(selected)
            res["n_selected"] = int(self.sel_total)
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
    q = np.empty(rows.shape[0], dtype=np.uint64)
    lib = _native.load()
    _native.check(lib.lzq_post_weights_host(term_structs(fit), len(fit.terms), float(offset), rows.ctypes.data,
                                            rows.shape[0], q.ctypes.data), lib)
    return q


# -- sums of weights as (hi, lo) pairs of words, value hi * 2^31 + lo (HostPosterior, HostObservables)
def _pair(w: np.ndarray, k: int) -> int:
    return (int(w[k]) << 31) + int(w[k + 1])


def _split(q: np.ndarray):
    """Weights q as the (hi, lo) they add to a pair."""
    return q >> np.uint64(31), q & np.uint64(0x7FFFFFFF)


def _add_pairs(w: np.ndarray, base: int, cell: np.ndarray, hi: np.ndarray, lo: np.ndarray) -> None:
    """Pair `cell[i]` of the pairs that start at word `base` += (hi[i], lo[i])."""
    np.add.at(w, base + 2 * cell, hi)
    np.add.at(w, base + 2 * cell + 1, lo)


def _pair_ints(pairs: np.ndarray) -> np.ndarray:
    """(n, 2) pairs as exact Python integers (an object array)."""
    return (pairs[:, 0].astype(object) << 31) + pairs[:, 1].astype(object)


def _pair_floats(pairs: np.ndarray) -> np.ndarray:
    """(n, 2) pairs as floats: hi * 2^31 is exact below 2^84, the sum rounds once."""
    return pairs[:, 0].astype(np.float64) * 2.0 ** 31 + pairs[:, 1].astype(np.float64)


def _first_reaching(cum: np.ndarray, p: float) -> int:
    """The first bin whose cumulated weight `cum` (exact integers, a total > 0) reaches the fraction
    p of the total: cum * den >= num * total, in integers."""
    fp = Fraction(p)
    return int(np.argmax((cum * fp.denominator >= fp.numerator * cum[-1]).astype(bool)))


class HostPosterior(_HostState):
    """The posterior state in numpy: `w`, the uint64 words of include/lzq.h's "posterior state".
    update (rows of flat indices [start, start + n)), merge, result."""
    WHAT, COUNT_WORDS = "a posterior", 4     # the rows a state holds: used, zero, above, invalid

    def __init__(self, fit: FitSpec, maps: Sequence[FitMap], offset: float, axis_values: Optional[dict] = None):
        self.fit, self.maps, self.offset = fit, list(maps), check_offset(offset, "posterior")
        if any(m.cells > MAX_CELLS for m in self.maps):
            raise ValueError("a fit map has at most 2^24 cells")
        self.axis_values = dict(axis_values or {})
        self.w = np.zeros(post_state_words(self.maps), dtype=np.uint64)
        self.rows = 0    # rows folded in, merges included (count_rows)

    def like(self) -> "HostPosterior":
        return HostPosterior(self.fit, self.maps, self.offset, self.axis_values)

    def update(self, rows, start: int) -> None:
        rows = _records(rows)
        n = rows.shape[0]
        if n == 0:
            return
        count_rows(self, n, self.WHAT)
        q = post_weights(self.fit, self.offset, rows)
        inv, above, zero = q == np.uint64(Q_INVALID), q == np.uint64(Q_ABOVE), q == np.uint64(0)
        used = ~(inv | above | zero)
        w = self.w
        for k, mask in ((PW_NUSED, used), (PW_NZERO, zero), (PW_NABOVE, above), (PW_NINVALID, inv)):
            w[k] += np.uint64(int(mask.sum()))
        if not used.any():
            return
        hi, lo = _split(q[used])
        c = chi2_rows(self.fit, rows)[used]
        idx = np.arange(start, start + n, dtype=np.int64)[used]

        def add(word, mask=None):
            w[word] += hi.sum(dtype=np.uint64) if mask is None else hi[mask].sum(dtype=np.uint64)
            w[word + 1] += lo.sum(dtype=np.uint64) if mask is None else lo[mask].sum(dtype=np.uint64)
        add(PW_Z)
        for l, lev in enumerate(self.fit.levels):
            add(PW_LEVEL + 2 * l, c <= lev)
        _add_pairs(w, PW_HIST, np.minimum(POST_BINS - 1, ((c - self.offset) * 16.0).astype(np.int64)), hi, lo)
        off = PW_MAPS
        for fm in self.maps:
            _add_pairs(w, off, fm.cell(idx), hi, lo)
            off += 2 * fm.cells

    def merge(self, o: "HostPosterior") -> None:
        """Fold in the state of other (disjoint) rows at the same offset: word-wise addition."""
        if o.offset != self.offset or o.w.size != self.w.size:
            raise ValueError("posterior merge: states of different offsets or layouts")
        count_rows(self, o.rows, self.WHAT)
        self.w += o.w

    @classmethod
    def from_words(cls, fit: FitSpec, maps: Sequence[FitMap], offset: float, words,
                   axis_values: Optional[dict] = None) -> "HostPosterior":
        return cls(fit, maps, offset, axis_values).load(words)

    def result(self, axis_values: Optional[dict] = None) -> dict:
        """Host values of the state.  Everything is computed from the exact integers in a fixed
        order (integer arithmetic, correctly rounded int / int divisions, math.fsum), so every rank
        that holds the same words gets the same floats.  axis_values: for the state's own."""
        axis_values = self.axis_values if axis_values is None else axis_values
        w = self.w
        Z = _pair(w, PW_Z)
        hist = w[PW_HIST:PW_MAPS].reshape(POST_BINS, 2).copy()
        cum, edges = np.cumsum(_pair_ints(hist)), []
        for p in self.fit.posterior["credible"] if self.fit.posterior else DEFAULT_CREDIBLE:
            edge = None
            if cum[-1] > 0:
                b = _first_reaching(cum, p)
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
            post = (_pair_floats(pairs) / np.float64(Z) if Z else np.full(m.cells, np.nan)).reshape(m.len)
            mean = std = None
            x = axis_values.get(m.axes[0]) if len(m.axes) == 1 else None
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


# ---- observables: histograms over yield fields ------------------------------------------------
_INF_BITS = np.uint64(0x7FF0000000000000)


def obs_state_words(observables: Sequence[Observable]) -> int:
    return sum(OBS_HEADER_WORDS + 4 * o.cells for o in observables)


def obs_cells_host(observables: Sequence[Observable], k: int, rows) -> np.ndarray:
    """The classes of (n, 6) records in observable k from the library's host build of the one
    definition (lzq_obs_cells_host; no GPU is touched): what Observable.cell is compared with."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, 6))
    out = np.empty(rows.shape[0], dtype=np.int32)
    lib = _native.load()
    _native.check(lib.lzq_obs_cells_host(obs_structs(observables), len(observables), int(k), rows.ctypes.data,
                                         rows.shape[0], out.ctypes.data), lib)
    return out


class HostObservables(_HostState):
    """The observable state in numpy: `w`, the uint64 words of include/lzq.h's "sweep observables".
    offset None: unweighted (counts and chi2 minima only); else rows weigh as the posterior's."""
    WHAT, COUNT_WORDS = "an observable", 3   # the valid rows a state holds: the first one's in, out, non-finite

    def __init__(self, fit: FitSpec, observables: Sequence[Observable], offset: Optional[float] = None):
        self.fit, self.observables = fit, list(observables)
        self.offset = check_offset(offset, "observables", optional=True)
        if len(self.observables) > OBS_MAX:
            raise ValueError(f"observables: at most {OBS_MAX}, got {len(self.observables)}")
        self.w = np.zeros(obs_state_words(self.observables), dtype=np.uint64)
        for off, o in self._offsets():
            self.w[off + OBS_HEADER_WORDS + 3 * o.cells:off + OBS_HEADER_WORDS + 4 * o.cells] = _INF_BITS
        self.rows = 0    # rows folded in, merges included (count_rows)

    def like(self) -> "HostObservables":
        return HostObservables(self.fit, self.observables, self.offset)

    def _offsets(self):
        off = 0
        for o in self.observables:
            yield off, o
            off += OBS_HEADER_WORDS + 4 * o.cells

    def update(self, rows, start: int = 0) -> None:
        """start: unused (a row's cell does not depend on its index); the states' common signature."""
        rows = _records(rows)
        n = rows.shape[0]
        if n == 0:
            return
        count_rows(self, n, self.WHAT)
        c = chi2_rows(self.fit, rows)
        valid = np.isfinite(c)
        if self.offset is not None:
            q = post_weights(self.fit, self.offset, rows)
            has = valid & (q >= np.uint64(1)) & (q <= np.uint64(POST_UNIT))
            hi, lo = _split(q)
        w = self.w
        for off, o in self._offsets():
            cell = o.cell(rows)
            w[off] += np.uint64(int((valid & (cell >= 0)).sum()))
            w[off + 1] += np.uint64(int((valid & (cell == OBS_OUT)).sum()))
            w[off + 2] += np.uint64(int((valid & (cell == OBS_NONFINITE)).sum()))
            m = valid & (cell >= 0)
            base = off + OBS_HEADER_WORDS
            np.add.at(w, base + 2 * o.cells + cell[m], np.uint64(1))
            np.minimum.at(w, base + 3 * o.cells + cell[m], c[m].view(np.uint64))   # chi2 >= 0 orders like its bits
            if self.offset is not None:
                mw = m & has
                _add_pairs(w, base, cell[mw], hi[mw], lo[mw])

    def _chi2_mask(self) -> np.ndarray:
        is_chi2 = np.zeros(self.w.size, dtype=bool)
        for off, o in self._offsets():
            is_chi2[off + OBS_HEADER_WORDS + 3 * o.cells:off + OBS_HEADER_WORDS + 4 * o.cells] = True
        return is_chi2

    def merge(self, o: "HostObservables") -> None:
        """Fold in the state of other (disjoint) rows: words add, the chi2 words take the minimum."""
        if o.offset != self.offset or o.w.size != self.w.size:
            raise ValueError("observables merge: states of different offsets or layouts")
        count_rows(self, o.rows, self.WHAT)
        self.w = np.where(self._chi2_mask(), np.minimum(self.w, o.w), self.w + o.w)

    @classmethod
    def from_words(cls, fit: FitSpec, observables: Sequence[Observable], offset: Optional[float],
                   words) -> "HostObservables":
        return cls(fit, observables, offset).load(words)

    def result(self, z_units: Optional[int] = None) -> List[dict]:
        """Host values of the state, one dictionary an observable.  As HostPosterior.result, everything
        is derived from the exact integers in a fixed order.  z_units: the posterior's Z in units of
        2^-62 (its "Z_units"), for the share of Z that fell inside each observable's range."""
        out = []
        for off, o in self._offsets():
            w, base = self.w, off + OBS_HEADER_WORDS
            pairs = w[base:base + 2 * o.cells].reshape(o.cells, 2).copy()
            val = _pair_ints(pairs)
            total = int(val.sum()) if o.cells else 0
            post = (_pair_floats(pairs) / np.float64(total) if total else np.full(o.cells, np.nan)).reshape(o.shape)
            res = {"axes": [a.to_json() for a in o.axes], "edges": [a.edges() for a in o.axes],
                   "weighted": self.offset is not None, "offset": self.offset,
                   "n_in": int(w[off]), "n_out": int(w[off + 1]), "n_nonfinite": int(w[off + 2]),
                   "count": w[base + 2 * o.cells:base + 3 * o.cells].astype(np.int64).reshape(o.shape),
                   "chi2_min": w[base + 3 * o.cells:base + 4 * o.cells].view(np.float64).reshape(o.shape).copy(),
                   "weight": pairs, "posterior": post, "total_units": str(total),
                   "in_range_share": (total / z_units if z_units else None), "quantiles": None, "mode": None}
            if len(o.axes) == 1 and self.offset is not None:
                e = res["edges"][0]
                span = lambda b: {"bin": int(b), "lo": float(e[b]), "hi": float(e[b + 1])}
                qs = []
                cum = np.cumsum(val) if total else None
                for p in o.quantiles:
                    entry = {"p": p, "bin": None, "lo": None, "hi": None}
                    if total:
                        entry.update(span(_first_reaching(cum, p)))
                    qs.append(entry)
                res["quantiles"] = qs
                if total:
                    res["mode"] = span(int(np.argmax((val == val.max()).astype(bool))))    # the lowest such bin
            out.append(res)
        return out


def obs_differences(a: Sequence[dict], b: Sequence[dict]) -> List[str]:
    """Where two observable results differ (exact integers, floats by bits); empty when equal."""
    out = []
    bits = lambda x: np.asarray(x, dtype=np.float64).view(np.int64)
    if len(a) != len(b):
        return ["number of observables"]
    for k, (oa, ob) in enumerate(zip(a, b)):
        for key in ("axes", "weighted", "offset", "n_in", "n_out", "n_nonfinite", "total_units", "in_range_share",
                    "quantiles", "mode"):
            if oa[key] != ob[key]:
                out.append(f"observable {k}: {key}: {oa[key]} != {ob[key]}")
        if oa["count"].shape != ob["count"].shape:
            out.append(f"observable {k}: shape")
            continue
        if any(not np.array_equal(bits(x), bits(y)) for x, y in zip(oa["edges"], ob["edges"])):
            out.append(f"observable {k}: edges")
        if not np.array_equal(oa["count"], ob["count"]):
            out.append(f"observable {k}: count differs in {int((oa['count'] != ob['count']).sum())} cells")
        if not np.array_equal(bits(oa["chi2_min"]), bits(ob["chi2_min"])):
            out.append(f"observable {k}: chi2_min differs in "
                       f"{int((bits(oa['chi2_min']) != bits(ob['chi2_min'])).sum())} cells")
        if not np.array_equal(oa["weight"], ob["weight"]):
            n = int((oa["weight"] != ob["weight"]).any(axis=1).sum())
            out.append(f"observable {k}: weight differs in {n} cells")
        elif not np.array_equal(bits(oa["posterior"]), bits(ob["posterior"])):
            out.append(f"observable {k}: posterior")
    return out


# ---- ranked points: the n rows of smallest chi2 with their records ------------------------------
def rank_state_words(n: int) -> int:
    return RANK_HEADER_WORDS + 8 * int(n)


class HostRanked(_HostState):
    """The ranked state in numpy: `w`, the uint64 words of include/lzq.h's "ranked points".  The
    rows seen are ordered by (chi2 bits, flat index); the n first are kept with their records."""
    WHAT = "a ranked"

    def __init__(self, fit: FitSpec, n: int):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= RANK_MAX_N:
            raise ValueError(f"ranked: n is an integer in 1..{RANK_MAX_N}, got {n!r}")
        self.fit, self.n = fit, int(n)
        self.w = np.zeros(rank_state_words(self.n), dtype=np.uint64)
        self.w[RW_N] = self.n
        self._entries()[:] = self._unfilled(self.n)
        self.rows = 0

    @staticmethod
    def _unfilled(k: int) -> np.ndarray:
        e = np.zeros((k, 8), dtype=np.uint64)
        e[:, 0], e[:, 1] = _INF_BITS, _ALL
        return e

    def _entries(self) -> np.ndarray:
        """The n entries as a (n, 8) view of the words."""
        return self.w[RANK_HEADER_WORDS:].reshape(self.n, 8)

    def like(self) -> "HostRanked":
        return HostRanked(self.fit, self.n)

    def _take(self, entries: np.ndarray) -> None:
        """The list <- the n first of its filled entries and `entries` ((k, 8) words of valid rows)."""
        filled = int(self.w[RW_FILLED])
        both = np.concatenate([self._entries()[:filled], entries])
        order = np.lexsort((both[:, 1], both[:, 0]))[:self.n]      # by chi2 bits, then by index
        self._entries()[:] = np.concatenate([both[order], self._unfilled(self.n - order.size)])
        self.w[RW_FILLED] = order.size

    def update(self, rows, start: int) -> None:
        rows = np.ascontiguousarray(_records(rows))
        n = rows.shape[0]
        if n == 0:
            return
        c = chi2_rows(self.fit, rows)
        valid = np.isfinite(c)
        self.w[RW_NVALID] += np.uint64(int(valid.sum()))
        self.w[RW_NINVALID] += np.uint64(int(n - valid.sum()))
        e = np.empty((int(valid.sum()), 8), dtype=np.uint64)
        e[:, 0] = c[valid].view(np.uint64)
        e[:, 1] = np.arange(start, start + n, dtype=np.int64)[valid].view(np.uint64)
        e[:, 2:] = rows.view(np.uint64)[valid]
        self._take(e)

    def merge(self, o: "HostRanked") -> None:
        """Fold in the state of other (disjoint) rows: the n first of both lists; the counts add."""
        if o.n != self.n:
            raise ValueError("ranked merge: states of different capacities")
        self.w[RW_NVALID] += o.w[RW_NVALID]
        self.w[RW_NINVALID] += o.w[RW_NINVALID]
        self._take(o._entries()[:int(o.w[RW_FILLED])])

    @classmethod
    def from_words(cls, fit: FitSpec, n: int, words) -> "HostRanked":
        return cls(fit, n).load(words)

    def result(self) -> dict:
        k = int(self.w[RW_FILLED])
        e = self._entries()[:k]
        return {"n": self.n, "count": k, "n_valid": int(self.w[RW_NVALID]), "n_invalid": int(self.w[RW_NINVALID]),
                "index": e[:, 1].astype(np.int64), "chi2": e[:, 0].copy().view(np.float64),
                "records": e[:, 2:].copy().view(np.float64)}


def rank_differences(a: dict, b: dict) -> List[str]:
    """Where two ranked results differ (integers exactly, floats by bits); empty when equal."""
    out = []
    bits = lambda x: np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    for k in ("n", "count", "n_valid", "n_invalid"):
        if a[k] != b[k]:
            out.append(f"{k}: {a[k]} != {b[k]}")
    if a["count"] != b["count"]:
        return out
    if not np.array_equal(a["index"], b["index"]):
        out.append(f"index differs in {int((a['index'] != b['index']).sum())} entries")
    if not np.array_equal(bits(a["chi2"]), bits(b["chi2"])):
        out.append(f"chi2 differs in {int((bits(a['chi2']) != bits(b['chi2'])).sum())} entries")
    if not np.array_equal(bits(a["records"]), bits(b["records"])):
        out.append(f"records differ in {int((bits(a['records']) != bits(b['records'])).any(axis=1).sum())} entries")
    return out


def ranked_params(sweep_spec, index) -> np.ndarray:
    """float64[count, n_axes]: the sweep axes' values at each flat index, by the C-order decode
    (SweepSpec.point_params for every index at once)."""
    idx = np.asarray(index, dtype=np.int64).reshape(-1).copy()
    out = np.empty((idx.size, len(sweep_spec.axes)), dtype=np.float64)
    for a in range(len(sweep_spec.axes) - 1, -1, -1):
        vals = np.asarray(sweep_spec.axes[a][1], dtype=np.float64)
        out[:, a] = vals[idx % len(vals)]
        idx //= len(vals)
    return out


# ---- the accumulator: what the sweep driver folds chunks into ---------------------------------
class Accumulator:
    """Chunks of records into a fit state `state` and, where the spec asks for them, a posterior
    state `post`, an observable state `obs` and a ranked state `rank`.  engine None: numpy states of
    CPU records (the gloo tests, any host table); else the engine's device-resident states, updated on the current stream
    behind the chunk's own kernels.  Nothing else here depends on which."""

    def __init__(self, fit: FitSpec, maps: Sequence[FitMap], engine=None, axis_values: Optional[dict] = None):
        self.fit, self.maps, self.axis_values = fit, list(maps), axis_values
        self._post_state = HostPosterior if engine is None else engine.post_state
        self._obs_state = HostObservables if engine is None else engine.obs_state
        self.state = (HostFit if engine is None else engine.fit_state)(fit, self.maps)
        self.post = None    # a numeric posterior offset is folded chunk by chunk; "best" after the combine
        self.obs = None     # observables: unweighted without a posterior, else begun with it
        self.rank = None    # the n best rows: needs nothing of the posterior
        if fit.ranked is not None:
            self.rank = (HostRanked if engine is None else engine.rank_state)(fit, fit.ranked)
        if fit.posterior is not None and fit.posterior["offset"] != "best":
            self.post_begin(fit.posterior["offset"])
        elif fit.posterior is None and fit.observables:
            self.obs = self._obs_state(fit, fit.observables, None)

    def update(self, rows, start: int) -> None:
        self.state.update(rows, start)    # (with the selection, where the spec has one)
        if self.rank is not None:
            self.rank.update(rows, start)
        self.post_update(rows, start)     # right behind the fit

    def post_begin(self, offset: float) -> None:
        self.post = self._post_state(self.fit, self.maps, offset)
        if self.fit.observables:
            self.obs = self._obs_state(self.fit, self.fit.observables, offset)

    def post_update(self, rows, start: int) -> None:
        """The states begun so far other than the fit's: the chunk's second half, and the whole of
        the second pass of the offset "best"."""
        if self.post is not None:
            self.post.update(rows, start)
        if self.obs is not None:
            self.obs.update(rows, start)

    def result(self) -> dict:
        """The fit of the rows folded in here (combine: of every rank's)."""
        return self.state.result()


def make_accumulator(fit: FitSpec, maps: Sequence[FitMap], engine=None, axis_values: Optional[dict] = None):
    """engine None: records are CPU tensors / arrays (numpy); else the engine's device.
    axis_values (FitSpec.axis_values): the sweep axes' values, for the posterior's means."""
    return Accumulator(fit, maps, engine, axis_values)


# ---- combine: the ranks' states gathered and merged ------------------------------------------
def _distributed() -> bool:
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


def _gather(src, group):
    """The ranks' int64 tensors `src` (of one size) as [world, n]; through the CPU unless the group
    is RCCL's."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    src = (src if dist.get_backend(group) == "nccl" else src.cpu()).contiguous()
    flat = torch.empty(world * src.numel(), dtype=torch.int64, device=src.device)   # (gloo takes a flat output)
    dist.all_gather_into_tensor(flat, src, group=group)
    return flat.view(world, src.numel())


def _merged(state, words):
    """An empty state like `state` with the ranks' `words` [world, n] merged in rank order."""
    tot = state.like()
    for w in words:
        tot.merge_words(w)
    return tot


def merged_fit(acc, words, selected=None) -> dict:
    """The fit of the ranks' states `words` [world, n]; selected: their selection lists combined."""
    return _merged(acc.state, words).result(selected)


def merged_posterior(acc, words) -> dict:
    return _merged(acc.post, words).result(acc.axis_values)


def merged_observables(acc, words, z_units: Optional[int] = None) -> List[dict]:
    return _merged(acc.obs, words).result(z_units)


def merged_ranked(acc, words) -> dict:
    return _merged(acc.rank, words).result()


def combine(acc, world: int = 1, group=None, local=None, start: int = 0) -> dict:
    """The fit of the whole grid on every rank: the ranks' fixed-size states all-gathered and
    merged in rank order, their selection lists concatenated in rank order and cut to `cap`
    (shards are contiguous and ascending, so the list stays ascending).  Without a process group
    the rank's own result.  A fit with a "posterior" key gets result["posterior"]
    (combine_posterior; `local`, `start`: the rank's shard, for the offset "best").  Every rank
    issues its collectives in one order: fit words, selection, posterior words, observable words,
    ranked words.  A fit with a "ranked" key gets result["ranked"] (HostRanked.result)."""
    res = acc.result() if not _distributed() else merged_fit(acc, *_gather_fit(acc, group))
    if acc.fit.posterior is not None:
        res["posterior"] = combine_posterior(acc, res, local, start, group)
    if acc.fit.observables:
        res["observables"] = combine_observables(acc, res, group)
    if acc.fit.ranked is not None:
        res["ranked"] = combine_ranked(acc, group)
    return res


def _gather_fit(acc, group):
    """The ranks' fit words [world, n] and, with a selection, their lists combined (else None)."""
    import torch
    allw = _gather(acc.state.words, group)
    if acc.fit.select is None:
        return allw, None
    cap = acc.fit.select[1]
    kept = [min(int(t), cap) for t in allw[:, W_SEL_TOTAL].cpu()]
    mine = acc.state.kept()
    pad = torch.zeros(max(kept + [1]), dtype=torch.int64, device=mine.device)   # one size on every rank
    pad[:mine.numel()] = mine
    alls = _gather(pad, group)
    return allw, torch.cat([alls[r, :kept[r]] for r in range(len(kept))])[:cap]


def combine_posterior(acc, res: dict, local=None, start: int = 0, group=None) -> dict:
    """The posterior of the whole grid on every rank.  A numeric offset was folded chunk by chunk;
    "best" is the combined fit's best chi2 (`res`, identical on every rank; 0 when no row is valid)
    and is applied now, in a second pass over the rank's own shard `local` (rows of flat indices
    from `start`).  The ranks' states are all-gathered and summed."""
    if acc.fit.posterior["offset"] == "best":
        if local is None:
            raise ValueError(NO_TABLE_BEST)
        acc.post_begin(float(res["best"]["chi2"]) if res["best"]["index"] >= 0 else 0.0)
        acc.post_update(local, start)
    if not _distributed():
        return acc.post.result(acc.axis_values)
    return merged_posterior(acc, _gather(acc.post.words, group))


def combine_observables(acc, res: dict, group=None) -> List[dict]:
    """The observables of the whole grid on every rank: the ranks' states (folded behind the fit, or
    with the offset "best" in the posterior's second pass, which combine_posterior has run) are
    all-gathered and merged.  The posterior's Z (`res`) gives each range's share of it."""
    z = int(res["posterior"]["Z_units"]) if res.get("posterior") is not None else None
    if not _distributed():
        return acc.obs.result(z)
    return merged_observables(acc, _gather(acc.obs.words, group), z)


def combine_ranked(acc, group=None) -> dict:
    """The n best rows of the whole grid on every rank: the ranks' lists all-gathered and merged in
    rank order (any order gives the same list)."""
    if not _distributed():
        return acc.rank.result()
    return merged_ranked(acc, _gather(acc.rank.words, group))


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
    point (index, axis values, yields); the maps and the selection go to their own files.  With
    ranked points their axis values are resolved here into result["ranked"]["params"] (write_files
    saves them: it does not see the sweep)."""
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
    if result.get("observables"):
        rep["observables"] = [{**{k: o[k] for k in ("axes", "weighted", "offset", "n_in", "n_out", "n_nonfinite",
                                                    "total_units", "in_range_share", "quantiles", "mode")},
                               "shape": list(o["count"].shape),
                               "range": [[float(e[0]), float(e[-1])] for e in o["edges"]],   # (log axes: rounded down)
                               "chi2_min": (float(o["chi2_min"].min()) if o["n_in"] else None)}
                              for o in result["observables"]]
    if result.get("ranked") is not None:
        r = result["ranked"]
        r["params"] = ranked_params(sweep_spec, r["index"])
        rep["ranked"] = {"n": r["n"], "count": r["count"],
                         "chi2_first": float(r["chi2"][0]) if r["count"] else None,
                         "chi2_last": float(r["chi2"][-1]) if r["count"] else None,
                         "axes": [n for n, _ in sweep_spec.axes]}
    return rep


def write_files(out_dir: str, rep: dict, result: dict) -> None:
    """fit.json, fit_maps.npz (map<k>_chi2_min / map<k>_argmin; with a posterior map<k>_posterior and
    map<k>_weight, the (cells, 2) uint64 pairs) and selected.npy in `out_dir`; with observables
    fit_obs.npz (obs<k>_weight, _count, _chi2_min, _posterior and _edges<a> per axis); with ranked
    points fit_ranked.npz (index, chi2, records, params)."""
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
    if result.get("observables"):
        arrays = {}
        for k, o in enumerate(result["observables"]):
            for name in ("weight", "count", "chi2_min", "posterior"):
                arrays[f"obs{k}_{name}"] = o[name]
            for a, e in enumerate(o["edges"]):
                arrays[f"obs{k}_edges{a}"] = e
        np.savez(os.path.join(out_dir, "fit_obs.npz"), **arrays)
    if result.get("ranked") is not None:
        r = result["ranked"]
        np.savez(os.path.join(out_dir, "fit_ranked.npz"), index=r["index"], chi2=r["chi2"], records=r["records"],
                 params=r["params"])
