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
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native

YIELD_FIELDS = _native.YIELD_FIELDS
MAX_TERMS, MAX_LEVELS, MAX_MAPS = _native.FIT_MAX_TERMS, _native.FIT_MAX_LEVELS, _native.FIT_MAX_MAPS
MAX_CELLS = _native.FIT_MAX_CELLS
HEADER_WORDS = _native.FIT_HEADER_WORDS
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
                 select: Optional[Tuple[float, int]] = None):
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

    @classmethod
    def from_json(cls, d: dict) -> "FitSpec":
        unknown = set(d) - {"terms", "levels", "maps", "select"}
        if unknown:
            raise ValueError(f"unknown fit-spec keys {sorted(unknown)}")
        try:
            terms = [FitTerm(str(t["field"]), float(t["target"]), float(t["sigma"])) for t in d.get("terms", [])]
            sel = d.get("select")
            select = None if sel is None else (float(sel["level"]), int(sel["cap"]))
            maps = [[m] if isinstance(m, str) else list(m) for m in d.get("maps", [])]
        except (KeyError, TypeError) as e:
            raise ValueError(f"malformed fit spec: {e!r}") from None
        return cls(terms, d.get("levels", []), maps, select)

    def to_json(self) -> dict:
        d = {"terms": [{"field": t.field, "target": t.target, "sigma": t.sigma} for t in self.terms],
             "levels": list(self.levels), "maps": [list(m) for m in self.maps]}
        if self.select is not None:
            d["select"] = {"level": self.select[0], "cap": self.select[1]}
        return d

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


# ---- accumulators: what the sweep driver folds chunks into -----------------------------------
class HostAccumulator:
    """Chunks of CPU records (the gloo tests, any host table) into a HostFit."""

    def __init__(self, fit: FitSpec, maps: Sequence[FitMap]):
        self.fit, self.maps = fit, list(maps)
        self.host = HostFit(fit, maps)

    def update(self, rows, start: int) -> None:
        self.host.update(rows.detach().numpy() if hasattr(rows, "detach") else rows, start)

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

    def __init__(self, fit: FitSpec, maps: Sequence[FitMap], engine):
        self.fit, self.maps, self.engine = fit, list(maps), engine
        self.state = engine.fit_state(fit, maps)

    def update(self, rows, start: int) -> None:
        self.engine.fit_update(self.state, rows, start)
        if self.fit.select is not None:
            self.engine.fit_select(self.state, rows, start)

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


def make_accumulator(fit: FitSpec, maps: Sequence[FitMap], engine=None):
    """engine None: records are CPU tensors / arrays (numpy); else the engine's device."""
    return HostAccumulator(fit, maps) if engine is None else DeviceAccumulator(fit, maps, engine)


def combine(acc, world: int = 1, group=None) -> dict:
    """The fit of the whole grid on every rank: the ranks' fixed-size states all-gathered and
    merged in rank order, their selection lists concatenated in rank order and cut to `cap`
    (shards are contiguous and ascending, so the list stays ascending).  Without a process group
    the rank's own result."""
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
    return {"spec": fit.to_json(), "sweep": sweep_spec.name, "n_points": int(n_points),
            "n_valid": result["n_valid"], "n_invalid": result["n_invalid"], "levels": list(fit.levels),
            "n_within": result["n_within"], "columns": result["columns"], "best": best,
            "maps": [{"axes": m["axes"], "shape": list(m["chi2_min"].shape)} for m in result["maps"]],
            "n_selected": result["n_selected"],
            "n_selected_kept": None if result["selected"] is None else int(len(result["selected"]))}


def write_files(out_dir: str, rep: dict, result: dict) -> None:
    """fit.json, fit_maps.npz (map<k>_chi2_min / map<k>_argmin) and selected.npy in `out_dir`."""
    import os
    with open(os.path.join(out_dir, "fit.json"), "w") as f:
        json.dump(rep, f, indent=2)
    arrays = {}
    for k, m in enumerate(result["maps"]):
        arrays[f"map{k}_chi2_min"], arrays[f"map{k}_argmin"] = m["chi2_min"], m["argmin"]
    np.savez(os.path.join(out_dir, "fit_maps.npz"), **arrays)
    sel = result["selected"] if result["selected"] is not None else np.empty(0, dtype=np.int64)
    np.save(os.path.join(out_dir, "selected.npy"), np.asarray(sel, dtype=np.int64), allow_pickle=False)
