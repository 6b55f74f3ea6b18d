"""Parameter-sweep driver (north_star (3); the reference has no sweep code).

A sweep = a base config in the reference schema (fpy:44-79) x up to 8 Cartesian axes,
flattened in C order (last axis fastest).  Points are generated ON DEVICE from the flat
index (lzq_sweep_grid), so no parameter table ever crosses PCIe.

Multi-GPU: one process per GPU; rank r owns the contiguous shard
[r*N//W, (r+1)*N//W) and evaluates it with no communication; one all-gather of the 48-B
per-point yield records (RCCL over xGMI on GPUs, gloo in CPU tests) assembles the table on
every rank.  Each point is reduced by one wavefront, so the gathered table is bit-identical
for W = 1, 2, 4, 8.  Grid-wide statistics are reduced on the host in index order.

Checkpoint/resume: with --out, every evaluated chunk is written as
`shard_<key>_<start>_<count>.npy` (allow_pickle=False), where <key> hashes the sweep
definition (spec_key: axes, base config, n_y, crossings, library ABI); --resume reloads
existing chunks of the SAME definition instead of recomputing them, so a killed 1e8-point
run restarts where it stopped, and a directory written by another sweep is never mixed in
(manifest.json records the definition; a mismatch refuses --resume).

Fits (--fit FILE | paper; fit.py): every chunk, computed or resumed, is also folded on its own
stream into a device-resident fit state (chi2 to targets: counts within levels, best point, profile
maps, selection; lzq_fit_*), the ranks' fixed-size states are all-gathered and merged in rank order,
and rank 0 writes fit.json, fit_maps.npz and selected.npy.  --no-table keeps only that: chunks pass
through two chunk-sized buffers, with no shard, no all-gather and no table.npy.  A fit spec with a
"posterior" key adds the likelihood-weighted sums (lzq_post_*: evidence, mass within levels, credible
thresholds, marginal maps) as a "posterior" block of fit.json and map<k>_posterior / map<k>_weight
arrays of fit_maps.npz; its offset "best" takes a second pass over the table, so not with --no-table.
An "observables" key adds histograms over one or two yield fields (lzq_obs_*: per cell the count of
valid rows, the smallest chi2 and, with a posterior, the weight; quantiles and the mode of 1-D ones)
as an "observables" block of fit.json and a file fit_obs.npz.  They are folded behind the fit --
unweighted without a posterior, weighted with a numeric offset, both of which work with --no-table --
or, with the offset "best", in the posterior's second pass.  A "ranked" key ({"n": 1000}, n up to 4096)
keeps the n points of smallest chi2 themselves, in order, with their records (lzq_rank_*): a "ranked"
block of fit.json and a file fit_ranked.npz (index, chi2, records, params).  It needs neither a level
guessed beforehand nor the table, so it works with --no-table.

    python -m <package>.sweep --spec C2 --out sweep_c2          # 1 GPU
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m <package>.sweep --spec C4 --out c4
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _native, solve as _solve
from .config import to_ode_params, to_point

YIELD_FIELDS = _native.YIELD_FIELDS

EQUAL_MASS = {  # /root/reference/yields_config_equal_mass.json
    "regime": "nonthermal", "m_chi_GeV": 0.95, "g_chi": 2, "chi_stats": "fermion",
    "sigma_v_chi_GeV_m2": 0.0, "T_p_GeV": 100.0, "beta_over_H": 100.0, "v_w": 0.30, "I_p": 0.34,
    "g_star": 106.75, "g_star_s": 106.75, "P_chi_to_B": 0.14925839040304145,
    "source_shape_sigma_y": 9.0, "Gamma_wash_over_H": 0.0, "incident_flux_scale": 1.07e-9,
    "deplete_DM_from_source": False, "T_max_over_Tp": 5.0, "T_min_over_Tp": 0.001,
    "Y_chi_init": 4.90e-10, "n_chi_at_Tp_GeV3": None,
}


@dataclass
class CrossingSpec:
    """Multi-crossing bounce profile per grid point (BASELINE config C5; no reference
    counterpart).  Crossing c of the point with grid values (m_mix, |Delta'|)
    has m_c = m_mix (1 + jitter a_c), |Delta'_c| = |Delta'| (1 + jitter b_c) and position
    xi_c = L (spacing_lz c + jitter d_c), L = sqrt(v_w/|Delta'|) max(1, sqrt(delta)), with
    (a, b, d) ~ U(-1, 1) drawn once from numpy default_rng(seed).  P is the coherent
    conversion probability through all crossings (lzq_lz_propagate)."""
    n_cross: int = 8
    spacing_lz: float = 40.0
    jitter: float = 0.1
    window_lz: float = 20.0
    steps: int = 64        # Magnus steps per crossing core (floor): <= 1e-10 from the exact solution
    seed: int = 5

    def pattern(self) -> np.ndarray:
        return np.random.default_rng(self.seed).uniform(-1.0, 1.0, (3, self.n_cross))


PROFILE_FIELDS = ("y_B", "y_chi", "lambda_tr_eff")   # PAPER eqs.(5),(7): sweep axes of a profile spec


@dataclass
class ProfileSpec:
    """P of every grid point from ONE bounce profile (PAPER p.3 eqs.(5)-(9); the plug-in path of
    fpy:170-187 as a sweep): the profile's phi, Phi (a CSV in transport_from_profile's `xi,phi,Phi`
    format, or shape `synthetic` of bounce.synthetic_shapes) with the couplings y_B, y_chi,
    lambda_tr_eff (these defaults, or sweep axes of those names) and the point's v_w.
    estimator: "auto" (one crossing -> eq.(9) of its delta_LZ; several -> the time-ordered
    propagation through the profile; none -> P = NaN, as the plug-in's Profile.probability raises
    'no avoided crossing' for it), "minimal" (eq.(9); points without exactly one crossing get
    P = NaN) or "propagate" (every point through the whole profile, crossings or not)."""
    csv: Optional[str] = None
    synthetic: int = 12     # bounce.synthetic_shapes index (12: one or three crossings across P1's couplings)
    estimator: str = "auto"
    y_B: float = 1.0
    y_chi: float = 1.0
    lambda_tr_eff: float = 0.1
    steps_per_radian: float = 4.0
    min_steps: int = 1

    def arrays(self):
        from . import bounce
        if self.csv:
            x, a, b, _ = bounce.read_bounce_csv(self.csv)
            return x, a, b
        if not 0 <= self.synthetic < 16:
            raise ValueError("profile.synthetic must index the 16-shape synthetic family (0..15)")
        X, A, B = bounce.synthetic_shapes(16)   # the family as tools/bench_profile.py draws it
        return X[self.synthetic], A[self.synthetic], B[self.synthetic]


# sweep axes over the fields of the spec's window block (include/lzq.h lzq_window)
WINDOW_AXES = {"window_y0": ("y0",), "window_half_width": ("half_width",), "window_sigma_lo": ("sigma_lo",),
               "window_sigma_hi": ("sigma_hi",), "window_sigma": ("sigma_lo", "sigma_hi"), "window_scale": ("scale",),
               "window_table": ("table",)}


@dataclass
class WindowSpec:
    """The source activity window W(y) of every grid point (PAPER §10 step 4; include/lzq.h
    lzq_window) in place of the Gaussian proxy of fpy:262: `block` is the base block
    ({"kind": "gauss" | "plateau" | "table", "y0", "half_width", "sigma_lo", "sigma_hi" | "sigma",
    "scale", "table"}; window.to_window), which the WINDOW_AXES sweep; u / tables are the tabulated
    profiles of the table kind (a spec JSON gives them inline, or names a two-column `u,W` file as
    "csv", which is read once and carried inline from then on, so a checkpoint key follows the
    file's contents)."""
    block: dict
    u: Optional[list] = None
    tables: Optional[list] = None

    def host_tables(self):
        from . import window as _window
        return None if self.u is None else _window.WindowTables(self.u, self.tables)

    def to_json(self) -> dict:
        d = dict(self.block)
        if self.u is not None:
            d["u"], d["tables"] = [float(x) for x in self.u], [[float(x) for x in r] for r in self.tables]
        return d

    @classmethod
    def from_json(cls, d: dict) -> "WindowSpec":
        from . import window as _window
        d = dict(d)
        csv, u, tables = d.pop("csv", None), d.pop("u", None), d.pop("tables", None)
        if csv is not None and (u is not None or tables is not None):
            raise ValueError("window: give 'csv' or inline 'u' / 'tables', not both")
        if (u is None) != (tables is None):
            raise ValueError("window: inline tables need both 'u' (knots) and 'tables' (rows of W)")
        if csv is not None:
            t = _window.WindowTables.from_csv(csv)
        elif u is not None:
            t = _window.WindowTables(u, tables)
        else:
            t = None
        rec = _window.to_window(d)   # unknown fields / kinds raise here
        if rec["kind"][0] == _native.WIN_TABLE and t is None:
            raise ValueError("window: kind 'table' needs 'csv' or inline 'u' / 'tables'")
        _window.check(rec, t)
        return cls(d, None if t is None else t.u.tolist(), None if t is None else t.W.tolist())


# sweep axes over the fields of the spec's momentum-kernel block (include/lzq.h lzq_fk)
FK_AXES = {"fk_p": "p", "fk_v_ref": "v_ref"}
LZ_AXES = ("delta_LZ", "m_mix", "dprime")


@dataclass
class FkSpec:
    """The momentum kernel F(k) of every grid point's LZ probability (PAPER §10 step 1; include/lzq.h
    lzq_fk): `block` is the base block ({"kind": "power", "p", "v_ref"}; fk.to_fk), which the FK_AXES
    sweep.  P-bar(m/T(y)) then stands inside the y-integral (Engine.yields(fk=)); delta_0 of a point is
    PAPER eq. (8) at F = 1 from the delta_LZ / m_mix / dprime axes, computed on the host, else the
    delta_0 of the base's P_chi_to_B."""
    block: dict

    def to_json(self) -> dict:
        return dict(self.block)

    @classmethod
    def from_json(cls, d: dict) -> "FkSpec":
        from . import fk as _fk
        d = dict(d)
        _fk.check(_fk.to_fk(d))   # unknown fields / kinds raise in to_fk
        return cls(d)


ODE_MAX_STEPS = 1 << 26   # a sweep's default cap on one ODE point's fixed Radau steps (LZQ_ODE_TOO_MANY_STEPS beyond)


@dataclass
class SweepSpec:
    name: str
    base: dict
    axes: List[Tuple[str, np.ndarray]]
    n_y: int = 8000
    notes: str = ""
    crossings: Optional[CrossingSpec] = None
    ode_method: str = "radau"   # ODE-path points: "radau" (the reference's integrator) | "quadrature" (opt-in)
    profile: Optional[ProfileSpec] = None
    nz: int = _native.LZQ_NZ          # the A/V kernel's z grid, AoverVKernel(..., z_max, nz) (fpy:141-156)
    z_max: float = _native.LZQ_Z_MAX
    # ODE-path points needing more fixed Radau steps than this are not integrated (a NaN row counted
    # as too_many_steps in summary.json): one long window would otherwise hold its shard for hours.
    # None = no cap (every window the reference accepts, as the single-point CLI does).
    ode_max_steps: Optional[int] = ODE_MAX_STEPS
    window: Optional[WindowSpec] = None   # None: the reference's window (fpy:262)
    # the inverse sweep (solve.py): one parameter per grid point solved for a target yield; the table
    # then holds the records at the solutions and solve.npy the results
    solve: Optional[dict] = None
    # "linspace": the reference's (nz, z_max) grid; "continuum": the converged z-integral on the
    # continuum z rule of z_max (include/lzq.h "A/V in the continuum limit"; nz is then not read)
    z_rule: str = "linspace"
    fk: Optional[FkSpec] = None   # None: the paper's F = 1 (one P per point)
    # "ode": Gamma_wash / depletion points take the ODE fallback, as the reference's fpy:372 sends them;
    # "quadrature" (opt-in): with sigma_v = 0 everywhere they run on the y-grid quadrature (include/lzq.h
    # "wash-out and source depletion"), where window, solve, --reuse-zsums and the continuum rule apply
    wash_rule: str = "ode"

    @property
    def continuum(self) -> bool:
        return self.z_rule == "continuum"

    @property
    def total(self) -> int:
        n = 1
        for _, v in self.axes:
            n *= len(v)
        return n

    def point_params(self, idx: int) -> dict:
        """Host-side decode of flat index -> axis values (for reporting / tests)."""
        out = {}
        for name, vals in reversed(self.axes):
            out[name] = float(vals[idx % len(vals)])
            idx //= len(vals)
        return out

    def to_json(self) -> dict:
        d = {"name": self.name, "base": self.base, "n_y": self.n_y, "notes": self.notes,
             "axes": [{"field": n, "values": [float(x) for x in v]} for n, v in self.axes]}
        if self.crossings is not None:
            d["crossings"] = dict(self.crossings.__dict__)
        if self.ode_method != "radau":
            d["ode_method"] = self.ode_method
        if self.profile is not None:
            d["profile"] = dict(self.profile.__dict__)
        if (self.nz, self.z_max) != (_native.LZQ_NZ, _native.LZQ_Z_MAX):
            d["nz"], d["z_max"] = int(self.nz), float(self.z_max)
        if self.ode_max_steps != ODE_MAX_STEPS:
            d["ode_max_steps"] = self.ode_max_steps
        if self.window is not None:
            d["window"] = self.window.to_json()
        if self.solve is not None:
            d["solve"] = _solve.normalize(self.solve)
        if self.z_rule != "linspace":
            d["z_rule"] = self.z_rule
        if self.fk is not None:
            d["fk"] = self.fk.to_json()
        if self.wash_rule != "ode":
            d["wash_rule"] = self.wash_rule
        return d

    def axis_values(self, start: int, count: int, device) -> dict:
        """{axis name: [count] torch tensor} of grid indices [start, start+count) (C order)."""
        import torch
        idx = torch.arange(start, start + count, dtype=torch.int64, device=device)
        vals, stride = {}, 1
        for name, v in reversed(self.axes):
            t = torch.as_tensor(np.asarray(v, dtype=np.float64), device=device)
            vals[name] = t[(idx // stride) % len(v)]
            stride *= len(v)
        return vals

    def crossing_arrays(self, start: int, count: int, device):
        """Per-point crossing parameters [count, n_cross] (torch, on `device`) for C5."""
        import torch
        cs = self.crossings
        names = [n for n, _ in self.axes]
        if "m_mix" not in names or "dprime" not in names:
            raise ValueError("a multi-crossing spec needs m_mix and dprime axes")
        idx = torch.arange(start, start + count, dtype=torch.int64, device=device)
        vals = {}
        stride = 1
        for name, v in reversed(self.axes):
            t = torch.as_tensor(np.asarray(v, dtype=np.float64), device=device)
            vals[name] = t[(idx // stride) % len(v)]
            stride *= len(v)
        v_w = vals["v_w"] if "v_w" in vals else torch.full_like(vals["m_mix"], float(self.base["v_w"]))
        m0, d0 = vals["m_mix"], vals["dprime"].abs()
        delta0 = m0 * m0 / (2.0 * v_w * d0)
        L = torch.sqrt(v_w / d0) * torch.clamp(torch.sqrt(delta0), min=1.0)
        a, b, dd = (torch.as_tensor(r, device=device) for r in cs.pattern())
        c = torch.arange(cs.n_cross, dtype=torch.float64, device=device)
        m = m0[:, None] * (1.0 + cs.jitter * a[None, :])
        dp = d0[:, None] * (1.0 + cs.jitter * b[None, :])
        xi = L[:, None] * (cs.spacing_lz * c[None, :] + cs.jitter * dd[None, :])
        return m.contiguous(), dp.contiguous(), xi.contiguous(), v_w


ODE_FIELDS = ("sigma_v_chi_GeV_m2", "Gamma_wash_over_H", "deplete_DM_from_source")  # fpy:372 gate


def is_ode_spec(spec: "SweepSpec") -> bool:
    """Does any point of the sweep leave the fast path (fpy:372) for the ODE fallback?  (Not under
    "wash_rule": "quadrature", whose wash-out / depletion points stay on the y-grid: check_wash_spec.)"""
    if spec.wash_rule == "quadrature":
        return False
    b = spec.base
    base_ode = bool(b.get("deplete_DM_from_source")) or float(b.get("sigma_v_chi_GeV_m2", 0.0)) != 0.0 or \
        float(b.get("Gamma_wash_over_H", 0.0)) != 0.0
    return base_ode or any(name in ODE_FIELDS and np.any(np.asarray(v) != 0) for name, v in spec.axes)


def uses_wash(spec: "SweepSpec") -> bool:
    """Does the sweep run through the wash-out quadrature's kernels (Engine.sweep(wash=))?  Under
    "wash_rule": "quadrature", when its base or axes set Gamma_wash_over_H / deplete_DM_from_source or its
    solve asks for Gamma_wash_over_H; a spec without any of it takes the routes it takes today."""
    if spec.wash_rule != "quadrature":
        return False
    b = spec.base
    if bool(b.get("deplete_DM_from_source")) or float(b.get("Gamma_wash_over_H", 0.0)) != 0.0:
        return True
    if any(name in _native.WASH_FIELD for name, _ in spec.axes):
        return True
    return spec.solve is not None and _solve.normalize(spec.solve)["field"] in _native.WASH_FIELD


def wash_block(spec: "SweepSpec") -> dict:
    """The base block of a wash sweep (wash.to_wash's mapping)."""
    b = spec.base
    return {"sigma_v_chi_GeV_m2": float(b.get("sigma_v_chi_GeV_m2", 0.0) or 0.0),
            "Gamma_wash_over_H": float(b.get("Gamma_wash_over_H", 0.0) or 0.0),
            "deplete_DM_from_source": bool(b.get("deplete_DM_from_source"))}


def check_wash_spec(spec: "SweepSpec") -> None:
    """A "wash_rule" the sweep cannot run, as a ValueError: an unknown rule; with "quadrature" any
    sigma_v != 0 (the Y_chi equation is then not linear: the ODE fallback's), a sigma_v axis at all (the
    kernels decode no such field), a momentum kernel next to wash-out, window axes that collide, and
    every value of a Gamma axis that the library refuses."""
    if spec.wash_rule not in ("ode", "quadrature"):
        raise ValueError(f"wash_rule must be 'ode' or 'quadrature', got {spec.wash_rule!r}")
    if spec.wash_rule != "quadrature":
        return
    if float(spec.base.get("sigma_v_chi_GeV_m2", 0.0) or 0.0) != 0.0:
        raise ValueError("wash_rule 'quadrature' with sigma_v_chi_GeV_m2 != 0 in the base: the linear form needs "
                         "sigma_v = 0 everywhere (drop the rule for the ODE fallback)")
    for n, v in spec.axes:
        if n == "sigma_v_chi_GeV_m2":
            raise ValueError("wash_rule 'quadrature' with a sigma_v_chi_GeV_m2 axis: the linear form needs sigma_v = 0 "
                             "everywhere" + ("" if np.any(np.asarray(v) != 0) else " (an all-zero axis sweeps nothing: drop it)"))
    if not uses_wash(spec):
        return
    if spec.fk is not None:
        raise ValueError("an 'fk' section on a spec with wash-out or depletion under wash_rule 'quadrature': the "
                         "momentum kernel together with wash-out is not built")
    if spec.window is not None and window_axes_collide(spec):
        raise ValueError("wash_rule 'quadrature' on a spec whose window axes collide (the grid entry points refuse them)")
    from . import wash as _wash
    for n, v in spec.axes:
        if n == "Gamma_wash_over_H":
            rec = np.repeat(_wash.to_wash(wash_block(spec)), len(v))
            rec[n] = np.asarray(v, dtype=np.float64)
            _wash.check(rec)
    _wash.check(_wash.to_wash(wash_block(spec)))


def grid_records(spec: "SweepSpec", start: int, count: int, engine=None):
    """Explicit point records of grid indices [start, start+count): (POINT_DTYPE, ODE_DTYPE)
    numpy arrays, decoded in C order like lzq_sweep_grid.  The LZ axes set P through the
    closed form evaluated on the GPU (lzq_p_closed_form, fpy:183-184)."""
    pts = np.repeat(to_point(spec.base), count)
    ods = np.repeat(to_ode_params(spec.base), count)
    idx = np.arange(start, start + count, dtype=np.int64)
    stride = 1
    lz = {}
    for name, vals in reversed(spec.axes):
        v = np.asarray(vals, dtype=np.float64)[(idx // stride) % len(vals)]
        stride *= len(vals)
        if name in ("delta_LZ", "m_mix", "dprime"):
            lz[name] = v
        elif name in PROFILE_FIELDS:
            continue          # P comes from the profile (profile_P)
        elif name in WINDOW_AXES:
            continue          # a field of the point's window block (window_records)
        elif name in FK_AXES:
            continue          # a field of the point's momentum-kernel block (fk_records)
        elif name in ODE_FIELDS:
            ods[name] = v if name != "deplete_DM_from_source" else (v != 0).astype(np.int32)
        elif name == "Y_chi_init":
            pts["Y_chi_init"], pts["has_Y_chi_init"] = v, 1
        elif name == "n_chi_at_Tp_GeV3":
            pts["n_chi_at_Tp_GeV3"], pts["has_n_chi_at_Tp"] = v, 1
        else:
            pts[name] = v
    if lz:
        if "m_mix" in lz:  # PAPER eq.(8), F = 1
            delta = lz["m_mix"] * lz["m_mix"] / (2.0 * np.maximum(pts["v_w"], 1e-12) * np.abs(lz["dprime"]))
        else:
            delta = lz["delta_LZ"]
        if engine is None:
            from .engine import default_engine
            engine = default_engine()
        pts["P_chi_to_B"] = engine.p_closed_form(delta).cpu().numpy()
    return pts, ods


def window_records(spec: "SweepSpec", start: int, count: int) -> np.ndarray:
    """The window blocks (WINDOW_DTYPE) of grid indices [start, start+count): the spec's base block
    with the WINDOW_AXES values decoded in C order, like grid_records."""
    from . import window as _window
    rec = np.repeat(_window.to_window(spec.window.block), count)
    idx = np.arange(start, start + count, dtype=np.int64)
    stride = 1
    for name, vals in reversed(spec.axes):
        if name in WINDOW_AXES:
            v = np.asarray(vals, dtype=np.float64)[(idx // stride) % len(vals)]
            for f in WINDOW_AXES[name]:
                rec[f] = v.astype(np.int32) if f == "table" else v
        stride *= len(vals)
    return rec


def fk_records(spec: "SweepSpec", start: int, count: int, pts: np.ndarray) -> tuple:
    """(FK_DTYPE blocks, delta_0) of grid indices [start, start+count): the spec's base block with the
    FK_AXES values decoded in C order, like grid_records (whose records `pts` are: v_w enters eq. (8));
    delta_0 from the delta_LZ or the m_mix / dprime axes by PAPER eq. (8) at F = 1 on the host, else
    from the records' P_chi_to_B."""
    from . import fk as _fk
    rec = np.repeat(_fk.to_fk(spec.fk.block), count)
    idx = np.arange(start, start + count, dtype=np.int64)
    stride = 1
    lz = {}
    for name, vals in reversed(spec.axes):
        if name in FK_AXES or name in LZ_AXES:
            v = np.asarray(vals, dtype=np.float64)[(idx // stride) % len(vals)]
            if name in FK_AXES:
                rec[FK_AXES[name]] = v
            else:
                lz[name] = v
        stride *= len(vals)
    if "m_mix" in lz:
        delta = lz["m_mix"] * lz["m_mix"] / (2.0 * np.maximum(pts["v_w"], 1e-12) * np.abs(lz["dprime"]))
    elif "delta_LZ" in lz:
        delta = lz["delta_LZ"]
    else:
        delta = _fk.delta_from_P(pts["P_chi_to_B"])
    return rec, np.ascontiguousarray(delta, dtype=np.float64)


def _axis_from_json(a: dict) -> Tuple[str, np.ndarray]:
    if "values" in a:
        v = np.asarray(a["values"], dtype=np.float64)
    elif "logspace" in a:
        v = np.logspace(*a["logspace"][:2], int(a["logspace"][2]))
    elif "linspace" in a:
        v = np.linspace(*a["linspace"][:2], int(a["linspace"][2]))
    else:
        raise ValueError(f"axis {a!r} needs values / linspace / logspace")
    if a["field"] not in _native.FIELD and a["field"] not in ODE_FIELDS and a["field"] not in PROFILE_FIELDS and \
            a["field"] not in WINDOW_AXES and a["field"] not in FK_AXES:
        raise ValueError(f"unknown sweep field {a['field']!r}")
    return a["field"], v


def spec_from_json(d: dict) -> SweepSpec:
    base = dict(EQUAL_MASS)
    if "config" in d:
        with open(d["config"]) as f:
            base.update(json.load(f))
    base.update(d.get("base", {}))
    cr = CrossingSpec(**d["crossings"]) if d.get("crossings") else None
    method = d.get("ode_method", "radau")
    if method not in ("radau", "quadrature"):
        raise ValueError(f"ode_method must be 'radau' or 'quadrature', got {method!r}")
    prof = ProfileSpec(**d["profile"]) if d.get("profile") else None
    if prof is not None and prof.estimator not in ("auto", "minimal", "propagate"):
        raise ValueError(f"profile estimator must be auto / minimal / propagate, got {prof.estimator!r}")
    axes = [_axis_from_json(a) for a in d["axes"]]
    if prof is None and any(n in PROFILE_FIELDS for n, _ in axes):
        raise ValueError(f"axes {PROFILE_FIELDS} need a 'profile' section")
    if prof is not None and cr is not None:
        raise ValueError("a spec takes either 'crossings' or 'profile'")
    win = WindowSpec.from_json(d["window"]) if d.get("window") else None
    for n, v in axes:
        if n == "window_table" and np.any(v != np.floor(v)):
            raise ValueError("window_table values must be integers (table indices)")
    nz, z_max = _native.zgrid(d.get("nz", _native.LZQ_NZ), d.get("z_max", _native.LZQ_Z_MAX))
    ms = d.get("ode_max_steps", ODE_MAX_STEPS)
    if ms is not None and int(ms) < 0:
        raise ValueError("ode_max_steps must be >= 0 (0 or null: no cap)")
    # 0 means "no cap", as --ode-max-steps 0 on the command line does (one meaning in both places)
    spec = SweepSpec(d.get("name", "custom"), base, axes, int(d.get("n_y", 8000)), d.get("notes", ""), cr, method, prof,
                     nz, z_max, None if ms is None or int(ms) == 0 else int(ms), win,
                     _solve.normalize(d["solve"]) if d.get("solve") else None, d.get("z_rule", "linspace"),
                     FkSpec.from_json(d["fk"]) if d.get("fk") is not None else None, d.get("wash_rule", "ode"))
    check_wash_spec(spec)
    check_z_rule(spec)
    check_fk_spec(spec)
    check_window_spec(spec)
    check_solve_spec(spec)
    return spec


def check_z_rule(spec: SweepSpec) -> None:
    """A "z_rule" the sweep cannot run, as a ValueError: an unknown rule, a z_max the continuum rule
    refuses, or the continuum rule on a spec whose points take the ODE fallback (the ODE spline tables
    stay on the linspace grids)."""
    if spec.z_rule not in ("linspace", "continuum"):
        raise ValueError(f"z_rule must be 'linspace' or 'continuum', got {spec.z_rule!r}")
    if spec.continuum:
        _native.cont_z_max(spec.z_max)
        if is_ode_spec(spec):
            raise ValueError("z_rule 'continuum' on a spec whose points take the ODE fallback (sigma_v / Gamma_wash / "
                             "depletion): the ODE spline tables are built on the linspace z grids only")


def check_solve_spec(spec: SweepSpec) -> None:
    """A "solve" section the sweep cannot run, as a ValueError that says why (before any upload): the
    solve's own refusals (solve.check: the library's host-side checks), a spec whose points take the ODE
    fallback, and a spec on the record path -- crossings or a profile P next to a solve for P or an LZ
    field, or window axes that collide."""
    if spec.solve is None:
        return
    sv = _solve.normalize(spec.solve)
    if is_ode_spec(spec):
        raise ValueError("a 'solve' section on a spec whose points take the ODE fallback (sigma_v / Gamma_wash / "
                         "depletion): the solve stays in the quadrature regime")
    if (spec.crossings is not None or spec.profile is not None) and \
            sv["field"] in ("P_chi_to_B", "delta_LZ", "m_mix", "dprime"):
        raise ValueError(f"solve for {sv['field']!r} on a spec whose P comes from crossings or a profile (a per-point "
                         "P override)")
    if spec.window is not None and window_axes_collide(spec):
        raise ValueError("a 'solve' section on a spec whose window axes collide (the grid entry points refuse them)")
    _solve.check(sv, [n for n, _ in grid_axes_for_kernel(spec)], None if spec.window is None else spec.window.block,
                 wash=wash_block(spec) if uses_wash(spec) else None)


def check_fk_spec(spec: SweepSpec) -> None:
    """An "fk" section the sweep cannot run, as a ValueError: fk axes without the section, a spec whose
    points take the ODE fallback, whose P comes from crossings or a profile (P-bar needs delta_0, not a
    P), or that carries a solve (the solve kernels take no momentum kernel); m_mix without dprime; and
    every block of the fk axes that the library refuses."""
    names = [n for n, _ in spec.axes]
    if spec.fk is None:
        if any(n in FK_AXES for n in names):
            raise ValueError(f"axes {tuple(FK_AXES)} need an 'fk' section")
        return
    if is_ode_spec(spec):
        raise ValueError("an 'fk' section on a spec whose points take the ODE fallback (sigma_v / Gamma_wash / "
                         "depletion): the ODE path takes no momentum kernel")
    if spec.crossings is not None or spec.profile is not None:
        raise ValueError("an 'fk' section on a spec whose P comes from crossings or a profile: P-bar is built "
                         "from delta_0 (the delta_LZ or m_mix / dprime axes)")
    if spec.solve is not None:
        raise ValueError("an 'fk' section next to a 'solve' section: the solve kernels take no momentum kernel")
    if ("m_mix" in names) != ("dprime" in names):
        raise ValueError("an 'fk' spec takes delta_0 from a delta_LZ axis or from m_mix and dprime axes together")
    from . import fk as _fk
    for n, v in spec.axes:
        if n in FK_AXES:
            rec = np.repeat(_fk.to_fk(spec.fk.block), len(v))
            rec[FK_AXES[n]] = np.asarray(v, dtype=np.float64)
            try:
                _fk.check(rec)
            except _native.LzqError as e:
                raise ValueError(f"axis {n!r}: {e}") from None


def check_window_spec(spec: SweepSpec) -> None:
    """A window on an ODE spec is a usage error: the ODE path keeps the reference's Gaussian
    (include/lzq.h); window axes need a window."""
    if spec.window is None:
        if any(n in WINDOW_AXES for n, _ in spec.axes):
            raise ValueError(f"axes {tuple(WINDOW_AXES)} need a 'window' section")
        return
    if is_ode_spec(spec):
        raise ValueError("a 'window' section on a spec whose points take the ODE fallback (sigma_v / Gamma_wash / "
                         "depletion): the ODE path takes no window")


def builtin_specs() -> dict:
    """BASELINE.json configs C2-C4 with the grids of SURVEY §8d."""
    ls, lin = np.logspace, np.linspace
    return {
        "C2": SweepSpec("C2", dict(EQUAL_MASS),
                        [("m_mix", ls(-3, 0, 1000)), ("dprime", ls(-3, 1, 1000))],
                        notes="equal-mass config, coupling x sweep-rate, v_w=0.30, F=1 -> delta -> P"),
        "C3": SweepSpec("C3", dict(EQUAL_MASS),
                        [("m_chi_GeV", ls(0, 3.5, 100)), ("I_p", lin(0.05, 1, 100)), ("delta_LZ", ls(-4, 0, 1000))],
                        notes="m_chi crosses T=m/3 inside the window"),
        "C5": SweepSpec("C5", dict(EQUAL_MASS),
                        [("m_mix", ls(-3, 0, 1000)), ("dprime", ls(-3, 1, 1000))],
                        notes="C2 grid, 8 jittered sequential crossings per point, coherent P (propagator)",
                        crossings=CrossingSpec()),
        "P1": SweepSpec("P1", dict(EQUAL_MASS),
                        [("y_B", lin(0.5, 2.0, 100)), ("y_chi", lin(0.5, 2.0, 100)), ("lambda_tr_eff", ls(-3, 0, 100))],
                        notes="P from a bounce profile (synthetic shape 12; PAPER eqs.(5)-(9)) over the couplings "
                              "y_B x y_chi x lambda_tr_eff, then the dense quadrature",
                        profile=ProfileSpec()),
        "C4": SweepSpec("C4", dict(EQUAL_MASS),
                        [("beta_over_H", ls(1, 3, 10)), ("I_p", lin(0.05, 1, 100)), ("v_w", lin(0.05, 0.95, 10)),
                         ("source_shape_sigma_y", lin(3, 30, 10)), ("m_chi_GeV", ls(-1, 3.5, 10)),
                         ("delta_LZ", ls(-4, 0, 100))],
                        notes="full cosmological scan, 1e8 points"),
    }


def shard_range(total: int, rank: int, world: int) -> Tuple[int, int]:
    """contiguous blocks [r*N/W, (r+1)*N/W)."""
    return rank * total // world, (rank + 1) * total // world


def spec_key(spec: SweepSpec) -> str:
    """Hash of everything a shard's contents depend on: the sweep definition (axes, base
    config, n_y, crossings, ODE method), the library's ABI version, its machine code
    (_native.library_id: any rebuild that changes a kernel changes the key) and the bit-changing
    tuning state (the inner-loop exponential).  --resume after such a change starts afresh
    instead of mixing shards of different numerics."""
    d = {"spec": spec.to_json(), "abi": _native.ABI_VERSION, "lib": _native.library_id(),
         "tune": dict(_native.TUNE_STATE)}
    d["spec"].pop("notes", None)
    return hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()[:16]


def _shard_file(out_dir: str, start: int, count: int, key: str = "") -> str:
    return os.path.join(out_dir, f"shard_{key + '_' if key else ''}{start:012d}_{count}.npy")


def prepare_out_dir(out_dir: str, spec: SweepSpec, resume: bool, rank: int = 0) -> str:
    """Create `out_dir`, check / write its manifest.json; returns the shard key.  --resume
    into a directory whose manifest describes another sweep raises instead of mixing tables."""
    os.makedirs(out_dir, exist_ok=True)
    key = spec_key(spec)
    man = os.path.join(out_dir, "manifest.json")
    if resume and os.path.exists(man):
        with open(man) as f:
            old = json.load(f).get("key")
        if old != key:
            raise RuntimeError(f"--resume: {out_dir} holds shards of another sweep (manifest key {old}, this "
                               f"sweep {key}); use a fresh --out directory")
    if rank == 0:
        tmp = man + f".tmp{os.getpid()}"
        with open(tmp, "w") as f:
            json.dump({"key": key, "abi": _native.ABI_VERSION, "lib": _native.library_id(),
                       "tune": dict(_native.TUNE_STATE), "spec_def": spec.to_json()}, f, indent=1)
        os.replace(tmp, man)
    return key


ComputeFn = Callable[[int, int, "object"], None]  # (start, count, out_tensor[count, 6]) -> None
MAX_INFLIGHT_WRITES = 3   # checkpoint chunks copied out and waiting for the disk (pinned ring of <= 4)


def _status_file(shard_path: str) -> str:
    """The ODE status counts of one checkpointed chunk (int64[8] per lzq_ode_status), so a resumed
    sweep's summary counts every chunk, not only those computed by this run."""
    return shard_path[:-len(".npy")] + ".status.npy"


def _solve_file(shard_path: str) -> str:
    """The solve results of one checkpointed chunk ((n, 6) float64), beside its records."""
    return shard_path[:-len(".npy")] + ".solve.npy"


def _save_shard(path: str, arr: np.ndarray) -> None:
    tmp = path + ".tmp.npy"
    np.save(tmp, arr, allow_pickle=False)
    os.replace(tmp, path)


def run_local(compute: ComputeFn, start: int, end: int, make_out: Callable[[int], "object"], chunk: int,
              out_dir: Optional[str] = None, resume: bool = False, sync: Callable[[], None] = lambda: None,
              log: Callable[[str], None] = lambda s: None, key: str = "", fit=None, keep_table: bool = True):
    """Evaluate [start, end) in chunks into one (end-start, 6) tensor, with optional
    per-chunk checkpoint files (named by `key`, see spec_key).

    fit: an accumulator (fit.make_accumulator) that every chunk's rows, computed or resumed from a
    checkpoint, are folded into on the chunk's own stream.  keep_table=False (only with a fit):
    chunk outputs go through a ring of two chunk-sized buffers instead of an (end-start, 6) shard,
    no checkpoint is written, and None is returned: the fit is all that is kept.

    On the GPU the checkpoint of chunk i is copied out on a side stream (device -> pinned host
    memory, ordered after chunk i's kernels by an event) and written by a worker thread while
    chunk i+1 computes, so checkpointing does not serialise the sweep.  The pinned buffers are a
    small ring reused chunk after chunk, and at most MAX_INFLIGHT_WRITES writes wait for the disk
    (a slow disk throttles the sweep rather than pinning the whole shard).  On CPU tensors
    (tests) it is written inline."""
    import torch
    if not keep_table:
        if fit is None:
            raise ValueError("keep_table=False needs a fit")
        if resume:
            raise ValueError("keep_table=False cannot resume: fit-only checkpoints are not written")
        out_dir = None
        n_ring = max(1, min(chunk, end - start))
        local = make_out(2 * n_ring)
    else:
        local = make_out(end - start)
    # a solving compute (make_compute with a "solve" section) passes each chunk's (n, 6) results back
    # on itself, as the ODE status counts travel: .solve_last after a call; the shard's results are
    # collected here into .solve_local, each checkpointed chunk writing a .solve.npy sibling
    solving = getattr(compute, "solve", None) is not None
    # keep_table=False: no result table either -- the x column alone (NaN where a row has no solution)
    # and integer counts, which is all the summary block needs (solve_summary_streamed)
    if solving and keep_table:
        compute.solve_local = make_out(end - start)
    elif solving:
        compute.solve_local = None
        compute.solve_x = local.new_empty(end - start)
        compute.solve_parts = torch.zeros(7, dtype=torch.int64, device=local.device)  # status counts, evals sum, max
    on_gpu = bool(getattr(local, "is_cuda", False)) and out_dir is not None
    pending = []    # (future, pinned buffer) of the writes in flight, oldest first
    ring = []       # pinned host buffers free for reuse
    if on_gpu:
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=1)
        copy_stream = torch.cuda.Stream(device=local.device)

    def flush(block: bool):
        while pending and (block or pending[0][0].done()):
            fut, buf = pending.pop(0)
            fut.result()   # re-raise a failed write here
            ring.append(buf)

    try:
        for c0 in range(start, end, chunk):
            n = min(chunk, end - c0)
            if keep_table:
                view = local[c0 - start:c0 - start + n]
            else:
                slot = ((c0 - start) // chunk) % 2
                view = local[slot * n_ring:slot * n_ring + n]
            path = _shard_file(out_dir, c0, n, key) if out_dir else None
            if path and resume and os.path.exists(path):
                arr = np.load(path, allow_pickle=False)
                if arr.shape != (n, 6):
                    raise RuntimeError(f"checkpoint {path} has shape {arr.shape}, expected {(n, 6)}")
                view.copy_(torch.from_numpy(arr))
                counts = getattr(compute, "ode_status", None)
                if counts is not None:   # the resumed chunk's ODE status counts (summary.json ode_status)
                    st = _status_file(path)
                    if not os.path.exists(st):
                        raise RuntimeError(f"checkpoint {path} has no ODE status record {st}")
                    counts += np.load(st, allow_pickle=False)
                if solving:
                    sp = _solve_file(path)
                    if not os.path.exists(sp):
                        raise RuntimeError(f"checkpoint {path} has no solve record {sp}")
                    sarr = np.load(sp, allow_pickle=False)
                    if sarr.shape != (n, 6):
                        raise RuntimeError(f"checkpoint {sp} has shape {sarr.shape}, expected {(n, 6)}")
                    compute.solve_local[c0 - start:c0 - start + n].copy_(torch.from_numpy(sarr))
                if fit is not None:
                    fit.update(view, c0)
                log(f"resumed {path}")
                continue
            compute(c0, n, view)
            if solving and keep_table:
                compute.solve_local[c0 - start:c0 - start + n].copy_(compute.solve_last)
            elif solving:
                r = compute.solve_last
                status, ev = r[:, 5].to(torch.int64), r[:, 4].to(torch.int64)
                compute.solve_x[c0 - start:c0 - start + n] = torch.where(status <= _native.SOLVE_MAX_EVALS, r[:, 0],
                                                                         torch.full_like(r[:, 0], float("nan")))
                compute.solve_parts[:5] += torch.bincount(status.clamp(0, 4), minlength=5)
                compute.solve_parts[5] += ev.sum()
                compute.solve_parts[6] = torch.maximum(compute.solve_parts[6], ev.max())
            if fit is not None:
                fit.update(view, c0)
            log(f"chunk [{c0}, {c0 + n}) launched")
            if not path:
                continue
            if getattr(compute, "ode_status", None) is not None:
                _save_shard(_status_file(path), np.asarray(compute.last_chunk, dtype=np.int64))
            if solving:   # (written before the records: a table shard never stands without its sibling)
                sync()
                _save_shard(_solve_file(path), compute.solve_last.detach().cpu().numpy())
            if not on_gpu:
                sync()
                _save_shard(path, view.detach().cpu().numpy())
                continue
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(local.device))
            # at most MAX_INFLIGHT_WRITES chunks wait for the disk: when the disk is slower than the
            # GPU the sweep waits here instead of pinning the whole shard in host memory
            flush(block=False)
            while len(pending) >= MAX_INFLIGHT_WRITES:
                fut, buf = pending.pop(0)
                fut.result()
                ring.append(buf)
            full = next((b for b in ring if b.shape[0] >= n), None)
            if full is not None:
                ring.remove(full)
            else:
                full = torch.empty((chunk, 6), dtype=view.dtype, pin_memory=True)
            host = full[:n]
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(ev)
                host.copy_(view, non_blocking=True)
                done_ev = torch.cuda.Event()
                done_ev.record(copy_stream)

            def write(path=path, host=host, done_ev=done_ev):
                done_ev.synchronize()
                _save_shard(path, host.numpy())
            pending.append((pool.submit(write), full))
            flush(block=False)
        if on_gpu:
            flush(block=True)
    finally:
        if on_gpu:
            pool.shutdown(wait=True)
    return local if keep_table else None


def solve_summary_streamed(compute, total: int, rank: int, world: int, group=None) -> dict:
    """The "solve" block of a keep_table=False sweep, the same on every rank and for every world size:
    the ranks' integer counts are summed (the evaluations' maximum taken), and their x columns --
    shards differ by at most one row, so each is padded to the longest with NaN -- gathered in one
    collective (8 B a point: the one thing of a fit-only solve that grows with the grid)."""
    import torch
    import torch.distributed as dist
    parts, x = compute.solve_parts.clone(), compute.solve_x
    if dist.is_available() and dist.is_initialized():
        nccl = dist.get_backend(group) == "nccl"
        if not nccl:
            parts, x = parts.cpu(), x.cpu()
        mx = parts[6:7].clone()
        dist.all_reduce(parts, group=group)
        dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=group)
        parts[6] = mx[0]
        m = max(e - b for b, e in (shard_range(total, r, world) for r in range(world)))
        pad = torch.full((m,), float("nan"), dtype=x.dtype, device=x.device)
        pad[:x.numel()] = x
        allx = torch.empty(world * m, dtype=x.dtype, device=x.device)
        dist.all_gather_into_tensor(allx, pad, group=group)
        x = allx
    parts = parts.cpu().numpy()
    return _solve.summary_from_parts(compute.solve, x.cpu().numpy(), parts[:5], int(parts[5]), int(parts[6]), total)


def launched_distributed(world: int) -> bool:
    """True under torch.distributed.run (any world size, 1 included: its rendezvous sets
    MASTER_ADDR / MASTER_PORT) or whenever WORLD_SIZE > 1."""
    return world > 1 or ("MASTER_ADDR" in os.environ and "MASTER_PORT" in os.environ)


GATHER_ROWS = 1 << 18   # rows per rank per collective when the shards differ in size


def gather_table(local, total: int, rank: int, world: int, group=None, rows_per_round: int = GATHER_ROWS):
    """All-gather the per-rank shards (sizes differ by <= 1) into the full (total, 6) table on
    every rank (the one collective of north_star (3); every rank keeps the table, 1.7% of a
    288-GB HBM at C4, so any rank can post-process the grid without a second collective).

    Equal shards (C4 at W = 2, 4, 8): one all_gather_into_tensor straight into the output --
    rank-major order IS flat-index order -- with no padding and no concatenation: the transient
    is nothing beyond the table and the rank's own shard.  Unequal shards: the common m0 rows of
    every shard in rounds of <= rows_per_round rows per rank (transient world x rows_per_round
    x 48 B), each round's rank-major block scattered to the shards' places, then one round for
    the last row of the shards that have m0 + 1.  RCCL moves device tensors over xGMI; gloo (CPU
    tests, one-GPU rehearsals) stages through host memory.  With no process group (a plain
    single-process run) the local shard is the table; under a launcher the collective runs even
    for one rank, so a 1-rank torchrun exercises RCCL."""
    import torch
    import torch.distributed as dist
    if world == 1 and not (dist.is_available() and dist.is_initialized()):
        return local
    rng = [shard_range(total, r, world) for r in range(world)]
    sizes = [e - s for s, e in rng]
    nccl = dist.get_backend(group) == "nccl"
    src = local if nccl else local.cpu()
    src = src.contiguous()
    out = torch.empty((total, 6), dtype=local.dtype, device=src.device)
    if len(set(sizes)) == 1:
        dist.all_gather_into_tensor(out, src, group=group)
        return out if nccl else out.to(local.device)
    m0 = min(sizes)
    c = max(1, min(rows_per_round, m0))
    tmp = torch.empty((world * c, 6), dtype=local.dtype, device=src.device)
    for k in range(0, m0, c):
        cc = min(c, m0 - k)
        buf = tmp[:world * cc]
        dist.all_gather_into_tensor(buf, src[k:k + cc], group=group)
        for r in range(world):
            out[rng[r][0] + k:rng[r][0] + k + cc] = buf[r * cc:(r + 1) * cc]
    last = torch.zeros((1, 6), dtype=local.dtype, device=src.device)
    if sizes[rank] > m0:
        last[0] = src[m0]
    lb = torch.empty((world, 6), dtype=local.dtype, device=src.device)
    dist.all_gather_into_tensor(lb, last, group=group)
    for r in range(world):
        if sizes[r] > m0:
            out[rng[r][0] + m0] = lb[r]
    return out if nccl else out.to(local.device)


def summarize(table: np.ndarray, spec: SweepSpec, elapsed: Optional[float] = None) -> dict:
    """Grid-wide statistics, reduced on the host in flat-index order (deterministic); keys
    match yields_out.json "final" (fpy:425-427) plus P_used."""
    stats = {}
    for j, k in enumerate(YIELD_FIELDS):
        col = table[:, j]
        fin = col[np.isfinite(col)]
        stats[k] = {"min": float(fin.min()) if fin.size else None, "max": float(fin.max()) if fin.size else None,
                    "mean": float(np.add.reduce(fin) / fin.size) if fin.size else None,
                    "n_nonfinite": int(col.size - fin.size)}
    best = int(np.nanargmin(np.abs(table[:, 4] - 5.357)))  # closest to the Planck ratio (PAPER eq.(22))
    return {"spec": spec.name, "n_points": int(table.shape[0]), "fields": list(YIELD_FIELDS), "final": stats,
            "closest_to_planck_ratio": {"index": best, "params": spec.point_params(best),
                                        "final": dict(zip(YIELD_FIELDS, map(float, table[best])))},
            "elapsed_s": elapsed}


def ode_status_summary(counts, group=None, device=None) -> Optional[dict]:
    """Grid-wide ODE point counts per lzq_ode_status (summed over ranks in rank order)."""
    if counts is None:
        return None
    import torch
    import torch.distributed as dist
    c = torch.as_tensor(np.asarray(counts, dtype=np.int64))
    if dist.is_available() and dist.is_initialized():
        if dist.get_backend(group) == "nccl":
            c = c.to(device)
        dist.all_reduce(c, group=group)
    c = c.cpu().numpy()
    names = {_native.ODE_OK: "ok", _native.ODE_BAD_GRID: "bad_grid", _native.ODE_BAD_STEP: "bad_step",
             _native.ODE_TOO_MANY_STEPS: "too_many_steps", _native.ODE_NEWTON: "newton_failed",
             _native.ODE_NOT_LINEAR: "not_linear", _native.ODE_UNRESOLVED: "quadrature_unresolved",
             _native.ODE_BAD_TABLE: "bad_table"}
    return {names.get(k, str(k)): int(v) for k, v in enumerate(c) if v}


def run_sweep(spec: SweepSpec, engine=None, rank: int = 0, world: int = 1, chunk: int = 1 << 20,
              out_dir: Optional[str] = None, resume: bool = False, group=None, log=print, reuse: bool = False,
              fit=None, keep_table: bool = True):
    """Evaluate `spec` on this rank's shard, all-gather, return the full table (torch, on
    the engine's device).

    fit: a fit.FitSpec; every chunk is folded into a device-resident fit state on the sweep's
    stream, the ranks' states are combined, and (table, fit result) is returned -- the result as
    fit.HostFit.result gives it, the same on every rank and for every world size.
    keep_table=False (only with a fit): no shard, no all-gather; (None, fit result)."""
    import torch
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    start, end = shard_range(spec.total, rank, world)
    key = prepare_out_dir(out_dir, spec, resume, rank) if out_dir else ""

    compute = make_compute(spec, engine, reuse=reuse)
    acc = None
    if fit is not None:
        from . import fit as _fit
        if not keep_table and fit.posterior is not None and fit.posterior["offset"] == "best":
            raise ValueError(_fit.NO_TABLE_BEST)
        acc = _fit.make_accumulator(fit, fit.resolve(spec), engine, fit.axis_values(spec))
    elif not keep_table:
        raise ValueError("keep_table=False needs a fit")
    local = run_local(compute, start, end,
                      lambda n: torch.empty((n, 6), dtype=torch.float64, device=engine.device), chunk,
                      out_dir, resume, sync=torch.cuda.synchronize, log=log, key=key, fit=acc,
                      keep_table=keep_table)
    run_sweep.ode_status = ode_status_summary(getattr(compute, "ode_status", None), group, engine.device)
    # the solve results: six doubles a row, gathered like the records (the same on every rank)
    solving = getattr(compute, "solve", None) is not None
    run_sweep.solve = gather_table(compute.solve_local, spec.total, rank, world, group) \
        if solving and keep_table else None
    run_sweep.solve_summary = None if not solving else (
        _solve.summary(compute.solve, run_sweep.solve.cpu().numpy()) if keep_table
        else solve_summary_streamed(compute, spec.total, rank, world, group))
    table = gather_table(local, spec.total, rank, world, group) if keep_table else None
    if acc is None:
        return table
    return table, _fit.combine(acc, world, group, local=local, start=start)


def coherent_P(spec: SweepSpec, s: int, n: int, engine):
    """Coherent conversion probability of grid points [s, s+n) through their crossings
    (spec.crossings; lzq_lz_propagate), a device tensor."""
    m, dp, xi, v_w = spec.crossing_arrays(s, n, engine.device)
    vw = float(v_w[0]) if bool((v_w == v_w[0]).all()) else v_w   # a v_w axis: per-point wall speeds
    return engine.lz_propagate(m, dp, xi, vw, spec.crossings.window_lz, spec.crossings.steps)


def profile_P(spec: SweepSpec, s: int, n: int, engine, cache: dict):
    """P of grid points [s, s+n) from the spec's bounce profile (ProfileSpec; PAPER eqs.(5)-(9)):
    the profile's splines once per sweep (cache), then per point the crossings and eq.(9) and/or
    the time-ordered propagation through the profile, all on the GPU; a device tensor."""
    import torch
    ps = spec.profile
    if "shape" not in cache:
        cache["shape"] = engine.profile_shapes(*ps.arrays())
    sh = cache["shape"]
    vals = spec.axis_values(s, n, engine.device)
    full = lambda k, d: vals[k] if k in vals else torch.full((n,), float(d), dtype=torch.float64, device=engine.device)
    cols = [full("y_B", ps.y_B), full("y_chi", ps.y_chi), full("lambda_tr_eff", ps.lambda_tr_eff),
            full("v_w", spec.base["v_w"])]
    rec = torch.zeros((n, 5), dtype=torch.float64, device=engine.device)
    for j, c in enumerate(cols):
        rec[:, j] = c
    pts = rec.view(torch.uint8)[:, :40].contiguous().view(-1)   # lzq_profile_point rows (shape 0, reserved 0)
    if ps.estimator == "propagate":
        return engine.lz_propagate_profile(sh, pts, ps.steps_per_radian, ps.min_steps)
    cr = engine.profile_crossings(sh, pts, 1)
    one = cr["count"] == 1
    # delta_lz[:, 0] is written only where a crossing was found: mask the rest before eq.(9)
    delta = torch.where(one, cr["delta_lz"][:, 0], torch.zeros_like(cols[0]))
    P = torch.where(one, engine.p_closed_form(delta), torch.full_like(cols[0], float("nan")))
    many = cr["count"] > 1
    if ps.estimator == "auto" and bool(many.any()):
        sel = torch.nonzero(many).reshape(-1)
        P[sel] = engine.lz_propagate_profile(sh, pts.view(n, 40)[sel].contiguous().view(-1), ps.steps_per_radian,
                                             ps.min_steps)
    return P


def window_axes_collide(spec: SweepSpec) -> bool:
    """Do two of the spec's axes write the same field of the window block (a repeated axis, or
    window_sigma next to window_sigma_lo / _hi)?  The grid entry points refuse such a list
    (include/lzq.h); make_compute then keeps the host-record path."""
    seen = set()
    for name, _ in spec.axes:
        for f in WINDOW_AXES.get(name, ()):
            if f in seen:
                return True
            seen.add(f)
    return False


def grid_axes_for_kernel(spec: SweepSpec):
    """The spec's axes for lzq_sweep_grid: a profile coupling axis has no lzq_point field, so it
    rides on P_chi_to_B, which the per-point P override replaces (the flat-index decode of the
    other axes is unchanged)."""
    return [("P_chi_to_B" if n in PROFILE_FIELDS else n, v) for n, v in spec.axes]


def make_compute(spec: SweepSpec, engine, reuse: bool = False, window_host_records: bool = False) -> ComputeFn:
    """(start, count, out) -> None on the GPU: [coherent multi-crossing P ->] quadrature, or
    the ODE fallback (lzq_ode_batch) for sweeps over sigma_v / Gamma_wash / depletion (with or
    without crossings).  reuse: the quadrature's z-sums shared across points with the same
    y-grid and A/V kernel (lzq_sweep_grid_reuse; bit-identical, not the dense headline path).
    window_host_records: a window spec through explicit host-built records even where the grid
    entry points would take it (the same bits; tools/bench_window.py's baseline)."""
    pcache = {}   # the profile's device splines, built once per sweep
    check_wash_spec(spec)
    check_z_rule(spec)
    check_window_spec(spec)
    check_solve_spec(spec)
    check_fk_spec(spec)
    if spec.fk is not None:
        # explicit host records (the device does not decode fk axes): each chunk's points, blocks and
        # delta_0, through Engine.yields(fk=) -- shared z-sum tables, the R tables of the chunk's classes
        d_tables = engine.window_tables_to_device(spec.window.host_tables()) if spec.window is not None else None

        def compute_fk(s, n, out):
            pts, _ = grid_records(spec, s, n, engine)
            fks, delta = fk_records(spec, s, n, pts)
            out.copy_(engine.yields(pts, n_y=spec.n_y, nz=spec.nz, z_max=spec.z_max, continuum=spec.continuum,
                                    fk=fks, fk_delta=delta,
                                    window=None if spec.window is None else window_records(spec, s, n),
                                    window_tables=d_tables))
            engine.last_reuse = engine.last_yields_path
        return compute_fk
    if uses_wash(spec):
        # wash-out / depletion on the y-grid (Engine.sweep(wash=)): always from the shared z-sum tables; the
        # Gamma and depletion axes ride in the axis list and are decoded in the kernel, like the window's;
        # with a solve the records at the solutions go to `out` and the results ride back on the function
        d_tables = engine.window_tables_to_device(spec.window.host_tables()) if spec.window is not None else None

        def compute_wash(s, n, out):
            P_points = coherent_P(spec, s, n, engine) if spec.crossings is not None else None
            if spec.profile is not None:
                P_points = profile_P(spec, s, n, engine, pcache)
            res = engine.sweep(spec.base, grid_axes_for_kernel(spec), s, n, n_y=spec.n_y, out=out, P_points=P_points,
                               nz=spec.nz, z_max=spec.z_max, window=None if spec.window is None else spec.window.block,
                               window_tables=d_tables, solve=spec.solve, continuum=spec.continuum,
                               wash=wash_block(spec))
            if spec.solve is not None:
                compute_wash.solve_last = res[1]
        if spec.solve is not None:
            compute_wash.solve = _solve.normalize(spec.solve)
            compute_wash.solve_last = compute_wash.solve_local = None
        return compute_wash
    if spec.solve is not None:
        # the inverse sweep: always from the shared z-sum tables (Engine.sweep(solve=)); the records at
        # the solutions go to `out`, the results ride back on the function (run_local collects them)
        d_tables = engine.window_tables_to_device(spec.window.host_tables()) if spec.window is not None else None

        def compute_solve(s, n, out):
            P_points = coherent_P(spec, s, n, engine) if spec.crossings is not None else None
            if spec.profile is not None:
                P_points = profile_P(spec, s, n, engine, pcache)
            _, compute_solve.solve_last = engine.sweep(
                spec.base, grid_axes_for_kernel(spec), s, n, n_y=spec.n_y, out=out, P_points=P_points, nz=spec.nz,
                z_max=spec.z_max, window=None if spec.window is None else spec.window.block, window_tables=d_tables,
                solve=spec.solve, continuum=spec.continuum)
        compute_solve.solve = _solve.normalize(spec.solve)
        compute_solve.solve_last = compute_solve.solve_local = None
        return compute_solve
    if spec.window is not None:
        d_tables = engine.window_tables_to_device(spec.window.host_tables())
        grid_regime = int(to_point(spec.base)["regime"][0]) in (_native.THERMAL, _native.NONTHERMAL)
        # (the grid entry points refuse a base of another regime, whose rows are NaN from records)
        if not window_axes_collide(spec) and grid_regime and not window_host_records:
            # the grid entry points: the window axes ride in the axis list and each point's block is
            # decoded from the flat index in the kernel, like its other fields (Engine.sweep(window=))
            def compute_window_grid(s, n, out):
                P_points = coherent_P(spec, s, n, engine) if spec.crossings is not None else None
                if spec.profile is not None:
                    P_points = profile_P(spec, s, n, engine, pcache)   # the per-point override
                engine.sweep(spec.base, grid_axes_for_kernel(spec), s, n, n_y=spec.n_y, out=out, P_points=P_points,
                             reuse=reuse, nz=spec.nz, z_max=spec.z_max, window=spec.window.block,
                             window_tables=d_tables, continuum=spec.continuum)
            return compute_window_grid

        # two axes write one field of the block (the entry points refuse that): explicit point
        # records, as the ODE specs', each with its window block (window_records resolves the
        # collision: the earlier axis wins); with reuse the z-sums (which no window enters) are shared by
        # the points equal in _native.ZSUM_KEY
        def compute_window(s, n, out):
            pts, _ = grid_records(spec, s, n, engine)
            P_points = coherent_P(spec, s, n, engine) if spec.crossings is not None else None
            if spec.profile is not None:
                P_points = profile_P(spec, s, n, engine, pcache)   # the per-point override
            out.copy_(engine.yields(pts, n_y=spec.n_y, P=P_points, reuse=reuse, nz=spec.nz, z_max=spec.z_max,
                                    window=window_records(spec, s, n), window_tables=d_tables,
                                    continuum=spec.continuum))
            engine.last_reuse = engine.last_yields_path
        return compute_window
    if is_ode_spec(spec):
        counts = np.zeros(8, dtype=np.int64)   # ODE points per lzq_ode_status, this rank (all chunks)
        tables = {"points": 0, "tables": 0, "per_point_chunks": 0, "chunks": 0}   # this run's chunks

        def compute_ode(s, n, out):
            import torch
            pts, ods = grid_records(spec, s, n, engine)
            if spec.crossings is not None:   # coherent multi-crossing P (propagator) for every point
                pts["P_chi_to_B"] = coherent_P(spec, s, n, engine).cpu().numpy()
            if spec.profile is not None:     # P from the bounce profile
                pts["P_chi_to_B"] = profile_P(spec, s, n, engine, pcache).cpu().numpy()
            # fpy:372 per point: points with no sink/depletion take the quadrature, the rest the ODE
            ode = (ods["sigma_v_chi_GeV_m2"] != 0.0) | (ods["Gamma_wash_over_H"] != 0.0) | \
                  (ods["deplete_DM_from_source"] != 0)
            sel = np.nonzero(ode)[0]
            if sel.size:
                # (a chunk with a single ODE point integrates it parallel in time: the same bits)
                tab, status = engine.ode(pts[sel], ods[sel], method=spec.ode_method, max_steps=spec.ode_max_steps,
                                         nz=spec.nz, z_max=spec.z_max)
                for k in tables:
                    tables[k] += engine.last_ode_tables[k]
                # a point the integrator did not finish normally (a Radau Newton failure reports the
                # state where it stopped, as fpy:408-410 does for the CLI) is a NaN row in a sweep
                # table, counted per status in the summary ("ode_status")
                bad = status != 0
                tab = torch.where(bad[:, None], torch.full_like(tab, float("nan")), tab)
                chunk = np.bincount(status.clamp(0, 7).cpu().numpy(), minlength=8)[:8]
                counts[:] += chunk
                compute_ode.last_chunk = chunk.astype(np.int64)   # written beside the chunk's checkpoint
                out[torch.as_tensor(sel, device=out.device)] = tab
            else:
                compute_ode.last_chunk = np.zeros(8, dtype=np.int64)
            sel = np.nonzero(~ode)[0]
            if sel.size:
                out[torch.as_tensor(sel, device=out.device)] = engine.yields(pts[sel], n_y=spec.n_y, reuse=reuse,
                                                                             nz=spec.nz, z_max=spec.z_max)
        compute_ode.ode_status = counts
        compute_ode.ode_tables = tables
        compute_ode.last_chunk = np.zeros(8, dtype=np.int64)
        return compute_ode

    def compute(s, n, out):
        P_points = coherent_P(spec, s, n, engine) if spec.crossings is not None else None
        if spec.profile is not None:
            P_points = profile_P(spec, s, n, engine, pcache)
        engine.sweep(spec.base, grid_axes_for_kernel(spec), s, n, n_y=spec.n_y, out=out, P_points=P_points,
                     reuse=reuse, nz=spec.nz, z_max=spec.z_max, continuum=spec.continuum)
    return compute


def main(argv=None):
    import torch
    import torch.distributed as dist
    ap = argparse.ArgumentParser(description="lzq parameter sweep (1..8 GPUs, RCCL all-gather)")
    ap.add_argument("--spec", required=True, help="C2 | C3 | C4 | C5 | P1 | path to a sweep-spec JSON")
    ap.add_argument("--out", default=None, help="directory for shard checkpoints, table.npy, summary.json")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--limit", type=int, default=None, help="evaluate only the first N grid points")
    ap.add_argument("--reuse-zsums", action="store_true",
                    help="share the quadrature's z-sums between points with the same y-grid and A/V kernel "
                         "(lzq_sweep_grid_reuse: bit-identical, much faster; not the dense headline mode)")
    ap.add_argument("--nz", type=int, default=None, help="z nodes of the A/V kernel (AoverVKernel nz, fpy:142)")
    ap.add_argument("--z-max", type=float, default=None, help="z_max of the A/V kernel (fpy:142)")
    ap.add_argument("--continuum", action="store_true",
                    help="the A/V z-sum as a converged z-integral on the continuum z rule of z_max in place of the "
                         "(nz, z_max) grid (a spec file's \"z_rule\": \"continuum\"); always through shared z-sum tables")
    ap.add_argument("--wash-quadrature", action="store_true",
                    help="Gamma_wash_over_H / deplete_DM_from_source points (sigma_v = 0 everywhere) on the y-grid "
                         "quadrature in place of the ODE fallback (a spec file's \"wash_rule\": \"quadrature\"): "
                         "window, --solve (Gamma_wash_over_H:LO:HI too), --reuse-zsums and --continuum then apply")
    ap.add_argument("--ode-max-steps", type=int, default=None,
                    help=f"cap on one ODE point's Radau steps (default {ODE_MAX_STEPS}; 0 = no cap)")
    ap.add_argument("--dist-backend", default="nccl",
                    help="nccl (= RCCL over xGMI, default) | gloo (rehearsal: several ranks on one GPU)")
    ap.add_argument("--fit", default=None, metavar="FILE|paper",
                    help="fit the yields to targets on the device, chunk by chunk: a fit-spec JSON (terms, levels, "
                         "maps, select, posterior, observables, ranked; see fit.py), or `paper`: Y_B = 8.72e-11 and DM_over_B = 5.357, "
                         "each with sigma at 1%% of its target (nominal tolerances, not measurement errors).  Writes "
                         "fit.json, fit_maps.npz, selected.npy, with \"observables\" (histograms over yield fields) "
                         "fit_obs.npz, with \"ranked\" (the n best points with their records) fit_ranked.npz, and a "
                         "\"fit\" block in summary.json")
    ap.add_argument("--solve", default=None, metavar="FIELD:LO:HI[:TARGETFIELD=VALUE]",
                    help="the inverse sweep: for every grid point solve FIELD in [LO, HI] for a target yield "
                         "(default DM_over_B=5.357), e.g. --spec C3 --solve source_shape_sigma_y:1:50; table.npy then "
                         "holds the records at the solutions, solve.npy (x, x_lo, x_hi, residual, evals, status) the "
                         "results, and summary.json a \"solve\" block (with --no-table only the block).  Replaces a spec file's "
                         "\"solve\" section")
    ap.add_argument("--no-table", action="store_true",
                    help="with --fit: keep only the fit -- chunks pass through two chunk-sized buffers, there is "
                         "no all-gather, no table.npy and no checkpoint (a grid larger than HBM or the disk)")
    args = ap.parse_args(argv)
    if args.no_table and args.fit is None:
        ap.error("--no-table needs --fit (nothing else would be kept)")
    if args.no_table and args.resume:
        ap.error("--no-table --resume: a fit-only run writes no checkpoints to resume from")

    specs = builtin_specs()
    if args.spec in specs:
        spec = specs[args.spec]
    else:
        with open(args.spec) as f:
            spec = spec_from_json(json.load(f))
    if args.nz is not None or args.z_max is not None:
        spec.nz, spec.z_max = _native.zgrid(spec.nz if args.nz is None else args.nz,
                                            spec.z_max if args.z_max is None else args.z_max)
    if args.wash_quadrature:
        spec.wash_rule = "quadrature"
    if args.continuum:
        spec.z_rule = "continuum"
    if args.solve is not None:
        spec.solve = _solve.parse_cli(args.solve)
    check_wash_spec(spec)
    check_z_rule(spec)
    if args.ode_max_steps is not None:
        spec.ode_max_steps = None if args.ode_max_steps == 0 else args.ode_max_steps
    if spec.solve is not None:
        check_solve_spec(spec)
    fitspec = fit_maps = None
    if args.fit is not None:
        from . import fit as _fit
        fitspec = _fit.load(args.fit)
        fit_maps = fitspec.resolve(spec)
        if args.no_table and fitspec.posterior is not None and fitspec.posterior["offset"] == "best":
            ap.error("--no-table: " + _fit.NO_TABLE_BEST)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    local_rank %= max(1, torch.cuda.device_count())  # gloo rehearsal: several ranks may share a GPU
    torch.cuda.set_device(local_rank)
    use_dist = launched_distributed(world)
    if use_dist:
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.dist_backend)
    spec_total = spec.total if args.limit is None else min(args.limit, spec.total)

    from .engine import Engine
    eng = Engine(local_rank)
    t0 = time.perf_counter()
    start, end = shard_range(spec_total, rank, world)
    key = prepare_out_dir(args.out, spec, args.resume, rank) if args.out else ""

    compute = make_compute(spec, eng, reuse=args.reuse_zsums)
    make_out = lambda n: torch.empty((n, 6), dtype=torch.float64, device=eng.device)
    acc = _fit.make_accumulator(fitspec, fit_maps, eng, fitspec.axis_values(spec)) if fitspec is not None else None
    local = run_local(compute, start, end, make_out, args.chunk,
                      args.out, args.resume, sync=torch.cuda.synchronize,
                      log=(print if rank == 0 else (lambda s: None)), key=key, fit=acc,
                      keep_table=not args.no_table)
    ode_status = ode_status_summary(getattr(compute, "ode_status", None), None, eng.device)
    table = None if args.no_table else gather_table(local, spec_total, rank, world)
    solved = gather_table(compute.solve_local, spec_total, rank, world) \
        if spec.solve is not None and not args.no_table else None
    # --no-table: no solve.npy either; the summary block from the x column and integer counts
    solve_block = solve_summary_streamed(compute, spec_total, rank, world) \
        if spec.solve is not None and args.no_table else None
    fit_result = _fit.combine(acc, world, local=local, start=start) if acc is not None else None
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if rank == 0:
        if table is not None:
            tab = table.cpu().numpy()
            summ = summarize(tab, spec, elapsed)
        else:   # fit only: the column extrema the fit kept stand in for summarize's statistics
            summ = {"spec": spec.name, "n_points": int(spec_total), "fields": list(YIELD_FIELDS),
                    "final": fit_result["columns"], "elapsed_s": elapsed}
        summ["points_per_s"] = spec_total / elapsed
        summ["n_gpus"] = world
        if ode_status is not None:
            summ["ode_status"] = ode_status   # ODE-path points per status (non-ok rows are NaN)
            t = getattr(compute, "ode_tables", None)
            if t is not None:   # rank 0's chunks computed by this run: shared A/V spline tables or one per point
                summ["ode_tables"] = dict(t, mode="shared" if t["per_point_chunks"] == 0 else (
                    "per_point" if t["per_point_chunks"] == t["chunks"] else "mixed"))
        if args.reuse_zsums:
            summ["reuse_zsums"] = eng.last_reuse
        if solve_block is not None:
            summ["solve"] = solve_block
        if solved is not None:
            sol = solved.cpu().numpy()
            summ["solve"] = _solve.summary(spec.solve, sol)
            if args.out:
                np.save(os.path.join(args.out, "solve.npy"), sol, allow_pickle=False)
        if fit_result is not None:
            best = fit_result["best"]["index"]
            fit_rep = _fit.report(fitspec, fit_result, spec, spec_total,
                                  _fit.best_point_yields(compute, best, make_out, eng))
            summ["fit"] = fit_rep
            if args.out:
                _fit.write_files(args.out, fit_rep, fit_result)
        if args.out:
            if table is not None:
                np.save(os.path.join(args.out, "table.npy"), tab, allow_pickle=False)
            with open(os.path.join(args.out, "summary.json"), "w") as f:
                json.dump({**summ, "spec_def": spec.to_json()}, f, indent=2)
        print(json.dumps({k: summ[k] for k in ("spec", "n_points", "points_per_s", "n_gpus", "elapsed_s")}))
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
