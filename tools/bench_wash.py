#!/usr/bin/env python3
"""Cost of wash-out and depletion on the y-grid quadrature (lzq_sweep_grid_from_ztables_wash) on one
MI355X, in one process.

Workload: a 2^20-point grid over the C2 axes (m_mix x dprime, 256 log-spaced values each over C2's ranges,
C2's base and n_y) times 16 values of Gamma_wash_over_H in [0, 4], depletion on, the points' window a
Gaussian block.  Every leg has an engine, and so a z-sum workspace, of its own: the grid's table is built
once, in the warm-up, and a timed run is the integrating call alone (as the parent leg's is).  The legs
alternate, `runs` runs each after the warm-up, HIP events on the launch stream:

1. wash     lzq_sweep_grid_from_ztables_wash on the whole grid.
2. window   lzq_sweep_grid_from_ztables_window on the same points: the third axis is a window axis the
            Gaussian kind does not read, so the two kernels integrate the same 2^20 points.
3. parent   (--parent-lib) leg 2 through another build of the library, loaded next to this one: an
            unchanged code object must sit within the run spread.
4. ode      Engine.ode(method="quadrature") beside Engine.yields(wash=) on a narrow-window subset
            (T in [0.6, 1.6] T_p, 4096 points): the two forms of the same linear system.

    python tools/bench_wash.py [--runs 5] [--parent-lib PATH] [--json profiles/wash/bench_wash.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "baryon-and-dark-matter-densities-from-bounce--sourced-distributed-landau--zener-transport_amd"
N_AXIS, N_GAMMA, N_ODE = 256, 16, 4096
WINDOW = {"kind": "gauss", "sigma": 9.0}
DEP = {"deplete_DM_from_source": True}


def git_head(root):
    try:
        return subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        return ""


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "runs": len(ts),
            "spread": (max(ts) - min(ts)) / statistics.median(ts)}


def event_ms(fn):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def parent_leg(path, nat, base, win, arr, n_axes, total, n_y, out, stream):
    """lzq_sweep_grid_ztables_window + lzq_sweep_grid_from_ztables_window of another build, bound by hand
    (an older build has no *_wash symbols for _native.load to bind)."""
    L = ctypes.CDLL(path)
    i32, i64, d, vp, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.POINTER
    L.lzq_init.argtypes = [ctypes.c_int]
    L.lzq_sweep_grid_reuse_workspace.argtypes = [P(nat.LzqAxis), i32, i32]
    L.lzq_sweep_grid_reuse_workspace.restype = i64
    L.lzq_sweep_grid_ztables_window.argtypes = [P(nat.LzqPoint), P(nat.LzqAxis), i32, i32, i32, d, vp, i64, vp]
    L.lzq_sweep_grid_from_ztables_window.argtypes = [P(nat.LzqPoint), P(nat.LzqWindow), P(nat.LzqAxis), i32, i64, i64,
                                                     i32, i32, d, vp, vp, i64, P(nat.LzqWindowTables), vp, vp]
    assert L.lzq_init(0) == 0
    need = L.lzq_sweep_grid_reuse_workspace(arr, n_axes, n_y)
    work = torch.empty(need, dtype=torch.float64, device=out.device)
    assert L.lzq_sweep_grid_ztables_window(ctypes.byref(base), arr, n_axes, n_y, nat.LZQ_NZ, nat.LZQ_Z_MAX,
                                           work.data_ptr(), need, stream()) == 0

    def run():
        rc = L.lzq_sweep_grid_from_ztables_window(ctypes.byref(base), ctypes.byref(win), arr, n_axes, 0, total, n_y,
                                                  nat.LZQ_NZ, nat.LZQ_Z_MAX, None, work.data_ptr(), need, None,
                                                  out.data_ptr(), stream())
        assert rc == 0
    run.keep = work
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "wash", "bench_wash.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("at least five runs each")
    S, E, W = (importlib.import_module(PKG + m) for m in (".sweep", ".engine", ".window"))
    nat, cfgm = importlib.import_module(PKG + "._native"), importlib.import_module(PKG + ".config")
    eng, eng_win, eng_pts = E.Engine(0), E.Engine(0), E.Engine(0)   # one z-sum workspace per leg
    c2 = S.builtin_specs()["C2"]
    lz = [(n, np.logspace(np.log10(v[0]), np.log10(v[-1]), N_AXIS)) for n, v in c2.axes]
    gam = ("Gamma_wash_over_H", np.linspace(0.0, 4.0, N_GAMMA))
    idle = ("window_scale", np.ones(N_GAMMA))     # the Gaussian kind does not read it
    total = N_AXIS * N_AXIS * N_GAMMA
    out = torch.empty((total, 6), dtype=torch.float64, device=eng.device)
    out2 = torch.empty_like(out)

    def wash():
        eng.sweep(c2.base, lz + [gam], 0, total, n_y=c2.n_y, out=out, window=WINDOW, wash=DEP)

    def window():
        eng_win.sweep(c2.base, lz + [idle], 0, total, n_y=c2.n_y, out=out2, reuse=True, window=WINDOW)

    legs = {"wash": wash, "window": window}
    if args.parent_lib:
        vals = [torch.as_tensor(np.asarray(v, dtype=np.float64), device=eng.device) for _, v in lz + [idle]]
        arr = (nat.LzqAxis * 3)()
        for a, ((n, _), t) in enumerate(zip(lz + [idle], vals)):
            arr[a].field = nat.FIELD.get(n, nat.WINDOW_FIELD.get(n))
            arr[a].n, arr[a].values = t.numel(), t.data_ptr()
        base = cfgm.to_ctypes_point(cfgm.to_point(c2.base))
        win = nat.LzqWindow.from_buffer_copy(W.to_window(WINDOW).tobytes())
        out3 = torch.empty_like(out)
        legs["parent"] = parent_leg(args.parent_lib, nat, base, win, arr, 3, total, c2.n_y, out3, eng._stream)
        legs["parent"].vals = vals
    # the narrow-window subset: both forms of the linear system on the same 4096 points
    narrow = dict(c2.base, T_max_over_Tp=1.6, T_min_over_Tp=0.6, deplete_DM_from_source=True)
    pts = np.repeat(cfgm.to_point(narrow), N_ODE)
    pts["P_chi_to_B"] = np.linspace(0.01, 0.9, N_ODE)
    ods = np.repeat(importlib.import_module(PKG + ".wash").to_wash(DEP), N_ODE)
    ods["Gamma_wash_over_H"] = np.tile(np.linspace(0.25, 4.0, 16), N_ODE // 16)
    keep = {}

    def ode_quadrature():
        keep["ode"] = eng_pts.ode(pts, ods, method="quadrature")

    def wash_points():
        keep["wash"] = eng_pts.yields(pts, wash=ods, n_y=c2.n_y)

    legs["ode_quadrature"], legs["wash_points"] = ode_quadrature, wash_points
    for fn in legs.values():     # warm-up: every grid's table is built here
        fn()
    torch.cuda.synchronize()
    keys = (eng._ztab_key, eng_win._ztab_key)
    assert None not in keys
    t = {k: [] for k in legs}
    for _ in range(args.runs):   # alternating
        for k, fn in legs.items():
            t[k].append(event_ms(fn))
    assert keys == (eng._ztab_key, eng_win._ztab_key)   # no timed run rebuilt a table
    ms = {k: stats(v) for k, v in t.items()}
    a, b = out.cpu().numpy(), out2.cpu().numpy()
    tab, status = keep["ode"]
    o, w = tab.cpu().numpy(), keep["wash"].cpu().numpy()
    okr = status.cpu().numpy() == 0
    res = {
        "tool": "tools/bench_wash.py", "git_head": git_head(ROOT), "device": torch.cuda.get_device_name(0),
        "grid": {"axes": [[n, len(v), float(v[0]), float(v[-1])] for n, v in lz + [gam]], "points": total,
                 "n_y": c2.n_y, "window": WINDOW, "wash": DEP},
        "ms": ms,
        "wash": {"kernel": "grid_reuse_wash_kernel", "points_per_s": total / (ms["wash"]["median"] * 1e-3)},
        "window": {"kernel": "grid_reuse_window_kernel", "points_per_s": total / (ms["window"]["median"] * 1e-3)},
        "ratio_wash_to_window": ms["wash"]["median"] / ms["window"]["median"],
        "gamma0_rows_equal_window_Y_B": bool(np.array_equal(a.reshape(-1, N_GAMMA, 6)[:, 0, 0], b.reshape(-1, N_GAMMA, 6)[:, 0, 0])),
        "narrow_subset": {"points": N_ODE, "T_window": [0.6, 1.6], "ode_status_ok": int(okr.sum()),
                          "ode_quadrature_points_per_s": N_ODE / (ms["ode_quadrature"]["median"] * 1e-3),
                          "wash_points_per_s": N_ODE / (ms["wash_points"]["median"] * 1e-3),
                          "worst_relative_distance_Y_B": float(np.max(np.abs(o[okr, 0] / w[okr, 0] - 1.0))) if okr.any() else None,
                          "note": "wash_points rebuilds its one z-sum table per call; the distance is between the "
                                  "800-knot spline in T and the y-grid, not an error of either"},
    }
    if args.parent_lib:
        res["parent"] = {"library": os.path.basename(args.parent_lib),
                         "ratio_to_this_build": ms["parent"]["median"] / ms["window"]["median"],
                         "within_spread": abs(ms["parent"]["median"] / ms["window"]["median"] - 1.0)
                         <= max(ms["parent"]["spread"], ms["window"]["spread"])}
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
