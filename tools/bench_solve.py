#!/usr/bin/env python3
"""Cost of the per-point root solve (lzq_sweep_grid_solve) on one MI355X, in one process.

Workload: a 2^20-point grid over the C2 axes (m_mix x dprime, 1024 log-spaced values each over C2's
ranges, C2's base and n_y) with a plateau window whose half-width is solved for DM_over_B = 5.357.
Three measurements alternate, `runs` runs each after a warm-up, HIP events on the launch stream:

1. solve    lzq_sweep_grid_solve on the whole grid (the z-sum table built before, once): solves/s, the
            evaluations (mean, max, total) and the time per evaluation.
2. forward  lzq_sweep_grid_from_ztables_window (grid_reuse_window_kernel) on the same grid with the
            half-width fixed: the time of one reuse-mode point, the baseline an evaluation is compared
            with (ratio = time per evaluation / time per forward point).
3. axis     what the same question costs without the solve: the grid with a 64-value
            window_half_width axis through the reuse-mode sweep (2^26 points, in chunks).

    python tools/bench_solve.py [--runs 5] [--json profiles/solve/bench_solve.json]
"""
import argparse
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
N_AXIS = 1024
WINDOW = {"kind": "plateau", "y0": -5.0, "half_width": 3.0, "sigma_lo": 4.0, "sigma_hi": 6.0}
SOLVE = {"field": "window_half_width", "lo": 0.0, "hi": 40.0, "target": {"field": "DM_over_B", "value": 5.357}}
AXIS_VALUES = 64
CHUNK = 1 << 22


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "solve", "bench_solve.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("at least five runs each")
    S = importlib.import_module(PKG + ".sweep")
    V = importlib.import_module(PKG + ".solve")
    E = importlib.import_module(PKG + ".engine")
    eng = E.Engine(0)
    c2 = S.builtin_specs()["C2"]
    axes = [(n, np.logspace(np.log10(v[0]), np.log10(v[-1]), N_AXIS)) for n, v in c2.axes]
    total = N_AXIS * N_AXIS
    hw_axis = ("window_half_width", np.linspace(SOLVE["lo"], SOLVE["hi"], AXIS_VALUES))
    out = torch.empty((total, 6), dtype=torch.float64, device=eng.device)
    big = torch.empty((CHUNK, 6), dtype=torch.float64, device=eng.device)
    keep = {}

    def solve():
        keep["rec"], keep["sol"] = eng.sweep(c2.base, axes, 0, total, n_y=c2.n_y, out=out, window=WINDOW, solve=SOLVE)

    def forward():
        eng.sweep(c2.base, axes, 0, total, n_y=c2.n_y, out=out, reuse=True, window=WINDOW)

    def axis():
        ax = axes + [hw_axis]
        for s in range(0, total * AXIS_VALUES, CHUNK):
            eng.sweep(c2.base, ax, s, CHUNK, n_y=c2.n_y, out=big, reuse=True, window=WINDOW)

    for fn in (solve, forward, axis):     # warm-up (the tables of both grids are built here or per switch)
        fn()
    torch.cuda.synchronize()
    t = {"solve": [], "forward": [], "axis": []}
    for _ in range(args.runs):            # alternating
        t["solve"].append(event_ms(solve))
        t["forward"].append(event_ms(forward))
        t["axis"].append(event_ms(axis))
    sol = keep["sol"].cpu().numpy()
    evals = sol[:, 4]
    summ = V.summary(SOLVE, sol)
    ms = {k: stats(v) for k, v in t.items()}
    per_eval_ns = ms["solve"]["median"] * 1e6 / float(evals.sum())
    per_point_ns = ms["forward"]["median"] * 1e6 / total
    res = {
        "tool": "tools/bench_solve.py", "git_head": git_head(ROOT), "device": torch.cuda.get_device_name(0),
        "grid": {"axes": [[n, len(v), float(v[0]), float(v[-1])] for n, v in axes], "points": total, "n_y": c2.n_y,
                 "window": WINDOW, "solve": V.normalize(SOLVE)},
        "ms": ms,
        "solve": {"solves_per_s": total / (ms["solve"]["median"] * 1e-3), "status": summ["status"], "x": summ["x"],
                  "evals_mean": float(evals.mean()), "evals_max": int(evals.max()), "evals_total": int(evals.sum()),
                  "evals_mean_of_solved": float(evals[sol[:, 5] <= 1].mean()) if np.any(sol[:, 5] <= 1) else None,
                  "ns_per_evaluation": per_eval_ns},
        "forward": {"kernel": "grid_reuse_window_kernel", "points_per_s": total / (ms["forward"]["median"] * 1e-3),
                    "ns_per_point": per_point_ns},
        "ratio_evaluation_to_forward_point": per_eval_ns / per_point_ns,
        "axis": {"values": AXIS_VALUES, "points": total * AXIS_VALUES,
                 "points_per_s": total * AXIS_VALUES / (ms["axis"]["median"] * 1e-3),
                 "time_over_solve": ms["axis"]["median"] / ms["solve"]["median"]},
        "note": "the runs alternate solve, forward, axis: the axis grid has its own z-sum table, so every axis run and "
                "every solve run after one rebuilds its grid's table (one table, one dense point) inside its "
                "time; forward finds the solve's table built",
    }
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
