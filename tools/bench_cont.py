#!/usr/bin/env python3
"""Cost of the continuum z rule (include/lzq.h "A/V in the continuum limit") on one MI355X.

a. tables  the z-sum tables of the C4 grid (1000 tables x 8000 y-nodes) by three builds, alternating
           in one process, `runs` runs each after a warm-up, HIP events on the launch stream: the
           live-range kernel (lzq_sweep_grid_ztables_cont, LZQ_TUNE_CONT_SKIP = 1), the every-node
           form (the same entry point with LZQ_TUNE_CONT_SKIP = 0: the linspace grids' table kernel on
           the continuum node table, one wavefront per table), and lzq_sweep_grid_ztables on the
           reference grid (1200, 30).  The two continuum builds are compared bit for bit.
b. sweep   points/s of the C4 reuse-mode integration from tables already built (the first 2^22
           points), continuum against linspace: the same integration kernel reads either table, so the
           expectation is parity.
c. yields  Engine.yields(continuum=True) on 65,536 explicit points with all-distinct I_p (a table per
           point, grouped and chunked by the engine), points/s on a host clock around work that ends
           in a device synchronise.

Adoption rule: the live-range kernel is the default only if (a) beats the every-node
form by more than the run-to-run spread.

    python tools/bench_cont.py [--runs 5] [--json profiles/cont/bench_cont.json]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "baryon-and-dark-matter-densities-from-bounce--sourced-distributed-landau--zener-transport_amd"
SWEEP_POINTS = 1 << 22
YIELD_POINTS = 65536
TABLES = 1000   # the C4 grid's z-sum tables


def git_head(root):
    try:
        return subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        return ""


def stats(ts):
    m = statistics.median(ts)
    return {"median": m, "min": min(ts), "max": max(ts), "runs": len(ts), "spread": (max(ts) - min(ts)) / m}


def event_ms(fn):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    out = fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def bench_tables(eng, sw, runs):
    spec = sw.builtin_specs()["C4"]
    axes = sw.grid_axes_for_kernel(spec)

    def build(cont, skip):
        # a fresh key per call: Engine.sweep rebuilds the tables; as many points as tables are
        # integrated from them, below which the linspace sweep would not build tables at all
        eng.tune_cont_skip(skip)
        eng._ztab_key = None
        out = eng.sweep(spec.base, axes, 0, TABLES, n_y=spec.n_y, reuse=True, continuum=cont)
        assert eng.last_reuse == "tables"
        return out

    legs = {"live_range": (True, True), "every_node": (True, False), "linspace_1200": (False, True)}
    tabs = {}
    for name, (cont, skip) in legs.items():   # warm-up, and the tables for the comparison
        build(cont, skip)
        torch.cuda.synchronize()
        tabs[name] = eng._zwork.clone()
    n_tables = tabs["live_range"].numel() // (spec.n_y + 6)
    same = torch.equal(tabs["live_range"].view(torch.int64), tabs["every_node"].view(torch.int64))
    ts = {k: [] for k in legs}
    for _ in range(runs):                      # alternating
        for name, (cont, skip) in legs.items():
            ts[name].append(event_ms(lambda: build(cont, skip))[0])
    eng.tune_cont_skip(True)
    out = {"tables": int(n_tables), "n_y": spec.n_y, "bit_identical": bool(same),
           "note": "each time includes 1000 points integrated from the tables (one short launch)"}
    for k in legs:
        out[k + "_ms"] = stats(ts[k])
    m = {k: out[k + "_ms"]["median"] for k in legs}
    out["every_node_over_live_range"] = m["every_node"] / m["live_range"]
    out["linspace_over_live_range"] = m["linspace_1200"] / m["live_range"]
    out["spread"] = max(out[k + "_ms"]["spread"] for k in ("live_range", "every_node"))
    out["live_range_adopted"] = bool(same and m["every_node"] / m["live_range"] > 1.0 + out["spread"])
    return out


def bench_sweep(eng, sw, runs):
    spec = sw.builtin_specs()["C4"]
    axes = sw.grid_axes_for_kernel(spec)
    out = torch.empty((SWEEP_POINTS, 6), dtype=torch.float64, device=eng.device)
    res = {"points": SWEEP_POINTS, "n_y": spec.n_y}
    ts = {"continuum": [], "linspace": []}
    for _ in range(runs + 1):                  # the first round is the warm-up; each leg rebuilds its tables untimed
        for name, cont in (("continuum", True), ("linspace", False)):
            eng.sweep(spec.base, axes, 0, TABLES, n_y=spec.n_y, reuse=True, continuum=cont)
            torch.cuda.synchronize()
            t = event_ms(lambda: eng.sweep(spec.base, axes, 0, SWEEP_POINTS, n_y=spec.n_y, reuse=True, out=out,
                                           continuum=cont))[0]
            assert eng.last_reuse == "tables"
            ts[name].append(t)
    for k in ts:
        res[k + "_ms"] = stats(ts[k][1:])
        res[k + "_points_per_s"] = SWEEP_POINTS / res[k + "_ms"]["median"] * 1e3
    res["continuum_over_linspace"] = res["continuum_ms"]["median"] / res["linspace_ms"]["median"]
    return res


def bench_yields(eng, cfgm, sw, runs):
    base = sw.builtin_specs()["C4"].base
    pts = np.repeat(cfgm.to_point(base), YIELD_POINTS)
    pts["I_p"] = np.linspace(0.05, 1.0, YIELD_POINTS)
    d_pts = eng.points_to_device(pts)
    ts = []
    for _ in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.yields(d_pts, n_y=8000, continuum=True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    s = stats(ts[1:])
    return {"points": YIELD_POINTS, "n_y": 8000, "distinct_tables": YIELD_POINTS, "chunks": eng.last_cont_chunks,
            "ms": s, "points_per_s": YIELD_POINTS / s["median"] * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "cont", "bench_cont.json"))
    ap.add_argument("--legs", default="abc")
    args = ap.parse_args()
    E, sw, cfgm, N = (importlib.import_module(f"{PKG}.{m}") for m in ("engine", "sweep", "config", "_native"))
    eng = E.Engine()
    res = {"device": torch.cuda.get_device_name(eng.device), "git_head": git_head(ROOT), "library_id": N.library_id(),
           "runs": args.runs}
    if "a" in args.legs:
        res["tables"] = bench_tables(eng, sw, args.runs)
        print(json.dumps(res["tables"]), flush=True)
    if "b" in args.legs:
        res["sweep"] = bench_sweep(eng, sw, args.runs)
        print(json.dumps(res["sweep"]), flush=True)
    if "c" in args.legs:
        res["yields"] = bench_yields(eng, cfgm, sw, args.runs)
        print(json.dumps(res["yields"]), flush=True)
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.json)


if __name__ == "__main__":
    main()
