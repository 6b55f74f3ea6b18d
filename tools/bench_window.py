#!/usr/bin/env python3
"""Cost of the source activity window (include/lzq.h lzq_window) on one MI355X.

1. dense   lzq_yields_batch_window with a GAUSS block per point against lzq_yields_batch on the
           same 1e5 points (the first rows of the C2 grid as explicit records, n_y = 8000, device
           resident), the two alternating in one process, `runs` runs each after a warm-up, HIP
           events on the launch stream.  The window adds per-y work only (tens of VALU against
           ~1200 x 6.6 per y-node), so the two are expected to agree within the run spread.  The
           results are compared bit for bit (a GAUSS block with the point's sigma_y is the headline).
2. sweep   points/s of a reuse-mode sweep over window axes (window_y0 x window_sigma x delta_LZ,
           through sweep.make_compute: explicit records built on the host, uploaded, integrated from
           shared z-sum tables), host record building included, beside the same-size
           source_shape_sigma_y x delta_LZ sweep through lzq_sweep_grid_reuse (points generated on
           the device).  A host clock around work that ends in a device synchronise; the window
           sweep's time is also split into host records, and upload + launches.

    python tools/bench_window.py [--runs 5] [--json profiles/window/bench_window.json]
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
DENSE_POINTS = 100_000
SWEEP_SHAPE = (200, 200, 250)   # 1e7 points: about a second per timed sweep
CHUNK = 1 << 18


def git_head(root):
    try:
        return subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        return ""


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "runs": len(ts)}


def event_ms(fn):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    out = fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def bench_dense(eng, sw, N, W, runs):
    spec = sw.builtin_specs()["C2"]
    pts, _ = sw.grid_records(spec, 0, DENSE_POINTS, eng)
    d_pts = eng.points_to_device(pts)
    d_none = eng.window_tables_to_device(None)
    d_win = eng.window_to_device(W.to_window({"kind": "gauss", "sigma_hi": float(spec.base["source_shape_sigma_y"])}),
                                 DENSE_POINTS, d_none)
    plain = lambda: eng.yields(d_pts, n_y=spec.n_y)
    window = lambda: eng.yields(d_pts, n_y=spec.n_y, window=d_win, window_tables=d_none)
    a, b = plain(), window()   # warm-up: code objects loaded, tables uploaded
    torch.cuda.synchronize()
    same = torch.equal(a.view(torch.int64), b.view(torch.int64))
    tp, tw = [], []
    for _ in range(runs):      # alternating
        tp.append(event_ms(plain)[0])
        tw.append(event_ms(window)[0])
    mp, mw = statistics.median(tp), statistics.median(tw)
    return {"points": DENSE_POINTS, "n_y": spec.n_y, "bit_identical": bool(same),
            "lzq_yields_batch_ms": stats(tp), "lzq_yields_batch_window_ms": stats(tw),
            "window_over_plain": mw / mp, "spread_plain": (max(tp) - min(tp)) / mp,
            "spread_window": (max(tw) - min(tw)) / mw,
            "points_per_s": {"plain": DENSE_POINTS / mp * 1e3, "window": DENSE_POINTS / mw * 1e3}}


def bench_sweep(eng, sw, runs):
    a, b, c = SWEEP_SHAPE
    total = a * b * c
    base = dict(sw.EQUAL_MASS)
    wspec = sw.SweepSpec("window_axes", base, [("window_y0", np.linspace(-10, 10, a)),
                                               ("window_sigma", np.linspace(3, 30, b)),
                                               ("delta_LZ", np.logspace(-4, 0, c))],
                         window=sw.WindowSpec({"kind": "plateau", "half_width": 2.0}))
    sspec = sw.SweepSpec("sigma_y_axis", base, [("source_shape_sigma_y", np.linspace(3, 30, a * b)),
                                                ("delta_LZ", np.logspace(-4, 0, c))])
    out = torch.empty((CHUNK, 6), dtype=torch.float64, device=eng.device)

    def run(spec):
        compute = sw.make_compute(spec, eng, reuse=True)
        t0 = time.perf_counter()
        for s in range(0, total, CHUNK):
            n = min(CHUNK, total - s)
            compute(s, n, out[:n])
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def host_records(spec):
        t0 = time.perf_counter()
        for s in range(0, total, CHUNK):
            n = min(CHUNK, total - s)
            sw.grid_records(spec, s, n, eng)
            sw.window_records(spec, s, n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    run(wspec), run(sspec)     # warm-up
    tw, ts, th = [], [], []
    for _ in range(runs):      # alternating
        ts.append(run(sspec))
        tw.append(run(wspec))
        th.append(host_records(wspec))
    mw, ms, mh = statistics.median(tw), statistics.median(ts), statistics.median(th)
    return {"points": total, "chunk": CHUNK, "n_y": wspec.n_y, "path": eng.last_yields_path,
            "window_axes_s": stats(tw), "sigma_y_axis_s": stats(ts), "window_host_records_s": stats(th),
            "points_per_s": {"window_axes": total / mw, "sigma_y_axis_device_grid": total / ms},
            "host_records_share_of_window_sweep": mh / mw}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--commit", default=None, help="the commit this tree was measured at (default: git HEAD)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sw = importlib.import_module(PKG + ".sweep")
    N = importlib.import_module(PKG + "._native")
    W = importlib.import_module(PKG + ".window")
    eng = importlib.import_module(PKG + ".engine").Engine()
    rec = {"what": "tools/bench_window.py", "commit": args.commit or git_head(ROOT),
           "device": torch.cuda.get_device_name(eng.device), "library": N.library_id()}
    rec["dense"] = bench_dense(eng, sw, N, W, args.runs)
    rec["sweep"] = bench_sweep(eng, sw, args.runs)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
