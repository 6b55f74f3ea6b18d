#!/usr/bin/env python3
"""Cost of the source activity window (include/lzq.h lzq_window) on one MI355X.

1. dense   lzq_yields_batch_window with a GAUSS block per point against lzq_yields_batch on the
           same 1e5 points (the first rows of the C2 grid as explicit records, n_y = 8000, device
           resident), the two alternating in one process, `runs` runs each after a warm-up, HIP
           events on the launch stream.  The window adds per-y work only (tens of VALU against
           ~1200 x 6.6 per y-node), so the two are expected to agree within the run spread.  The
           results are compared bit for bit (a GAUSS block with the point's sigma_y is the headline).
2. dense_grid  lzq_sweep_grid_window (the point and its block decoded from the flat index in the
           kernel; a GAUSS base block, no window axis) against lzq_sweep_grid on the first 1e5 points
           of the C2 grid, n_y = 8000, alternating likewise, compared bit for bit.
3. sweep   points/s of a reuse-mode sweep over window axes (window_y0 x window_sigma x delta_LZ,
           through sweep.make_compute) by its two paths -- explicit records built on the host,
           uploaded, grouped and integrated from shared z-sum tables (window_host_records: the path
           every window sweep took before the grid entry points, kept for axes that collide), and
           the grid path (lzq_sweep_grid_ztables_window once, lzq_sweep_grid_from_ztables_window per
           chunk: nothing built or uploaded per point) -- beside the same-size source_shape_sigma_y x
           delta_LZ sweep through lzq_sweep_grid_reuse.  The three alternate in one process.  A host
           clock around work that ends in a device synchronise; the record path's time is also split
           into host records, and upload + launches.  The three tables' first chunk is compared bit
           for bit between the two window paths.

    python tools/bench_window.py [--runs 5] [--json profiles/window/bench_window_grid.json]
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


def bench_dense_grid(eng, sw, runs):
    spec = sw.builtin_specs()["C2"]
    axes = sw.grid_axes_for_kernel(spec)
    block = {"kind": "gauss", "sigma_hi": float(spec.base["source_shape_sigma_y"])}
    out_p = torch.empty((DENSE_POINTS, 6), dtype=torch.float64, device=eng.device)
    out_w = torch.empty_like(out_p)
    plain = lambda: eng.sweep(spec.base, axes, 0, DENSE_POINTS, n_y=spec.n_y, out=out_p)
    window = lambda: eng.sweep(spec.base, axes, 0, DENSE_POINTS, n_y=spec.n_y, out=out_w, window=block)
    a, b = plain(), window()   # warm-up
    torch.cuda.synchronize()
    same = torch.equal(a.view(torch.int64), b.view(torch.int64))
    tp, tw = [], []
    for _ in range(runs):      # alternating
        tp.append(event_ms(plain)[0])
        tw.append(event_ms(window)[0])
    mp, mw = statistics.median(tp), statistics.median(tw)
    return {"points": DENSE_POINTS, "n_y": spec.n_y, "bit_identical": bool(same),
            "lzq_sweep_grid_ms": stats(tp), "lzq_sweep_grid_window_ms": stats(tw),
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

    def run(spec, **kw):
        compute = sw.make_compute(spec, eng, reuse=True, **kw)
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

    def first_chunk(**kw):
        sw.make_compute(wspec, eng, reuse=True, **kw)(0, CHUNK, out)
        return out.clone()

    same = torch.equal(first_chunk(window_host_records=True).view(torch.int64), first_chunk().view(torch.int64))
    run(wspec, window_host_records=True), run(wspec), run(sspec)     # warm-up
    paths = [eng.last_reuse]
    tr, tw, ts, th = [], [], [], []
    for _ in range(runs):      # alternating
        ts.append(run(sspec))
        tr.append(run(wspec, window_host_records=True))
        tw.append(run(wspec))
        paths.append(eng.last_reuse)
        th.append(host_records(wspec))
    mr, mw, ms, mh = (statistics.median(t) for t in (tr, tw, ts, th))
    spread = lambda t, m: (max(t) - min(t)) / m
    return {"points": total, "chunk": CHUNK, "n_y": wspec.n_y, "path": sorted(set(paths)),
            "window_paths_bit_identical_first_chunk": bool(same),
            "window_axes_host_records_s": stats(tr), "window_axes_grid_s": stats(tw), "sigma_y_axis_s": stats(ts),
            "window_host_records_s": stats(th),
            "spread": {"window_axes_host_records": spread(tr, mr), "window_axes_grid": spread(tw, mw),
                       "sigma_y_axis_device_grid": spread(ts, ms)},
            "points_per_s": {"window_axes_host_records": total / mr, "window_axes_grid": total / mw,
                             "sigma_y_axis_device_grid": total / ms},
            "grid_over_host_records_speedup": mr / mw,
            "grid_beats_host_records_by_more_than_the_spreads": bool(mr - mw > max(max(tr) - min(tr), max(tw) - min(tw))),
            "window_grid_over_sigma_y_grid_rate": ms / mw,
            "host_records_share_of_record_path": mh / mr}


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
    rec["dense_grid"] = bench_dense_grid(eng, sw, args.runs)
    rec["sweep"] = bench_sweep(eng, sw, args.runs)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
