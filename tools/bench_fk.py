#!/usr/bin/env python3
"""Cost of the momentum-averaged LZ probability (include/lzq.h lzq_fk; csrc/lzq_fk.hip) on one MI355X.

2^20 explicit points in 1000 classes (1000 values of m_chi; one z-sum table: m is not in its key) at
n_y = 8000, p = 1, v_ref = 1.  Legs alternating in one process, `runs` runs each after a warm-up, HIP events
on the launch stream:

  r_tables       lzq_fk_tables: the 1000 R tables (also per class, and with p = 0: no log / exp per node)
  fk             lzq_yields_batch_reuse_fk from tables already built, the points' Gaussian window
  fk_window      the same with a window block per point (a GAUSS block of the point's sigma_y)
  reuse_window   lzq_yields_batch_reuse_window on the same points and blocks (it rebuilds its one z-sum
                 table in every call, 1 wavefront next to 2^20)
  parent_reuse_window   the same entry point of another build of the library (--parent-lib: the parent
                 commit's), loaded into the same process: the existing reuse-mode figure has to be within
                 the run-to-run spread of it

    python tools/bench_fk.py [--runs 7] [--parent-lib PATH] [--json profiles/fk/bench_fk.json]
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
POINTS, CLASSES, NY = 1 << 20, 1000, 8000


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
    fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--points", type=int, default=POINTS)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "fk", "bench_fk.json"))
    a = ap.parse_args()
    E, sw, cfgm, N, fk, W = (importlib.import_module(f"{PKG}.{m}") for m in
                             ("engine", "sweep", "config", "_native", "fk", "window"))
    eng = E.Engine()
    dev = eng.device
    n = a.points
    base = sw.builtin_specs()["C4"].base
    pts = np.repeat(cfgm.to_point(base), n)
    pts["m_chi_GeV"] = np.logspace(-1, 3, CLASSES)[np.arange(n) % CLASSES]
    delta = np.full(n, 0.0237)
    rep_c, cls = fk.class_groups(pts[:CLASSES], delta[:CLASSES], fk.to_fks({"p": 1.0}, CLASSES))
    assert rep_c.size == CLASSES
    cls = cls[np.arange(n) % CLASSES]
    d_pts = eng.points_to_device(pts)
    d_delta = eng._f64(delta)
    d_rep_c, d_cls = torch.as_tensor(rep_c, device=dev), torch.as_tensor(cls, device=dev)
    blocks = {p: E._to_device_bytes(fk.to_fks({"p": p, "v_ref": 1.0}, n), dev) for p in (1.0, 0.0)}
    wins = np.repeat(W.to_window({"kind": "gauss"}), n)
    wins["sigma_hi"] = pts["source_shape_sigma_y"]
    d_win = E._to_device_bytes(wins, dev)
    zstride, rstride = NY + N.REUSE_TABLE_HEADER, int(eng.lib.lzq_fk_table_stride(NY))
    zwork = torch.empty(zstride, dtype=torch.float64, device=dev)
    Rt = torch.empty(CLASSES * rstride, dtype=torch.float64, device=dev)
    out = torch.empty((n, 6), dtype=torch.float64, device=dev)
    rep_z = torch.zeros(1, dtype=torch.int64, device=dev)
    idx_z = torch.zeros(n, dtype=torch.int32, device=dev)
    st = eng._stream()

    def reuse_window(lib):
        N.check(lib.lzq_yields_batch_reuse_window(vp(d_pts), n, NY, N.LZQ_NZ, N.LZQ_Z_MAX, None, vp(rep_z), vp(idx_z), 1,
                                                  vp(zwork), zwork.numel(), vp(d_win), None, vp(out), st), lib)

    def r_tables(p):
        eng._check(eng.lib.lzq_fk_tables(vp(d_pts), vp(d_delta), vp(blocks[p]), vp(d_rep_c), CLASSES, NY, vp(Rt),
                                         Rt.numel(), None, st))

    def integrate(win):
        eng._check(eng.lib.lzq_yields_batch_reuse_fk(vp(d_pts), n, NY, N.LZQ_NZ, N.LZQ_Z_MAX, vp(d_delta), vp(blocks[1.0]),
                                                     vp(idx_z), vp(zwork), zwork.numel(), vp(d_cls), vp(Rt), Rt.numel(),
                                                     vp(win), None, vp(out), st))

    legs = {"r_tables": lambda: r_tables(1.0), "fk": lambda: integrate(None), "fk_window": lambda: integrate(d_win),
            "reuse_window": lambda: reuse_window(eng.lib), "r_tables_p0": lambda: r_tables(0.0)}
    if a.parent_lib:
        # (the parent has none of the lzq_fk_* symbols _native.load declares: a plain handle with the two
        # entry points this leg calls, declared as _native declares them)
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.lzq_last_error.restype = ctypes.c_char_p
        parent.lzq_init.argtypes = eng.lib.lzq_init.argtypes
        parent.lzq_yields_batch_reuse_window.argtypes = eng.lib.lzq_yields_batch_reuse_window.argtypes
        with torch.cuda.device(dev):
            N.check(parent.lzq_init(dev.index), parent)
        legs["parent_reuse_window"] = lambda: reuse_window(parent)
    order = [k for k in legs if k != "r_tables_p0"] + ["r_tables_p0"]   # p = 0 last: the integration reads p = 1 tables
    ts = {k: [] for k in legs}
    with torch.cuda.device(dev):
        for r in range(a.runs + 1):                 # the first round is the warm-up
            for k in order:
                t = event_ms(legs[k])
                if r:
                    ts[k].append(t)
        integrate(None)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[:, 0]).all()), "a p = 1 integration from p = 0 tables has to be refused"
        r_tables(1.0)
        integrate(None)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
    res = {"device": torch.cuda.get_device_name(dev), "git_head": git_head(ROOT), "library_id": N.library_id(N.LIB_PATH),
           "parent_library_id": N.library_id(a.parent_lib) if a.parent_lib else None, "runs": a.runs, "points": n,
           "classes": CLASSES, "n_y": NY, "nodes": int(fk.nodes()[0].size)}
    for k in legs:
        res[k + "_ms"] = stats(ts[k])
    for k in ("fk", "fk_window", "reuse_window", "parent_reuse_window"):
        if k in legs:
            res[k + "_points_per_s"] = n / res[k + "_ms"]["median"] * 1e3
    res["r_table_us_per_class"] = res["r_tables_ms"]["median"] * 1e3 / CLASSES
    res["r_table_p0_us_per_class"] = res["r_tables_p0_ms"]["median"] * 1e3 / CLASSES
    if a.parent_lib:
        ratio = res["reuse_window_ms"]["median"] / res["parent_reuse_window_ms"]["median"]
        spread = max(res["reuse_window_ms"]["spread"], res["parent_reuse_window_ms"]["spread"])
        res["reuse_window_over_parent"] = ratio
        res["reuse_window_within_spread_of_parent"] = bool(abs(ratio - 1.0) <= spread)
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    print("wrote", a.json)


if __name__ == "__main__":
    main()
