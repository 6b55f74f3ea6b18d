#!/usr/bin/env python3
"""A/B of lzq_profile_crossings in one process: this tree's library against another build of it
(e.g. the parent commit's liblzq.so), on tools/bench_profile.py's shape (16 shapes x 256 knots,
100000 points, max_cross 8), timings interleaved; also whether the counts, the xi* and the
propagation's P are the same bits.

    python tools/ab_profile_crossings.py OTHER_LIBLZQ_SO [--json OUT]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("other", help="path of the other liblzq.so")
ap.add_argument("--json", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "baryon-and-dark-matter-densities-from-bounce--sourced-distributed-landau--zener-transport_amd"
B = importlib.import_module(PKG + ".bounce")
E = importlib.import_module(PKG + ".engine")
new = E.Engine(0)
old = E.Engine(0, os.path.abspath(args.other))
assert new.lib is not old.lib
n, ns, nk = 100_000, 16, 256
X, phi, Phi = B.synthetic_shapes(ns, nk)
yB, ychi, lam, vw, shape = B.synthetic_couplings(n, ns)
pts = new.profile_points(yB, ychi, lam, vw, shape)
sh = new.profile_shapes(X, phi, Phi)
sh_old = old.profile_shapes(X, phi, Phi)
assert torch.equal(sh.coef, sh_old.coef)

def timed(fn, launches=20):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(launches):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / launches

for eng in (new, old):
    for _ in range(3):
        eng.profile_crossings(sh, pts, 8)
torch.cuda.synchronize()
t = {"new": [], "old": []}
for rep in range(7):
    for name, eng in (("new", new), ("old", old), ("old", old), ("new", new)):
        t[name].append(timed(lambda: eng.profile_crossings(sh, pts, 8)))
cn = {k: v.cpu().numpy() for k, v in new.profile_crossings(sh, pts, 8).items()}
co = {k: v.cpu().numpy() for k, v in old.profile_crossings(sh, pts, 8).items()}
same_count = int((cn["count"] == co["count"]).sum())
m = cn["count"] == co["count"]
k = np.arange(8)[None, :] < cn["count"][:, None]
same_xi = bool(np.array_equal(cn["xi"][m][k[m]], co["xi"][m][k[m]]))
Pn = new.lz_propagate_profile(sh, pts).cpu().numpy()
Po = old.lz_propagate_profile(sh, pts).cpu().numpy()
rec = {"points": n, "shapes": ns, "knots": nk, "max_cross": 8,
       "new_seconds": sorted(t["new"]), "old_seconds": sorted(t["old"]),
       "new_points_per_s_median": n / float(np.median(t["new"])), "old_points_per_s_median": n / float(np.median(t["old"])),
       "counts_equal": same_count, "xi_bit_identical_where_counts_equal": same_xi,
       "propagate_bit_identical": bool(np.array_equal(Pn, Po, equal_nan=True)), "P_finite": bool(np.isfinite(Pn).all())}
if args.json:
    json.dump(rec, open(args.json, "w"), indent=1)
print(json.dumps(rec))
