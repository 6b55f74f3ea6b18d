#!/usr/bin/env python3
"""Cost of the device-side sweep observables (include/lzq.h lzq_obs_*) on one MI355X.

The chunk of tools/bench_fit.py and tools/bench_post.py -- rows [0, 2^20) of the C4 grid, computed
in reuse mode, device resident -- folded into two observables, each alone, weighted (at the offset
"best", the chunk's own best chi2) and unweighted:

  log1d   DM_over_B in 8 sub-bins an octave over [0.01, 1000): 133 cells, block-private in LDS
  lin2d   Y_B x DM_over_B in 200 x 100 linear bins: 20,000 cells, straight to global memory

Two likelihoods as in bench_post.py: `paper` (1% sigmas: almost every row weighs nothing) and
`wide` (sigmas 100% of the targets: most rows carry weight).  Timed with HIP events on the launch
stream, median of `reps` after a warm-up, in the same process as the two yardsticks:

  obs_update   ms per lzq_obs_update into a state that has seen the chunk (a sweep's steady state)
  fit_update   ms per lzq_fit_update, same terms, bench_post.py's three maps
  post_update  ms per lzq_post_update, same terms, maps and offset
  clone        torch.clone of the chunk: the streaming yardstick

    python tools/bench_obs.py [--reps 30] [--json profiles/fit/bench_obs.json]
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_fit import PKG, ROWS, git_head, timed   # noqa: E402

OBS = {"log1d": {"axes": [{"field": "DM_over_B", "lo": 0.01, "hi": 1000.0, "per_octave": 8}]},
       "lin2d": {"axes": [{"field": "Y_B", "lo": 0.0, "hi": 2e-10, "bins": 200},
                          {"field": "DM_over_B", "lo": 0.0, "hi": 10.0, "bins": 100}]}}
REUSE_CHUNK_MS = 60.7   # the chunk's own reuse-mode kernels (profiles/fit/bench_fit.json)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--commit", default=None, help="the commit this tree was measured at (default: git HEAD)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    sw = importlib.import_module(PKG + ".sweep")
    F = importlib.import_module(PKG + ".fit")
    eng = importlib.import_module(PKG + ".engine").Engine()
    spec = sw.builtin_specs()["C4"]
    compute = sw.make_compute(spec, eng, reuse=True)
    chunk = torch.empty((ROWS, 6), dtype=torch.float64, device=eng.device)
    compute(0, ROWS, chunk)
    torch.cuda.synchronize()
    nbytes = ROWS * 48
    rec = {"what": "tools/bench_obs.py", "commit": args.commit or git_head(ROOT),
           "device": torch.cuda.get_device_name(eng.device), "rows": ROWS, "bytes": nbytes,
           "lds_cells": F.OBS_LDS_CELLS, "reuse_chunk_ms": REUSE_CHUNK_MS, "cases": {}}
    rec["clone"] = timed(lambda: torch.clone(chunk), args.reps)
    maps_json = [["beta_over_H", "I_p"], ["m_chi_GeV", "delta_LZ"], ["v_w"]]
    wide = [{**t, "sigma": abs(t["target"])} for t in F.PAPER["terms"]]
    for case, terms in (("paper", F.PAPER["terms"]), ("wide", wide)):
        fit = F.FitSpec.from_json({"terms": terms, "levels": F.PAPER["levels"], "maps": maps_json, "posterior": {}})
        maps = fit.resolve(spec)
        fs = eng.fit_state(fit, maps)
        eng.fit_update(fs, chunk, 0)
        best = eng.fit_result(fs)["best"]
        ps = eng.post_state(fit, maps, best["chi2"])
        c = {"terms": terms, "offset": best["chi2"], "obs": {}}
        for name, fn in (("fit_update", lambda: eng.fit_update(fs, chunk, 0)),
                         ("post_update", lambda: eng.post_update(ps, chunk, 0))):
            c[name] = timed(fn, args.reps)
        both = c["fit_update"]["ms_median"] + c["post_update"]["ms_median"]
        for oname, o in OBS.items():
            ospec = F.FitSpec.from_json({"terms": terms, "observables": [o]})
            for weighted in (True, False):
                st = eng.obs_state(ospec, ospec.observables, best["chi2"] if weighted else None)
                # (the same rows again: reps x 2^20 stays far below the 2^32 limit)
                t = timed(lambda: eng.obs_update(st, chunk), args.reps)
                t["GB_per_s"] = nbytes / (t["ms_median"] * 1e-3) / 1e9
                t["over_fit"] = t["ms_median"] / c["fit_update"]["ms_median"]
                t["over_post"] = t["ms_median"] / c["post_update"]["ms_median"]
                t["over_fit_plus_post"] = t["ms_median"] / both
                t["over_clone"] = t["ms_median"] / rec["clone"]["ms_median"]
                t["share_of_reuse_chunk"] = t["ms_median"] / REUSE_CHUNK_MS
                once = eng.obs_state(ospec, ospec.observables, best["chi2"] if weighted else None)
                eng.obs_update(once, chunk)
                r = eng.obs_result(once)[0]
                t["chunk"] = {"cells": ospec.observables[0].cells, "n_in": r["n_in"], "n_out": r["n_out"],
                              "n_nonfinite": r["n_nonfinite"], "cells_hit": int((r["count"] > 0).sum()),
                              "total_units": r["total_units"]}
                c["obs"][f"{oname}_{'weighted' if weighted else 'unweighted'}"] = t
        rec["cases"][case] = c
    print(json.dumps(rec))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
