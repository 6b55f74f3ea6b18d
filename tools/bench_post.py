#!/usr/bin/env python3
"""Cost of the device-side sweep posterior (include/lzq.h lzq_post_*) on one MI355X.

The chunk of tools/bench_fit.py -- rows [0, 2^20) of the C4 grid, computed in reuse mode, device
resident -- with the same three maps (two slowest axes: a whole wave in one cell; two fastest: a
wave over 64 cells; a 1-D one), weighted at the offset "best" (the chunk's own best chi2).  Two
likelihoods: `paper` (1% sigmas: almost every row is far out and weighs nothing) and `wide` (the
sigmas 100% of the targets: most rows carry weight, the histogram and the maps take a pair of
atomic adds for every wave or row).  Timed with HIP events on the launch stream, median of `reps`
after a warm-up, lzq_fit_update of the same chunk in the same process as the yardstick:

  post_update       ms per lzq_post_update into a state that has seen the chunk (a sweep's steady
                    state; integer sums cost the same whatever the state holds)
  post_update_cold  the same into an empty state (reset + update, less the reset alone)
  fit_update        ms per lzq_fit_update (steady state), same fit, same maps
  clone             torch.clone of the chunk: the streaming yardstick

    python tools/bench_post.py [--reps 30] [--json profiles/fit/bench_post.json]
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
    rec = {"what": "tools/bench_post.py", "commit": args.commit or git_head(ROOT),
           "device": torch.cuda.get_device_name(eng.device), "rows": ROWS, "bytes": nbytes, "cases": {}}
    rec["clone"] = timed(lambda: torch.clone(chunk), args.reps)
    L = eng.lib
    stream = lambda: torch.cuda.current_stream(eng.device).cuda_stream
    maps_json = [["beta_over_H", "I_p"], ["m_chi_GeV", "delta_LZ"], ["v_w"]]
    wide = [{**t, "sigma": abs(t["target"])} for t in F.PAPER["terms"]]
    for case, terms in (("paper", F.PAPER["terms"]), ("wide", wide)):
        fit = F.FitSpec.from_json({"terms": terms, "levels": F.PAPER["levels"], "maps": maps_json, "posterior": {}})
        maps = fit.resolve(spec)
        fs = eng.fit_state(fit, maps)
        eng.fit_update(fs, chunk, 0)
        best = eng.fit_result(fs)["best"]
        st = eng.post_state(fit, maps, best["chi2"])

        def update():
            eng.post_update(st, chunk, 0)   # (the same rows again: reps x 2^20 stays far below the 2^32 limit)

        def reset():
            eng._check(L.lzq_post_reset(st.c_maps, len(st.maps), st.words.data_ptr(), stream()))

        def cold():
            reset()
            update()
        c = {"fit": fit.to_json(), "offset": best["chi2"],
             "maps": [{"axes": list(m.axes), "stride": list(m.stride), "len": list(m.len)} for m in maps]}
        for name, fn in (("post_reset", reset), ("reset_plus_update", cold), ("post_update", update),
                         ("fit_update", lambda: eng.fit_update(fs, chunk, 0))):
            c[name] = timed(fn, args.reps)
            c[name]["GB_per_s"] = nbytes / (c[name]["ms_median"] * 1e-3) / 1e9
        c["post_update_cold"] = {"ms_median": c["reset_plus_update"]["ms_median"] - c["post_reset"]["ms_median"]}
        c["post_over_fit"] = c["post_update"]["ms_median"] / c["fit_update"]["ms_median"]
        c["post_over_clone"] = c["post_update"]["ms_median"] / rec["clone"]["ms_median"]
        once = eng.post_state(fit, maps, best["chi2"])
        eng.post_update(once, chunk, 0)
        res = eng.post_result(once, fit.axis_values(spec))
        c["chunk_posterior"] = {k: res[k] for k in ("n_used", "n_zero", "n_above", "n_invalid", "Z", "mass_within",
                                                    "credible")}
        rec["cases"][case] = c
    print(json.dumps(rec))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
