#!/usr/bin/env python3
"""Cost of the device-side sweep fit (include/lzq.h lzq_fit_*) on one MI355X.

A device-resident chunk of 2^20 yield records -- rows [0, 2^20) of the C4 grid, computed in reuse
mode -- is fitted to the `paper` terms with three maps: over the two slowest C4 axes (a whole wave
lands in one cell), over the two fastest (a wave spreads over 64 cells) and a 1-D one.  Timed with
HIP events on the launch stream, median of `reps` after a warm-up:

  fit_update     ms per lzq_fit_update, and rows x 48 B / time, into a state that has seen the chunk
                 (a sweep's steady state: few cells still improve)
  fit_update_cold  the same into an empty state (reset + update, less the reset alone): every cell
                 of every map is set for the first time
  fit_select     ms per lzq_fit_select of the same chunk
  clone          torch.clone of the same chunk in the same process: the streaming yardstick
  chunk_compute  the reuse-mode sweep kernels of the chunk (what the update is added to)
  host_path      table.cpu() + sweep.summarize on the same rows: what the fit replaces

    python tools/bench_fit.py [--reps 30] [--cli [--parent DIR]] [--json profiles/fit/bench_fit.json]

--cli also times the sweep CLI on `--spec C4 --reuse-zsums --limit 4194304 --out <tmp>` as child
processes: plain (from --parent DIR, a checkout of the parent commit with its library built, when
given; else this tree), with `--fit paper`, and with `--fit paper --no-table`; wall time of the
process and the elapsed_s of its result line.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "baryon-and-dark-matter-densities-from-bounce--sourced-distributed-landau--zener-transport_amd"
ROWS = 1 << 20
CLI_ARGS = ["--spec", "C4", "--reuse-zsums", "--limit", "4194304"]


def timed(fn, reps, warm=3):
    s = torch.cuda.current_stream()
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "reps": reps}


def git_head(root):
    try:
        return subprocess.run(["git", "-C", root, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def cli_run(root, extra):
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, PYTHONPATH=root)
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, "-m", PKG + ".sweep", *CLI_ARGS, "--out", os.path.join(d, "out"), *extra],
                           cwd=root, env=env, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(f"sweep CLI failed in {root}: {r.stderr[-2000:]}")
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        files = {n: os.path.getsize(os.path.join(d, "out", n)) for n in sorted(os.listdir(os.path.join(d, "out")))
                 if not n.startswith("shard_")}
    return {"args": CLI_ARGS + extra, "wall_s": wall, "elapsed_s": line["elapsed_s"],
            "points_per_s": line["points_per_s"], "files_bytes": files}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--parent", default=None, help="checkout of the parent commit (library built) for the plain CLI run")
    ap.add_argument("--parent-commit", default=None, help="its commit id, recorded with the timing")
    ap.add_argument("--commit", default=None, help="the commit this tree was measured at (default: git HEAD)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    sw = importlib.import_module(PKG + ".sweep")
    F = importlib.import_module(PKG + ".fit")
    eng = importlib.import_module(PKG + ".engine").Engine()
    spec = sw.builtin_specs()["C4"]
    compute = sw.make_compute(spec, eng, reuse=True)
    chunk = torch.empty((ROWS, 6), dtype=torch.float64, device=eng.device)
    compute(0, ROWS, chunk)          # builds the z-sum tables, then the chunk
    torch.cuda.synchronize()

    d = F.PAPER
    fit = F.FitSpec.from_json({**d, "maps": [["beta_over_H", "I_p"], ["m_chi_GeV", "delta_LZ"], ["v_w"]]})
    maps = fit.resolve(spec)
    st = eng.fit_state(fit, maps)
    nbytes = ROWS * 48
    rec = {"what": "tools/bench_fit.py", "commit": args.commit or git_head(ROOT), "device": torch.cuda.get_device_name(eng.device),
           "rows": ROWS, "bytes": nbytes, "fit": fit.to_json(),
           "maps": [{"axes": list(m.axes), "stride": list(m.stride), "len": list(m.len)} for m in maps]}
    L, vp = eng.lib, lambda t: t.data_ptr()
    stream = lambda: torch.cuda.current_stream(eng.device).cuda_stream

    def reset():
        eng._check(L.lzq_fit_reset(st.c_maps, len(st.maps), vp(st.words), stream()))

    def cold():
        reset()
        eng.fit_update(st, chunk, 0)
    for name, fn in (("fit_reset", reset), ("reset_plus_update", cold),
                     ("fit_update", lambda: eng.fit_update(st, chunk, 0)),
                     ("fit_select", lambda: eng.fit_select(st, chunk, 0)),
                     ("clone", lambda: torch.clone(chunk)),
                     ("chunk_compute", lambda: compute(0, ROWS, chunk))):
        rec[name] = timed(fn, args.reps)
        rec[name]["GB_per_s"] = nbytes / (rec[name]["ms_median"] * 1e-3) / 1e9
    rec["fit_update_cold"] = {"ms_median": rec["reset_plus_update"]["ms_median"] - rec["fit_reset"]["ms_median"]}
    rec["fit_update_cold"]["GB_per_s"] = nbytes / (rec["fit_update_cold"]["ms_median"] * 1e-3) / 1e9
    rec["update_over_chunk_compute"] = rec["fit_update"]["ms_median"] / rec["chunk_compute"]["ms_median"]
    rec["update_over_clone"] = rec["fit_update"]["ms_median"] / rec["clone"]["ms_median"]
    res = eng.fit_result(eng.fit_state(fit, maps))      # (an empty state: the read-back path once)
    st2 = eng.fit_state(fit, maps)
    eng.fit_update(st2, chunk, 0)
    res = eng.fit_result(st2)
    rec["chunk_fit"] = {"n_valid": res["n_valid"], "n_within": res["n_within"], "best": res["best"]}

    ts = []
    for _ in range(3):       # the host path on the same rows
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tab = chunk.cpu().numpy()
        t1 = time.perf_counter()
        sw.summarize(tab, spec)
        ts.append((time.perf_counter() - t0, t1 - t0))
    rec["host_path"] = {"ms_total_median": 1e3 * statistics.median(t[0] for t in ts),
                        "ms_copy_median": 1e3 * statistics.median(t[1] for t in ts), "reps": 3}

    if args.cli:
        del chunk, st, st2
        torch.cuda.empty_cache()
        rec["cli"] = {"parent": dict(cli_run(args.parent or ROOT, []),
                                     commit=(args.parent_commit or git_head(args.parent)) if args.parent else rec["commit"],
                                     tree="parent checkout" if args.parent else "this tree, no --fit"),
                      "fit": cli_run(ROOT, ["--fit", "paper"]),
                      "fit_no_table": cli_run(ROOT, ["--fit", "paper", "--no-table"])}
    line = json.dumps(rec)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
