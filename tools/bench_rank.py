#!/usr/bin/env python3
"""Cost of the device-side ranked points (include/lzq.h lzq_rank_*) on one MI355X.

The chunk of tools/bench_fit.py -- rows [0, 2^20) of the C4 grid, computed in reuse mode, device
resident -- and the `paper` terms, folded into ranked states of capacity 64 and 4096 in three cases:

  steady      into a state that has seen the chunk and then n rows that sit on the targets (chi2 0):
              no row of the timed chunk ranks before the list's last entry, which is what almost
              every chunk of a sweep finds once its early chunks have filled the list.  (The same
              chunk at the same indices again would not do: the rows already listed would rank
              before the last entry once more and be listed twice.)
  cold        into an empty state: every valid row of the chunk is a candidate
  beats_full  into a full list of n rows far from the targets: every valid row of the chunk ranks
              before every entry and the whole list is replaced

Timed with HIP events on the launch stream, median of `reps` after a warm-up; the state is put
back before each timed call (a device copy ahead of the first event).  In the same process:

  fit_update  ms per lzq_fit_update, same terms, bench_post.py's three maps, into a state that has
              seen the chunk: the yardstick each time is reported beside
  clone       torch.clone of the chunk: the streaming yardstick

    python tools/bench_rank.py [--reps 30] [--json profiles/fit/bench_rank.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_fit import PKG, ROWS, git_head, timed   # noqa: E402

CAPACITIES = (64, 4096)


def timed_from(words, saved, fn, reps, warm=3):
    """timed(), with `words` put back to `saved` ahead of every call's first event."""
    s = torch.cuda.current_stream()
    ts = []
    for k in range(warm + reps):
        words.copy_(saved)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        if k >= warm:
            ts.append(e0.elapsed_time(e1))
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "reps": reps}


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
    terms = F.PAPER["terms"]
    rec = {"what": "tools/bench_rank.py", "commit": args.commit or git_head(ROOT),
           "device": torch.cuda.get_device_name(eng.device), "rows": ROWS, "bytes": nbytes, "terms": terms, "cases": {}}
    rec["clone"] = timed(lambda: torch.clone(chunk), args.reps)
    fit = F.FitSpec.from_json({"terms": terms, "levels": F.PAPER["levels"],
                               "maps": [["beta_over_H", "I_p"], ["m_chi_GeV", "delta_LZ"], ["v_w"]]})
    fs = eng.fit_state(fit, fit.resolve(spec))
    eng.fit_update(fs, chunk, 0)
    rec["fit_update"] = timed(lambda: eng.fit_update(fs, chunk, 0), args.reps)
    fit_ms = rec["fit_update"]["ms_median"]
    host_chunk = chunk.cpu().numpy()
    n_valid = int(np.isfinite(F.chi2_rows(fit, host_chunk)).sum())
    rec["chunk_valid_rows"] = n_valid

    def rows_at(field_values, n):
        t = np.ones((n, 6))
        for f, v in field_values.items():
            t[:, F.YIELD_FIELDS.index(f)] = v
        return torch.from_numpy(t).to(eng.device)

    for n in CAPACITIES:
        on_target = rows_at({t["field"]: t["target"] for t in terms}, n)            # chi2 0
        far = rows_at({t["field"]: t["target"] + 1e12 * t["sigma"] for t in terms}, n)   # chi2 2e24
        c = {}
        # steady: nothing is a candidate, nothing but two counters is written
        st = eng.rank_state(fit, n)
        eng.rank_update(st, chunk, 0)
        eng.rank_update(st, on_target, ROWS)
        before = st.words.clone()
        c["steady"] = timed(lambda: eng.rank_update(st, chunk, ROWS + n), args.reps)
        c["steady"]["list_unchanged"] = bool(torch.equal(st.words[8:], before[8:]) and st.words[1] == before[1])
        # cold: the whole chunk is candidate
        st = eng.rank_state(fit, n)
        empty = st.words.clone()
        c["cold"] = timed_from(st.words, empty, lambda: eng.rank_update(st, chunk, 0), args.reps)
        c["cold"]["candidates"] = n_valid
        ref = F.HostRanked(fit, n)
        ref.update(host_chunk, 0)
        c["cold"]["equals_host"] = bool(np.array_equal(st.words.cpu().numpy(), ref.to_words()))
        # beats_full: a full list of worse rows is replaced entry for entry
        st = eng.rank_state(fit, n)
        eng.rank_update(st, far, ROWS)
        full = st.words.clone()
        c["beats_full"] = timed_from(st.words, full, lambda: eng.rank_update(st, chunk, 0), args.reps)
        c_far = F.chi2_rows(fit, far[:1].cpu().numpy())[0]
        c["beats_full"]["candidates"] = int((F.chi2_rows(fit, host_chunk) <= c_far).sum())
        ref = F.HostRanked(fit, n)
        ref.update(far.cpu().numpy(), ROWS)
        ref.update(host_chunk, 0)
        c["beats_full"]["equals_host"] = bool(np.array_equal(st.words.cpu().numpy(), ref.to_words()))
        for t in c.values():
            t["GB_per_s"] = nbytes / (t["ms_median"] * 1e-3) / 1e9
            t["over_fit_update"] = t["ms_median"] / fit_ms
            t["over_clone"] = t["ms_median"] / rec["clone"]["ms_median"]
        rec["cases"][str(n)] = c
    print(json.dumps(rec))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
