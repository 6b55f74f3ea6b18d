#!/usr/bin/env python3
"""Build tuning variants of liblzq.so (compile-time knobs of csrc/) into
<package>/_build/variants/ for tools/ablate_builds.py.  Runs on the CPU (hipcc)."""
import glob
import importlib
import itertools
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "baryon-and-dark-matter-densities-from-bounce--sourced-distributed-landau--zener-transport_amd"
B = importlib.import_module(PKG + ".build")

GRID = {"LZQ_KUNROLL": [4, 8], "LZQ_YB": [1, 2]}
# explicit list (overrides the full product when non-empty); keys omitted take the defaults
CONFIGS = [dict(LZQ_KUNROLL=8), dict(LZQ_KUNROLL=10), dict(LZQ_KUNROLL=12)]


def switches():
    """The names csrc/ lets a build set: every `#ifndef NAME` of its sources and headers (and the
    `#ifdef NAME` of a debug switch that has no default)."""
    names = set()
    for f in glob.glob(os.path.join(B.CSRC, "*")):
        with open(f) as fh:
            names.update(re.findall(r"^\s*#\s*ifn?def\s+(\w+)", fh.read(), flags=re.M))
    return names


def check_names(confs):
    """Refuse a define that no source reads: it would build the default library under another name."""
    unknown = sorted({k for d in confs for k in d} - switches())
    if unknown:
        raise SystemExit(f"no '#ifndef NAME' or '#ifdef NAME' under csrc/ for: {', '.join(unknown)}")


def main():
    """argv: optional variant list, one 'KEY=VAL[,KEY=VAL...]' per variant (overrides CONFIGS)."""
    check_names([GRID, *CONFIGS])
    outdir = os.path.join(B.BUILD_DIR, "variants")
    import shutil
    keys = list(GRID)
    confs = CONFIGS or [dict(zip(keys, vals)) for vals in itertools.product(*(GRID[k] for k in keys))]
    if len(sys.argv) > 1:
        confs = [dict(kv.split("=", 1) for kv in arg.split(",")) for arg in sys.argv[1:]]
        check_names(confs)
    shutil.rmtree(outdir, ignore_errors=True)
    for d in confs:
        name = "_".join(f"{k[4:].lower()}{v}" for k, v in d.items())
        B.build(defines=d, out=os.path.join(outdir, f"liblzq_{name}.so"))
        print(name)


if __name__ == "__main__":
    main()
