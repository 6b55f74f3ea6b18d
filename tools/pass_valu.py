#!/usr/bin/env python3
"""The once-per-pass VALU work of the headline kernel yields_grid_kernel<1,1,1200>, counted in its
gfx950 ISA (device-only compile, no GPU): the VALU instructions of one iteration of the y-loop OUTSIDE
the z-loops, per path, weighted by the C2 plan.

The kernel's control-flow graph is built from the assembly (basic blocks, dominators, natural loops).
The y-loop is its largest natural loop; the loops nested in it are the z-loops (told apart by the VALU
census of their 8-node batch: 8 G pure fma for the accumulate-only loops of G chains, 32 for the zero
and frozen-t nodes, 48 for the uniform node, 64 / 72 for the clamp-free / clamped general node) and the
batch searches (seg_first_batch: a few VALU per iteration, ~log2(150) iterations).  With the back edges
cut and the bodies of the nested loops taken out, the y-loop body is a DAG; the cheapest path from the
loop header to a latch that passes through a given z-loop is what a pass that takes that loop executes
where no rare branch fires (an interior pass, T > m_chi/3, no truncation).  A search loop on the path
counts SEARCH_ITERS times.

Paths: a group of four and of two (per pass: the path divided by the group size), a single zero-type
pass (through an accumulate-only loop of one chain), a clamp-free pass (through the 64-VALU loop) and a
clamped pass (through the 72-VALU loop).  The C2 weights are the host plan that
tools/uniform_segment_share.py prints.

    python tools/pass_valu.py [-DNAME=VAL ...] [--json OUT]
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools")]
import isa_kernel as K  # noqa: E402

KERNEL = "yields_grid_kernelILi1ELi1ELi1200"
SEARCH_ITERS = 8          # seg_first_batch over 150 batches
BRANCH = re.compile(r"s_(cbranch_\w+|branch)\s+(\.LBB\S+)")


def instructions(body):
    """[(label or None, text)] of the real instructions of a function body."""
    out, pending = [], None
    for l in body:
        t = l.strip()
        m = re.match(r"^(\.LBB\S+):", t)
        if m:
            pending = m.group(1)
            continue
        if not t or t.startswith((";", ".", "//", "#")) or t.endswith(":"):
            continue
        out.append((pending, t.split(";")[0].strip()))
        pending = None
    return out


def is_valu(t):
    return K.classify(t) in ("valu", "valu_f64")


def analyse(ins):
    """Basic blocks, their successors, dominators (bit sets), and the natural loops {header: body}."""
    label_at = {lab: i for i, (lab, _) in enumerate(ins) if lab}
    n = len(ins)
    leaders = {0} | set(label_at.values())
    for i, (_, t) in enumerate(ins):
        if BRANCH.match(t) or t.startswith("s_endpgm"):
            leaders.add(i + 1)
    starts = sorted(x for x in leaders if x < n)
    blocks = [(st, (starts[bi + 1] - 1 if bi + 1 < len(starts) else n - 1)) for bi, st in enumerate(starts)]
    block_of = {st: bi for bi, (st, _) in enumerate(blocks)}
    succ = []
    for bi, (st, en) in enumerate(blocks):
        t = ins[en][1]
        out = []
        m = BRANCH.match(t)
        if m and m.group(2) in label_at:
            out.append(block_of[label_at[m.group(2)]])
        if not t.startswith(("s_branch", "s_endpgm")) and bi + 1 < len(blocks):
            out.append(bi + 1)
        succ.append(sorted(set(out)))
    nb = len(blocks)
    pred = [[] for _ in range(nb)]
    for u in range(nb):
        for v in succ[u]:
            pred[v].append(u)
    full = (1 << nb) - 1
    dom = [full] * nb
    dom[0] = 1
    changed = True
    while changed:
        changed = False
        for v in range(1, nb):
            d = full
            for u in pred[v]:
                d &= dom[u]
            d |= 1 << v
            if d != dom[v]:
                dom[v], changed = d, True
    loops = {}
    for u in range(nb):
        for h in succ[u]:
            if dom[u] >> h & 1:                                   # back edge u -> h
                body = loops.setdefault(h, {h})
                stack = [u]
                while stack:
                    x = stack.pop()
                    if x not in body:
                        body.add(x)
                        stack.extend(pred[x])
    return blocks, succ, dom, loops


def census(ins, blocks, body):
    ops = [t.split()[0] for b in body for _, t in ins[blocks[b][0]:blocks[b][1] + 1] if is_valu(t)]
    f64 = [o for o in ops if "f64" in o]
    acc = {t.split()[1].rstrip(",") for b in body for _, t in ins[blocks[b][0]:blocks[b][1] + 1]
           if t.startswith(("v_fma_f64", "v_fmac_f64"))}
    return {"valu": len(ops), "fma": sum(o.startswith(("v_fma_f64", "v_fmac_f64")) for o in f64),
            "mul": sum(o.startswith("v_mul_f64") for o in f64), "f64": len(f64), "fma_destinations": len(acc)}


def kind_of(c):
    if c["valu"] == c["fma"] and c["valu"] % 8 == 0 and c["fma_destinations"] in (1, 2, 4):
        return f"acc{c['fma_destinations']}"      # G chains; the compiler may have unrolled the batch loop
    if c["valu"] in (32, 48, 64, 72) and c["f64"] >= 32:
        return {32: "four_op", 48: "uniform", 64: "free", 72: "clamped"}[c["valu"]]
    return "search" if c["valu"] <= 12 else "other"


def path_costs(ins, blocks, succ, dom, loops):
    """min / max VALU of one y-loop iteration (header to a latch) through each z-loop, nested bodies
    excluded (a search loop's body times SEARCH_ITERS)."""
    yh = max(loops, key=lambda h: len(loops[h]))                  # the y-loop: the largest natural loop
    ybody = loops[yh]
    inner = {h: b for h, b in loops.items() if h != yh and h in ybody}
    top = {h: b for h, b in inner.items() if not any(h in b2 and h2 != h for h2, b2 in inner.items())}
    kinds = {h: kind_of(census(ins, blocks, b)) for h, b in top.items()}
    in_inner = {x: h for h, b in top.items() for x in b}
    cost = {}
    for x in ybody:
        if x in in_inner:
            h = in_inner[x]
            cost[x] = SEARCH_ITERS * census(ins, blocks, top[h])["valu"] if (x == h and kinds[h] == "search") else 0
        else:
            cost[x] = census(ins, blocks, [x])["valu"]
    fwd = {x: [v for v in succ[x] if v in ybody and not (dom[x] >> v & 1)] for x in ybody}
    latches = [x for x in ybody if yh in succ[x]]
    order, seen = [], {yh}
    stack = [(yh, iter(fwd[yh]))]
    while stack:                                                  # post-order DFS, reversed: topological
        node, it = stack[-1]
        for v in it:
            if v not in seen:
                seen.add(v)
                stack.append((v, iter(fwd[v])))
                break
        else:
            order.append(node)
            stack.pop()
    order.reverse()

    def sweep(src, best):
        d = {src: cost[src]}
        for x in order:
            if x in d:
                for v in fwd[x]:
                    c = d[x] + cost[v]
                    d[v] = c if v not in d else best(d[v], c)
        return d

    out = {}
    for h, k in kinds.items():
        if k in ("search", "other"):
            continue
        rec = {"kind": k, "instruction_range": list(blocks[h]), "batch_census": census(ins, blocks, top[h])}
        to_h = sweep(yh, min).get(h)
        d = sweep(h, min)
        ends = [d[x] for x in latches if x in d]
        rec["min"] = None if to_h is None or not ends else to_h + min(ends) - cost[h]
        out[f"{k}@{blocks[h][0]}"] = rec
    nested = {f"{k}@{blocks[h][0]}": census(ins, blocks, top[h])["valu"] for h, k in kinds.items()}
    return out, nested, len(ybody)


def c2_weights():
    """Passes per path on C2, from the host plan of tools/uniform_segment_share.py."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import test_zsum_frozen_host as HF
    import test_zsum_group_host as HG
    import zsum_ref as Z
    g = Z.grid(1200, 30.0)
    c2 = HG.c2_points()
    plan4 = HG.run(HG.load_lib(), g, c2, 4)[3]
    _, _, plan = HF.run(HF.load_lib(), g, c2, HF.FROZEN, 0)
    size = plan4[:, 0]
    single = size == 1
    path = plan[:, 0]
    return {"group4": int((size == 4).sum()), "group2": int((size == 2).sum()),
            "zero_single": int((single & ((path == HF.ZERO) | (path == HF.DEAD))).sum()),
            "free": int((single & (path == HF.FREE)).sum()), "clamped": int((single & (path == HF.SPLIT)).sum()),
            "passes": int(len(path))}


def main():
    defines = [a for a in sys.argv[1:] if a.startswith("-D")]
    out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    asm = os.path.join("/tmp", "pass_valu_lzq_kernels.s")
    K.compile_asm("lzq_kernels.hip", defines, asm)
    s = open(asm).read().split("\n")
    i0 = next(i for i, l in enumerate(s) if l.startswith("_ZN") and KERNEL in l and l.split(":")[0].endswith("i"))
    i1 = next(i for i in range(i0, len(s)) if s[i].startswith(".Lfunc_end"))
    ins = instructions(s[i0 + 1:i1])
    blocks, succ, dom, loops = analyse(ins)
    paths, nested, nblocks = path_costs(ins, blocks, succ, dom, loops)

    def cheapest(kind):
        c = [p["min"] for p in paths.values() if p["kind"] == kind and p["min"] is not None]
        return min(c) if c else None

    per_iter = {"group4": cheapest("acc4"), "group2": cheapest("acc2"), "zero_single": cheapest("acc1"),
                "free": cheapest("free"), "clamped": cheapest("clamped")}
    rec = {"kernel": KERNEL, "defines": defines, "search_iterations": SEARCH_ITERS, "y_loop_blocks": nblocks,
           "nested_loops_batch_valu": nested, "paths_through_z_loops": paths, "valu_per_y_loop_iteration": per_iter}
    if all(v is not None for v in per_iter.values()):
        w = c2_weights()
        per_pass = {"group4": per_iter["group4"] / 4.0, "group2": per_iter["group2"] / 2.0,
                    **{k: float(per_iter[k]) for k in ("zero_single", "free", "clamped")}}
        # a group of G is one y-loop iteration for G passes
        weighted = (per_iter["group4"] * w["group4"] / 4.0 + per_iter["group2"] * w["group2"] / 2.0
                    + sum(per_iter[k] * w[k] for k in ("zero_single", "free", "clamped"))) / w["passes"]
        rec.update({"valu_per_pass": per_pass, "c2_passes": w, "c2_weighted_valu_per_pass": weighted,
                    "c2_weighted_valu_per_wave_node": weighted / 1200.0})
    txt = json.dumps(rec, indent=1)
    print(txt)
    if out_json:
        with open(out_json, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
