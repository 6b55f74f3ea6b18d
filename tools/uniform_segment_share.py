#!/usr/bin/env python3
"""The share of the headline kernel's (pass, z-node) pairs that run the uniform-entry loop
(csrc/lzq_quad.h zsum_uniform) on the C2 workload, counted on the host.

Every C2 point has the same y grid and the same c, so the 125 passes of one point are the whole
grid.  The passes are planned by tests/zsum_dead_segment_host.cpp, i.e. by the LZQ_HD predicates and
batch search of csrc/lzq_exp2.h that the device's zsum_dispatch calls, the dead rule among them (c2
with numpy's exp, <= 1 ulp from the device's exp_sc: a pass whose boundary lane sits within 1e-16 of
a predicate's threshold could be planned differently, by one 8-node batch of 150,000).

Also printed: the share of nodes in whole-uniform (zero) passes, which run without the range
reduction (LZQ_ZERO_SEG, zsum_uniform<YB, true>), and the VALU instructions per wave-node that share
predicts from the PMC of the build without it (profiles/round8/parent_pmc_summary.json); and the
all-dead passes among them, which form the node's value once (LZQ_DEAD_SEG, zsum_dead: F's fma alone
per node, two FMA and one MUL fewer), with the VALU count and mix their share predicts from the PMC
of the build without that (profiles/round9/parent_pmc_summary.json), to set beside the shipped
kernel's PMC (profiles/round6/pmc_summary.json).

Last, the frozen tails (LZQ_FROZEN_SEG), planned by tests/zsum_frozen_host.cpp (the same predicates plus
seg_frozen_s / seg_frozen_t): the live zero passes whose s = A at every node, the tails of the other
live zero passes on which every lane's s has reached its last value (both run F's accumulate alone:
two FMA and one MUL fewer per node), and the tails of the clamp-free passes on which every lane's t
has (the four-operation node: one FMA, one ADD, two INT32 and the LDS read fewer), with the VALU count
and the FMA / MUL / ADD / INT32 / LDS mix they predict from the PMC of the build without them
(profiles/round10/parent_pmc_summary.json).

And the grouped passes (LZQ_GROUP_SEG), planned by tests/zsum_group_host.cpp (yb_wave's pass loop with
seg_group_slot / seg_group_kind): how many of the point's passes run in groups of four and two, frozen
and dead, their share of the (pass, node) pairs, and the classifications that come to nothing.  The
instruction counts do not change; what the groups buy is issue time (profiles/round11).

Last, the lean passes (LZQ_PASS_LEAN).  The one pass that mixes dead and clamped lanes is planned by
tests/zsum_mixed_host.cpp (seg_clamped_or_dead): its k2 and the nodes from there on, which run the
six-operation node with the entry held per lane instead of the nine-operation clamped general node
(the max, the address and the insert fewer; the LDS read too).  The once-per-pass work is counted in the
ISA by tools/pass_valu.py (profiles/round12/pass_valu.json: both builds, per path, weighted by this
plan); together they predict the VALU per wave-node from the PMC of the build without them
(profiles/round12/parent_pmc_summary.json).

And the packed feed (LZQ_ACC_FEED), planned by tests/zsum_feed_host.cpp on the grid's device image as the
library builds it: the nodes whose omega' comes from the packed array (the grouped sweeps, the whole
accumulate-only passes outside a group, the held tails), and the 64-byte lines of the z table that one
point's scalar loads touch before and after -- an 8-node batch is two lines of the interleaved nodes, one
of the packed array; a group's sweep loads each batch once for all its chains.  No instruction count
changes; what the array buys is feed time (profiles/round13).

Last, the clamped argument (LZQ_CLAMP_ARG), planned by tests/zsum_clamp_arg_host.cpp: the passes that take
zsum_dispatch's clamped branch, their k2, the suffix nodes that run as F's accumulate alone instead of the
six-operation node (t, w, s, q and v fewer: three FMA, one ADD and one MUL) and the prefix nodes of the clamped
general loop, which gain the select (a compare and two v_cndmask_b32), with the VALU count and mix they predict
from the PMC of the build without it (profiles/round15/parent_pmc_summary.json) and the time at four
SIMD-cycles per VALU instruction.  `--write` records that section as profiles/round15/clamp_arg_plan.json.

    python tools/uniform_segment_share.py [--write]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_zsum_dead_segment_host as H  # noqa: E402
import test_zsum_frozen_host as HF        # noqa: E402
import test_zsum_group_host as HG         # noqa: E402
import test_zsum_mixed_host as HM         # noqa: E402
import test_zsum_feed_host as HFD         # noqa: E402
import test_zsum_clamp_arg_host as HCA    # noqa: E402
import zsum_ref as Z                      # noqa: E402


def _parent(rnd):
    with open(os.path.join(ROOT, "profiles", rnd, "parent_pmc_summary.json")) as f:
        return json.load(f)


def frozen_counts(g, c2):
    """The three stretches of LZQ_FROZEN_SEG on the passes of c2, and what they predict from the parent's PMC."""
    _, _, plan = HF.run(HF.load_lib(), g, c2, HF.FROZEN, 0)
    path, kend, k3 = plan[:, 0], plan[:, 2], plan[:, 3]
    nodes = int(kend.sum())
    whole = (path == HF.ZERO) & (k3 == 0)
    ztail = (path == HF.ZERO) & (k3 > 0) & (k3 < kend)
    ttail = (path == HF.FREE) & (k3 < kend)
    n_whole, n_ztail, n_ttail = (int((kend - k3)[m].sum()) for m in (whole, ztail, ttail))
    fs, ft = (n_whole + n_ztail) / nodes, n_ttail / nodes
    p10 = _parent("round10")
    mix = dict(p10["valu_mix_per_wave_node"])
    mix["fma_f64"] -= 2.0 * fs + ft          # frozen s: s and q; frozen t: t
    mix["mul_f64"] -= fs                     # frozen s: v
    mix["add_f64"] -= ft                     # frozen t: w
    mix["int32"] -= 2.0 * ft                 # frozen t: the address and the exponent insert
    return {"frozen_seg": {
        "passes_live_zero_whole_frozen": int(whole.sum()), "nodes_whole_frozen": n_whole,
        "passes_live_zero_with_tail": int(ztail.sum()), "passes_live_zero_other": int(((path == HF.ZERO) & ~whole).sum()),
        "nodes_zero_tails": n_ztail,
        "passes_clamp_free": int((path == HF.FREE).sum()), "passes_clamp_free_with_tail": int(ttail.sum()),
        "nodes_clamp_free_tails": n_ttail, "clamp_free_tail_lengths": sorted((kend - k3)[ttail].tolist()),
        "frozen_s_share": fs, "frozen_t_share": ft,
        "predicted_valu_per_wave_node": p10["valu_insts_per_wave_node"] - 3.0 * fs - 4.0 * ft,
        "predicted_valu_per_wave_node_frozen_s_only": p10["valu_insts_per_wave_node"] - 3.0 * fs,
        "predicted_valu_mix_per_wave_node": mix,
        "predicted_lds_per_wave_node": p10["lds_insts_per_wave_node"] - ft}}


def group_counts(g, c2_nodes, gmax=4):
    """The grouped passes of LZQ_GROUP_SEG = gmax on the point's y-nodes c2_nodes (unpadded)."""
    _, _, _, plan = HG.run(HG.load_lib(), g, c2_nodes, gmax)
    size, path, tried = plan[:, 0], plan[:, 1], plan[:, 2]
    groups = HG.group_counts(plan)
    n_grouped = int((size > 1).sum())
    return {"group_seg": {
        "max_group": gmax, "passes": int(len(plan)), "passes_grouped": n_grouped,
        "passes_grouped_frozen": int(((size > 1) & (path == HG.ZERO)).sum()),
        "passes_grouped_dead": int(((size > 1) & (path == HG.DEAD)).sum()),
        "groups": {f"{s}x_{'dead' if p == HG.DEAD else 'frozen'}": n for (s, p), n in sorted(groups.items())},
        "grouped_node_share": n_grouped / len(plan),
        "classifications_refused": int(((size == 1) & (tried == 1)).sum())}}


def lean_counts(g, c2):
    """The mixed pass of LZQ_PASS_LEAN on the passes of c2 and, with the per-pass count of
    profiles/round12/pass_valu.json, what both predict from the parent's PMC."""
    import ctypes
    import subprocess
    import tempfile
    so = os.path.join(tempfile.mkdtemp(), "zsum_mixed_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, HM.PKG_NAME, "csrc"), os.path.join(ROOT, "tests", "zsum_mixed_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.zmixed_passes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, HM.DP, HM.DP, ctypes.c_int, HM.DP,
                                ctypes.c_long, HM.DP, HM.DP, HM.UP, HM.IP]
    plan = HM.run(L, g, c2, HM.NEW, 0)[3]
    mixed = plan[:, 0] == HM.MIXED
    nodes = int(plan[:, 2].sum())
    n_mixed = int((plan[:, 2] - plan[:, 1])[mixed].sum())
    p12 = _parent("round12")
    out = {"passes_mixed": np.flatnonzero(mixed).tolist(), "mixed_dead_lanes": plan[mixed, 3].tolist(),
           "mixed_k2": plan[mixed, 1].tolist(), "nodes_mixed_suffix": n_mixed, "mixed_suffix_share": n_mixed / nodes,
           "mixed_saved_valu_per_wave_node": 3.0 * n_mixed / nodes}
    pv = os.path.join(ROOT, "profiles", "round12", "pass_valu.json")
    if os.path.exists(pv):
        with open(pv) as f:
            rec = json.load(f)
        out.update({"per_pass_valu_parent": rec["parent"]["c2_weighted_valu_per_pass"],
                    "per_pass_valu_new": rec["new"]["c2_weighted_valu_per_pass"],
                    "per_pass_saved_valu_per_wave_node": rec["saved_valu_per_wave_node"],
                    "predicted_valu_per_wave_node": p12["valu_insts_per_wave_node"] - rec["saved_valu_per_wave_node"]
                    - 3.0 * n_mixed / nodes,
                    "predicted_valu_per_wave_node_per_pass_only": p12["valu_insts_per_wave_node"]
                    - rec["saved_valu_per_wave_node"],
                    "predicted_valu_per_wave_node_mixed_only": p12["valu_insts_per_wave_node"] - 3.0 * n_mixed / nodes,
                    "predicted_int32_per_wave_node": p12["valu_mix_per_wave_node"]["int32"] - 2.0 * n_mixed / nodes,
                    "predicted_lds_per_wave_node": p12["lds_insts_per_wave_node"] - n_mixed / nodes})
    return {"pass_lean": out}


def feed_counts(g, c2_nodes):
    """The nodes of LZQ_ACC_FEED on the point's y-nodes c2_nodes (unpadded), and the z-table lines touched."""
    _, _, _, plan, _, fed = HFD.run(HFD.load_lib(), g, c2_nodes, 1)
    size, path, first, k3 = plan[:, 0], plan[:, 1], plan[:, 2], plan[:, 3]
    nodes = int(len(plan)) * g.nz
    sweeps = int((size == 1).sum() + ((size > 1) & (first == 1)).sum())       # one pass over z each
    fed_batches = int(fed[size == 1].sum() + fed[(size > 1) & (first == 1)].sum()) // 8
    before = 2 * sweeps * (g.nz // 8)
    tails = (size == 1) & (path == HFD.ZERO) & (k3 > 0) & (fed > 0)
    return {"acc_feed": {
        "nodes_fed": int(fed.sum()), "fed_share": float(fed.sum()) / nodes,
        "nodes_fed_in_groups": int(fed[size > 1].sum()),
        "nodes_fed_whole_single_passes": int(fed[(size == 1) & (fed == g.nz)].sum()),
        "nodes_fed_held_tails": int(fed[tails].sum()), "held_tails": int(tails.sum()),
        "z_sweeps_per_point": sweeps, "batches_fed": fed_batches,
        "z_table_lines_per_point_before": before, "z_table_lines_per_point_after": before - fed_batches,
        "lines_saved_share": fed_batches / before}}


def clamp_arg_counts(g, c2):
    """The clamped branch of LZQ_CLAMP_ARG on the passes of c2, and what it predicts from the parent's PMC."""
    import ctypes
    import subprocess
    import tempfile
    so = os.path.join(tempfile.mkdtemp(), "zsum_clamp_arg_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, HCA.PKG_NAME, "csrc"), os.path.join(ROOT, "tests", "zsum_clamp_arg_host.cpp"),
                    "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.zca_passes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, HCA.DP, HCA.DP, ctypes.c_int, HCA.DP,
                             ctypes.c_long, HCA.DP, HCA.DP, HCA.UP, HCA.IP]
    plan = HCA.run(L, g, c2, HCA.SEG)[3]
    branch = (plan[:, 0] == HCA.SPLIT) | (plan[:, 0] == HCA.MIXED)
    nodes = int(plan[:, 2].sum())
    k2, kend = plan[branch, 1], plan[branch, 2]
    suffix, prefix = int((kend - k2).sum()), int(k2.sum())
    p15 = _parent("round15")
    saved = (5.0 * suffix - 3.0 * prefix) / nodes
    mix = dict(p15["valu_mix_per_wave_node"])
    mix["fma_f64"] -= 3.0 * suffix / nodes       # t, s, q
    mix["add_f64"] -= suffix / nodes             # w
    mix["mul_f64"] -= suffix / nodes             # v
    valu = p15["valu_insts_per_wave_node"] - saved
    return {"clamp_arg": {
        "passes_clamped_branch": np.flatnonzero(branch).tolist(), "k2": k2.tolist(),
        "passes_with_suffix": int((k2 < kend).sum()), "passes_mixed": np.flatnonzero(plan[:, 0] == HCA.MIXED).tolist(),
        "nodes_suffix_accumulate_only": suffix, "suffix_share": suffix / nodes,
        "nodes_clamped_general_loop": prefix, "clamped_general_share": prefix / nodes,
        "valu_saved_per_point": 5 * suffix, "valu_added_per_point": 3 * prefix,
        "parent_valu_per_wave_node": p15["valu_insts_per_wave_node"],
        "predicted_valu_per_wave_node": valu,
        "predicted_valu_mix_per_wave_node": mix,
        "predicted_flop_per_point": 64.0 * (2.0 * mix["fma_f64"] + mix["mul_f64"] + mix["add_f64"]) * nodes,
        "parent_cycles_per_wave_node": p15["cycles_per_wave_node_per_simd"],
        "predicted_cycles_saved_per_wave_node_at_4_per_valu": 4.0 * saved,
        "predicted_time_ratio_at_4_cycles_per_valu": 1.0 - 4.0 * saved / p15["cycles_per_wave_node_per_simd"]}}


def main():
    B, Tp, I_p = 100.0, 100.0, 0.34                  # yields_config_equal_mass.json (C2's base)
    y_of = lambda T: 0.5 * B * ((Tp / T) ** 2 - 1.0)
    ys = np.linspace(max(y_of(5.0 * Tp), -80.0), min(y_of(1e-3 * Tp), 50.0), 8000)
    g = Z.grid(1200, 30.0)
    c2 = ((-(I_p / 6.0) * np.exp(np.clip(ys, -50.0, 50.0))) * Z.LOG2E) * 8192.0
    grouped = {**group_counts(g, c2), **feed_counts(g, c2)}
    c2 = np.concatenate([c2, np.full(-len(c2) % 64, c2[-1])])      # tail lanes recompute the last node
    L = H.load_lib()
    _, _, plan = H.run(L, g, c2, H.DEADSEG, 0)
    path, k2, kend = plan[:, 0], plan[:, 1], plan[:, 2]
    nodes = int(kend.sum())
    dead = int(kend[path == H.DEAD].sum())
    zero = int(kend[path == H.ZERO].sum()) + dead                  # the all-dead passes are zero passes
    suffix = int((kend - k2)[path == H.SPLIT].sum())
    split = path == H.SPLIT
    lanes_dead = np.array([[bool(L.zdead_dead(float(c), float(g.g4[1]))) for c in w] for w in c2.reshape(-1, 64)])
    mixed = lanes_dead.any(axis=1) & ~lanes_dead.all(axis=1)
    # LZQ_ZERO_SEG: a node of a whole-uniform (zero) pass runs without t and w, an FMA and an ADD fewer
    # on every node of those passes; set beside the PMC of profiles/round8/parent_pmc_summary.json
    # (the six-operation node everywhere) this predicts the VALU per wave-node of the kernel with it
    p8 = _parent("round8")
    mix8 = dict(p8["valu_mix_per_wave_node"])
    mix8["fma_f64"] -= zero / nodes
    mix8["add_f64"] -= zero / nodes
    # LZQ_DEAD_SEG: a node of an all-dead pass runs F's fma alone: s (FMA), q (FMA) and v (MUL) are formed
    # once per pass; against profiles/round9/parent_pmc_summary.json (the four-operation node on them)
    p9 = _parent("round9")
    mix9 = dict(p9["valu_mix_per_wave_node"])
    mix9["fma_f64"] -= 2.0 * dead / nodes
    mix9["mul_f64"] -= dead / nodes
    ca = clamp_arg_counts(g, c2)
    if "--write" in sys.argv[1:]:
        os.makedirs(os.path.join(ROOT, "profiles", "round15"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "round15", "clamp_arg_plan.json"), "w") as f:
            json.dump(ca["clamp_arg"], f, indent=1)
    print(json.dumps({**grouped, **frozen_counts(g, c2), **lean_counts(g, c2), **ca,
        "passes": int(len(path)), "nodes_per_point": nodes,
        "passes_whole_uniform": int(((path == H.ZERO) | (path == H.DEAD)).sum()),
        "passes_clamp_free": int((path == H.FREE).sum()),
        "passes_clamped": int(split.sum()), "clamped_passes_with_suffix": int((split & (k2 < kend)).sum()),
        "k2_of_clamped_passes": k2[split].tolist(),
        "uniform_nodes_whole_pass": zero, "uniform_nodes_clamped_suffix": suffix,
        "uniform_share": (zero + suffix) / nodes,
        "zero_pass_share": zero / nodes,
        "predicted_valu_per_wave_node": p8["valu_insts_per_wave_node"] - 2.0 * zero / nodes,
        "predicted_valu_mix_per_wave_node": mix8,
        "passes_all_dead": int((path == H.DEAD).sum()), "all_dead_passes": np.flatnonzero(path == H.DEAD).tolist(),
        "passes_live_zero": int((path == H.ZERO).sum()),
        "passes_dead_and_live_lanes": int(mixed.sum()),
        "all_dead_nodes": dead, "all_dead_share": dead / nodes,
        "dead_seg_predicted_valu_per_wave_node": p9["valu_insts_per_wave_node"] - 3.0 * dead / nodes,
        "dead_seg_predicted_valu_mix_per_wave_node": mix9}))


if __name__ == "__main__":
    main()
