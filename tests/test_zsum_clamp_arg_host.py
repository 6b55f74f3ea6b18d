"""The clamped argument of the dense z-sum (LZQ_CLAMP_ARG; csrc/lzq_exp2.h clamp_arg_s /
exp2_tab_scaled_clamp_arg / clamp_arg_value / clamp_arg_rounds_away, csrc/lzq_quad.h zsum<.., CLAMP = true> and
zsum_dispatch's clamped branch), on the CPU.

The parent clamps the magic sum t, that is the table index, and forms s from the unclamped t: an underflowed
node's stand-in value T''(KMIN) ((r_k + A)^2 + beta) carries a fractional part that moves at every node.  With
the switch on, a node with t <= M + KMIN is evaluated at the clamped argument u = KMIN itself (r = 0, s = A):
its value is the one number v_c = T''(KMIN) fma(A, A, beta), and from the batch k2 at which the last live lane
of a wave clamps the pass is F's accumulate alone.  Either stand-in's term omega' v ~ omega 2^-1506 is below
half the smallest subnormal, so F's bits cannot move; that bound is a condition on the grid's weights which
the library asserts for every grid it builds.

tests/zsum_clamp_arg_host.cpp evaluates one lane and a 64-lane pass from the LZQ_HD functions the device code
itself calls: the =0 general loop (OLD), the new general loop (NEW) and the new dispatch (SEG).
  * NEW against OLD: F bit for bit; node by node equal bits above the clamp and exactly v_c at and below it,
    with u within an ulp of KMIN, far below it and at |u| >= 2^51; F entering the clamped stretch as +0, a
    subnormal and a normal number.
  * SEG against NEW: F, the raw sums of the dead lanes and a checksum over every node's value, on uniform and
    mixed waves, k2 at the first batch, mid-grid, one batch before the end and at the end, truncation on and off.
  * three seeded defects (a wrong v_c, the suffix a batch early, a lost node) must each be caught.
  * the bound omega' v_c < 2^-1075 on every grid here, and its failure on a grid that breaks it.
  * -DLZQ_CLAMP_ARG=0 is the parent's machine code (profiles/round15/parent_pmc_summary.json).
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import test_zsum_dead_segment_host as HD
import zsum_ref as Z
from conftest import PKG_NAME, ROOT, pkg

HERE = os.path.dirname(os.path.abspath(__file__))
# the default grid, a runtime grid padded 13 -> 16, a fine one whose live lanes reach |u| >= 2^51, and a padded
# grid (29 -> 32) on which gamma4 still moves over the last batches, so that k2 can sit one batch before the end
GRIDS = ((1200, 30.0), (13, 3.0), (2400, 30.0), (29, 6.0))
OLD, NEW, SEG = -1, 0, 1                          # `mode` of zca_passes
ZERO, FREE, SPLIT, DEAD, MIXED = 0, 1, 2, 3, 4    # plan[0]
WRONG_VC, BATCH_EARLY, LOST_NODE = 1, 2, 3        # `defect`
DP, IP, UP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)
bits, padded = HD.bits, HD.padded


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(tempfile.mkdtemp(), "zsum_clamp_arg_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, PKG_NAME, "csrc"), os.path.join(HERE, "zsum_clamp_arg_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.zca_passes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, DP, DP, ctypes.c_int, DP, ctypes.c_long,
                             DP, DP, UP, IP]
    L.zca_nodes.argtypes = [DP, DP, ctypes.c_int, DP]
    L.zca_lane.argtypes = [ctypes.c_int, ctypes.c_double, DP, DP, ctypes.c_int, ctypes.c_double]
    L.zca_lane.restype = ctypes.c_double
    for f in (L.zca_vc, L.zca_vc_from_table, L.zca_tclamp, L.zca_kmin):
        f.restype = ctypes.c_double
    L.zca_rounds_away.argtypes = [ctypes.c_double, ctypes.c_double]
    L.zca_grid_ok.argtypes = [DP, ctypes.c_int]
    return L


@pytest.fixture(scope="module")
def dlib():
    return HD.load_lib()


def run(L, g, c2, mode, truncate=0, defect=0):
    """(raw F, F, checksum of the node values, plan = [path, k2, kend, dead lanes, nodes executed])."""
    c2 = np.ascontiguousarray(np.asarray(c2, float).reshape(-1, 64))
    raw, F, V = np.empty_like(c2), np.empty_like(c2), np.empty(c2.shape, np.uint64)
    plan = np.empty((c2.shape[0], 5), np.int32)
    g4, om = np.ascontiguousarray(g.g4), np.ascontiguousarray(g.om)
    rc = L.zca_passes(int(mode), int(defect), int(truncate), g4.ctypes.data_as(DP), om.ctypes.data_as(DP), g.nz,
                      c2.ctypes.data_as(DP), c2.shape[0], raw.ctypes.data_as(DP), F.ctypes.data_as(DP),
                      V.ctypes.data_as(UP), plan.ctypes.data_as(IP))
    assert rc == 0
    return raw, F, V, plan


def nodes(L, c2N, g4):
    """(=0 node, new node, t) at the arguments (c2N[i], g4[i])."""
    c2N, g4 = np.broadcast_arrays(np.asarray(c2N, float), np.asarray(g4, float))
    c2N, g4 = np.ascontiguousarray(c2N.ravel()), np.ascontiguousarray(g4.ravel())
    v = np.empty((3, g4.size))
    assert L.zca_nodes(c2N.ctypes.data_as(DP), g4.ctypes.data_as(DP), g4.size, v.ctypes.data_as(DP)) == 0
    return v


def same(a, b):
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
            and np.array_equal(a[2], b[2]) and np.array_equal(a[3][:, 4], b[3][:, 4]))


def three(L, g, c2, truncate):
    """SEG's result after checking it against NEW (raw F, F, node checksum, executed nodes: node by node) and
    against OLD (raw F and F: the bits the parent returns)."""
    seg, new, old = (run(L, g, c2, m, truncate) for m in (SEG, NEW, OLD))
    assert np.array_equal(bits(seg[0]), bits(new[0])) and np.array_equal(bits(seg[1]), bits(new[1])), "F: SEG / NEW"
    assert np.array_equal(seg[2], new[2]), "node values: SEG / NEW"
    assert np.array_equal(seg[3], new[3]), "plan: SEG / NEW"
    assert np.array_equal(bits(new[0]), bits(old[0])) and np.array_equal(bits(new[1]), bits(old[1])), "F: NEW / OLD"
    assert np.array_equal(seg[3][:, 4], seg[3][:, 2])          # every node up to kend is executed
    return seg


def scan_k2(L, live, gp, kend):
    """Brute force over ALL executed nodes: the first batch start from which every live lane's t is <= M + KMIN;
    kend if there is none.  Also checks that 'clamped' is monotone in k for every lane."""
    tclamp = L.zca_tclamp()
    ok = np.ones(kend, bool)
    for c in np.unique(live):
        f = nodes(L, c, gp[:kend])[2] <= tclamp
        assert np.all(np.diff(f.astype(int)) >= 0), c
        ok &= f
    starts = np.flatnonzero(ok[::8] & np.array([ok[i:].all() for i in range(0, kend, 8)])) * 8
    return int(starts[0]) if starts.size else kend


def clamped_lanes(dlib, g, n, deep=False):
    """n live lanes that clamp inside the pass (tests/test_zsum_mixed_host.py's)."""
    _, c_free, c_live, _ = HD.thresholds(dlib, g)
    return -np.geomspace(abs(c_live) * 0.9 if deep else abs(c_free) * 1.001, abs(c_live), n)


def lane_clamping_at(L, g, k):
    """A c2N whose t first reaches M + KMIN at node k of the padded grid (None if no double does)."""
    gp = padded(g)
    c = (L.zca_kmin() - 0.75) / gp[k]
    for _ in range(64):
        f = nodes(L, c, gp)[2] <= L.zca_tclamp()
        first = int(np.argmax(f)) if f.any() else gp.size
        if first == k:
            return c
        c = float(np.nextafter(c, -np.inf if first > k else 0.0))
    return None


# ---- one lane: the new node and the new general loop against the =0 ones --------------------------------------
def test_vc_is_one_number(lib):
    vc = lib.zca_vc()
    assert vc == lib.zca_vc_from_table()                                   # the host's one entry is the table's
    assert 2.0 ** -995 < vc < 2.0 ** -993                                  # C (A^2 + beta) 2^(-1506 + 512), C (A^2 + beta) ~ 1


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_node_at_the_onset_far_below_and_beyond_2p51(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    gp = padded(g)
    kmin, tclamp, vc = lib.zca_kmin(), lib.zca_tclamp(), lib.zca_vc()
    gs = gp[[1, gp.size // 2, g.nz - 1]]
    cs, gg = [], []
    for gk in gs:
        for u in (kmin + 1.5, kmin + 0.5, kmin, kmin - 0.5, kmin - 1.5, 10.0 * kmin, -2.0 ** 51, -2.0 ** 52,
                  -2.0 ** 60, -2.0 ** 199):
            c = u / gk
            for _ in range(3):
                c = float(np.nextafter(c, 0.0))
            for _ in range(7):                                            # three doubles either side of u / g
                cs.append(c), gg.append(gk)
                c = float(np.nextafter(c, -np.inf))
    old, new, t = nodes(lib, cs, gg)
    clamped = t <= tclamp
    assert clamped.any() and (~clamped).any()
    assert np.any(t == tclamp) and np.any(t == tclamp + 1.0) and np.any(t == tclamp - 1.0)   # the onset itself
    assert np.array_equal(bits(new[~clamped]), bits(old[~clamped]))       # above the clamp: the parent's bits
    assert np.all(new[clamped] == vc)                                     # at and below it: the one value
    assert np.any(old[clamped] != vc)                                     # (the parent's stray fraction)
    # both stand-ins stay normal and of the clamped entry's size, also where the reduction is meaningless
    assert np.all(np.isfinite(old)) and np.all(old[clamped] > 0.0)


@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_general_loop_F_is_the_parents(lib, dlib, nz, z_max):
    """One-lane sums over the whole grid from every regime, and from the onset node with F entering the clamped
    stretch as +0, subnormal and normal: NEW = OLD bit for bit, and the stretch leaves F as it entered."""
    g = Z.grid(nz, z_max)
    gp = padded(g)
    oms = np.concatenate([np.ldexp(g.om, -512), np.zeros(gp.size - g.nz)])
    c_zero, c_free, c_live, c_dead = HD.thresholds(dlib, g)
    lanes = np.concatenate([clamped_lanes(dlib, g, 24), clamped_lanes(dlib, g, 24, deep=True),
                            [c_free, float(np.nextafter(c_free, -np.inf)), c_live, c_zero]])
    P = lambda a: np.ascontiguousarray(a).ctypes.data_as(DP)
    entered = set()
    for c in lanes:
        c = float(c)
        F_old = lib.zca_lane(OLD, c, P(gp), P(oms), gp.size, 0.0)
        F_new = lib.zca_lane(NEW, c, P(gp), P(oms), gp.size, 0.0)
        assert bits(F_old) == bits(F_new), c
        f = nodes(lib, c, gp)[2] <= lib.zca_tclamp()
        if not f.any():
            continue
        k = int(np.argmax(f))
        natural = lib.zca_lane(NEW, c, P(gp), P(oms), k, 0.0)              # F as the lane itself enters the stretch
        for F0 in (natural, 0.0, 5e-324, 2.0 ** -1060, 2.0 ** -1022, float(np.nextafter(2.0 ** -1022, 0.0)), 1e-300, 1.0):
            got = [lib.zca_lane(m, c, P(gp[k:]), P(oms[k:]), gp.size - k, F0) for m in (OLD, NEW)]
            assert bits(got[0]) == bits(got[1]) == bits(F0), (c, k, F0)
        entered.add("zero" if natural == 0.0 else "subnormal" if natural < 2.0 ** -1022 else "normal")
    assert "normal" in entered
    print(f"({nz}, {z_max}): F enters the clamped stretch as {sorted(entered)} on the lanes themselves")


# ---- the segmented dispatch against the new general loop -----------------------------------------------------
def masks():
    out = {"uniform": np.zeros(64, bool)}
    for d in (1, 32, 63):
        m = np.zeros(64, bool)
        m[np.linspace(5, 58, d).round().astype(int) if d < 63 else np.arange(64) != 40] = True
        out[f"d{d}"] = m
    return out


def wave(dlib, g, where, deep=False, last=None):
    """64 lanes: dead at the mask, clamped elsewhere; `last`: the c2N of the live lane that clamps last."""
    c_dead = HD.thresholds(dlib, g)[3]
    lanes = np.empty(64)
    lanes[where] = HD.dead_lanes(c_dead)[:int(where.sum())]
    live = clamped_lanes(dlib, g, int((~where).sum()), deep)
    if last is not None:
        live = -np.geomspace(abs(last), abs(live[-1]), live.size)
    lanes[~where] = live
    return lanes


@pytest.mark.parametrize("deep", [False, True])
@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("mix", list(masks()))
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_dispatch_is_the_new_general_loop(lib, dlib, nz, z_max, mix, truncate, deep):
    g = Z.grid(nz, z_max)
    where = masks()[mix]
    lanes = wave(dlib, g, where, deep)
    raw, F, V, plan = three(lib, g, lanes, truncate)
    path, k2, kend, ndead, executed = plan[0].tolist()
    assert path == (MIXED if where.any() else SPLIT) and ndead == int(where.sum())
    assert np.all(F[0, where] == 0.0) and not np.any(np.signbit(F[0, where]))
    assert np.array_equal(bits(F[0, ~where]), bits(raw[0, ~where]))
    if where.any():    # what the zeroing hides: a dead lane summed omega'_k T''[0] (A^2 + beta) over the executed nodes
        assert np.all(raw[0, where] > 0.0) and len(set(bits(raw[0, where]).tolist())) == 1
    assert kend % 8 == 0 and k2 % 8 == 0 and k2 == scan_k2(lib, lanes[~where], padded(g), kend)
    if truncate and kend < padded(g).size:
        assert k2 == kend                                        # -1080 octaves comes before -1506: no suffix
    if deep and not truncate:
        assert k2 < kend
    print(f"({nz}, {z_max}) {mix} truncate={truncate}: k2 = {k2} of {kend}")


@pytest.mark.parametrize("mix", ["uniform", "d32"])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_k2_at_the_first_batch_mid_grid_and_the_end(lib, dlib, nz, z_max, mix):
    """k2 = 8, mid-grid, kend - 8 and kend on the dense pass, placed with the lane that clamps last.  Where
    gamma4 has saturated (the last batches of the z_max = 30 grids move u by less than one unit) no lane clamps
    first inside them; the (29, 6) grid reaches kend - 8, and kend where the last lane clamps past the last
    batch start."""
    g = Z.grid(nz, z_max)
    gp = padded(g)
    kend = gp.size
    where = masks()[mix]
    hit = {}
    for name, k in (("first", 8), ("mid", kend // 2 // 8 * 8), ("end-8", kend - 8), ("end", min(kend - 5, g.nz - 1))):
        c = lane_clamping_at(lib, g, k)
        if c is None:
            continue
        lanes = wave(dlib, g, where, last=c)
        raw, F, V, plan = three(lib, g, lanes, 0)
        if plan[0, 0] not in (SPLIT, MIXED):
            continue
        assert plan[0, 1] == scan_k2(lib, lanes[~where], gp, kend)
        hit[name] = int(plan[0, 1])
    print(f"({nz}, {z_max}) {mix}: k2 = {hit} of {kend}")
    if kend >= 16:
        assert hit.get("first") == 8
    if nz >= 1200:
        assert hit.get("mid") == kend // 2 // 8 * 8
    if (nz, z_max) == (29, 6.0):
        assert hit.get("mid") == 16 and hit.get("end-8") == 24 and hit.get("end") == 32


@pytest.mark.parametrize("truncate", [0, 1])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_controls_keep_their_plan(lib, dlib, nz, z_max, truncate):
    """All-dead, zero and clamp-free waves (with and without dead lanes) never take the clamped branch."""
    g = Z.grid(nz, z_max)
    c_zero, c_free, c_live, c_dead = HD.thresholds(dlib, g)
    assert three(lib, g, HD.dead_lanes(c_dead), truncate)[3][0, 0] == DEAD
    for live, path in ((-np.geomspace(abs(c_zero) * 4.0, abs(c_free), 32), FREE),
                       (-np.geomspace(abs(c_zero) * 1e-30, abs(c_zero), 32), ZERO)):
        lanes = HD.dead_lanes(c_dead)
        lanes[0::2] = live
        assert three(lib, g, lanes, truncate)[3][0, 0] == path
        assert three(lib, g, np.resize(live, 64), truncate)[3][0, 0] == path


@pytest.mark.parametrize("mix", ["uniform", "d32"])
@pytest.mark.parametrize("nz,z_max", GRIDS)
def test_seeded_defects_are_caught(lib, dlib, nz, z_max, mix):
    g = Z.grid(nz, z_max)
    where = masks()[mix]
    lanes = wave(dlib, g, where, deep=True)
    good = run(lib, g, lanes, SEG)
    assert same(good, run(lib, g, lanes, NEW))
    k2, kend = int(good[3][0, 1]), int(good[3][0, 2])
    assert 0 < k2 < kend
    # a wrong v_c (the =0 node's value at k2, stray fraction and all): every live lane's node values differ
    bad = run(lib, g, lanes, SEG, defect=WRONG_VC)
    assert not same(bad, good) and not np.any(bad[2][0, ~where] == good[2][0, ~where])
    assert np.array_equal(bad[2][0, where], good[2][0, where])
    # the suffix a batch early: the lane that clamps last has not clamped there
    bad = run(lib, g, lanes, SEG, defect=BATCH_EARLY)
    assert not same(bad, good) and not np.array_equal(bad[2][0, ~where], good[2][0, ~where])
    # a lost node: one node fewer is executed, in every lane
    bad = run(lib, g, lanes, SEG, defect=LOST_NODE)
    assert not same(bad, good) and bad[3][0, 4] == good[3][0, 4] - 1 and not np.any(bad[2][0] == good[2][0])
    # ... none of which F's rounding can show on its own: the reason the checksum and the count are compared
    assert np.array_equal(bits(bad[1]), bits(good[1]))


def test_c2_plan_suffix_count(lib):
    """The C2 workload on the default grid: passes 72..93 take the clamped branch, k2 from 184 down to 8, and
    25,664 of the point's 150,000 nodes (17.1%) are the suffix that is now F's accumulate alone."""
    import test_zsum_group_host as HG
    g = Z.grid(1200, 30.0)
    seg = three(lib, g, HG.c2_points(), 0)
    plan = seg[3]
    branch = np.flatnonzero((plan[:, 0] == SPLIT) | (plan[:, 0] == MIXED))
    clamped = branch[plan[branch, 1] < 1200]                    # the passes with a suffix
    k2 = plan[clamped, 1]
    suffix, prefix = int((1200 - k2).sum()), int(plan[branch, 1].sum())
    print(f"C2 plan: passes {branch.tolist()} take the clamped branch, k2 = {plan[branch, 1].tolist()}; {suffix} suffix "
          f"nodes ({suffix / 150000:.1%}) accumulate-only, {prefix} nodes in the general clamped loop")
    assert clamped.tolist() == list(range(72, 94)) and np.flatnonzero(plan[:, 0] == MIXED).tolist() == [93]
    assert k2.max() == 184 and k2.min() == 8 and np.all(np.diff(k2) <= 0)
    assert suffix == 25664 and abs(suffix / 150000 - 0.171) < 0.0005


# ---- the condition, and the switch -----------------------------------------------------------------------------
@pytest.mark.parametrize("nz,z_max", GRIDS + ((12000, 30.0), (5, 7.5)))
def test_the_bound_holds_on_every_grid(lib, nz, z_max):
    g = Z.grid(nz, z_max)
    om = np.ascontiguousarray(g.om)
    assert lib.zca_grid_ok(om.ctypes.data_as(DP), om.size) == 1
    vc = lib.zca_vc()
    import mpmath as mp
    worst = max(mp.mpf(float(x)) * mp.mpf(2) ** -512 * mp.mpf(vc) for x in om)
    assert worst < mp.mpf(2) ** -1075
    print(f"({nz}, {z_max}): max omega' v_c = 2^{float(mp.log(worst, 2)):.1f}")


def test_the_bound_is_a_real_condition(lib):
    vc = lib.zca_vc()
    assert lib.zca_rounds_away(0.0, vc) == 1 and lib.zca_rounds_away(2.0 ** -518, vc) == 1
    assert lib.zca_rounds_away(2.0 ** -82, vc) == 1                       # 2^-82 * 2^-994 < 2^-1075
    assert lib.zca_rounds_away(2.0 ** -80, vc) == 0 and lib.zca_rounds_away(1.0, vc) == 0
    assert lib.zca_rounds_away(float("nan"), vc) == 0 and lib.zca_rounds_away(float("inf"), vc) == 0
    assert lib.zca_rounds_away(-1.0, vc) == 0
    om = np.full(8, 2.0 ** 440)                                            # weights no z grid has
    assert lib.zca_grid_ok(om.ctypes.data_as(DP), 8) == 0


def test_continuum_and_runtime_grids_pass_the_library_check():
    """The library's own builders (lzq_ztables / the continuum table) accept their grids with the check in."""
    nat = pkg("_native")
    for nz, z_max in ((1200, 30.0), (13, 3.0), (2400, 30.0)):
        assert len(nat.ztables(nz, z_max)[2]) == nz


def test_clamp_arg_off_is_the_parent_machine_code(tmp_path):
    """-DLZQ_CLAMP_ARG=0 compiles the headline kernels to the ISA the parent's profile was taken on."""
    b, codeobj = pkg("build"), pkg("codeobj")
    out = str(tmp_path / "lzq_kernels_off.so")
    subprocess.run([b.hipcc(), *b.FLAGS, "-DLZQ_CLAMP_ARG=0", "-I", b.INCLUDE, os.path.join(b.CSRC, "lzq_kernels.hip"),
                    "-o", out], check=True)
    got = codeobj.kernel_isa_sha256(out)
    assert got is not None, "llvm-objdump (ROCm) is needed to disassemble the code object"
    with open(os.path.join(ROOT, "profiles", "round15", "parent_pmc_summary.json")) as f:
        want = json.load(f)["kernel_isa_sha256"]
    assert want == "92d7dbd6174569273faf82154ddf3378c9547a5ce8d5067cba3526c928eceeb3"   # the parent's, pinned
    assert got == want


def test_headline_kernels_keep_registers_and_occupancy():
    """tools/kernel_resources.py: every yields_* and window quadrature kernel at 64 VGPRs or fewer and 8
    waves/SIMD, and the spill bytes of the dense ones where the =0 build has them."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    for src in ("lzq_kernels.hip", "lzq_window.hip"):
        new = {r["kernel"]: r for r in kr.resources(src, [])}
        off = {r["kernel"]: r for r in kr.resources(src, ["-DLZQ_CLAMP_ARG=0"])}
        rows = [k for k in new if "yields_" in k or "window_kernel" in k]
        assert rows and set(new) == set(off)
        for k in rows:
            assert int(new[k]["VGPRs"]) <= 64 and int(new[k]["Occupancy [waves/SIMD]"]) == 8, new[k]
            assert int(new[k]["ScratchSize [bytes/lane]"]) <= int(off[k]["ScratchSize [bytes/lane]"]), (new[k], off[k])
