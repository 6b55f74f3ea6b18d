"""The clamped argument of the dense z-sum (csrc/lzq_quad.h zsum<.., CLAMP = true> and zsum_dispatch's clamped
branch, csrc/lzq_exp2.h clamp_arg_s; LZQ_CLAMP_ARG) on the device.  Needs an MI355X.

A node whose magic sum is clamped is evaluated at the clamped argument u = KMIN (s = A), and from the batch at
which the last live lane of a wave clamps the pass runs as F's accumulate alone.  The stand-in value of an
underflowed node changes; F cannot, because either stand-in's term is below half the smallest subnormal.  The
control is the library built with -DLZQ_CLAMP_ARG=0 (the parent's machine code; __graft_entry__.build() puts it
beside the default one, as `tools/build_variants.py LZQ_CLAMP_ARG=0` does): the two are loaded into one process
and must return equal bits.

  * A/V at 192 y on the three grids: a wavefront straddling the clamp onset, one mixing clamp-free, clamped and
    dead lanes, one mixing clamped and dead lanes (the per-lane suffix).  Equal bits, and both within
    tests/zsum_ref.py's tolerance of the 60-digit sum.
  * 8 grid points at the smallest n_y the ABI accepts: dense against the control library, against the truncated
    sweep and against the shared z-sums (reuse=True), equal bits.

Which path a wave took cannot be seen from here; that these paths are taken is shown by the host plan
(tests/test_zsum_clamp_arg_host.py, the same predicates) and by the time and PMC record (profiles/round15).
"""
import os

import numpy as np
import pytest

import zsum_ref as Z
from conftest import BASE_CFG, full_cfg, pkg

pytestmark = pytest.mark.gpu
I_P = BASE_CFG["I_p"]
GRIDS = [(1200, 30.0), (13, 3.0), (2400, 30.0)]
IDS = ["1200-30.0", "13-3.0", "2400-30.0"]
AXES8 = [("I_p", np.geomspace(0.05, 2.0, 4)), ("beta_over_H", np.array([50.0, 200.0]))]
NY_MIN = Z.NY_MIN


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def off_engine(gpu_engine):
    """The engine on the -DLZQ_CLAMP_ARG=0 library, built with the default one (never on the GPU box)."""
    b = pkg("build")
    lib = os.path.join(b.BUILD_DIR, "variants", "liblzq_clamp_arg0.so")
    want = b.inputs_hash({"LZQ_CLAMP_ARG": "0"})
    try:
        with open(b.stamp_path(lib)) as f:
            stamp = f.read().strip()
    except OSError:
        stamp = None
    if not os.path.exists(lib) or stamp != want:
        pytest.fail(f"{lib} is not the -DLZQ_CLAMP_ARG=0 build of these sources; run __graft_entry__.build()",
                    pytrace=False)
    return pkg("engine").Engine(lib_path=lib)


def wave_ys(g):
    """Three wavefronts of 64 y: across the clamp onset; clamp-free, clamped and dead lanes in turn; clamped and
    dead lanes in turn."""
    y_clamp, _, y_dead = g.boundaries(I_P)
    onset = np.linspace(y_clamp - 0.5, y_clamp + 0.5, 64)
    free = np.linspace(y_clamp - 3.0, y_clamp - 0.1, 22)
    clamped = np.linspace(y_clamp + 0.1, y_dead - 0.05, 43)
    dead = np.linspace(y_dead + 0.01, min(y_dead + 3.0, 49.0), 63)
    three = np.empty(64)
    three[0::3], three[1::3], three[2::3] = free, clamped[:21], dead[:21]
    two = np.empty(64)
    two[0::2], two[1::2] = clamped[21:43].repeat(2)[:32] + np.tile([0.0, 1e-3], 16), dead[21:53]
    return [float(y) for y in np.concatenate([onset, three, two])]


@pytest.mark.parametrize("nz,z_max", GRIDS, ids=IDS)
def test_aov_equals_the_control_library_and_the_reference(gpu_engine, off_engine, nz, z_max):
    g = Z.grid(nz, z_max)
    kernel = full_cfg(BASE_CFG)
    ys = wave_ys(g)
    assert len(ys) == 192
    new = gpu_engine.aov(kernel, ys, nz=nz, z_max=z_max).cpu().numpy()
    off = off_engine.aov(kernel, ys, nz=nz, z_max=z_max).cpu().numpy()
    items = Z.av_ref(kernel, ys, g)
    acc = Z.accumulation([r for _, r, _ in items])
    for name, got in (("default", new), ("LZQ_CLAMP_ARG=0", off)):
        worst, ratio, bad = Z.compare(got, items, "table", acc)
        print(f"A/V vs mp, {name} [({nz}, {z_max})]: {len(ys)} y, worst rel err {worst:.3e}, worst err/tol {ratio:.3f}")
        assert not bad, (name, bad[:4])
    assert np.array_equal(bits(new), bits(off)), "the default library differs from the LZQ_CLAMP_ARG=0 one"
    assert np.all(new[:64] > 0.0) and len(set(bits(new).tolist())) >= 96


@pytest.mark.parametrize("nz,z_max", GRIDS, ids=IDS)
def test_eight_grid_points_dense_control_truncated_and_reuse(gpu_engine, off_engine, nz, z_max):
    base = full_cfg(BASE_CFG)
    kw = dict(n_y=NY_MIN, nz=nz, z_max=z_max)
    prev = gpu_engine.tune_truncate(False)
    prev_off = off_engine.tune_truncate(False)
    try:
        dense = gpu_engine.sweep(base, AXES8, 0, 8, **kw).cpu().numpy()
        reuse = gpu_engine.sweep(base, AXES8, 0, 8, reuse=True, **kw).cpu().numpy()
        off = off_engine.sweep(base, AXES8, 0, 8, **kw).cpu().numpy()
        gpu_engine.tune_truncate(True)
        trunc = gpu_engine.sweep(base, AXES8, 0, 8, **kw).cpu().numpy()
    finally:
        gpu_engine.tune_truncate(prev)
        off_engine.tune_truncate(prev_off)
    assert dense.shape[0] == 8 and np.all(np.isfinite(dense)) and np.all(dense[:, 0] > 0.0)
    assert len(set(bits(dense[:, 0]).tolist())) >= 4             # (beta_over_H hardly moves Y_B on the coarse grid)
    assert np.array_equal(bits(dense), bits(off)), "dense differs from the LZQ_CLAMP_ARG=0 library"
    assert np.array_equal(bits(dense), bits(trunc)), "dense differs from truncated"
    assert np.array_equal(bits(dense), bits(reuse)), "dense differs from the shared z-sums"
