"""The accumulate-only z-loops fed from the packed omega' array of the z grid's device image
(csrc/lzq_quad.h acc_omega in zsum_dead / zsum_held, single and grouped; LZQ_ACC_FEED) on the device.  Needs
an MI355X.

Only the dense, untruncated passes and the A/V kernels read the packed array.  The truncated passes and
reuse=True (the table mode) run the same loops on the nodes' own weights and are the controls: both are
bit-identical to the dense sweep by construction of the single pass, so a packed array that is not the nodes'
weights bit for bit -- a producer that did not write it, wrote it elsewhere, or padded it otherwise -- or a
loop that reads it from the wrong node shows as a difference.  The three producers are the default grid's
(whose exp table follows the array), a runtime grid's and the continuum grid's.  Which path a wave took
cannot be seen from here; that these paths are taken is shown by the host plan
(tests/test_zsum_feed_host.py, the same predicates) and by the time and PMC record (profiles/round13).

The 256 points and the y-counts are tests/test_gpu_zsum_group.py's: frozen runs, tails, dead runs, and the
end of the y-grid at every place in a group.
"""
import numpy as np
import pytest

import zsum_ref as Z
from conftest import BASE_CFG, full_cfg
from test_gpu_cont import skip_form
from test_gpu_zsum_group import AXES, WINDOW_AXES, bits, dense_and_controls

pytestmark = pytest.mark.gpu
I_P = BASE_CFG["I_p"]


@pytest.mark.parametrize("nz,z_max", [(1200, 30.0), (13, 3.0), (2400, 30.0)], ids=["1200-30.0", "13-3.0", "2400-30.0"])
@pytest.mark.parametrize("n_y", [2000, 2048, 2112, 4000])
def test_fed_dense_equals_truncated_and_reuse(gpu_engine, n_y, nz, z_max):
    dense_and_controls(gpu_engine, AXES, n_y=n_y, nz=nz, z_max=z_max)


@pytest.mark.parametrize("nz,z_max", [(1200, 30.0), (13, 3.0), (2400, 30.0)], ids=["1200-30.0", "13-3.0", "2400-30.0"])
def test_fed_dense_through_a_window_sweep(gpu_engine, nz, z_max):
    dense_and_controls(gpu_engine, WINDOW_AXES, n_y=2000, nz=nz, z_max=z_max,
                       window={"kind": "plateau", "half_width": 3.0})


def wave_ys():
    """Whole wavefronts of 64 y each: cold ones (zero passes: whole-frozen, then with a held tail), a mixed one,
    and hot ones up to the clip (dead lanes where the grid has them)."""
    return [float(y) for lo, hi in [(-50.0, -38.0), (-37.0, -24.0), (-23.0, -12.0), (-11.0, 20.0), (30.0, 42.0),
                                    (44.0, 50.0)] for y in np.linspace(lo, hi, 64)]


@pytest.mark.parametrize("nz,z_max", [(13, 3.0), (2400, 30.0)], ids=["13-3.0", "2400-30.0"])
def test_runtime_grid_aov_vs_mp(gpu_engine, nz, z_max):
    """Engine.aov on a runtime grid, whose cold wavefronts run zsum_held and whose all-dead ones zsum_dead on the
    packed array zgrid_for uploads, against the 60-digit reference within zsum_ref.tol (exact zeros where it
    demands them)."""
    g = Z.grid(nz, z_max)
    kernel = full_cfg(BASE_CFG)
    ys = wave_ys()
    items = Z.av_ref(kernel, ys, g)
    acc = Z.accumulation([r for _, r, _ in items])
    got = gpu_engine.aov(kernel, ys, nz=nz, z_max=z_max).cpu().numpy()
    worst, ratio, bad = Z.compare(got, items, "table", acc)
    print(f"A/V vs mp, packed feed [({nz}, {z_max})]: {len(ys)} y, worst rel err {worst:.3e}, worst err/tol {ratio:.3f}")
    assert not bad, bad[:4]
    assert np.all(got[:192] > 0.0)


def test_continuum_grid_aov_fed_equals_live_range(gpu_engine):
    """Engine.aov(continuum=True) at every node (the packed array cont_grid_for uploads) against its live-range
    form (truncated: the nodes' own weights), bit for bit."""
    kernel = full_cfg(BASE_CFG)
    ys = wave_ys()
    with skip_form(gpu_engine, True):
        live = gpu_engine.aov(kernel, ys, continuum=True).cpu().numpy()
    with skip_form(gpu_engine, False):
        every = gpu_engine.aov(kernel, ys, continuum=True).cpu().numpy()
    assert np.all(every > 0.0) and len(set(bits(every).tolist())) >= 300
    assert np.array_equal(bits(every), bits(live))
