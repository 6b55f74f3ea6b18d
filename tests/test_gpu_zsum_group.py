"""Grouped passes of the dense z-sum (csrc/lzq_quad.h yb_group, LZQ_GROUP_SEG) on the device.  Needs an
MI355X.

The dense yb_wave sweeps runs of accumulate-only passes (whole-frozen zero passes at the cold end of
the y-grid, all-dead passes at the hot end) through z four or two at a time.  Two paths through the
same library cannot group and are the controls: the truncated passes (grouping is off under truncation)
and reuse=True (the table mode computes every pass singly, the reuse mode integrates from its table).
Both are bit-identical to the dense sweep by construction of the single pass, so a group that summed a
chain in another order, zeroed the wrong lane, took a pass it should not have, or integrated the passes
out of order shows as a difference.  Which path a wave took cannot be seen from here; that the groups
are taken is shown by the host plan (tests/test_zsum_group_host.py, the same predicates) and by the
time and PMC record (profiles/round11).

256 points: I_p x beta_over_H as in tests/test_gpu_zsum_frozen.py, crossed with T_min_over_Tp so that
the y-grids of some points end before the dead range (T_min/T_p = 0.97: y_hi <= 16) while small
beta_over_H leaves others without a frozen run (beta_over_H = 20: y_lo = -9.6).  The y-counts put the
end of the grid at every place in a group: 2000 (31 passes + 16 lanes), 2048 (32 passes), 2112 (33)
and 4000 (62 passes + 32 lanes).
"""
import numpy as np
import pytest

from conftest import BASE_CFG, full_cfg

pytestmark = pytest.mark.gpu
AXES = [("I_p", np.geomspace(0.05, 2.0, 8)), ("beta_over_H", np.geomspace(20.0, 500.0, 8)),
        ("T_min_over_Tp", np.array([1e-3, 0.5, 0.9, 0.97]))]
WINDOW_AXES = [("I_p", np.geomspace(0.05, 2.0, 8)), ("beta_over_H", np.geomspace(20.0, 500.0, 8)),
               ("window_y0", np.array([-40.0, -6.0, 8.0, 30.0]))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dense_and_controls(eng, axes, **kw):
    """The dense sweep of the 256 points, after checking it bit for bit against the truncated sweep and
    against reuse=True."""
    base = full_cfg(BASE_CFG)
    prev = eng.tune_truncate(False)
    try:
        dense = eng.sweep(base, axes, 0, 256, **kw).cpu().numpy()
        reuse = eng.sweep(base, axes, 0, 256, reuse=True, **kw).cpu().numpy()
        eng.tune_truncate(True)
        trunc = eng.sweep(base, axes, 0, 256, **kw).cpu().numpy()
    finally:
        eng.tune_truncate(prev)
    assert dense.shape[0] == 256
    assert np.all(np.isfinite(dense[:, 0])) and np.all(dense[:, 0] >= 0.0) and np.any(dense[:, 0] > 0.0)   # Y_B
    assert len(set(bits(dense[:, 0]).tolist())) >= 32             # no single point repeated
    assert np.array_equal(bits(dense), bits(trunc)), "dense differs from truncated"
    assert np.array_equal(bits(dense), bits(reuse)), "dense differs from reuse"
    return dense


@pytest.mark.parametrize("n_y", [2000, 2048, 2112, 4000])
def test_grouped_dense_equals_truncated_and_reuse(gpu_engine, n_y):
    dense_and_controls(gpu_engine, AXES, n_y=n_y)


@pytest.mark.parametrize("nz,z_max", [(13, 3.0), (2400, 30.0)], ids=["13-3.0", "2400-30.0"])
def test_grouped_dense_on_runtime_z_grids(gpu_engine, nz, z_max):
    dense_and_controls(gpu_engine, AXES, n_y=2000, nz=nz, z_max=z_max)


def test_grouped_dense_through_a_window_sweep(gpu_engine):
    """The window kernels take the groups through the header (two passes at most)."""
    dense_and_controls(gpu_engine, WINDOW_AXES, n_y=2000, window={"kind": "plateau", "half_width": 3.0})
