"""The lean per-pass work of the dense y-loop (csrc/lzq_quad.h LZQ_PASS_LEAN: y, e^y and the weight kept
across the loops that have room, the clamps that cannot fire dropped, the interior forms of
csrc/lzq_ynode.h) on the device.  Needs an MI355X.

The table and reuse modes keep the pre- and post-loop code of before (general y_node / y_weight, the
select clamps, everything re-formed after the z-loop) and are the on-device control: reuse=True computes
every F(y_j) in the table mode and integrates in the reuse mode.  The truncated sweep is the second
control: it takes the lean code but never a group, and its passes end elsewhere.  All three are
bit-identical by construction, so a value kept from the wrong pass, an interior form taken on a pass
that touches an end of the grid, or a clamp dropped where it can fire shows as a difference.

256 points: I_p x beta_over_H x T_min_over_Tp as tests/test_gpu_zsum_group.py chooses them.  Among them
are points whose y-grid starts below -50 (beta_over_H > 100 at T_max/T_p = 5: the lower e^y clamp is
active in the first lanes) and points whose y_hi is the cap 50 (the upper one at the last node); the test
asserts both.  n_y = 2000 (31 passes + 16 lanes: a partial last pass), 2048, 2112 (full passes) and 4000
(62 passes + 32 lanes).  A second base with m_chi = 300 GeV puts T < m_chi/3 on the part of every y-grid
with y > 0.1 B (the exp_sc branch of y_factors, which keeps its full clamp).
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


def y_ends(base):
    """(unclipped y_lo, y_hi) of the 256 points of AXES: y(T) = (B/2)((T_p/T)^2 - 1), fpy:234-243."""
    B = np.repeat(AXES[1][1], 4).reshape(1, -1).repeat(8, 0).ravel()
    r_lo = np.tile(AXES[2][1], 64)
    y_of = lambda r: 0.5 * B * ((1.0 / r) ** 2 - 1.0)
    return y_of(base["T_max_over_Tp"]), np.minimum(y_of(r_lo), 50.0)


def dense_and_controls(eng, base, axes, **kw):
    """The dense sweep of the 256 points, after checking it bit for bit against reuse=True and against the
    truncated sweep."""
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
    assert np.array_equal(bits(dense), bits(reuse)), "dense differs from reuse"
    assert np.array_equal(bits(dense), bits(trunc)), "dense differs from truncated"
    return dense


def test_the_points_reach_both_clamps_of_exp_y():
    y_lo, y_hi = y_ends(full_cfg(BASE_CFG))
    assert np.any(y_lo < -50.0) and np.any(y_hi == 50.0) and np.any(y_hi < 50.0) and np.any(y_lo > -50.0)


@pytest.mark.parametrize("n_y", [2000, 2048, 2112, 4000])
def test_lean_dense_equals_reuse_and_truncated(gpu_engine, n_y):
    dense_and_controls(gpu_engine, full_cfg(BASE_CFG), AXES, n_y=n_y)


@pytest.mark.parametrize("nz,z_max", [(13, 3.0), (2400, 30.0)], ids=["13-3.0", "2400-30.0"])
def test_lean_dense_on_runtime_z_grids(gpu_engine, nz, z_max):
    dense_and_controls(gpu_engine, full_cfg(BASE_CFG), AXES, n_y=2000, nz=nz, z_max=z_max)


def test_lean_dense_with_the_nonrelativistic_branch(gpu_engine):
    """m_chi = 300 GeV at T_p = 100 GeV: T = T_p / sqrt(1 + 2y/B) is below m_chi/3 = T_p for y > 0, above it for
    y < 0, so every y-grid that crosses 0 takes both branches of y_factors."""
    base = full_cfg({**BASE_CFG, "m_chi_GeV": 300.0})
    y_lo, y_hi = y_ends(base)
    assert np.any((y_lo < 0.0) & (y_hi > 0.0))
    heavy = dense_and_controls(gpu_engine, base, AXES, n_y=2000)
    light = gpu_engine.sweep(full_cfg(BASE_CFG), AXES, 0, 256, n_y=2000).cpu().numpy()
    assert not np.array_equal(bits(heavy[:, 0]), bits(light[:, 0]))   # the branch is taken: Y_B moves


def test_lean_dense_through_a_window_sweep(gpu_engine):
    """The window kernels take the lean passes through the header (groups of two at most)."""
    dense_and_controls(gpu_engine, full_cfg(BASE_CFG), WINDOW_AXES, n_y=2000,
                       window={"kind": "plateau", "half_width": 3.0})
