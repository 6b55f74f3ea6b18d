"""The clamped pass that holds dead lanes (csrc/lzq_quad.h zsum_dispatch's last branch, zsum_uniform_lane,
LZQ_PASS_LEAN) on the device.  Needs an MI355X.

A wave with dead lanes (c2 g4_1 <= -1077 octaves) among clamped ones runs the clamped general loop up to
the batch at which every live lane is clamped, and the rest through the uniform node with the entry held
per lane: T''[0] for a dead lane, the entry of M + KMIN for the others.  Every y must get the bits it gets
in a wave that cannot take that path.

Engine.aov puts 64 consecutive y into one wavefront.  The waves here, per grid:

  clamped   the control: 64 clamped y from the clamp onset to just below the dead threshold (no dead lane:
            the wave-uniform entry, as before);
  dead      the control: 64 dead y (the all-dead loop);
  mixed d   d = 1, 32 and 63 dead lanes spread over the wave, the other lanes clamped; each lane carries
            the y the control wave of its kind has in that lane.

A clamped lane of a mixed wave must have the bits of that y in the all-clamped wave, and a dead lane the
+0 of the all-dead wave.  What a dead lane sums before the zeroing cannot be seen from here;
tests/test_zsum_mixed_host.py pins it on the CPU against the general loop, with k2 and the broken variants.

Engine.aov is always dense; the truncated mixed passes go through the grid kernel, truncated against
dense on 256 points whose y-grids cross the dead threshold inside a pass.
"""
import numpy as np
import pytest

import zsum_ref as Z
from conftest import BASE_CFG, full_cfg

pytestmark = pytest.mark.gpu
I_P = BASE_CFG["I_p"]
GRIDS = ((1200, 30.0), (13, 3.0), (2400, 30.0))
DEAD_COUNTS = (1, 32, 63)
AXES = [("I_p", np.geomspace(0.05, 2.0, 8)), ("beta_over_H", np.geomspace(20.0, 500.0, 8)),
        ("T_min_over_Tp", np.array([1e-3, 0.5, 0.9, 0.97]))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def is_pos_zero(a):
    return bool(np.all(a == 0.0) and not np.any(np.signbit(a)))


def dead_mask(d):
    m = np.zeros(64, bool)
    m[np.linspace(5, 58, d).round().astype(int) if d < 63 else np.arange(64) != 40] = True
    assert m.sum() == d
    return m


@pytest.mark.parametrize("nz,z_max", GRIDS, ids=[f"{n}-{z}" for n, z in GRIDS])
def test_mixed_waves_equal_their_control_waves(gpu_engine, nz, z_max):
    g = Z.grid(nz, z_max)
    y_clamp, _, y_dead = g.boundaries(I_P)
    assert y_clamp + 0.1 < y_dead and y_dead + 20.0 < 50.0
    clamped = np.linspace(y_clamp + 0.02, y_dead - 0.01, 64)        # every lane clamps inside the pass, none is dead
    dead = np.linspace(y_dead + 0.1, y_dead + 20.0, 64)
    ys = [clamped, dead]
    for d in DEAD_COUNTS:
        ys.append(np.where(dead_mask(d), dead, clamped))
    out = gpu_engine.aov(full_cfg(BASE_CFG), [float(y) for w in ys for y in w], nz=nz, z_max=z_max).cpu().numpy()
    assert np.all(np.isfinite(out))
    out = out.reshape(len(ys), 64)
    ctl_clamped, ctl_dead = out[0], out[1]
    assert is_pos_zero(ctl_dead)
    assert np.all(ctl_clamped >= 0.0) and np.any(ctl_clamped > 0.0)
    assert len(set(bits(ctl_clamped).tolist())) > 8                  # the control is no constant
    for d, w in zip(DEAD_COUNTS, out[2:]):
        m = dead_mask(d)
        assert np.array_equal(bits(w[~m]), bits(ctl_clamped[~m])), (d, "a clamped lane differs from its control")
        assert is_pos_zero(w[m]), (d, "a dead lane is not +0")
    print(f"grid ({nz}, {z_max}): y_clamp = {y_clamp:.4f}, y_dead = {y_dead:.4f}; the mixed waves with "
          f"{DEAD_COUNTS} dead lanes equal their control waves bit for bit")


def test_truncated_grid_kernel_equals_dense(gpu_engine):
    """256 points through the grid kernel at n_y = 2000; the y-grids that run to 50 cross the dead threshold
    inside a pass, which is then a mixed one.  Truncated against dense."""
    base = full_cfg(BASE_CFG)
    prev = gpu_engine.tune_truncate(False)
    try:
        dense = gpu_engine.sweep(base, AXES, 0, 256, n_y=2000).cpu().numpy()
        gpu_engine.tune_truncate(True)
        trunc = gpu_engine.sweep(base, AXES, 0, 256, n_y=2000).cpu().numpy()
    finally:
        gpu_engine.tune_truncate(prev)
    assert np.all(np.isfinite(dense[:, 0])) and np.any(dense[:, 0] > 0.0)           # Y_B
    assert np.array_equal(bits(dense), bits(trunc))
