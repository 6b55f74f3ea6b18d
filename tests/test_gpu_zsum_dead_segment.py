"""The all-dead passes of the z-sum with the node's value formed once (csrc/lzq_quad.h zsum_dead,
LZQ_DEAD_SEG; csrc/lzq_exp2.h seg_node_dead) on the device.  Needs an MI355X.

A wave whose 64 lanes are all dead (c2 g4_1 <= -1077 octaves: every node k >= 1 underflows) runs
with c2e = +0.0 in every lane; the device then forms v = T''[0] (A^2 + beta) once and runs F's
accumulate alone at every node, and the lanes are zeroed as before.  One live lane in the wave must
take it off that path, and the live lane must get the bits it gets in any other wave.

Engine.aov puts 64 consecutive y into one wavefront.  The waves here:

  all dead    64 y from y_dead + 0.1 to y_dead + 20: exactly +0 in every lane;
  one live    63 dead lanes and one live lane, at lane 0, 31 and 63, with y = y_zero - 1 (a zero-type
              lane), 0 (clamp-free) and y_dead - 0.5 (clamped): the dead lanes are +0 and the live lane
              has the bits of the same y in a control wave of 64 live lanes;
  straddling  64 y within 1e-3 of y_dead, each evaluated again in control waves that one y = 0 lane
              forces off the dead path whatever the other lanes are: equal bits.

What the dead loop sums before the zeroing cannot be seen from here; tests/test_zsum_dead_segment_host.py
pins it on the CPU, bit for bit against the zero node and the general loop, and the dispatch to the
ulp at the dead threshold.

Engine.aov is always dense; the truncated all-dead passes go through the grid kernel: the shipped
config's y-grid at n_y = 2000 runs from -48 to 50, so its last passes are all-dead, and Y_B with
truncation on must have the bits of the dense one.
"""
import math

import numpy as np
import pytest

import zsum_ref as Z
from conftest import BASE_CFG, full_cfg

pytestmark = pytest.mark.gpu
I_P = BASE_CFG["I_p"]
GRIDS = ((1200, 30.0), (13, 3.0), (2400, 30.0))
LIVE_AT = (0, 31, 63)   # the live lane of a "one live" wave
CTL_LANE = 7            # where the control wave of 64 live lanes carries the y under test
SWAP = (5, 42)          # the lanes replaced by y = 0 in the two control copies of the straddling wave


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def is_pos_zero(a):
    return bool(np.all(a == 0.0) and not np.any(np.signbit(a)))


@pytest.mark.parametrize("nz,z_max", GRIDS, ids=[f"{n}-{z}" for n, z in GRIDS])
def test_dead_waves(gpu_engine, nz, z_max):
    g = Z.grid(nz, z_max)
    k = Z.LOG2E * (I_P / 6.0)
    y_zero = math.log(0.5 / (8192.0 * k * float(g.g4[-1])))          # |c2N| g_max = 1/2
    _, _, y_dead = g.boundaries(I_P)
    assert y_zero < -1.0 and 1.0 < y_dead and y_dead + 20.0 < 50.0
    live_y = {"zero": y_zero - 1.0, "free": 0.0, "clamped": y_dead - 0.5}
    dead = np.linspace(y_dead + 0.1, y_dead + 20.0, 64)
    straddle = np.linspace(y_dead - 1e-3, y_dead + 1e-3, 64)
    ys, where = [], {}

    def add(key, wave):
        assert len(wave) == 64
        where[key] = len(ys)
        ys.extend(float(y) for y in wave)

    add("dead", dead)
    for name, y in live_y.items():
        ctl = np.linspace(-3.0, 3.0, 64)                              # 64 live lanes, clamp-free ones among them
        ctl[CTL_LANE] = y
        add(("ctl", name), ctl)
        for lane in LIVE_AT:
            w = dead.copy()
            w[lane] = y
            add((name, lane), w)
    for swap in (None,) + SWAP:
        w = straddle.copy()
        if swap is not None:
            w[swap] = 0.0
        add(("straddle", swap), w)
    out = gpu_engine.aov(full_cfg(BASE_CFG), ys, nz=nz, z_max=z_max).cpu().numpy()
    assert np.all(np.isfinite(out))
    wave = lambda key: out[where[key]:where[key] + 64]

    assert is_pos_zero(wave("dead"))
    for name in live_y:
        ref = wave(("ctl", name))[CTL_LANE]
        assert ref > 0.0, name
        for lane in LIVE_AT:
            w = wave((name, lane))
            others = np.arange(64) != lane
            assert bits(w[lane:lane + 1])[0] == bits(ref.reshape(1))[0], (name, lane, w[lane], ref)
            assert is_pos_zero(w[others]), (name, lane)
    uni = wave(("straddle", None))
    seen = np.zeros(64, bool)
    for swap in SWAP:
        keep = np.arange(64) != swap
        assert np.array_equal(bits(uni[keep]), bits(wave(("straddle", swap))[keep])), swap
        seen |= keep
    assert seen.all()
    assert is_pos_zero(uni[straddle > y_dead + 1e-6]) and np.all(uni[straddle < y_dead - 1e-6] >= 0.0)
    print(f"grid ({nz}, {z_max}): y_dead = {y_dead:.4f}; dead wave +0, {len(live_y) * len(LIVE_AT)} one-live waves "
          f"and the straddling wave equal their controls bit for bit")


def test_truncated_grid_kernel_equals_dense(gpu_engine):
    """The shipped config through the grid kernel (0 axes, 1 point) at n_y = 2000: y runs from -48 to
    50, so the last passes are all-dead; truncated (kend = 8 there) against dense."""
    prev = gpu_engine.tune_truncate(False)
    try:
        dense = gpu_engine.sweep(full_cfg(BASE_CFG), [], 0, 1, n_y=2000).cpu().numpy()
        gpu_engine.tune_truncate(True)
        trunc = gpu_engine.sweep(full_cfg(BASE_CFG), [], 0, 1, n_y=2000).cpu().numpy()
    finally:
        gpu_engine.tune_truncate(prev)
    assert np.isfinite(dense[0, 0]) and dense[0, 0] > 0.0           # Y_B
    assert np.array_equal(bits(dense), bits(trunc))
