"""The frozen tails of the z-sum (csrc/lzq_quad.h zsum_held / zsum_frozen_t, LZQ_FROZEN_SEG) on the
device.  Needs an MI355X.

From the batch at which every lane of a wave holds the s (zero pass) or t (clamp-free pass) it has
at the last executed node, the device forms what depends on that value once per lane and runs the
rest of the node.  Which path a wave took cannot be seen from here, so every y of a wave that takes
a frozen path is evaluated again in control waves that one extra lane takes off it, and the bits
must be equal:

  above zero  a y 0.3 above the zero boundary (|c2N| g_max = 0.675): the wave is no zero pass any
              more, which defeats frozen s (it runs the clamp-free loop, and t's own tail);
  moving t    a mid-range lane whose t changes between the last batch start and the last node
              (|u| at g_max just beyond 1e6 + 1/2, chosen in the middle of the window the last batch
              leaves, 1e5 x wider than the device's rounding of c2): the wave is clamp-free without a
              tail, i.e. the general loop node by node, which defeats frozen s and frozen t.

Engine.aov puts 64 consecutive y into one wavefront.  The waves, per grid (the lanes of
tests/test_zsum_frozen_host.py, which plans them with the library's own predicates on the CPU and pins
k3 against a scan of all nodes):

  whole     |c2N| g_max from 2^-57 to 2^-43, far below half an ulp of A: s = A at every node, k3 = 0;
  zero tail |c2N| g_max from 1e-9 to 1e-4: s freezes inside the pass;
  free tail |c2N| g_max from 2 to 2000: t freezes inside the pass
  (on the 16-node grid the two tails are the waves that change once, between nodes 7 and 8).

Engine.aov is always dense; the truncated passes go through the grid kernel, on a few hundred points
whose y-grids cross every regime: truncated against dense, bit for bit.
"""
import numpy as np
import pytest

import zsum_ref as Z
from conftest import BASE_CFG, full_cfg

pytestmark = pytest.mark.gpu
I_P = BASE_CFG["I_p"]
GRIDS = ((1200, 30.0), (13, 3.0), (2400, 30.0))
SWAP = (5, 42)          # the lanes replaced by the defeating y in the two control copies of a wave
N = 8192.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def y_of_x(g, x):
    """y at which |c2N| g_max = x."""
    return np.log(np.asarray(x, float) / (N * Z.LOG2E * (I_P / 6.0) * float(g.g4[-1])))


def moving_t_y(g):
    """y of a clamp-free lane whose t = M + round(u) differs between node nzp - 8 and the last node."""
    nzp = (max(g.nz, 8) + 7) // 8 * 8
    gp = np.concatenate([g.g4, np.full(nzp - g.nz, g.g4[-1])]).astype(np.longdouble)
    w = float((gp[-1] - gp[nzp - 8]) / gp[-1])                   # the window the last batch leaves, relative
    assert w > 1e-11
    n = 1e6 if g.nz > 13 else 3.0
    x = (n + 0.5) * (1.0 + min(0.5 * w, 0.1))                    # |u| at g_max: mid-window beyond the boundary
    y = float(y_of_x(g, x))
    for eps in (-1e-13, 0.0, 1e-13):                             # whatever the device's last bits of c2 are
        c = -np.longdouble(x * (1.0 + eps)) / gp[-1]
        assert np.rint(c * gp[nzp - 8]) != np.rint(c * gp[-1])
    assert x < 1506.0 * N                                        # clamp-free
    return y


@pytest.mark.parametrize("nz,z_max", GRIDS, ids=[f"{n}-{z}" for n, z in GRIDS])
def test_frozen_waves_equal_their_controls(gpu_engine, nz, z_max):
    g = Z.grid(nz, z_max)
    y_above = float(y_of_x(g, 0.5)) + 0.3
    y_move = moving_t_y(g)
    if nz == 13:
        tails = {"zero tail": y_of_x(g, np.geomspace(1.25, 1.45, 64) * 2.0 ** -39),
                 "free tail": y_of_x(g, np.geomspace(1.25, 1.45, 64))}
    else:
        tails = {"zero tail": y_of_x(g, np.geomspace(1e-9, 1e-4, 64)),
                 "free tail": y_of_x(g, np.geomspace(2.0, 2000.0, 64))}
    waves = {"whole": y_of_x(g, np.geomspace(2.0 ** -57, 2.0 ** -43, 64)), **tails}
    controls = {"whole": {"above zero": y_above, "moving t": y_move},
                "zero tail": {"above zero": y_above, "moving t": y_move},
                "free tail": {"moving t": y_move}}
    ys, where = [], {}

    def add(key, wave):
        assert len(wave) == 64 and np.all(np.abs(wave) < 50.0)
        where[key] = len(ys)
        ys.extend(float(y) for y in wave)

    for name, wave in waves.items():
        add(name, wave)
        for ctl, y in controls[name].items():
            for swap in SWAP:
                w = wave.copy()
                w[swap] = y
                add((name, ctl, swap), w)
    out = gpu_engine.aov(full_cfg(BASE_CFG), ys, nz=nz, z_max=z_max).cpu().numpy()
    assert np.all(np.isfinite(out)) and np.all(out > 0.0)
    take = lambda key: out[where[key]:where[key] + 64]
    n = 0
    for name in waves:
        got = take(name)
        for ctl in controls[name]:
            seen = np.zeros(64, bool)
            for swap in SWAP:
                keep = np.arange(64) != swap
                assert np.array_equal(bits(got[keep]), bits(take((name, ctl, swap))[keep])), (name, ctl, swap)
                seen |= keep
                n += 1
            assert seen.all()
    # the defeating lanes themselves: one y, one value, whatever wave carries it
    for ctl, lanes in (("above zero", ("whole", "zero tail")), ("moving t", ("whole", "zero tail", "free tail"))):
        vals = {int(bits(take((name, ctl, swap))[swap:swap + 1])[0]) for name in lanes for swap in SWAP}
        assert len(vals) == 1, ctl
    print(f"grid ({nz}, {z_max}): {len(waves)} frozen waves equal their {n} control waves bit for bit")


def test_truncated_grid_kernel_equals_dense(gpu_engine):
    """256 points of the shipped config over I_p x beta_over_H through the grid kernel at n_y = 2000 (the
    y-grid runs from the whole-frozen zero passes to the all-dead ones): truncated against dense."""
    axes = [("I_p", np.geomspace(0.05, 2.0, 16)), ("beta_over_H", np.geomspace(20.0, 500.0, 16))]
    prev = gpu_engine.tune_truncate(False)
    try:
        dense = gpu_engine.sweep(full_cfg(BASE_CFG), axes, 0, 256, n_y=2000).cpu().numpy()
        gpu_engine.tune_truncate(True)
        trunc = gpu_engine.sweep(full_cfg(BASE_CFG), axes, 0, 256, n_y=2000).cpu().numpy()
    finally:
        gpu_engine.tune_truncate(prev)
    assert np.all(np.isfinite(dense[:, 0])) and np.all(dense[:, 0] >= 0.0) and np.any(dense[:, 0] > 0.0)   # Y_B
    # the sweep is no single point repeated: the 16 I_p values give 16 different Y_B at least (Y_B saturates
    # in beta_over_H, so not all 256 differ)
    assert len(set(bits(dense[:, 0]).tolist())) >= 16
    assert np.array_equal(bits(dense), bits(trunc))
