"""The zero stretch of the z-sum without its range reduction (csrc/lzq_quad.h zsum_uniform<YB, true>,
LZQ_ZERO_SEG; csrc/lzq_exp2.h seg_node_zero) on the device.  Needs an MI355X.

A wave whose 64 lanes all have t = fma(c2N, g_max, M) = M -- |c2N| g_max <= 1/2, or dead lanes
running with c2 = 0 -- forms s = fma(c2N, g, A) at every node instead of recomputing t = M and
w = (M + A) - t = A.  tests/test_gpu_zsum_segments.py compares the waves "below zero", "straddling
zero" and "dead" with general-loop controls; here are the two it lacks:

  mixed     dead and below-zero lanes alternating in one wave: the dispatch takes the zero path with
            c2e = 0 on the dead lanes, which are zeroed afterwards;
  at zero   64 y within 1e-3 below the boundary |c2N| g_max = 1/2, where round(u) is still 0 at
            g_max but |u| is as large as the zero path ever sees (s = A + u, |u| up to 1/2).

Engine.aov puts 64 consecutive y into one wavefront.  Each wave is evaluated again with ONE lane
replaced by y = 0 (mid-range and clamp-free: the wave fails the zero test and runs the general
loop), twice with different lanes, so every y is repeated in a general-loop wave; equal y must give
equal bits.  The node and the dispatch are pinned against the general loop on the CPU, to the ulp
at the boundary, by tests/test_zsum_zero_segment_host.py.

Engine.aov is always dense; the truncated zero passes go through the grid kernel: the shipped
config's Y_B at n_y = 2000 with truncation on must have the bits of the dense one.
"""
import math

import numpy as np
import pytest

import zsum_ref as Z
from conftest import BASE_CFG, full_cfg

pytestmark = pytest.mark.gpu
I_P = BASE_CFG["I_p"]
GRIDS = ((1200, 30.0), (13, 3.0), (2400, 30.0))
SWAP = (5, 42)          # the lanes replaced by y = 0 in the two control copies: one dead, one small


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def waves_of(g):
    k = Z.LOG2E * (I_P / 6.0)
    y_zero = math.log(0.5 / (8192.0 * k * float(g.g4[-1])))          # |c2N| g_max = 1/2
    _, _, y_dead = g.boundaries(I_P)
    assert y_zero < -1.0 and y_dead + 3.0 < 50.0
    mixed = np.empty(64)
    mixed[0::2] = np.linspace(y_zero - 5.0, y_zero - 0.1, 32)         # even lanes: round(u) = 0
    mixed[1::2] = np.linspace(y_dead + 0.1, y_dead + 3.0, 32)         # odd lanes: dead
    # 1e-6 below the boundary: a 1-ulp difference in e^y moves u by 1e-16, so every lane passes the zero test
    return {"mixed": mixed, "at zero": np.linspace(y_zero - 1e-3, y_zero - 1e-6, 64)}


@pytest.mark.parametrize("nz,z_max", GRIDS, ids=[f"{n}-{z}" for n, z in GRIDS])
def test_zero_waves_equal_general_waves(gpu_engine, nz, z_max):
    g = Z.grid(nz, z_max)
    waves = waves_of(g)
    ys, where = [], {}
    for name, w in waves.items():
        for swap in (None,) + SWAP:
            v = [float(y) for y in w]
            if swap is not None:
                v[swap] = 0.0
            where[(name, swap)] = len(ys)
            ys += v
    assert len(ys) % 64 == 0
    out = gpu_engine.aov(full_cfg(BASE_CFG), ys, nz=nz, z_max=z_max).cpu().numpy()
    assert np.all(np.isfinite(out))
    at_zero = {int(b) for (name, swap), o in where.items() if swap is not None for b in bits(out[o + swap:o + swap + 1])}
    assert len(at_zero) == 1 and out[where[("mixed", SWAP[0])] + SWAP[0]] > 0.0      # y = 0 itself, in every wave
    for name, w in waves.items():
        uni = out[where[(name, None)]:][:64]
        seen = np.zeros(64, bool)
        for swap in SWAP:
            ctl = out[where[(name, swap)]:][:64]
            keep = np.arange(64) != swap
            assert np.array_equal(bits(uni[keep]), bits(ctl[keep])), (name, swap)
            seen |= keep
        assert seen.all()
        if name == "mixed":
            assert np.all(uni[1::2] == 0.0) and not np.any(np.signbit(uni[1::2])) and np.all(uni[0::2] > 0.0)
        else:
            assert np.all(uni > 0.0), name
        print(f"grid ({nz}, {z_max}) {name}: 64 y equal bits in zero-path and general waves")


def test_truncated_grid_kernel_equals_dense(gpu_engine):
    """The shipped config through the grid kernel (0 axes, 1 point) at n_y = 2000: its y-grid runs
    from -48 to 50, so the first passes are zero passes; truncated against dense."""
    prev = gpu_engine.tune_truncate(False)
    try:
        dense = gpu_engine.sweep(full_cfg(BASE_CFG), [], 0, 1, n_y=2000).cpu().numpy()
        gpu_engine.tune_truncate(True)
        trunc = gpu_engine.sweep(full_cfg(BASE_CFG), [], 0, 1, n_y=2000).cpu().numpy()
    finally:
        gpu_engine.tune_truncate(prev)
    assert np.all(np.isfinite(dense)) and dense[0, 0] > 0.0
    assert np.array_equal(bits(dense), bits(trunc))
