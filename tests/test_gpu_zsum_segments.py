"""The uniform-entry segments of the z-sum (csrc/lzq_quad.h zsum_dispatch / zsum_uniform) on the
device: equal y must give equal bits whether its wavefront takes the uniform-entry loop or the
general one.  Needs an MI355X.

Engine.aov puts 64 consecutive y into one wavefront.  A wave whose 64 y all lie below the zero
boundary (|c2N| g_max <= 1/2), or are all dead, runs the whole pass with one table value; a wave
whose y are all clamped runs the nodes from k2 on that way (k2: the first 8-node batch at which
its least negative lane is clamped).  Each such wave is evaluated again with ONE lane replaced by
y = 0 -- a mid-range, clamp-free y: it fails the zero test and never clamps, so the wave runs the
general loop throughout -- twice, with different lanes replaced, so that every y is repeated.  The
values themselves are pinned against mpmath by tests/test_gpu_zsum.py, and the dispatch and the
uniform node against the general loop, bit for bit and at the boundaries to the ulp, by
tests/test_zsum_segments_host.py on the CPU.

Engine.aov is always dense; the truncated passes (LZQ_TUNE_TRUNCATE) go through Engine.yields,
whose y-grid crosses every regime: Y_B with truncation on must have the bits of the dense one.
"""
import math

import numpy as np
import pytest

import zsum_ref as Z
from conftest import BASE_CFG, full_cfg, pkg

pytestmark = pytest.mark.gpu
I_P = BASE_CFG["I_p"]
GRIDS = ((1200, 30.0), (13, 3.0), (2400, 30.0))
SWAP = (5, 42)          # the lanes replaced by y = 0 in the two control copies of a wave


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def waves_of(g):
    """{name: 64 y} of the uniform waves on grid g, from its own tables."""
    k = Z.LOG2E * (I_P / 6.0)
    nzp = (max(g.nz, 8) + 7) // 8 * 8
    g_max = float(g.g4[-1])
    y_zero = math.log(0.5 / (8192.0 * k * g_max))          # |c2N| g_max = 1/2
    y_clamp, _, y_dead = g.boundaries(I_P)
    assert y_zero < -1.0 and 0.0 < y_clamp - 1.0 and y_dead + 3.0 < 50.0
    w = {"below zero": np.linspace(y_zero - 5.0, y_zero - 0.1, 64),
         "straddling zero": np.linspace(y_zero - 0.01, y_zero + 0.01, 64),
         "dead": np.concatenate([np.linspace(y_dead + 0.1, y_dead + 3.0, 62), [50.0, 60.0]])}
    # all clamped: the least negative lane (the smallest y) decides k2.  t = fma(c2N, g, M) is
    # M + round(u), so a lane is clamped at a node iff u = c2N g <= KMIN + 1/2: the smallest y lies
    # midway between the y that clamp at the batch starts kb and kb - 8 (u at kb - 8 misses the
    # bound by >= 1e-3 there, a 1-ulp difference in e^y moves u by 3e-9), which puts k2 at kb: the
    # second batch, mid-grid and the last batch; and midway between the last batch start and the
    # last node, where the pass clamps but no batch start does (k2 = kend, no suffix)
    def y_at(k):
        return math.log((Z.CLAMP_OCT * 8192.0 - 0.5) / (8192.0 * kk * float(g.g4[min(k, g.nz - 1)])))

    kk = k
    for kb in sorted({16, nzp // 16 * 8, nzp - 8} & set(range(8, nzp - 7, 8))) + [nzp]:
        ys = 0.5 * (y_at(kb) + (y_at(kb - 8) if kb > 8 else y_at(kb) + 0.2)) + 0.005 * np.arange(64)   # g4_0 = 0 never clamps
        assert abs(ys[0] - y_clamp) < 20.0 and ys[-1] < y_dead - 0.1, (kb, ys[0], ys[-1])
        w[f"clamped, k2 = {kb}" + (" = kend" if kb == nzp else "")] = ys
    return w, y_dead


@pytest.mark.parametrize("nz,z_max", GRIDS, ids=[f"{n}-{z}" for n, z in GRIDS])
def test_uniform_waves_equal_general_waves(gpu_engine, nz, z_max):
    g = Z.grid(nz, z_max)
    waves, y_dead = waves_of(g)
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
    assert len(at_zero) == 1 and out[where[("dead", SWAP[0])] + SWAP[0]] > 0.0      # y = 0 itself, in every wave
    for name, w in waves.items():
        uni = out[where[(name, None)]:][:64]
        seen = np.zeros(64, bool)
        for swap in SWAP:
            ctl = out[where[(name, swap)]:][:64]
            keep = np.arange(64) != swap
            assert np.array_equal(bits(uni[keep]), bits(ctl[keep])), (name, swap)
            seen |= keep
        assert seen.all()
        if name == "dead":
            assert np.all(uni == 0.0) and not np.any(np.signbit(uni))
        else:
            assert np.all(uni > 0.0), name
        print(f"grid ({nz}, {z_max}) {name}: y in [{w[0]:.3f}, {w[-1]:.3f}], 64 y equal bits in uniform and general waves")


@pytest.mark.parametrize("nz,z_max", GRIDS, ids=[f"{n}-{z}" for n, z in GRIDS])
def test_truncated_passes_equal_dense(gpu_engine, nz, z_max):
    """Y_B of the shipped config (y from -48 to 50: zero, clamp-free, clamped and dead passes) with
    the truncated passes against the dense ones."""
    cfgm = pkg("config")
    pts = cfgm.to_point(full_cfg(BASE_CFG))
    prev = gpu_engine.tune_truncate(False)
    try:
        dense = gpu_engine.yields(pts, n_y=2000, nz=nz, z_max=z_max).cpu().numpy()
        gpu_engine.tune_truncate(True)
        trunc = gpu_engine.yields(pts, n_y=2000, nz=nz, z_max=z_max).cpu().numpy()
    finally:
        gpu_engine.tune_truncate(prev)
    assert np.all(np.isfinite(dense)) and dense[0, 0] > 0.0
    assert np.array_equal(bits(dense), bits(trunc))
