"""The A/V z-sum kernels (csrc/lzq_quad.h zsum / zsum_dispatch, the exponential of
csrc/lzq_exp2.h) against the mpmath reference of tests/zsum_ref.py, at their edges.  Needs an MI355X.

Every other GPU comparison of A/V or Y_B is FP64 against FP64 at 1e-10 .. 1e-12; the kernel's own
error budget (the table form's 1.73e-14 minimax bound plus rounding) sits three to four decades
below that.  Here the device sums are compared with a 60-digit sum over the very doubles the device
holds (_native.ztables), within the tolerance derived in zsum_ref.py, on y sets that sample every
regime change densely: the +-50 clip, clamp onset, the saturation of poly11's integer conversion,
the dead-lane threshold and the band where A/V is subnormal -- all computed per grid from the
tables.  tests/test_zsum_host.py shows on the CPU that correct arithmetic stays inside this
tolerance and that eight defects of the kind this code could have are rejected by it.

The dense yields kernels are tested bit-identical to the reuse mode, whose tables are these F
values (test_gpu_sweep.py), so pinning F and A/V pins the headline path.
"""
import ctypes
import math

import mpmath as mp
import numpy as np
import pytest
import torch

import zsum_ref as Z
from conftest import BASE_CFG, full_cfg, pkg

pytestmark = pytest.mark.gpu
I_P = BASE_CFG["I_p"]
NY_MIN = Z.NY_MIN
HDR = 6        # LZQ_REUSE_TABLE_HEADER


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class tuned:
    """Engine tune state for a block, restored on exit."""

    def __init__(self, eng, exp=None, truncate=None, wide=None):
        self.eng, self.exp, self.truncate, self.wide = eng, exp, truncate, wide

    def __enter__(self):
        self.prev = {}
        try:
            if self.exp is not None:
                self.prev["exp"] = self.eng.tune_exp(self.exp)
            if self.truncate is not None:
                self.prev["truncate"] = self.eng.tune_truncate(self.truncate)
            if self.wide is not None:
                self.prev["wide"] = self.eng.tune_ode_table_wide(self.wide)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        if "wide" in self.prev:
            self.eng.tune_ode_table_wide(self.prev["wide"])
        if "truncate" in self.prev:
            self.eng.tune_truncate(self.prev["truncate"])
        if "exp" in self.prev:
            self.eng.tune_exp(self.prev["exp"])
        return False


# ---------------------------------------------------------------------------------------------
# A/V against the reference
# ---------------------------------------------------------------------------------------------
AOV_CASES = [(v, g, None) for v in Z.VARIANTS for g in Z.GRIDS] + [("table", Z.GRIDS[0], 0.0)]


@pytest.mark.parametrize("variant,grid,v_w", AOV_CASES,
                         ids=[f"{v}-{g[0]}-{g[1]}" + ("" if w is None else "-vw0") for v, g, w in AOV_CASES])
def test_aov_vs_mp(gpu_engine, variant, grid, v_w):
    """Engine.aov of the shipped kernel (v_w = 0: the 1e-12 floor of fpy:146) against av_ref within
    zsum_ref.tol, exact zeros where the reference demands them (y > 50, F below half a subnormal).

    Measured on an MI355X (worst relative error over the normal-range results, worst error /
    tolerance): see README "Parity"."""
    nz, z_max = grid
    g = Z.grid(nz, z_max)
    kernel = full_cfg(BASE_CFG) if v_w is None else {**full_cfg(BASE_CFG), "v_w": v_w}
    ys = Z.y_set(g, I_P, Z.density_of(nz))
    items = Z.av_ref(kernel, ys, g)
    acc = Z.accumulation([r for _, r, _ in items])
    with tuned(gpu_engine, exp=variant):
        got = gpu_engine.aov(kernel, ys, nz=nz, z_max=z_max).cpu().numpy()
    worst, ratio, bad = Z.compare(got, items, variant, acc)
    print(f"A/V vs mp [{variant}, ({nz}, {z_max})" + ("" if v_w is None else ", v_w = 0") + f"]: {len(ys)} y, "
          f"accumulation {acc:.2e}, worst rel err {worst:.3e}, worst err/tol {ratio:.3f}")
    assert not bad, bad[:4]
    zeros = [x for x, y in zip(got, ys) if y > 50.0]
    assert len(zeros) == 2 and all(x == 0.0 for x in zeros)
    sub = [x for x in got if 0.0 < x < 2.0 ** -1022]
    assert sub, "the y set misses the subnormal band"


# ---------------------------------------------------------------------------------------------
# A/V of a y is a pure function of y
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", Z.VARIANTS)
def test_wave_composition_bit_identical(gpu_engine, variant):
    """aov_kernel puts 64 consecutive y into one wavefront, and zsum_dispatch picks the clamp-free
    instantiation per wave (__all(small)), zeroes dead lanes after running them with c2 = 0, and
    runs tail lanes on y = 0.  Equal y must give equal bits whatever shares its wave."""
    g = Z.grid(1200, 30.0)
    y_clamp, _, y_dead = g.boundaries(I_P)
    # clamp-free; clamped and live; live with node 1 at -990 octaves (77 short of dead); dead
    y_free, y_cl, y_near, y_gone = y_clamp - 1.0, y_dead - 1.0, y_dead + math.log(990.0 / Z.DEAD_OCT), y_dead + 1.0
    palette = [y_free, y_cl, y_near, y_gone, -60.0, 50.0, 60.0, y_clamp + 0.01, 0.0, y_dead - 0.05,
               math.nextafter(y_dead, -math.inf), y_dead]

    def wave(fill):
        w = [fill] * 64
        for lane in (0, 17, 63):
            w[lane] = y_free
        return w

    dead_but_one = [y_gone] * 64
    dead_but_one[5] = y_cl
    batches = {
        "free x 64": [y_free] * 64,                                           # (i) clamp-free instantiation
        "free among clamped / near-dead / dead": wave(y_cl) + wave(y_near) + wave(y_gone),   # (ii)
        "clamped alone": [y_cl],                                              # (iii) tail lanes run y = 0
        "clamped among dead": dead_but_one,
        # (iv) 1024 + 64 + 37 values: a second block and a ragged last wave
        "two blocks, ragged": (wave(y_cl) + wave(y_gone) + [palette[i % len(palette)] for i in range(1125 - 128)]),
    }
    assert len(batches["two blocks, ragged"]) % 64 != 0 and len(batches["two blocks, ragged"]) > 1024
    seen = {}
    with tuned(gpu_engine, exp=variant):
        for name, ys in batches.items():
            out = gpu_engine.aov(full_cfg(BASE_CFG), ys).cpu().numpy()
            for y, b in zip(ys, bits(out)):
                seen.setdefault(y, {}).setdefault(int(b), []).append(name)
    for y, pats in seen.items():
        assert len(pats) == 1, (variant, y, {hex(b): sorted(set(n)) for b, n in pats.items()})
    val = {y: np.int64(next(iter(p))).view(np.float64) for y, p in seen.items()}
    assert val[y_free] > 0 and val[y_cl] > 0 and val[y_near] > 0 and val[y_gone] == 0.0 and val[60.0] == 0.0


# ---------------------------------------------------------------------------------------------
# the F tables of the reuse mode
# ---------------------------------------------------------------------------------------------
FT_CFG = {**BASE_CFG, **Z.FT_WINDOW}
FT_AXES = [("m_chi_GeV", np.logspace(-1, 3, 64))]   # not a field of the z-sums: ONE table, 64 points


class FTable:
    """lzq_sweep_grid_ztables / _from_ztables / lzq_sweep_grid through the raw ABI on cfg x axes at n_y nodes
    (FT_CFG x FT_AXES at LZQ_NY_MIN unless given; tests/test_gpu_yquad.py reads its cases' F from it)."""

    def __init__(self, eng, nz, z_max, cfg=None, axes=None, n_y=NY_MIN):
        nat, cfgm = pkg("_native"), pkg("config")
        axes = FT_AXES if axes is None else axes
        self.eng, self.nat, self.nz, self.z_max, self.n_y, self.axes = eng, nat, nz, z_max, n_y, axes
        self.base = cfgm.to_ctypes_point(cfgm.to_point(full_cfg(FT_CFG if cfg is None else cfg)))
        self.vals = [torch.as_tensor(np.asarray(v, dtype=np.float64), device=eng.device) for _, v in axes]
        self.arr = (nat.LzqAxis * len(axes))()
        for a, ((name, _), t) in enumerate(zip(axes, self.vals)):
            self.arr[a].field, self.arr[a].n, self.arr[a].values = nat.FIELD[name], t.numel(), t.data_ptr()
        self.need = eng.lib.lzq_sweep_grid_reuse_workspace(self.arr, len(axes), n_y)
        assert self.need == n_y + HDR               # one table
        self.n = len(axes[0][1])

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.eng.device).cuda_stream)

    def table(self):
        work = torch.full((self.need,), float("nan"), dtype=torch.float64, device=self.eng.device)
        with torch.cuda.device(self.eng.device):
            self.nat.check(self.eng.lib.lzq_sweep_grid_ztables(ctypes.byref(self.base), self.arr, len(self.axes), self.n_y,
                                                               self.nz, self.z_max, ctypes.c_void_p(work.data_ptr()),
                                                               self.need, self.stream()), self.eng.lib)
        return work

    def from_table(self, work):
        out = torch.empty((self.n, 6), dtype=torch.float64, device=self.eng.device)
        with torch.cuda.device(self.eng.device):
            self.nat.check(self.eng.lib.lzq_sweep_grid_from_ztables(
                ctypes.byref(self.base), self.arr, len(self.axes), 0, self.n, self.n_y, self.nz, self.z_max, None,
                ctypes.c_void_p(work.data_ptr()), self.need, ctypes.c_void_p(out.data_ptr()), self.stream()),
                self.eng.lib)
        return out.cpu().numpy()

    def dense(self):
        out = torch.empty((self.n, 6), dtype=torch.float64, device=self.eng.device)
        with torch.cuda.device(self.eng.device):
            self.nat.check(self.eng.lib.lzq_sweep_grid(ctypes.byref(self.base), self.arr, len(self.axes), 0, self.n, self.n_y,
                                                       self.nz, self.z_max, None, ctypes.c_void_p(out.data_ptr()),
                                                       self.stream()), self.eng.lib)
        return out.cpu().numpy()


@pytest.mark.parametrize("variant", Z.VARIANTS)
@pytest.mark.parametrize("grid", [(1200, 30.0), (13, 3.0)], ids=["1200-30.0", "13-3.0"])
def test_ftable_vs_mp_and_truncation(gpu_engine, variant, grid):
    """The F values themselves, on a y-grid from the -80 clip to the +50 clip (2000 nodes, step
    0.065): each of the 32 passes of 64 lanes has its own truncation end, and the passes cross every
    regime.  (1) header = the numpy restatement; (2) F_j against f_ref(c(y_j)) at every 16th node
    and every node of the three transition zones; (3) the table built under tune_truncate(True) has
    the bits of the one built without.  NOTE on (3): lzq_sweep_grid_ztables truncates on every
    monotone grid whatever LZQ_TUNE_TRUNCATE says, so today both builds run the truncated passes;
    the truncated-against-dense comparison on the device is test_ftable_feeds_identical_yields
    (lzq_sweep_grid is dense by default) and test_ode_knots_vs_mp (Engine.aov is always dense),
    per value in the model of tests/test_zsum_host.py."""
    nz, z_max = grid
    g = Z.grid(nz, z_max)
    ft = FTable(gpu_engine, nz, z_max)
    with tuned(gpu_engine, exp=variant, truncate=False):
        t0 = ft.table().cpu().numpy()
        with tuned(gpu_engine, truncate=True):
            t1 = ft.table().cpu().numpy()
    y_lo, y_hi, cneg, ys = Z.ft_ygrid(FT_CFG)
    assert (y_lo, y_hi) == (-80.0, 50.0)
    assert list(t0[:HDR]) == [y_lo, y_hi, float(NY_MIN), cneg, float(nz), z_max]
    F = t0[HDR:]
    assert F.size == NY_MIN and np.all(np.isfinite(F)) and np.all(F >= 0.0)
    _, _, y_dead = g.boundaries(I_P)
    idx = Z.ft_pick(g, I_P, ys)
    refs = Z.refs_for(g, I_P, [float(y) for y in ys[idx]])
    acc = Z.accumulation(refs)
    worst, ratio, bad = Z.compare(F[idx], Z.f_items(refs), variant, acc)
    print(f"F table vs mp [{variant}, ({nz}, {z_max})]: {idx.size} of {NY_MIN} nodes, accumulation {acc:.2e}, "
          f"worst rel err {worst:.3e}, worst err/tol {ratio:.3f}")
    assert not bad, bad[:4]
    assert F[0] > 0 and F[-1] == 0.0 and np.all(F[ys > y_dead + 1e-9] == 0.0)
    assert np.array_equal(bits(t0), bits(t1))


@pytest.mark.parametrize("variant", Z.VARIANTS)
def test_ftable_feeds_identical_yields(gpu_engine, variant):
    """The link from F to the headline kernel at the window of the test above: 64 points integrated
    from the (truncated) table have the bits of lzq_sweep_grid on the same points, dense
    (LZQ_TUNE_TRUNCATE off, the default) and truncated."""
    ft = FTable(gpu_engine, 1200, 30.0)
    with tuned(gpu_engine, exp=variant, truncate=False):
        reuse = ft.from_table(ft.table())
        dense = ft.dense()
        with tuned(gpu_engine, truncate=True):
            trunc = ft.dense()
    assert np.all(np.isfinite(reuse)) and np.all(reuse[:, 0] > 0.0)
    assert np.array_equal(bits(reuse), bits(dense))
    assert np.array_equal(bits(trunc), bits(dense))


# ---------------------------------------------------------------------------------------------
# the ODE tables' A/V knots: the production user of the truncation
# ---------------------------------------------------------------------------------------------
ODE_CFG = {**BASE_CFG, **Z.ODE_WINDOW}
ODE_NT = Z.ODE_NT


def ode_knots(eng, wide):
    cfgm = pkg("config")
    with tuned(eng, wide=wide):
        work, status = eng.ode_tables(cfgm.to_point(full_cfg(ODE_CFG)), nt=ODE_NT)
    assert int(status[0].item()) == 0
    w = work.cpu().numpy()
    assert w.size == 4 * ODE_NT
    # csrc/lzq_internal.h: row k = the cubic of interval k, its c3 = A/V at knot k; the last knot's
    # value in the workspace's last double
    knots = np.concatenate([w[3:4 * (ODE_NT - 1):4], w[-1:]])
    # lzq_ode_aov_T at a knot's own T evaluates its cubic at s = 0: the stored value exactly (the
    # last knot is read through the cubic of the interval before it, so it is not compared)
    c = full_cfg(ODE_CFG)
    Ts = Z.ode_knot_y(c)[0]
    at_T = eng.ode_aov_T(cfgm.to_point(c), Ts[0], Ts[-1], work, Ts[:-1], nt=ODE_NT).cpu().numpy()
    assert np.array_equal(bits(at_T), bits(knots[:-1]))
    return knots


@pytest.mark.parametrize("variant", Z.VARIANTS)
def test_ode_knots_vs_mp(gpu_engine, variant):
    """ode_aov_table_kernel always truncates and runs in both LZQ_TUNE_ODE_TABLE_WIDE shapes: A/V at
    the 200 knots against av_ref with y(T) of fpy:126-128 in mpmath from the knot T, the two shapes
    bit-identical, and bit-identical to the dense Engine.aov at the same y."""
    c = full_cfg(ODE_CFG)
    Tp, B = c["T_p_GeV"], c["beta_over_H"]
    Ts, q, ys = Z.ode_knot_y(c)
    g = Z.grid(1200, 30.0)
    _, _, y_dead = g.boundaries(I_P)
    assert ys.min() < y_dead - 2 and ys.max() > y_dead + 2
    with tuned(gpu_engine, exp=variant):
        narrow = ode_knots(gpu_engine, 0)
        wide = ode_knots(gpu_engine, 3)
        dense = gpu_engine.aov(c, ys).cpu().numpy()
    assert np.array_equal(bits(narrow), bits(wide))
    assert np.array_equal(bits(narrow), bits(dense))
    with mp.workdps(Z.DPS):
        y_mp = [mp.mpf(B) / 2 * ((mp.mpf(Tp) / mp.mpf(float(T))) ** 2 - 1) for T in Ts]
    items = Z.av_ref(c, y_mp, g)
    acc = Z.accumulation([r for _, r, _ in items])
    # |dy| (1 + S): the device's T (two roundings of linspace) and y (quotient, square, difference,
    # product) against the exact y of the knot: d(q^2)/q^2 <= 7 u, then u |q^2 - 1| and u |y|
    dy = (0.5 * B * 7.0 * q * q + 2.0 * np.abs(ys)) * Z.U
    extra = [float(d) * (1.0 + r.S) for d, (_, r, _) in zip(dy, items)]
    worst, ratio, bad = Z.compare(narrow, items, variant, acc, extra_rel=extra)
    print(f"ODE knots vs mp [{variant}]: {ODE_NT} knots, y {ys.min():.2f} .. {ys.max():.2f}, accumulation {acc:.2e}, "
          f"worst rel err {worst:.3e}, worst err/tol {ratio:.3f}")
    assert not bad, bad[:4]
    assert (narrow == 0.0).any() and (narrow > 0.0).any()
