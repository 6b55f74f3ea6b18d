// lzq_window.hip -- the quadrature kernels whose source activity window W(y) is a per-point block
// (include/lzq.h lzq_window; PAPER §10 step 4: the Gaussian proxy of fpy:262 replaced by a plateau
// family or a tabulated profile), W(y) alone, and the window's host build.  Two forms of each
// quadrature kernel: explicit records (points and blocks in device arrays), and the grid form, where
// the point (grid_point) and its block (lzq_window.h window_grid_block: the base block with the
// window axes' values) are decoded from the flat grid index in the kernel.
//
// The kernels are the headline ones (lzq_quad.h: same setup, same z-sum, same y-loop, same
// butterfly, same epilogue) with the window factor of y_factors taken from the block parked in the
// wave's LDS slot.  The per-y work stays after the z-loop, so nothing new is live across it.  They
// live in their own translation unit so the headline code object (lzq_kernels.hip, whose rocprof
// PMC profile the bench's roofline is tied to by hash) is unchanged by them.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#define LZQ_QUAD_CONST_LINKAGE static
#include "lzq_quad.h"
#include "lzq_internal.h"
#include "lzq_quad_window.h"  // window_W, WinWaveSlot, SlotWindow, park_window, win_table_of
#include "lzq_window.h"

namespace lzq {

// lzq_yields_batch_window: yields_points_kernel (lzq_kernels.hip) with the window of win[idx]
template <int YB, int EXPV, int NZ>
__global__ __launch_bounds__(kBlock, LZQ_MIN_WAVES) void yields_points_window_kernel(
    const lzq_point* __restrict__ pts, const lzq_window* __restrict__ win, lzq_window_tables wt, int64_t n,
    int32_t n_y, const double* __restrict__ T_lo, const double* __restrict__ T_hi, const double* __restrict__ Pov,
    const ZNode* __restrict__ zt, int32_t nzp, const double* __restrict__ gtab, lzq_yield* __restrict__ out,
    int truncate) {
  __shared__ double lds_tab[kTabN];
  const double* tab = stage_table<EXPV>(gtab, lds_tab);
  __shared__ WinWaveSlot slots[kWavesPerBlock];
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t idx = (int64_t)blockIdx.x * kWavesPerBlock + w;
  if (idx >= n) return;  // wave-uniform
  {
    const lzq_point pt = pts[idx];
    const double P = Pov ? Pov[idx] : pt.P_chi_to_B;
    const double tlo = T_lo ? T_lo[idx] : pt.T_min_over_Tp * pt.T_p_GeV;  // fpy:369
    const double thi = T_hi ? T_hi[idx] : pt.T_max_over_Tp * pt.T_p_GeV;  // fpy:368
    park_window(slots[w], quad_setup(pt, P, tlo, thi, n_y), epilogue_pre(pt, P),
                window_params(win[idx], wt.n_tables, wt.n_knots, wt.u, wt.W), lane);
  }
  const double Y_B = yb_wave<YB, EXPV, kYbDense, NZ, SlotWindow>(slots, w, zt, nzp, tab, truncate);
  if (lane == 0) out[idx] = epilogue_finish(slots[w].e, Y_B);
}

// lzq_yields_batch_reuse_window: points_reuse_kernel (lzq_kernels.hip) with the window of win[idx];
// the tables are points_ztable_kernel's (header: y grid, c and z grid, LZQ_REUSE_TABLE_HEADER doubles)
__global__ __launch_bounds__(kBlock, LZQ_REUSE_MIN_WAVES) void points_reuse_window_kernel(
    const lzq_point* __restrict__ pts, const lzq_window* __restrict__ win, lzq_window_tables wt, int64_t n,
    int32_t n_y, const double* __restrict__ Pov, double key_nz, double key_z_max, const int32_t* __restrict__ tidx,
    const double* __restrict__ Fw, int64_t tstride, lzq_yield* __restrict__ out) {
  __shared__ WinWaveSlot slots[kWavesPerBlock];
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t idx = (int64_t)blockIdx.x * kWavesPerBlock + w;
  if (idx >= n) return;
  const lzq_point pt = pts[idx];
  const double P = Pov ? Pov[idx] : pt.P_chi_to_B;
  const QuadSetup qs = quad_setup(pt, P, pt.T_min_over_Tp * pt.T_p_GeV, pt.T_max_over_Tp * pt.T_p_GeV, n_y);
  const double* F = Fw + (int64_t)tidx[idx] * tstride;
  // match is wave-uniform: every lane formed the same setup
  const bool match = qs.empty || (F[0] == qs.y_lo && F[1] == qs.y_hi && F[2] == (double)qs.n && F[3] == qs.cneg &&
                                  F[4] == key_nz && F[5] == key_z_max);
  park_window(slots[w], qs, epilogue_pre(pt, P), window_params(win[idx], wt.n_tables, wt.n_knots, wt.u, wt.W), lane);
  const double Y_B = match ? yb_wave<kYB, kExpTable, kYbReuse, 0, SlotWindow>(slots, w, nullptr, 0, nullptr, 0,
                                                                                F + LZQ_REUSE_TABLE_HEADER)
                           : 0.0;
  if (lane == 0) {
    lzq_yield o = epilogue_finish(slots[w].e, Y_B);
    if (!match) o.Y_B = o.rho_B_kg_m3 = o.DM_over_B = __builtin_nan("");
    out[idx] = o;
  }
}

// lzq_sweep_grid_window: yields_points_window_kernel with the point (grid_point) and its block
// (window_grid_block) decoded from the flat index start + local, once per wavefront, before the
// z-loop; both end in the wave's slot, so nothing new is live across it.  A block the decode leaves
// unusable (a NaN, sigma <= 0, a table value that is no integer in range, ...) is kWinBad in
// window_params: NaN yields, no table read.
template <int YB, int EXPV, int NZ>
__global__ __launch_bounds__(kBlock, LZQ_MIN_WAVES) void yields_grid_window_kernel(
    lzq_point base, lzq_window base_win, GridSpec grid, lzq_window_tables wt, int64_t start, int64_t count,
    int32_t n_y, const double* __restrict__ Pov, const ZNode* __restrict__ zt, int32_t nzp,
    const double* __restrict__ gtab, lzq_yield* __restrict__ out, int truncate) {
  __shared__ double lds_tab[kTabN];
  const double* tab = stage_table<EXPV>(gtab, lds_tab);
  __shared__ WinWaveSlot slots[kWavesPerBlock];
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t local = (int64_t)blockIdx.x * kWavesPerBlock + w;
  if (local >= count) return;  // wave-uniform
  {
    lzq_point pt;
    const double Pg = grid_point(base, grid, start + local, pt);
    const double P = Pov ? Pov[local] : Pg;
    const lzq_window blk = window_grid_block(base_win, grid, start + local);
    park_window(slots[w], quad_setup(pt, P, pt.T_min_over_Tp * pt.T_p_GeV, pt.T_max_over_Tp * pt.T_p_GeV, n_y),
                epilogue_pre(pt, P), window_params(blk, wt.n_tables, wt.n_knots, wt.u, wt.W), lane);
  }
  // inlined at this call whatever the inliner's budget says after the two decodes: yb_wave keeps its
  // wave index in a scalar register, which only the kernel's own (readfirstlane) w can supply
  double Y_B;
  [[clang::always_inline]] Y_B = yb_wave<YB, EXPV, kYbDense, NZ, SlotWindow>(slots, w, zt, nzp, tab, truncate);
  if (lane == 0) out[local] = epilogue_finish(slots[w].e, Y_B);
}

// lzq_sweep_grid_from_ztables_window: points_reuse_window_kernel with the point, its block and its
// table index decoded from the flat index
__global__ __launch_bounds__(kBlock, LZQ_REUSE_MIN_WAVES) void grid_reuse_window_kernel(
    lzq_point base, lzq_window base_win, GridSpec grid, lzq_window_tables wt, int64_t start, int64_t count,
    int32_t n_y, const double* __restrict__ Pov, double key_nz, double key_z_max, const double* __restrict__ Fw,
    int64_t tstride, lzq_yield* __restrict__ out) {
  __shared__ WinWaveSlot slots[kWavesPerBlock];
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t local = (int64_t)blockIdx.x * kWavesPerBlock + w;
  if (local >= count) return;
  lzq_point pt;
  const double Pg = grid_point(base, grid, start + local, pt);
  const double P = Pov ? Pov[local] : Pg;
  const QuadSetup qs = quad_setup(pt, P, pt.T_min_over_Tp * pt.T_p_GeV, pt.T_max_over_Tp * pt.T_p_GeV, n_y);
  const double* F = Fw + win_table_of(grid, start + local) * tstride;
  // match is wave-uniform: every lane formed the same setup
  const bool match = qs.empty || (F[0] == qs.y_lo && F[1] == qs.y_hi && F[2] == (double)qs.n && F[3] == qs.cneg &&
                                  F[4] == key_nz && F[5] == key_z_max);
  const lzq_window blk = window_grid_block(base_win, grid, start + local);
  park_window(slots[w], qs, epilogue_pre(pt, P), window_params(blk, wt.n_tables, wt.n_knots, wt.u, wt.W), lane);
  double Y_B = 0.0;
  if (match)  // (inlined here, as in the dense kernel)
    [[clang::always_inline]] Y_B = yb_wave<kYB, kExpTable, kYbReuse, 0, SlotWindow>(slots, w, nullptr, 0, nullptr, 0,
                                                                                      F + LZQ_REUSE_TABLE_HEADER);
  if (lane == 0) {
    lzq_yield o = epilogue_finish(slots[w].e, Y_B);
    if (!match) o.Y_B = o.rho_B_kg_m3 = o.DM_over_B = __builtin_nan("");
    out[local] = o;
  }
}

// lzq_window_batch: W(y) of one block, one lane per y
__global__ __launch_bounds__(256) void window_eval_kernel(lzq_window win, lzq_window_tables wt,
                                                          const double* __restrict__ ys, int64_t n,
                                                          double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const WinParams p = window_params(win, wt.n_tables, wt.n_knots, wt.u, wt.W);
  out[i] = window_W(p, p.kind, ys[i]);
}

}  // namespace lzq

namespace {

int win_fail(const char* fmt, long long a = 0, double b = 0.0) {
  char msg[256];
  snprintf(msg, sizeof(msg), fmt, a, b);
  return lzq_set_error(LZQ_EINVAL, msg);
}

const lzq_window_tables kNoTables = {0, 0, nullptr, nullptr};

// the limits of a table set, wherever its arrays live
int check_table_shape(const lzq_window_tables& t, const char* who) {
  char msg[256];
  if (t.n_tables < 0 || t.n_tables > LZQ_WIN_MAX_TABLES) {
    snprintf(msg, sizeof(msg), "%s: n_tables = %d outside [0, %d]", who, t.n_tables, LZQ_WIN_MAX_TABLES);
    return lzq_set_error(LZQ_EINVAL, msg);
  }
  if (t.n_tables > 0 && (t.n_knots < 2 || t.n_knots > LZQ_WIN_MAX_KNOTS)) {
    snprintf(msg, sizeof(msg), "%s: n_knots = %d outside [2, %d]", who, t.n_knots, LZQ_WIN_MAX_KNOTS);
    return lzq_set_error(LZQ_EINVAL, msg);
  }
  if (t.n_tables > 0 && (!t.u || !t.W)) {
    snprintf(msg, sizeof(msg), "%s: %d window tables without their u / W arrays", who, t.n_tables);
    return lzq_set_error(LZQ_EINVAL, msg);
  }
  return LZQ_OK;
}

int check_block(const lzq_window& w, int64_t i, const lzq_window_tables& t) {
  switch (lzq::window_block_error(w, t.n_tables, t.n_knots)) {
    case lzq::kWinOk: return LZQ_OK;
    case lzq::kWinNaN: return win_fail("window %lld: a field is NaN", (long long)i);
    case lzq::kWinSigma:
      return win_fail("window %lld: sigma_lo and sigma_hi must be finite and > 0", (long long)i);
    case lzq::kWinScale: return win_fail("window %lld: scale = %g must be finite and > 0", (long long)i, w.scale);
    case lzq::kWinHalfWidth: return win_fail("window %lld: half_width = %g < 0", (long long)i, w.half_width);
    case lzq::kWinKind: {
      char msg[128];
      snprintf(msg, sizeof(msg), "window %lld: unknown kind %d", (long long)i, w.kind);
      return lzq_set_error(LZQ_EINVAL, msg);
    }
    case lzq::kWinTable: {
      char msg[128];
      snprintf(msg, sizeof(msg), "window %lld: table index %d outside [0, %d)", (long long)i, w.table, t.n_tables);
      return lzq_set_error(LZQ_EINVAL, msg);
    }
    default: return win_fail("window %lld: the table kind needs 2 <= n_knots <= 4096", (long long)i);
  }
}

}  // namespace

extern "C" {

int lzq_window_check_host(const lzq_window* win, int64_t n, const lzq_window_tables* host_tables) {
  if (n < 0 || (n > 0 && !win)) return lzq_set_error(LZQ_EINVAL, "lzq_window_check_host: bad arguments");
  const lzq_window_tables& t = host_tables ? *host_tables : kNoTables;
  int rc = check_table_shape(t, "lzq_window_check_host");
  if (rc) return rc;
  if (t.n_tables > 0) {
    for (int k = 0; k < t.n_knots; ++k) {
      if (!isfinite(t.u[k])) return win_fail("window tables: knot %lld = %g is not finite", k, t.u[k]);
      if (k > 0 && !(t.u[k] > t.u[k - 1])) return win_fail("window tables: knots not strictly ascending at %lld", k);
    }
    for (int64_t j = 0; j < (int64_t)t.n_tables * t.n_knots; ++j)
      if (!(t.W[j] >= 0.0) || !isfinite(t.W[j]))
        return win_fail("window tables: W[%lld] = %g must be finite and >= 0", (long long)j, t.W[j]);
  }
  for (int64_t i = 0; i < n; ++i) {
    rc = check_block(win[i], i, t);
    if (rc) return rc;
  }
  return LZQ_OK;
}

int lzq_window_eval_host(const lzq_window* win, const lzq_window_tables* host_tables, const double* y, int64_t n,
                         double* q_or_v, double* W) {
  if (!win || n < 0 || (n > 0 && !y)) return lzq_set_error(LZQ_EINVAL, "lzq_window_eval_host: bad arguments");
  int rc = lzq_window_check_host(win, 1, host_tables);
  if (rc) return rc;
  const lzq_window_tables& t = host_tables ? *host_tables : kNoTables;
  const lzq::WinParams p = lzq::window_params(*win, t.n_tables, t.n_knots, t.u, t.W);
  for (int64_t i = 0; i < n; ++i) {
    if (p.kind == LZQ_WIN_TABLE) {
      const double v = lzq::window_v(p, y[i]);
      if (q_or_v) q_or_v[i] = v;
      if (W) W[i] = lzq::window_table_W(p, v);
    } else {
      const double q = lzq::window_q(p, p.kind, y[i]);
      if (q_or_v) q_or_v[i] = q;
      if (W) W[i] = exp(-0.5 * (q * q));
    }
  }
  return LZQ_OK;
}

int lzq_window_batch(const lzq_window* win, const lzq_window_tables* d_tables, const double* d_y, int64_t n,
                     double* d_W, void* stream) {
  if (!win || n < 0 || (n > 0 && (!d_y || !d_W))) return lzq_set_error(LZQ_EINVAL, "lzq_window_batch: bad arguments");
  const lzq_window_tables& t = d_tables ? *d_tables : kNoTables;
  int rc = check_table_shape(t, "lzq_window_batch");
  if (rc) return rc;
  rc = check_block(*win, 0, t);
  if (rc) return rc;
  if (n == 0) return LZQ_OK;
  const int64_t nb = (n + 255) / 256;
  if (nb > 2147483647LL) return lzq_set_error(LZQ_EINVAL, "lzq_window_batch: n too large");
  hipLaunchKernelGGL(lzq::window_eval_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, *win, t, d_y, n,
                     d_W);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? LZQ_OK : lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
}

}  // extern "C"

namespace {

// The axes of a host-side window grid call as window_grid_block reads them (C order strides); the
// checks are lzq_sweep_grid's for the parts read here, and window_axes_check.
int host_win_grid(const lzq_axis* axes, int32_t n_axes, const char* who, lzq::HostWinGrid& g, int64_t& total) {
  char msg[256];
  if (n_axes < 0 || n_axes > LZQ_MAX_AXES || (n_axes > 0 && !axes)) {
    snprintf(msg, sizeof(msg), "%s: bad arguments", who);
    return lzq_set_error(LZQ_EINVAL, msg);
  }
  g = lzq::HostWinGrid();
  g.n_axes = n_axes;
  total = 1;
  for (int a = n_axes - 1; a >= 0; --a) {
    const int32_t f = axes[a].field;
    const bool win = lzq::window_field(f);
    if (!(win || (f >= 0 && f <= 14) || f == LZQ_F_DELTA_LZ || f == LZQ_F_M_MIX || f == LZQ_F_DPRIME)) {
      snprintf(msg, sizeof(msg), "%s: axis %d has unknown field %d", who, a, f);
      return lzq_set_error(LZQ_EINVAL, msg);
    }
    if (axes[a].n <= 0 || (win && !axes[a].values)) {
      snprintf(msg, sizeof(msg), "%s: axis %d is empty", who, a);
      return lzq_set_error(LZQ_EINVAL, msg);
    }
    g.field[a] = f;
    g.n[a] = axes[a].n;
    g.values[a] = axes[a].values;
    g.stride[a] = total;
    if (total > INT64_MAX / axes[a].n) {
      snprintf(msg, sizeof(msg), "%s: grid too large", who);
      return lzq_set_error(LZQ_EINVAL, msg);
    }
    total *= axes[a].n;
  }
  return lzq::window_axes_check(axes, n_axes, who);
}

}  // namespace

extern "C" {

int lzq_window_grid_blocks_host(const lzq_window* base_win, const lzq_axis* axes, int32_t n_axes, int64_t start,
                                int64_t count, lzq_window* out_blocks) {
  if (!base_win || start < 0 || count < 0 || (count > 0 && !out_blocks))
    return lzq_set_error(LZQ_EINVAL, "lzq_window_grid_blocks_host: bad arguments");
  lzq::HostWinGrid g;
  int64_t total;
  const int rc = host_win_grid(axes, n_axes, "lzq_window_grid_blocks_host", g, total);
  if (rc) return rc;
  if (start > total || count > total - start) {
    char msg[256];
    snprintf(msg, sizeof(msg), "lzq_window_grid_blocks_host: range [%lld, %lld) outside grid of %lld points",
             (long long)start, (long long)(start + count), (long long)total);
    return lzq_set_error(LZQ_EINVAL, msg);
  }
  for (int64_t i = 0; i < count; ++i) out_blocks[i] = lzq::window_grid_block(*base_win, g, start + i);
  return LZQ_OK;
}

int lzq_window_grid_check_host(const lzq_window* base_win, const lzq_axis* axes, int32_t n_axes,
                               const lzq_window_tables* host_tables) {
  if (!base_win) return lzq_set_error(LZQ_EINVAL, "lzq_window_grid_check_host: bad arguments");
  lzq::HostWinGrid g;
  int64_t total;
  int rc = host_win_grid(axes, n_axes, "lzq_window_grid_check_host", g, total);
  if (rc) return rc;
  rc = lzq_window_check_host(base_win, 1, host_tables);  // the tables and the base block
  if (rc) return rc;
  const lzq_window_tables& t = host_tables ? *host_tables : kNoTables;
  for (int a = 0; a < n_axes; ++a) {
    if (!lzq::window_field(g.field[a])) continue;
    for (int64_t c = 0; c < g.n[a]; ++c) {
      lzq_window w = *base_win;
      const double v = g.values[a][c];
      lzq::window_set_field(w, g.field[a], v);
      char msg[256];
      if (g.field[a] == LZQ_F_WIN_TABLE && w.kind == LZQ_WIN_TABLE && (w.table < 0 || w.table >= t.n_tables)) {
        snprintf(msg, sizeof(msg), "window axis %d (field %d), value %lld = %.17g: not an integer table index in [0, %d)",
                 a, g.field[a], (long long)c, v, t.n_tables);
        return lzq_set_error(LZQ_EINVAL, msg);
      }
      if (check_block(w, 0, t)) {
        // check_block's message is "window 0: <what>"; keep the <what>
        const char* what = lzq_last_error();
        const char* colon = strchr(what, ':');
        char tail[160];
        snprintf(tail, sizeof(tail), "%s", colon ? colon + 2 : what);
        snprintf(msg, sizeof(msg), "window axis %d (field %d), value %lld = %.17g: %s", a, g.field[a], (long long)c, v,
                 tail);
        return lzq_set_error(LZQ_EINVAL, msg);
      }
    }
  }
  return LZQ_OK;
}

}  // extern "C"

int lzq::window_axes_check(const lzq_axis* axes, int32_t n_axes, const char* who) {
  uint32_t seen = 0;
  for (int a = 0; a < n_axes; ++a) {
    const uint32_t m = window_field_mask(axes[a].field);
    if (seen & m) {
      char msg[256];
      snprintf(msg, sizeof(msg), "%s: axis %d (field %d) writes a window field that an earlier axis writes", who, a,
               axes[a].field);
      return lzq_set_error(LZQ_EINVAL, msg);
    }
    seen |= m;
  }
  return LZQ_OK;
}

int lzq::launch_yields_grid_window(int exp_variant, bool default_grid, const lzq_point& base,
                                   const lzq_window& base_win, const GridSpec& grid, const lzq_window_tables& wt,
                                   int64_t start, int64_t count, int32_t n_y, const double* d_P, const ZNode* zt,
                                   int32_t nzp, const double* gtab, lzq_yield* d_out, int truncate, hipStream_t s) {
  const int64_t nb = (count + kWavesPerBlock - 1) / kWavesPerBlock;
#define LZQ_GRID_WIN(EXPV, NZ)                                                                                   \
  hipLaunchKernelGGL((yields_grid_window_kernel<kYB, EXPV, NZ>), dim3((unsigned)nb), dim3(kBlock), 0, s, base,  \
                     base_win, grid, wt, start, count, n_y, d_P, zt, nzp, gtab, d_out, truncate)
  if (exp_variant == kExpTable) {
    if (default_grid) LZQ_GRID_WIN(kExpTable, kNZ);
    else LZQ_GRID_WIN(kExpTable, 0);
  } else {
    if (default_grid) LZQ_GRID_WIN(kExpPoly11, kNZ);
    else LZQ_GRID_WIN(kExpPoly11, 0);
  }
#undef LZQ_GRID_WIN
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? LZQ_OK : lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
}

int lzq::launch_grid_reuse_window(const lzq_point& base, const lzq_window& base_win, const GridSpec& grid,
                                  const lzq_window_tables& wt, int64_t start, int64_t count, int32_t n_y,
                                  const double* d_P, double key_nz, double key_z_max, const double* d_work,
                                  int64_t stride, lzq_yield* d_out, hipStream_t s) {
  const int64_t nb = (count + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(grid_reuse_window_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, base, base_win, grid, wt, start,
                     count, n_y, d_P, key_nz, key_z_max, d_work, stride, d_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? LZQ_OK : lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
}

int lzq::window_tables_arg(const lzq_window_tables* d_tables, const char* who, lzq_window_tables& out) {
  out = d_tables ? *d_tables : kNoTables;
  return check_table_shape(out, who);
}

int lzq::launch_yields_points_window(int exp_variant, bool default_grid, const lzq_point* d_points,
                                     const lzq_window* d_win, const lzq_window_tables& wt, int64_t n, int32_t n_y,
                                     const double* d_T_lo, const double* d_T_hi, const double* d_P, const ZNode* zt,
                                     int32_t nzp, const double* gtab, lzq_yield* d_out, int truncate, hipStream_t s) {
  const int64_t nb = (n + kWavesPerBlock - 1) / kWavesPerBlock;
#define LZQ_POINTS_WIN(EXPV, NZ)                                                                                     \
  hipLaunchKernelGGL((yields_points_window_kernel<kYB, EXPV, NZ>), dim3((unsigned)nb), dim3(kBlock), 0, s, d_points, \
                     d_win, wt, n, n_y, d_T_lo, d_T_hi, d_P, zt, nzp, gtab, d_out, truncate)
  if (exp_variant == kExpTable) {
    if (default_grid) LZQ_POINTS_WIN(kExpTable, kNZ);
    else LZQ_POINTS_WIN(kExpTable, 0);
  } else {
    if (default_grid) LZQ_POINTS_WIN(kExpPoly11, kNZ);
    else LZQ_POINTS_WIN(kExpPoly11, 0);
  }
#undef LZQ_POINTS_WIN
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? LZQ_OK : lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
}

int lzq::launch_points_reuse_window(const lzq_point* d_points, const lzq_window* d_win, const lzq_window_tables& wt,
                                    int64_t n, int32_t n_y, const double* d_P, double key_nz, double key_z_max,
                                    const int32_t* d_table_index, const double* d_work, int64_t stride,
                                    lzq_yield* d_out, hipStream_t s) {
  const int64_t nb = (n + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(points_reuse_window_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, d_points, d_win, wt, n, n_y,
                     d_P, key_nz, key_z_max, d_table_index, d_work, stride, d_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? LZQ_OK : lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
}
