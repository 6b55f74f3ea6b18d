// lzq_window.h -- the source activity window W(y) of a point (include/lzq.h lzq_window), one
// definition for host and device.
//
// The reference's window is the Gaussian proxy of fpy:262; PAPER §10 step 4 asks for it to be
// replaced by other activity profiles.  A window is a per-y factor of the integrand formed after
// the z-loop (lzq_quad.h y_factors), independent of the z-sums.  Only IEEE -, *, /, comparisons and
// selects are used here, each rounded on its own (-ffp-contract=off), so the host build of these
// functions gives the device's q and table values bit for bit (tests/test_window_host.py,
// tests/test_gpu_window.py); the exponential on top of q is the caller's (libm on the host, exp_sc
// in the kernels).  The decode of a grid sweep's flat index into a point's block (window_grid_block)
// is here too, one definition for the kernels and for lzq_window_grid_blocks_host.
#pragma once
#include "../../include/lzq.h"
#include "lzq_exp2.h"
#include "lzq_physics.h"

namespace lzq {

// A block resolved for evaluation: the reciprocals of the clamped sigmas and the block's table row.
// 72 bytes; it lives in the wave's LDS slot in the quadrature kernels.
struct WinParams {
  double y0, half_width, r_lo, r_hi, scale;
  const double* u;  // [n_knots]
  const double* W;  // the block's row, [n_knots]
  int32_t kind;     // enum lzq_window_kind; kWinBad: every W is NaN
  int32_t n_knots;
};
constexpr int32_t kWinBad = -1;

// 0 if the block can be evaluated, else which refusal of include/lzq.h it meets (window_error_text)
enum WinError { kWinOk = 0, kWinNaN, kWinSigma, kWinScale, kWinHalfWidth, kWinKind, kWinTable, kWinKnots };

LZQ_HD bool win_pos_finite(double x) { return x > 0.0 && x <= 0x1.fffffffffffffp1023; }

LZQ_HD int window_block_error(const lzq_window& w, int32_t n_tables, int32_t n_knots) {
  if (w.y0 != w.y0 || w.half_width != w.half_width || w.sigma_lo != w.sigma_lo || w.sigma_hi != w.sigma_hi ||
      w.scale != w.scale)
    return kWinNaN;
  if (!win_pos_finite(w.sigma_lo) || !win_pos_finite(w.sigma_hi)) return kWinSigma;
  if (!win_pos_finite(w.scale)) return kWinScale;
  if (w.half_width < 0.0) return kWinHalfWidth;
  if (w.kind != LZQ_WIN_GAUSS && w.kind != LZQ_WIN_PLATEAU && w.kind != LZQ_WIN_TABLE) return kWinKind;
  if (w.kind == LZQ_WIN_TABLE) {
    if (w.table < 0 || w.table >= n_tables) return kWinTable;
    if (n_knots < 2 || n_knots > LZQ_WIN_MAX_KNOTS) return kWinKnots;
  }
  return kWinOk;
}

// The block as the evaluation reads it.  A refused block (or a table kind without tables) is
// marked kWinBad and reads no table.
LZQ_HD WinParams window_params(const lzq_window& w, int32_t n_tables, int32_t n_knots, const double* u,
                               const double* W) {
  WinParams p;
  const bool tab = w.kind == LZQ_WIN_TABLE;
  const bool ok = window_block_error(w, n_tables, n_knots) == kWinOk && (!tab || (u != nullptr && W != nullptr));
  p.y0 = w.y0;
  p.half_width = w.half_width;
  p.r_lo = 1.0 / pymax(w.sigma_lo, 1e-6);
  p.r_hi = 1.0 / pymax(w.sigma_hi, 1e-6);
  p.scale = w.scale;
  p.u = (ok && tab) ? u : nullptr;
  p.W = (ok && tab) ? W + (int64_t)w.table * n_knots : nullptr;
  p.kind = ok ? w.kind : kWinBad;
  p.n_knots = (ok && tab) ? n_knots : 0;
  return p;
}

// q of the Gaussian kinds (include/lzq.h): W = exp(-0.5 (q q)).  kind: p.kind (the kernels pass
// it from a scalar register).
LZQ_HD double window_q(const WinParams& p, int32_t kind, double y) {
  if (kind == LZQ_WIN_GAUSS) return y * p.r_hi;
  const double u = y - p.y0;
  const double d = pymax(fabs(u) - p.half_width, 0.0);
  return d * (u < 0.0 ? p.r_lo : p.r_hi);
}

// v of the table kind.
LZQ_HD double window_v(const WinParams& p, double y) { return (y - p.y0) / p.scale; }

// The table kind's W at v: linear on the knot interval [u_k, u_{k+1}) that holds v (the largest k
// with u_k <= v, by bisection: n_knots >= 2, so k and k + 1 index the row), the end values outside.
LZQ_HD double window_table_W(const WinParams& p, double v) {
  const int n = p.n_knots;
  if (v < p.u[0]) return p.W[0];
  if (v >= p.u[n - 1]) return p.W[n - 1];
  int lo = 0, hi = n - 1;  // u[lo] <= v < u[hi] (a NaN v stays on the first interval and gives NaN)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p.u[mid] <= v) lo = mid;
    else hi = mid;
  }
  const double uk = p.u[lo], Wk = p.W[lo];
  return Wk + (v - uk) * ((p.W[lo + 1] - Wk) / (p.u[lo + 1] - uk));
}

// ---- window axes of a grid sweep (include/lzq.h LZQ_F_WIN_*) -------------------------------------
LZQ_HD bool window_field(int32_t f) { return f >= LZQ_F_WIN_Y0 && f <= LZQ_F_WIN_TABLE; }

// The block fields an axis field writes, as a bit mask (0: not a window field): two axes whose
// masks meet write the same field, which the entry points refuse.
LZQ_HD uint32_t window_field_mask(int32_t f) {
  switch (f) {
    case LZQ_F_WIN_Y0: return 1u;
    case LZQ_F_WIN_HALF_WIDTH: return 2u;
    case LZQ_F_WIN_SIGMA_LO: return 4u;
    case LZQ_F_WIN_SIGMA_HI: return 8u;
    case LZQ_F_WIN_SIGMA: return 4u | 8u;
    case LZQ_F_WIN_SCALE: return 16u;
    case LZQ_F_WIN_TABLE: return 32u;
    default: return 0u;
  }
}

// A table axis value: the double is tested before it is converted (an int32 conversion of a NaN or
// of a value out of range is undefined); anything but an integer in [0, 2^31) gives -1, which
// window_block_error refuses for a table-kind block whatever n_tables is.
LZQ_HD int32_t window_table_value(double v) {
  if (!(v >= 0.0 && v < 2147483648.0)) return -1;
  const int32_t t = (int32_t)v;
  return (double)t == v ? t : -1;
}

LZQ_HD void window_set_field(lzq_window& w, int32_t f, double v) {
  switch (f) {  // explicit switch, as set_field (lzq_quad.h): no runtime-indexed store
    case LZQ_F_WIN_Y0: w.y0 = v; break;
    case LZQ_F_WIN_HALF_WIDTH: w.half_width = v; break;
    case LZQ_F_WIN_SIGMA_LO: w.sigma_lo = v; break;
    case LZQ_F_WIN_SIGMA_HI: w.sigma_hi = v; break;
    case LZQ_F_WIN_SIGMA: w.sigma_lo = v; w.sigma_hi = v; break;
    case LZQ_F_WIN_SCALE: w.scale = v; break;
    case LZQ_F_WIN_TABLE: w.table = window_table_value(v); break;
    default: break;
  }
}

// The window block of flat grid index idx: base with the window axes' values written into it, a
// second pass over the axes next to grid_point's (lzq_quad.h) that reads the window fields only.
// Grid: n_axes, field[], n[], stride[] (int64, C order) and values[] -- lzq_quad.h's GridSpec in the
// kernels (values in device memory), HostWinGrid below on the host.  64-bit index arithmetic.
template <class Grid>
LZQ_HD lzq_window window_grid_block(const lzq_window& base, const Grid& g, int64_t idx) {
  lzq_window w = base;
  for (int a = 0; a < g.n_axes; ++a) {
    if (!window_field(g.field[a])) continue;
    const int64_t c = (idx / g.stride[a]) % g.n[a];
    window_set_field(w, g.field[a], g.values[a][c]);
  }
  return w;
}

struct HostWinGrid {
  int32_t n_axes;
  int32_t field[LZQ_MAX_AXES];
  int64_t n[LZQ_MAX_AXES];
  int64_t stride[LZQ_MAX_AXES];
  const double* values[LZQ_MAX_AXES];
};

}  // namespace lzq
