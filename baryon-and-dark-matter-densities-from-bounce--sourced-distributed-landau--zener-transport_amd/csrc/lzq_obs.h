// lzq_obs.h -- the cell of a row in an observable (a histogram over one or two lzq_yield fields),
// one definition for host and device.
//
// Linear axis (lo < hi, bins >= 1, inv = bins / (hi - lo) formed once on the host in float64):
//   x < lo -> below, x >= hi -> above, else b = min(bins - 1, (int64)((x - lo) * inv)); the clamp
//   matters: just under hi the product can round up to bins.
// Binary-log axis (0 < lo < hi, 2^s sub-bins per octave): key(x) = bits(x) >> (52 - s) for x > 0 --
//   the exponent and the top s mantissa bits, i.e. sub-bins linear inside the octave; no logarithm
//   is taken.  b = key(x) - key(lo); x <= 0 or key(x) < key(lo) -> below, key(x) >= key(hi) -> above.
// A row's class in an observable: kObsNonfinite if one of its fields is NaN or +-inf, else kObsOut
// if one is below or above, else the cell b0 (one axis) or b0 * bins1 + b1 (two).
// Only IEEE -, * (each rounded on its own: -ffp-contract=off), an exact truncation and integer
// operations are used, so numpy reproduces it (tests/test_obs_host.py) and the host build of this
// function gives the device's cells (tests/test_gpu_obs.py).
#pragma once
#include "lzq_exp2.h"   // LZQ_HD
#include "lzq_fit_common.h"

namespace lzq {

constexpr int32_t kObsOut = -1;
constexpr int32_t kObsNonfinite = -2;

struct ObsAxisDev {
  int32_t field, kind;   // kind: LZQ_OBS_LINEAR / LZQ_OBS_LOG2
  int32_t bins, shift;   // shift = 52 - s (log axes)
  double lo, hi, inv;    // linear axes
  int64_t key_lo;        // log axes: key(lo); key(hi) = key_lo + bins
};

struct ObsDev {
  int32_t n_axes, cells;
  int32_t lds_off;   // first cell in the block-private LDS image, or -1: straight to global memory
  int32_t pad;
  int64_t off;       // word offset of the observable's header in the state
  ObsAxisDev ax[2];
};

struct ObsParams {
  int32_t n_obs, lds_cells;
  ObsDev obs[LZQ_OBS_MAX];
};

LZQ_HD int64_t obs_key(double x, int32_t shift) {   // x > 0
  return (int64_t)((uint64_t)__builtin_bit_cast(int64_t, x) >> shift);
}

// the bin of a FINITE x on one axis, or kObsOut
LZQ_HD int32_t obs_axis_bin(const ObsAxisDev& A, double x) {
  if (A.kind == LZQ_OBS_LINEAR) {
    if (x < A.lo || x >= A.hi) return kObsOut;
    const double t = (x - A.lo) * A.inv;
    const int64_t b = (int64_t)t;
    return (int32_t)(b < A.bins - 1 ? b : A.bins - 1);
  }
  if (!(x > 0.0)) return kObsOut;
  const int64_t b = obs_key(x, A.shift) - A.key_lo;
  return b < 0 || b >= A.bins ? kObsOut : (int32_t)b;
}

LZQ_HD int32_t obs_cell(const ObsDev& O, const double x[6]) {
  const double x0 = fit_pick(x, O.ax[0].field);
  const double x1 = O.n_axes == 2 ? fit_pick(x, O.ax[1].field) : 0.0;
  if (!__builtin_isfinite(x0) || !__builtin_isfinite(x1)) return kObsNonfinite;
  const int32_t b0 = obs_axis_bin(O.ax[0], x0);
  if (O.n_axes == 1) return b0;
  const int32_t b1 = obs_axis_bin(O.ax[1], x1);
  return b0 < 0 || b1 < 0 ? kObsOut : b0 * O.ax[1].bins + b1;
}

}  // namespace lzq
