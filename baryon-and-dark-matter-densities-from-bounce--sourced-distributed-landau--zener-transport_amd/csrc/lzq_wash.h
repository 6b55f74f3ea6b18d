// lzq_wash.h -- wash-out and source depletion on the y-grid quadrature (include/lzq.h "wash-out and
// source depletion"), one definition for host and device.
//
// For sigma_v = 0 the reference's Boltzmann system (fpy:270-286) is linear: Y_B has the integrating
// factor (x/x_1)^Gamma = (T_lo/T)^Gamma, and the depletion term is the unwashed source, so
//     Y_B(x_1)   = sum_j w_j g_j omega(T_j),   omega(T) = exp(-Gamma log(T / T_lo)),
//     Y_chi(x_1) = Y_chi0 - [deplete] sum_j w_j g_j
// with g the fast path's integrand (fpy:264-265) on its y-grid, Gamma = max(Gamma_wash_over_H, 0) and
// T_lo = max(T_min_over_Tp T_p, 1e-30) (fpy:369, 389).  Wash-out is one more per-y-node factor next to
// the window W(y); depletion is a second accumulator over the same nodes.
//
// The exponent e = -(Gamma log(T / T_lo)) is formed here: one IEEE division, the library's log, one
// product and a sign, each rounded on its own (-ffp-contract=off).  The exponential on top of it is the
// caller's (libm on the host, exp_sc in the kernels), as for the window's q (lzq_window.h).  Gamma = 0
// takes neither the logarithm nor the exponential: omega is exactly 1.
#pragma once
#include <math.h>

#include "../../include/lzq.h"
#include "lzq_exp2.h"
#include "lzq_physics.h"

namespace lzq {

// 0 if the block can go through the quadrature, else the refusal it meets
enum WashError { kWashOk = 0, kWashNaNSigma, kWashNaNGamma, kWashSigma };

LZQ_HD int wash_error(const lzq_ode_params& o) {
  if (o.sigma_v_chi_GeV_m2 != o.sigma_v_chi_GeV_m2) return kWashNaNSigma;
  if (o.Gamma_wash_over_H != o.Gamma_wash_over_H) return kWashNaNGamma;
  if (pymax(o.sigma_v_chi_GeV_m2, 0.0) > 0.0) return kWashSigma;  // fpy:279: the Y_chi equation is not linear
  return kWashOk;
}

// A block resolved for evaluation.  ok == 0: every yield of the point is NaN.
struct WashParams {
  double gamma;  // max(Gamma_wash_over_H, 0)                 fpy:284
  double T_lo;   // max(T_min_over_Tp T_p, 1e-30)             fpy:369, 389
  int32_t deplete;
  int32_t ok;
};

LZQ_HD WashParams wash_params(const lzq_point& pt, const lzq_ode_params& o) {
  WashParams p;
  p.ok = wash_error(o) == kWashOk;
  p.gamma = p.ok ? pymax(o.Gamma_wash_over_H, 0.0) : 0.0;
  p.T_lo = pymax(pt.T_min_over_Tp * pt.T_p_GeV, 1e-30);
  p.deplete = o.deplete_DM_from_source != 0;
  return p;
}

// e with omega = exp(e); gamma > 0 (the caller gives 1 for gamma == 0 without coming here)
LZQ_HD double wash_exponent(double gamma, double T_lo, double T) { return -(gamma * log(T / T_lo)); }

// T(y) of the quadrature's y-grid, fpy:252-254, by the operations of the host build (the kernels take
// y_factors' own, lzq_quad.h)
inline double wash_T_of_y_host(const lzq_point& pt, double y) {
  const double denom = pymax(1.0 + 2.0 * y / pymax(pt.beta_over_H, 1e-30), 1e-12);
  return pt.T_p_GeV / sqrt(denom);
}

// ---- wash axes of a grid sweep (include/lzq.h LZQ_F_GAMMA_WASH, LZQ_F_DEPLETE) -------------------
LZQ_HD bool wash_field(int32_t f) { return f == LZQ_F_GAMMA_WASH || f == LZQ_F_DEPLETE; }

LZQ_HD void wash_set_field(lzq_ode_params& o, int32_t f, double v) {
  switch (f) {  // explicit switch, as set_field (lzq_quad.h)
    case LZQ_F_GAMMA_WASH: o.Gamma_wash_over_H = v; break;
    case LZQ_F_DEPLETE: o.deplete_DM_from_source = v != 0.0; break;  // (a NaN value depletes)
    default: break;
  }
}

// The block of flat grid index idx: base with the wash axes' values written into it, a pass over the
// axes next to grid_point's and window_grid_block's that reads the wash fields only.
template <class Grid>
LZQ_HD lzq_ode_params wash_grid_block(const lzq_ode_params& base, const Grid& g, int64_t idx) {
  lzq_ode_params o = base;
  for (int a = 0; a < g.n_axes; ++a) {
    if (!wash_field(g.field[a])) continue;
    const int64_t c = (idx / g.stride[a]) % g.n[a];
    wash_set_field(o, g.field[a], g.values[a][c]);
  }
  return o;
}

}  // namespace lzq
