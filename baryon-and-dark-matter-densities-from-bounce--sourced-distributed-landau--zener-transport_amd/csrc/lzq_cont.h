// lzq_cont.h -- A/V in the continuum limit of the z grid, one definition for host
// and device.
//
// The reference integrates z on linspace(0, z_max, nz) with trapezoid weights and the cancelling
// gamma4 of fpy:156; Y_B is not converged in that grid.  The continuum mode replaces
// the z-sum alone by a converged z-integral on a fixed, y-independent node rule:
//
//   A/V_cont(y) = 0                                  for y > 50
//               = pref0 e^yh F_cont(c)               yh = clip(y, +-50), c = -(I_p/6) e^yh
//   F_cont(c)   = sum_k omega_k exp(c gamma4_k)      over the N nodes below, ascending in z
//   omega_k     = z_k^2 e^{-z_k} w_k,  gamma4_k = gamma(4, z_k)
//
// pref0, the clip and the y > 50 zero are the reference's (fpy:158-165).  The rule is composite
// Gauss-Legendre, kContGL points per panel, on panels geometric in z: edges z_max kContRatio^-j
// down to the first one at or below kContZMin, plus the panel from 0 to that edge.  The integrand's
// only scale is the cut-off z_c = (4/a)^(1/4) of exp(-a gamma4), a = -c, which moves over seven
// decades of z for y in [-50, 50]; on panels of fixed ratio it is resolved alike wherever it falls.
// For z_max = 30: 26 panels, N = 520 nodes, rule error 1.7e-16 relative (tests/test_cont_host.py).
//
// gamma(4, z) is evaluated without the cancellation of fpy:156: the series z^4 sum (-z)^j/(j!(j+4))
// below z = 1 and the closed form 6 - e^-z (z^3 + 3 z^2 + 6 z + 6) from there on, both in the
// host's long double (64-bit mantissa) from the node's double and rounded once; omega likewise.
//
// On the device the sum runs through the table z-loops of lzq_quad.h (zsum_dispatch) like any z
// grid's: the node table leads with a (gamma4 = 0, omega = 0) node, which the dead-lane rule and
// the padding are keyed on (a linspace grid's node 0), and adds an exact +0.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/lzq.h"
#include "lzq_exp2.h"
#include "lzq_physics.h"

namespace lzq {

constexpr int kContGL = 20;          // Gauss-Legendre points per panel
constexpr double kContRatio = 2.0;   // panel edges z_max * ratio^-j
constexpr double kContZMin = 1e-6;   // the last geometric edge is the first at or below this

// pref0 and c's factor of AoverVKernel(I_p, beta_over_H, T_p, v_w, g_star), fpy:146-151, 162-163
// (quad_setup's operations)
struct ContKernel {
  double pref0, cneg;
};
LZQ_HD ContKernel cont_kernel(double I_p, double beta_over_H, double T_p, double v_w, double g_star) {
  ContKernel k;
  const double vw = pymax(v_w, 1e-12);
  const double beta = beta_over_H * H_std(T_p, g_star);
  k.pref0 = (I_p / 2.0) * (beta / vw);
  k.cneg = -(I_p / 6.0);
  return k;
}

// The definition, given e^x as the caller's exponential (libm on the host): a plain left-to-right
// FP64 sum over the table's n nodes.
template <typename Exp>
LZQ_HD double cont_aov(const ContKernel& k, double y, const double* g4, const double* omega, int32_t n, Exp ex) {
  if (y > 50.0) return 0.0;
  const double expy = ex(pymax(pymin(y, 50.0), -50.0));
  const double c = k.cneg * expy;
  double F = 0.0;
  for (int32_t i = 0; i < n; ++i) F += omega[i] * ex(c * g4[i]);
  return (k.pref0 * expy) * F;
}

// ---------------------------------------------------------------------------------------
// the node table (host)
// ---------------------------------------------------------------------------------------
// Gauss-Legendre nodes (ascending) and weights on [-1, 1]: Newton on P_m from the Chebyshev guess.
static inline void cont_gauss_legendre(int m, long double* x, long double* w) {
  const long double pi = 3.14159265358979323846264338327950288L;
  for (int i = 0; i < m; ++i) {
    long double t = cosl(pi * ((long double)i + 0.75L) / ((long double)m + 0.5L)), dp = 1.0L;
    for (int it = 0; it < 100; ++it) {
      long double p0 = 1.0L, p1 = t;
      for (int j = 2; j <= m; ++j) {
        const long double p2 = ((2 * j - 1) * t * p1 - (j - 1) * p0) / j;
        p0 = p1;
        p1 = p2;
      }
      dp = m * (t * p1 - p0) / (t * t - 1.0L);
      const long double dt = p1 / dp;
      t -= dt;
      if (fabsl(dt) < 1e-19L) break;
    }
    // dp at the converged node
    long double p0 = 1.0L, p1 = t;
    for (int j = 2; j <= m; ++j) {
      const long double p2 = ((2 * j - 1) * t * p1 - (j - 1) * p0) / j;
      p0 = p1;
      p1 = p2;
    }
    dp = m * (t * p1 - p0) / (t * t - 1.0L);
    x[m - 1 - i] = t;
    w[m - 1 - i] = 2.0L / ((1.0L - t * t) * dp * dp);
  }
}

// gamma(4, z) for z >= 0, stable at every z (header comment)
static inline long double cont_gamma4(long double z) {
  if (z < 1.0L) {
    long double s = 0.0L, t = 1.0L;  // t = (-z)^j / j!
    for (int j = 0; j < 64; ++j) {
      const long double a = t / (long double)(j + 4);
      s += a;
      if (fabsl(a) <= 0x1p-70L * fabsl(s)) break;
      t = -t * z / (long double)(j + 1);
    }
    return ((z * z) * (z * z)) * s;
  }
  return 6.0L - expl(-z) * (((z + 3.0L) * z + 6.0L) * z + 6.0L);
}

struct ContTable {
  double z_max = 0.0;
  std::vector<double> z, g4, omega;  // N nodes, ascending in (0, z_max)
};

// 0, or why z_max is refused (a static string)
static inline const char* cont_build(double z_max, ContTable& t) {
  if (!(z_max > 0.0) || !(z_max <= 0x1.fffffffffffffp1023)) return "z_max must be finite and > 0";
  std::vector<double> edge{z_max};  // descending
  while (edge.back() > kContZMin) edge.push_back(edge.back() / kContRatio);
  if (!(edge.back() > 0.0)) return "z_max underflows the panel edges";
  edge.push_back(0.0);
  long double x[kContGL], w[kContGL];
  cont_gauss_legendre(kContGL, x, w);
  t.z_max = z_max;
  t.z.clear();
  t.g4.clear();
  t.omega.clear();
  for (size_t p = edge.size() - 1; p-- > 0;) {  // panels [edge[p + 1], edge[p]], ascending
    const long double a = edge[p + 1], h = 0.5L * ((long double)edge[p] - a);
    for (int i = 0; i < kContGL; ++i) {
      const double z = (double)(a + h * (1.0L + x[i]));
      const long double zl = z;
      t.z.push_back(z);
      t.g4.push_back((double)cont_gamma4(zl));
      t.omega.push_back((double)((zl * zl) * expl(-zl) * (h * w[i])));
    }
  }
  const size_t n = t.z.size();
  for (size_t k = 0; k < n; ++k) {
    if (!(t.z[k] > (k ? t.z[k - 1] : 0.0)) || !(t.z[k] < z_max)) return "z_max: the nodes do not separate";
    if (k && t.g4[k] < t.g4[k - 1]) return "z_max: gamma4 is not non-decreasing";
  }
  // the inner loop's limits (lzq_quad.h zsum_dispatch; build_ztable's check for a linspace grid):
  // the first node's gamma4 bounds a live lane's |u|, and omega 2^-512 (kOmegaBias) has to stay a
  // normal double at the small-z end, where the terms matter at every y (at the large-z end of a
  // long range e^-z takes the weights, and the terms with them, below anything F can hold)
  if (!(t.g4[0] > 0.0) || !((double)kTabN * 1077.0 * t.g4[n - 1] / t.g4[0] < 0x1p200))
    return "z_max: gamma4 of the first node breaks the inner loop's reduction";
  if (!(ldexp(t.omega[0], -kOmegaBias) >= 0x1p-1022)) return "z_max: the first node's weight underflows";
  // a clamped node's term omega'_k v_c rounds away at every node (LZQ_CLAMP_ARG, lzq_exp2.h)
  if (!clamp_arg_grid_ok([&](int k) { return ldexp(t.omega[k], -kOmegaBias); }, (int)n))
    return "z_max: a weight is too large for a clamped node's term to round away";
  return nullptr;
}

}  // namespace lzq
