// lzq_fk.h -- the momentum-averaged Landau-Zener probability P-bar of a point (include/lzq.h lzq_fk;
// PAPER §10 step 1), one definition for host and device.
//
// With the momentum kernel F(k) of PAPER eq. (8) other than 1, the conversion probability of a
// particle depends on its speed v = k/E in the plasma frame: P(v) = 1 - exp(-2 pi delta_0 F(v)),
// delta_0 eq. (8) at F = 1.  Its average over the thermal flux onto the wall depends on mu = m/T:
//
//   t = (E - m)/T in (0, inf),  eps = t + mu,  k^2/T^2 = t (t + 2 mu),  v = sqrt(t (t + 2 mu))/eps
//   omega(t) = t (t + 2 mu) e^-t / (1 +- e^-mu e^-t)      + fermion, - boson; the common e^-mu is cancelled
//   P-bar(mu) = int omega(t) [-expm1(-g F(v))] dt / int omega(t) dt,   g = 2 pi delta_0
//   F(v) = (v_ref / v)^p                                   LZQ_FK_POWER, p = 0: the paper's F = 1
//
// The rule: composite Gauss-Legendre, kFkGL points per panel, on panels geometric in t (lzq_cont.h's
// construction for z): edges kFkTMax kFkRatio^-j down to the first at or below kFkTMin, plus the panel
// from 0 to that edge.  The table holds t_i, e^-t_i and W_i e^-t_i; the only exponential that depends
// on mu is e^-mu, taken once per call.  Numerator and denominator are summed in node order with the
// same weights, so g = +inf gives exactly 1 (every bracket is 1: the two sums are the same sum) and
// g = 0 exactly +0 (every bracket is -expm1(-0) = +0).  v^-p comes from one log and one exp per node,
// exp(p log v_ref - (p/2) log(t (t + 2 mu)/eps^2)); p = 0 takes neither.
//
// The table: 2 panels per decade from 90 down to 1e-10, 14 points each, and the panel [0, ~1e-10]:
// 350 nodes, rule error 3.6e-14 relative on the box mu in {0, .3, 3, 42, 849} x g in {1e-9 .. 10} x
// p in {0, 1, 2, 3.5} x v_ref in {0.1, 1} x both statistics (profiles/fk/rule_error.json;
// tests/test_fk_host.py).  Cheaper tables stay inside 1e-12 on the v_ref = 1 half of the box (294 nodes
// with the last edge at 1e-8: 3.6e-14 there) and leave it on the other (4.3e-12 at v_ref = 0.1, g = 1e-9:
// the bracket saturates below t ~ g v_ref^2 mu, which the first panel has to reach down to); 252 nodes
// with the range cut at t = 45 are inside for one alignment of the panels only.  This is the cheapest
// found whose neighbours in t_max and t_min stay inside too.
//
// Host: libm's exp / log / expm1; device: the HIP device library's (<= 1 ulp each).  Everything else is
// IEEE +, *, / rounded one by one (-ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/lzq.h"
#include "lzq_cont.h"  // cont_gauss_legendre
#include "lzq_physics.h"

namespace lzq {

constexpr int kFkGL = 14;                         // Gauss-Legendre points per panel
constexpr double kFkRatio = 3.16227766016837933;  // sqrt(10): two panels per decade
constexpr double kFkTMax = 90.0;                  // e^-90 = 8e-40
constexpr double kFkTMin = 1e-10;                 // the last geometric edge is the first at or below this

struct FkNode {
  double t;   // node
  double we;  // W e^-t  (Gauss-Legendre weight times the Boltzmann factor)
  double e;   // e^-t
};

// 0 if the block can be evaluated, else which refusal of include/lzq.h it meets
enum FkError { kFkOk = 0, kFkKind, kFkP, kFkVref };

LZQ_HD int fk_block_error(const lzq_fk& b) {
  if (b.kind != LZQ_FK_POWER) return kFkKind;
  if (!(b.p >= 0.0 && b.p <= LZQ_FK_P_MAX)) return kFkP;  // NaN fails both
  if (!(b.v_ref > 0.0 && b.v_ref <= 1.0)) return kFkVref;
  return kFkOk;
}

// delta_0 of a point: refused when NaN or < 0 (+inf is P = 1)
LZQ_HD bool fk_delta_ok(double delta0) { return delta0 >= 0.0; }

// g = 2 pi delta_0, one rounding
LZQ_HD double fk_g(double delta0) { return (2.0 * kPi) * delta0; }

// P-bar(mu) of the header comment on the n nodes of tab.  A refused block, g or mu (NaN or < 0) is NaN.
LZQ_HD double fk_pbar(double mu, double g, const lzq_fk& b, int32_t stats, const FkNode* __restrict__ tab,
                      int32_t n) {
  if (fk_block_error(b) != kFkOk || !(g >= 0.0) || !(mu >= 0.0)) return __builtin_nan("");
  const double emu = exp(-mu);
  const double sg = stats == 0 ? emu : -emu;  // LZQ_FERMION: 1 + e^-mu e^-t
  const double mu2 = 2.0 * mu;
  double num = 0.0, den = 0.0;
  if (b.p == 0.0) {
    const double br = -expm1(-g);
    for (int32_t i = 0; i < n; ++i) {
      const double t = tab[i].t;
      const double w = (t * (t + mu2)) * tab[i].we / (1.0 + sg * tab[i].e);
      num += w * br;
      den += w;
    }
  } else {
    const double hp = -0.5 * b.p, lr = b.p * log(b.v_ref);
    for (int32_t i = 0; i < n; ++i) {
      const double t = tab[i].t;
      const double a = t * (t + mu2), eps = t + mu;
      const double w = a * tab[i].we / (1.0 + sg * tab[i].e);
      // F = (v_ref / v)^p, kept finite so that g = 0 stays 0 where v underflows
      const double F = pymin(exp(hp * log(a / (eps * eps)) + lr), 0x1.fffffffffffffp1023);
      const double x = F > 0.0 ? g * F : 0.0;  // (an F that underflowed converts nothing, whatever g)
      num += w * -expm1(-x);
      den += w;
    }
  }
  return num / den;
}

// ---------------------------------------------------------------------------------------
// the node table (host)
// ---------------------------------------------------------------------------------------
static inline void fk_build(std::vector<FkNode>& out) {
  std::vector<long double> edge{(long double)kFkTMax};  // descending
  while (edge.back() > (long double)kFkTMin) edge.push_back(edge.back() / (long double)kFkRatio);
  edge.push_back(0.0L);
  long double x[kFkGL], w[kFkGL];
  cont_gauss_legendre(kFkGL, x, w);
  out.clear();
  for (size_t p = edge.size() - 1; p-- > 0;) {  // panels [edge[p + 1], edge[p]], ascending
    const long double a = edge[p + 1], h = 0.5L * (edge[p] - a);
    for (int i = 0; i < kFkGL; ++i) {
      const double t = (double)(a + h * (1.0L + x[i]));
      const long double tl = t, e = expl(-tl);
      out.push_back(FkNode{t, (double)(h * w[i] * e), (double)e});
    }
  }
}

// ---------------------------------------------------------------------------------------
// the R table of a class: header key and layout (lzq_fk.hip)
// ---------------------------------------------------------------------------------------
// R table of a class: kFkHdr header doubles, R_j = P-bar(mu_j) for the n y-nodes, then P-bar(m/T_p)
// (the record's P_used).  The key names everything R depends on: the y-grid (y_lo, y_hi, n), the
// statistics and kind (packed with n: all three are small integers), m, g and a 64-bit fold of the
// bits of T_p, max(B, 1e-30), p and v_ref, stored as a double's bit pattern and compared as bits.
constexpr int kFkHdr = LZQ_FK_TABLE_HEADER;

LZQ_HD uint64_t fk_fold(uint64_t h, double x) {
  h ^= __builtin_bit_cast(uint64_t, x);
  h *= 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}

struct FkKey {
  double k[kFkHdr];
};
LZQ_HD FkKey fk_key(double y_lo, double y_hi, int64_t n, double Tp, double Bc, double m, int32_t stats, double g,
                    const lzq_fk& b) {
  FkKey key;
  key.k[0] = y_lo;
  key.k[1] = y_hi;
  key.k[2] = (double)n + 4294967296.0 * (stats == 0 ? 0.0 : 1.0) + 8589934592.0 * (double)(b.kind & 0xffff);
  key.k[3] = m;
  key.k[4] = g;
  uint64_t h = fk_fold(0x6c7a715f666b0001ull, Tp);
  h = fk_fold(h, Bc);
  h = fk_fold(h, b.p);
  h = fk_fold(h, b.v_ref);
  key.k[5] = __builtin_bit_cast(double, h);
  return key;
}
// bitwise, so a NaN in a key matches itself and the fold needs no care; -0 and +0 differ (a y-grid
// end formed by the same operations has the same sign)
LZQ_HD bool fk_key_match(const FkKey& key, const double* __restrict__ hdr) {
  bool ok = true;
  for (int i = 0; i < kFkHdr; ++i)
    ok = ok && __builtin_bit_cast(uint64_t, key.k[i]) == __builtin_bit_cast(uint64_t, hdr[i]);
  return ok;
}

}  // namespace lzq
