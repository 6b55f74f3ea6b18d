// lzq_post.h -- the likelihood weight of a row, one definition for host and device.
//
// c is the row's chi2 (fit_chi2's expression), offset a finite number >= 0, a = c - offset:
//   c not finite  -> the row is invalid                       (kPostInvalid)
//   a < 0         -> the row is "above": counted, no weight   (kPostAbove)
//   else            w = exp(-a/2) = 2^(a K), K = -log2(e)/2 (the halving is exact), by lzq_exp2.h's
//                   reduction and degree-11 polynomial, in (0, 1];
//                   q = min(trunc(w 2^62), 2^62): the weight in fixed point, units of 2^-62.
// q = 0 from a ~ 124 ln 2 = 85.95 on (w < 2^-62).  Only IEEE *, fma, rint, ldexp and an exact
// double -> integer truncation are used, each rounded on its own, so the host build of this
// function gives the device's bits (tests/test_post_host.py, tests/test_gpu_post.py).
#pragma once
#include "lzq_exp2.h"

namespace lzq {

constexpr uint64_t kPostInvalid = ~0ull;
constexpr uint64_t kPostAbove = ~0ull - 1;
constexpr uint64_t kPostOne = 1ull << 62;   // the weight of a = 0

LZQ_HD uint64_t post_q(double a) {   // a >= 0, finite
  constexpr double K = -0.5 * kLog2E;
  // exp(-a/2) is below the smallest double from a = 1490 on: say so before the reduction, whose
  // remainder r is only small while |a K| < 2^52 (the polynomial of a huge r is not a number)
  if (a >= 2048.0) return 0;
  const double u = a * K;
  const double kd = __builtin_rint(u);
  const double r = __builtin_fma(a, K, -kd);
  const int32_t k = cvt_i32_sat(kd);
  const double w = __builtin_ldexp(exp2_poly(r), k);
  const double s = w * 0x1p62;   // exact
  return s >= 0x1p62 ? kPostOne : (uint64_t)s;
}

LZQ_HD uint64_t post_weight(double c, double offset) {
  if (!__builtin_isfinite(c)) return kPostInvalid;
  const double a = c - offset;
  return a < 0.0 ? kPostAbove : post_q(a);
}

// a row carries weight iff 1 <= q <= 2^62 (0, kPostAbove and kPostInvalid do not)
LZQ_HD bool post_weighted(uint64_t q) { return q - 1 < kPostOne; }

}  // namespace lzq
