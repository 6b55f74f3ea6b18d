// lzq_solve.h -- the stepping rule of the per-point root solve (include/lzq.h lzq_sweep_grid_solve),
// one definition for host and device.
//
// The solve finds x in [lo, hi] with f(x) = field(x) - target = 0 for one yield field of one grid
// point, by a bracketing state machine that the caller drives: solve_init, then
//     while (solve_next(st, x)) { f = field(x) - target; slot = solve_feed(st, x, f); ... }
// and solve_result.  Only IEEE + - * /, comparisons and selects are used, each rounded on its own
// (-ffp-contract=off), as in lzq_window.h: a host build takes exactly the device's decisions
// (tests/test_solve_host.py drives this header through a callback).
//
// The rule:
//   start      f(lo), then f(hi).  An exact zero ends the solve at that end; a non-finite f gives
//              LZQ_SOLVE_NAN; two values of the same strict sign give LZQ_SOLVE_NO_BRACKET.
//   candidate  the regula-falsi point (a gb - b ga)/(gb - ga) of the bracket [a, b], where ga, gb are
//              fa, fb with the value of an end that was retained twice running scaled down by the
//              Anderson-Bjorck factor 1 - f_new/f_replaced (1/2, Illinois' factor, when that is not
//              positive), so that the next point crosses to the other side of the root.
//   safeguard  the midpoint a + (b - a)/2 instead when the candidate is not strictly inside (a, b), or
//              when the width after the last evaluation is more than half the width two evaluations
//              before it.  The midpoint then halves it, so the width at least halves over any three
//              consecutive evaluations after the first two.  The evaluation after such a midpoint
//              takes the midpoint too: a field that interpolation does not follow (a jump) is then
//              bisected two steps in three.
//   stop       |b - a| <= xtol max(|a|, |b|); no double strictly between a and b; an exact zero;
//              max_evals evaluations (LZQ_SOLVE_MAX_EVALS, the bracket still valid).
//   invariant  fa and fb have opposite strict signs whenever the bracket is open (a < b).
//   result     x = the end with the smaller |f| (ties: the lower end), residual = f(x) as evaluated
//              there; x_lo <= x <= x_hi.  An exact zero closes the bracket on it: x_lo = x = x_hi.
#pragma once
#include "../../include/lzq.h"
#include "lzq_exp2.h"

namespace lzq {

constexpr int kSolveMinEvals = 2, kSolveMaxEvals = 256;

struct SolveState {
  double a, b;          // bracket ends, a <= b
  double fa, fb;        // f as evaluated at a and b
  double ga, gb;        // fa, fb as the candidate reads them (scaled at a retained end)
  double w, w1, w2;     // |b - a| now, one and two evaluations ago
  double lo, hi, xtol;  // as given
  int32_t evals, max_evals;
  int32_t side;    // the end the last evaluation replaced: -1 a, +1 b, 0 none yet
  int32_t force;   // the number of coming evaluations that take the midpoint
  int32_t status;  // enum lzq_solve_status
  int32_t done;
};

LZQ_HD int32_t solve_clamp_evals(int32_t m) {
  return m < kSolveMinEvals ? kSolveMinEvals : (m > kSolveMaxEvals ? kSolveMaxEvals : m);
}

LZQ_HD bool solve_finite(double f) { return f - f == 0.0; }  // false for NaN and +-inf
LZQ_HD double solve_abs(double x) { return x < 0.0 ? -x : x; }

LZQ_HD SolveState solve_init(double lo, double hi, double xtol, int32_t max_evals) {
  SolveState s;
  s.a = s.lo = lo;
  s.b = s.hi = hi;
  s.fa = s.fb = s.ga = s.gb = 0.0;
  s.w = hi - lo;
  s.w1 = s.w2 = 0x1.fffffffffffffp1023;  // no history yet: nothing to compare with
  s.xtol = xtol;
  s.evals = 0;
  s.max_evals = solve_clamp_evals(max_evals);
  s.side = 0;
  s.force = 0;
  s.status = LZQ_SOLVE_OK;
  s.done = 0;
  return s;
}

// the open bracket's stop tests (the bracket [a, b] has a sign change)
LZQ_HD bool solve_converged(const SolveState& s) {
  const double aa = solve_abs(s.a), ab = solve_abs(s.b);
  if (s.b - s.a <= s.xtol * (aa > ab ? aa : ab)) return true;
  const double mid = s.a + (s.b - s.a) / 2.0;
  return !(mid > s.a && mid < s.b);  // adjacent doubles
}

// The next abscissa, or false when the solve has ended.
LZQ_HD bool solve_next(const SolveState& s, double& x) {
  if (s.done) return false;
  if (s.evals == 0) {
    x = s.lo;
    return true;
  }
  if (s.evals == 1) {
    x = s.hi;
    return true;
  }
  const double mid = s.a + (s.b - s.a) / 2.0;
  const double c = (s.a * s.gb - s.b * s.ga) / (s.gb - s.ga);
  const bool inside = c > s.a && c < s.b;             // false for a NaN candidate
  x = (inside && s.force == 0) ? c : mid;
  return true;
}

// Take f = f(x) at the abscissa solve_next gave.  Returns the record slots the evaluation belongs to
// as a bit mask (1: it is now the bracket's lower end, 2: its upper end, 3: both, an exact zero), or
// 0 when it is neither (a non-finite f, which ends the solve).
LZQ_HD int32_t solve_feed(SolveState& s, double x, double f) {
  s.evals += 1;
  if (!solve_finite(f)) {
    s.status = LZQ_SOLVE_NAN;
    s.done = 1;
    return 0;
  }
  int32_t slot;
  if (s.evals == 1) {
    s.fa = s.ga = f;
    if (f == 0.0) {  // the root is the lower end
      s.b = s.a;
      s.fb = f;
      s.done = 1;
      return 3;
    }
    return 1;
  }
  if (s.evals == 2) {
    s.fb = s.gb = f;
    slot = 2;
    if (f == 0.0) {
      s.a = s.b;
      s.fa = f;
      s.done = 1;
      return 3;
    }
    if ((s.fa < 0.0) == (f < 0.0)) {
      s.status = LZQ_SOLVE_NO_BRACKET;
      s.done = 1;
      return slot;
    }
  } else if (f == 0.0) {  // an exact zero closes the bracket on x
    s.a = s.b = x;
    s.fa = s.fb = f;
    s.done = 1;
    return 3;
  } else if ((f < 0.0) == (s.fa < 0.0)) {  // x replaces a; b is retained
    const double m = 1.0 - f / s.fa;
    s.a = x;
    s.fa = s.ga = f;
    if (s.side == -1) s.gb = s.gb * (m > 0.0 ? m : 0.5);
    s.side = -1;
    slot = 1;
  } else {
    const double m = 1.0 - f / s.fb;
    s.b = x;
    s.fb = s.gb = f;
    if (s.side == +1) s.ga = s.ga * (m > 0.0 ? m : 0.5);
    s.side = +1;
    slot = 2;
  }
  if (s.evals > 2) {
    s.w2 = s.w1;
    s.w1 = s.w;
    s.w = s.b - s.a;
  }
  // the width is more than half of what it was two evaluations ago: the next evaluation must halve
  // it, and the one after it does too (a field that interpolation does not follow, such as a jump)
  if (!(s.w <= 0.5 * s.w2)) s.force = 2;
  else if (s.force > 0) s.force -= 1;
  if (solve_converged(s)) s.done = 1;
  else if (s.evals >= s.max_evals) {
    s.status = LZQ_SOLVE_MAX_EVALS;
    s.done = 1;
  }
  return slot;
}

// The result (include/lzq.h lzq_solve_result); *slot: the record slot of x (0 or 1), -1 for a status
// without a solution.
LZQ_HD lzq_solve_result solve_result(const SolveState& s, int32_t* slot) {
  lzq_solve_result r;
  r.evals = (double)s.evals;
  r.status = (double)s.status;
  if (s.status == LZQ_SOLVE_OK || s.status == LZQ_SOLVE_MAX_EVALS) {
    const bool upper = solve_abs(s.fb) < solve_abs(s.fa);
    r.x = upper ? s.b : s.a;
    r.residual = upper ? s.fb : s.fa;
    r.x_lo = s.a;
    r.x_hi = s.b;
    *slot = upper ? 1 : 0;
  } else {
    r.x = r.residual = __builtin_nan("");
    r.x_lo = s.lo;
    r.x_hi = s.hi;
    *slot = -1;
  }
  return r;
}

// A result for a point that is not evaluated at all (a refused window block, a table of another setup).
LZQ_HD lzq_solve_result solve_refused(double lo, double hi, int32_t status, int32_t evals) {
  lzq_solve_result r;
  r.x = r.residual = __builtin_nan("");
  r.x_lo = lo;
  r.x_hi = hi;
  r.evals = (double)evals;
  r.status = (double)status;
  return r;
}

}  // namespace lzq
