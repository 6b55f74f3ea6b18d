// Host build of the root solve's stepping rule (csrc/lzq_solve.h: LZQ_HD, the functions the GPU
// kernel itself calls) for tests/test_solve_host.py (TEST INFRASTRUCTURE).  The rule is driven
// exactly as lzq_solve.hip drives it -- solve_init, then solve_next / f / solve_feed until
// solve_next says stop, then solve_result -- with f = field(x) - target from a callback.
//
// trace: one row of 6 doubles per evaluation, (x, f, a, b, fa, fb) after the evaluation was fed
// (fa, fb are f as evaluated at the bracket's ends), so the test can check the sign invariant and
// the halving of the width evaluation by evaluation.  masks: solve_feed's record-slot mask per
// evaluation.  Returns the number of evaluations; result6 = lzq_solve_result; *slot = the record slot.
#include <stdint.h>

#include "lzq_solve.h"

using namespace lzq;

extern "C" {

typedef double (*field_fn)(double x);

int solve_run(field_fn field, double lo, double hi, double target, double xtol, int max_evals, double* result6,
              double* trace, int* masks, int* slot) {
  SolveState st = solve_init(lo, hi, xtol, max_evals);
  int n = 0;
  double x;
  while (n < kSolveMaxEvals && solve_next(st, x)) {
    const double f = field(x) - target;
    const int32_t mask = solve_feed(st, x, f);
    if (trace) {
      double* t = trace + 6 * n;
      t[0] = x, t[1] = f, t[2] = st.a, t[3] = st.b, t[4] = st.fa, t[5] = st.fb;
    }
    if (masks) masks[n] = mask;
    ++n;
  }
  int32_t s = -1;
  const lzq_solve_result r = solve_result(st, &s);
  result6[0] = r.x, result6[1] = r.x_lo, result6[2] = r.x_hi, result6[3] = r.residual, result6[4] = r.evals,
  result6[5] = r.status;
  if (slot) *slot = s;
  return n;
}

int solve_clamp(int max_evals) { return solve_clamp_evals(max_evals); }

}  // extern "C"
