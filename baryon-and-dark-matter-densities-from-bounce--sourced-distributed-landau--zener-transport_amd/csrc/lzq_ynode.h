// lzq_ynode.h -- the y-grid of the dense Y_B quadrature, ys = numpy.linspace(y_lo, y_hi, n)
// (fpy:247) with its trapezoid weights (fpy:267), as plain host/device functions: the general
// forms, which handle the grid's ends, and the interior forms yb_wave / yb_group take on a pass
// that touches neither end (LZQ_PASS_LEAN, lzq_quad.h).  tests/pass_lean_host.cpp compiles this
// header on the CPU.  Not ABI.
#pragma once
#include "lzq_exp2.h"

namespace lzq {

// S: the grid's record -- y_lo, y_hi, step = delta / (n - 1), delta = y_hi - y_lo, n (QuadSetup on the
// device, read field by field where it is needed).

// numpy.linspace element (handles numpy's step == 0 branch as well)
template <class S>
LZQ_HD double y_node_general(const S& s, int j) {  // n_y is int32
  const int n = (int)s.n;
  if (j == n - 1) return s.y_hi;
  if (s.step == 0.0) return ((double)j / (double)(n - 1)) * s.delta + s.y_lo;
  return (double)j * s.step + s.y_lo;
}

// trapezoid weight of y-node j: (d_{j-1} + d_j)/2 with d = diff(ys)      fpy:267
template <class S>
LZQ_HD double y_weight_general(const S& s, int j, double y) {
  double dl = (j > 0) ? y - y_node_general(s, j - 1) : 0.0;
  double dr = (j + 1 < (int)s.n) ? y_node_general(s, j + 1) - y : 0.0;
  return 0.5 * (dl + dr);
}

// Interior passes.  A pass of `span` y-nodes from `base` (64 for a single pass, 64 G for a group of G)
// is interior when j - 1, j and j + 1 lie in [0, n - 2] for every one of its nodes j: the pass is full,
// none of the three is the last element (which linspace sets to y_hi) and both neighbours exist.  The
// tests are on wave-uniform values.  n_lin is n where step != 0 and 0 where numpy's step == 0 branch
// would be taken (y_lin_count), so such a grid has no interior pass.
LZQ_HD int y_lin_count(double step, int n) { return step != 0.0 ? n : 0; }
LZQ_HD bool y_pass_interior(int base, int span, int n_lin) { return base >= 64 && base + span + 1 < n_lin; }

// y_node_general / y_weight_general on an interior pass: the same convert, multiply, add and subtract,
// without the selects whose outcome the pass test has fixed
LZQ_HD double y_node_interior(double y_lo, double step, int j) { return (double)j * step + y_lo; }
LZQ_HD double y_weight_interior(double y_lo, double step, int j, double y) {
  const double dl = y - y_node_interior(y_lo, step, j - 1);
  const double dr = y_node_interior(y_lo, step, j + 1) - y;
  return 0.5 * (dl + dr);
}

}  // namespace lzq
