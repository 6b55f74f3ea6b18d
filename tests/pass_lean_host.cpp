// Host side of tests/test_pass_lean_host.py (TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off):
// the y-grid functions of csrc/lzq_ynode.h that yb_wave / yb_group call on the device -- the general
// y_node / y_weight, the interior forms an interior pass takes (LZQ_PASS_LEAN) and the pass gate --
// evaluated for one pass of 64 y-nodes of linspace(y_lo, y_hi, n), set up as quad_setup does.
#include <stdint.h>

#include "lzq_ynode.h"

using namespace lzq;

namespace {

struct Grid {  // the fields of QuadSetup the y-grid reads
  double y_lo, y_hi, step, delta;
  int64_t n;
};

Grid grid_of(double y_lo, double y_hi, int n) {
  Grid s;
  s.y_lo = y_lo;
  s.y_hi = y_hi;
  s.n = n;
  s.delta = y_hi - y_lo;
  s.step = s.delta / (double)(s.n - 1);
  return s;
}

}  // namespace

extern "C" {

// the gate of a pass (span = 64) or of a group of G passes (span = 64 G) from `base`
int ylean_gate(double y_lo, double y_hi, int n, int base, int span) {
  const Grid s = grid_of(y_lo, y_hi, n);
  return y_pass_interior(base, span, y_lin_count(s.step, n)) ? 1 : 0;
}

// y and weight of the 64 nodes base .. base + 63, general (with the tail rule of yb_wave: a node past
// the grid is the last node with weight 0) and, where every index the interior forms touch is inside the
// grid, interior; elsewhere the interior outputs are left alone.  Returns the gate.
int ylean_pass(double y_lo, double y_hi, int n, int base, double* yg, double* wg, double* yi, double* wi) {
  const Grid s = grid_of(y_lo, y_hi, n);
  for (int l = 0; l < 64; ++l) {
    const int j = base + l;
    const int jj = j < n ? j : n - 1;
    yg[l] = y_node_general(s, jj);
    wg[l] = j < n ? y_weight_general(s, jj, yg[l]) : 0.0;
    yi[l] = y_node_interior(s.y_lo, s.step, j);
    wi[l] = y_weight_interior(s.y_lo, s.step, j, yi[l]);
  }
  return y_pass_interior(base, 64, y_lin_count(s.step, n)) ? 1 : 0;
}

}  // extern "C"
