// Host restatement of lzq::zsum_dispatch (csrc/lzq_quad.h) for ONE lane, for tests/test_zsum_host.py
// (TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off).  The per-node arithmetic is the
// LZQ_HD code of csrc/lzq_exp2.h that the kernels inline (exp2_tab_scaled, exp2_nonpos with
// kOmegaBias); around it this file mirrors what lzq_quad.h / lzq_kernels.hip do per lane and per
// pass: the dead rule, the clamp and its clamp-free instantiation, the omega * 2^-512 scaling, the
// padding nodes of a runtime grid, the truncation end and the fma accumulate.  lzq_quad.h itself
// needs the HIP runtime, so its few rule constants are restated here (kUnroll, kDeadOct, kTruncOct).
//
// `mutant` switches ONE deliberate defect on, so that the test can show that its comparison with
// the high-precision reference rejects it (0 = the faithful model):
//   1 table entry `mut_index` wrong by 2^-40 relative     5 the last real node dropped
//   2 kSqBeta off by 1e-9 relative                         6 padding nodes carry the last real omega
//   3 dead threshold at 1000 instead of 1077 octaves       7 kend rounded down to the unroll
//   4 clamp constant 1506 raised by 64 octaves             8 poly11: non-saturating int conversion
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "lzq_exp2.h"

using namespace lzq;

namespace {

constexpr int kUnroll = 8;           // LZQ_KUNROLL
constexpr double kDeadOct = 1077.0;  // zsum_dispatch: dead iff c2 g4_1 <= -1077 octaves
constexpr double kTruncOct = 1080.0; // zsum_dispatch: nodes below -1080 octaves are not executed
constexpr double kMagic = 0x1.8p52;

double g_tab[kTabN];
bool g_tab_ready = false;

void build_tab() {
  if (g_tab_ready) return;
  for (int j = 0; j < kTabN; ++j) {
    const uint64_t b = tab_entry_bits(tab_exact(j), j);
    memcpy(&g_tab[j], &b, 8);
  }
  g_tab_ready = true;
}

// exp2_tab_scaled (completed-square form) with the clamp, its constant and beta as parameters:
// clamp = false is zsum<.., CLAMP = false>, the instantiation of a pass no lane of which can clamp
double node_tab(double c2N, double g, const double* tabp, bool clamp, int32_t kmin, double beta) {
  const double t = __builtin_fma(c2N, g, kMagic);
  const double tc = clamp ? __builtin_fmax(t, kMagic + (double)kmin) : t;
  const uint32_t k = (uint32_t)__builtin_bit_cast(uint64_t, tc);
  const double Ts = tab_scale(tabp[tab_byte_addr(k) >> 3], k);
  const double s = __builtin_fma(c2N, g, (kMagic + kSqA) - t);
  return Ts * __builtin_fma(s, s, beta);
}

// exp2_nonpos with the conversion as a parameter (mutant 8)
double node_poly(double c2, double g, bool saturate) {
  if (saturate) return exp2_nonpos(c2, g, kOmegaBias);
  const double u = c2 * g;
  const double kd = __builtin_rint(u);
  const double r = __builtin_fma(c2, g, -kd);
  const int32_t k = (int32_t)(int64_t)kd;  // wraps for |kd| >= 2^31
  return __builtin_ldexp(exp2_poly(r), (int)((uint32_t)k + (uint32_t)kOmegaBias));
}

}  // namespace

extern "C" {

// out: kLog2E, kTabN, kTabKMin / kTabN (octaves), kSqForm, unroll, dead octaves, truncation octaves
void zsum_consts(double* out) {
  out[0] = kLog2E;
  out[1] = (double)kTabN;
  out[2] = (double)kTabKMin / (double)kTabN;
  out[3] = kSqForm ? 1.0 : 0.0;
  out[4] = (double)kUnroll;
  out[5] = kDeadOct;
  out[6] = kTruncOct;
}

// lzq_kernels.hip padded_nodes
int zsum_padded_nodes(int nz) {
  const int n = nz > kUnroll ? nz : kUnroll;
  return (n + kUnroll - 1) / kUnroll * kUnroll;
}

// table index a node reads (the clamped magic sum's low bits), as the model forms it
int zsum_tab_index(double c2N, double g) {
  const double t = __builtin_fma(c2N, g, kMagic);
  const double tc = __builtin_fmax(t, kMagic + (double)kTabKMin);
  return (int)(tab_byte_addr((uint32_t)__builtin_bit_cast(uint64_t, tc)) >> 3);
}

// F[i] = zsum_dispatch of one lane with c2[i] (already in the variant's scale: c2 * N for the
// table) over the grid (g4, omega)[nz] as lzq_ztables returns it.  variant: 1 table, 0 poly11.
// force_clamp: run the clamped instantiation even where the lane alone would run clamp-free (the
// lane then stands in a wave with a clamping neighbour).  kend_out[i]: nodes executed.
// Returns 0, or -1 on bad arguments, or 1 + the number of faithful-model nodes at which the
// parameterised node_tab differs from lzq::exp2_tab_scaled (must be 0).
int zsum_model(int variant, int mutant, int mut_index, int truncate, int force_clamp, const double* g4,
               const double* omega, int nz, const double* c2, long n, double* F, int* kend_out) {
  if (nz < 2 || !kSqForm || (variant != 0 && variant != 1)) return -1;
  build_tab();
  std::vector<double> tab(g_tab, g_tab + kTabN);
  if (mutant == 1) tab[mut_index & (kTabN - 1)] *= 1.0 + 0x1p-40;
  const double beta = mutant == 2 ? kSqBeta * (1.0 + 1e-9) : kSqBeta;
  const int32_t kmin = mutant == 4 ? kTabKMin - 64 * kTabN : kTabKMin;
  const double dead_oct = mutant == 3 ? 1000.0 : kDeadOct;
  const double scale = variant == 1 ? (double)kTabN : 1.0;
  // device image of the grid (device_nodes): omega' = omega * 2^-512, padding = last g4, omega' = 0
  const int nzp = zsum_padded_nodes(nz);
  std::vector<double> g(nzp), om(nzp);
  for (int k = 0; k < nzp; ++k) {
    g[k] = k < nz ? g4[k] : g4[nz - 1];
    om[k] = k < nz ? ldexp(omega[k], -kOmegaBias) : (mutant == 6 ? ldexp(omega[nz - 1], -kOmegaBias) : 0.0);
  }
  if (mutant == 5) om[nz - 1] = 0.0;
  long mismatch = 0;
  for (long i = 0; i < n; ++i) {
    const double g_1 = g[1], g_max = g[nz - 1];
    const bool dead = c2[i] * g_1 <= -scale * dead_oct;
    const double c2e = dead ? 0.0 : c2[i];
    const bool small = c2e * g_max >= (double)kmin;
    int kend = nzp;
    if (truncate) {
      const double thr = dead ? 0.0 : (c2e < 0.0 ? (-kTruncOct * scale) / c2e : INFINITY);
      int lo = 0, hi = nzp;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g[mid] > thr) hi = mid;
        else lo = mid + 1;
      }
      kend = mutant == 7 ? lo / kUnroll * kUnroll : (lo + kUnroll - 1) / kUnroll * kUnroll;
    }
    const bool clamp = force_clamp || !small;
    double acc = 0.0;
    for (int k = 0; k < kend; ++k) {
      double v;
      if (variant == 1) {
        v = node_tab(c2e, g[k], tab.data(), clamp, kmin, beta);
        if (mutant == 0 && clamp && v != exp2_tab_scaled(c2e, g[k], tab.data())) ++mismatch;
      } else {
        v = node_poly(c2e, g[k], mutant != 8);
      }
      acc = __builtin_fma(om[k], v, acc);
    }
    F[i] = dead ? 0.0 : acc;
    if (kend_out) kend_out[i] = kend;
  }
  return mismatch ? (int)(1 + mismatch) : 0;
}

}  // extern "C"
