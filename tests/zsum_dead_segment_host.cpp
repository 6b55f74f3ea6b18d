// Host restatement of lzq::zsum_dispatch (csrc/lzq_quad.h) with the all-dead passes run through the
// dead loop (LZQ_DEAD_SEG: zsum_dead), for ONE 64-lane wavefront; for
// tests/test_zsum_dead_segment_host.py (TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off).
// The predicates (seg_zero, seg_clamped), the segment's table value (seg_entry), the dead node
// (seg_node_dead), the zero node (seg_node_zero), the six-operation uniform node (seg_node) and the
// general node (exp2_tab_scaled) are the LZQ_HD functions of csrc/lzq_exp2.h that the device code
// calls.  Around them this file mirrors what zsum_dispatch does per pass, as
// tests/zsum_zero_segment_host.cpp does: the dead rule, the all-dead test ahead of the zero test, the
// clamp-free test, the truncation end, the padding nodes of a runtime grid and the fma accumulate in
// node order; lzq_quad.h itself needs the HIP runtime, so its rule constants are restated (kUnroll,
// kDeadOct, kTruncOct).  Besides F the harness hands back the raw sums, before dead lanes are
// zeroed: the zeroing hides what an all-dead pass computed.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "lzq_exp2.h"

using namespace lzq;

namespace {

constexpr int kLanes = 64;           // kWaveSize
constexpr int kUnroll = 8;           // LZQ_KUNROLL
constexpr double kDeadOct = 1077.0;  // zsum_dispatch: dead iff c2 g4_1 <= -1077 octaves
constexpr double kTruncOct = 1080.0; // zsum_dispatch: nodes below -1080 octaves are not executed

enum Mode { kGeneral = 0, kDeadSeg = 1, kZeroSeg = 2 };  // kZeroSeg: the dispatch of -DLZQ_DEAD_SEG=0
enum Path { kPathGeneral = -1, kPathZero = 0, kPathFree = 1, kPathSplit = 2, kPathDead = 3 };

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

// zsum<.., CLAMP = false>: exp2_tab_scaled without the max
double node_free(double c2N, double g, const double* tabp) {
  const double t = __builtin_fma(c2N, g, kTabMagic);
  const uint32_t k = (uint32_t)__builtin_bit_cast(uint64_t, t);
  const double Ts = tab_scale(tabp[tab_byte_addr(k) >> 3], k);
  const double s = __builtin_fma(c2N, g, (kTabMagic + kSqA) - t);
  return Ts * __builtin_fma(s, s, kSqBeta);
}

int padded_nodes(int nz) {
  const int n = nz > kUnroll ? nz : kUnroll;
  return (n + kUnroll - 1) / kUnroll * kUnroll;
}

// one pass; plan = {path, k2, kend}; Fraw = the sums before the dead lanes are zeroed
void pass(int mode, bool truncate, const std::vector<double>& g, const std::vector<double>& om, int nz,
          const double* c2, double* F, double* Fraw, int* plan) {
  const int nzp = (int)g.size();
  const double g_1 = g[1], g_max = g[nz - 1];
  bool dead[kLanes], small = true, all_dead = true;
  double c2e[kLanes];
  for (int l = 0; l < kLanes; ++l) {
    dead[l] = c2[l] * g_1 <= -(double)kTabN * kDeadOct;
    c2e[l] = dead[l] ? 0.0 : c2[l];
    small = small && c2e[l] * g_max >= (double)kTabKMin;
    all_dead = all_dead && dead[l];
  }
  int kend = nzp;
  if (truncate) {
    double thr = 0.0;
    for (int l = 0; l < kLanes; ++l) {
      const double tb = dead[l] ? 0.0 : (c2e[l] < 0.0 ? (-kTruncOct * (double)kTabN) / c2e[l] : INFINITY);
      thr = thr > tb ? thr : tb;
    }
    int lo = 0, hi = nzp;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (g[mid] > thr) hi = mid;
      else lo = mid + 1;
    }
    kend = (lo + kUnroll - 1) / kUnroll * kUnroll;
  }
  const double* tab = g_tab;
  int path, k2;
  if (mode == kGeneral) {
    path = kPathGeneral;
    k2 = kend;
    for (int l = 0; l < kLanes; ++l) {
      double acc = 0.0;
      for (int k = 0; k < kend; ++k) acc = __builtin_fma(om[k], exp2_tab_scaled(c2e[l], g[k], tab), acc);
      F[l] = acc;
    }
  } else {
    bool zero = true;
    for (int l = 0; l < kLanes; ++l) zero = zero && seg_zero(c2e[l], g_max, kTabMagic);
    if (mode == kDeadSeg && all_dead) {
      // zsum_dead: the node's value once per pass, then F's accumulate at every node
      path = kPathDead;
      k2 = 0;
      const double v0 = seg_node_dead(kSqA, seg_entry(tab, kTabMagic));
      for (int l = 0; l < kLanes; ++l) {
        double acc = 0.0;
        for (int k = 0; k < kend; ++k) acc = __builtin_fma(om[k], v0, acc);
        F[l] = acc;
      }
    } else if (zero) {
      path = kPathZero;
      k2 = 0;
      const double Ts = seg_entry(tab, kTabMagic);
      for (int l = 0; l < kLanes; ++l) {
        double acc = 0.0;
        for (int k = 0; k < kend; ++k) acc = __builtin_fma(om[k], seg_node_zero(c2e[l], g[k], kSqA, Ts), acc);
        F[l] = acc;
      }
    } else {
      if (small) {
        path = kPathFree;
        k2 = kend;
      } else {
        path = kPathSplit;
        k2 = seg_first_batch(
            [&](double gk) {
              bool c = true;
              for (int l = 0; l < kLanes; ++l) c = c && seg_clamped(c2e[l], gk, kTabMagic);
              return c;
            },
            [&](int k) { return g[k]; }, kend, kUnroll);
      }
      const double Ts = seg_entry(tab, kTabTClamp);
      for (int l = 0; l < kLanes; ++l) {
        double acc = 0.0;
        for (int k = 0; k < k2; ++k)
          acc = __builtin_fma(om[k], path == kPathFree ? node_free(c2e[l], g[k], tab) : exp2_tab_scaled(c2e[l], g[k], tab),
                              acc);
        for (int k = k2; k < kend; ++k) acc = __builtin_fma(om[k], seg_node(c2e[l], g[k], kTabMagic, Ts), acc);
        F[l] = acc;
      }
    }
  }
  for (int l = 0; l < kLanes; ++l) {
    if (Fraw) Fraw[l] = F[l];
    F[l] = dead[l] ? 0.0 : F[l];
  }
  if (plan) {
    plan[0] = path;
    plan[1] = k2;
    plan[2] = kend;
  }
}

}  // namespace

extern "C" {

int zdead_zero(double c2N, double g_max) { return seg_zero(c2N, g_max, kTabMagic) ? 1 : 0; }
int zdead_dead(double c2N, double g_1) { return c2N * g_1 <= -(double)kTabN * kDeadOct ? 1 : 0; }
int zdead_small(double c2N, double g_max) { return c2N * g_max >= (double)kTabKMin ? 1 : 0; }

// n passes of 64 lanes each; mode 0 the single general loop, 1 the dispatch with the dead loop,
// 2 the dispatch without it (all-dead passes take the zero path)
int zdead_passes(int mode, int truncate, const double* g4, const double* omega, int nz, const double* c2, long n,
                 double* F, double* Fraw, int* plan) {
  if (nz < 2 || !kSqForm || mode < 0 || mode > 2) return -1;
  build_tab();
  const int nzp = padded_nodes(nz);
  std::vector<double> g(nzp), om(nzp);
  for (int k = 0; k < nzp; ++k) {
    g[k] = k < nz ? g4[k] : g4[nz - 1];
    om[k] = k < nz ? ldexp(omega[k], -kOmegaBias) : 0.0;
  }
  for (long i = 0; i < n; ++i)
    pass(mode, truncate != 0, g, om, nz, c2 + i * kLanes, F + i * kLanes, Fraw ? Fraw + i * kLanes : nullptr,
         plan ? plan + 3 * i : nullptr);
  return 0;
}

// one lane, node by node over g4[n], with the zero stretch's entry T''[0]: v[0][k] = seg_node_dead
// (no c2N, no g), v[1][k] = seg_node_zero, v[2][k] = seg_node, v[3][k] = exp2_tab_scaled (its own
// lookup), the last three with the given c2N
int zdead_nodes(double c2N, const double* g4, int n, double* v) {
  if (!kSqForm) return -1;
  build_tab();
  const double Ts = seg_entry(g_tab, kTabMagic);
  for (int k = 0; k < n; ++k) {
    v[k] = seg_node_dead(kSqA, Ts);
    v[n + k] = seg_node_zero(c2N, g4[k], kSqA, Ts);
    v[2 * n + k] = seg_node(c2N, g4[k], kTabMagic, Ts);
    v[3 * n + k] = exp2_tab_scaled(c2N, g4[k], g_tab);
  }
  return 0;
}

}  // extern "C"
