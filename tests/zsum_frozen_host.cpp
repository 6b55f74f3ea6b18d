// Host restatement of lzq::zsum_dispatch (csrc/lzq_quad.h) with the frozen tails (LZQ_FROZEN_SEG:
// zsum_held on zero passes, zsum_frozen_t on clamp-free passes), for ONE 64-lane wavefront; for
// tests/test_zsum_frozen_host.py and tools/uniform_segment_share.py (TEST INFRASTRUCTURE, compiled with
// g++ -ffp-contract=off).  The predicates (seg_zero, seg_clamped, seg_frozen_s, seg_frozen_t), the batch
// search (seg_first_batch), the table values (seg_entry), the held value (seg_value_frozen_s), w
// (seg_frozen_w) and the nodes (seg_node_dead, seg_node_zero, seg_node, seg_node_frozen,
// exp2_tab_scaled) are the LZQ_HD functions of csrc/lzq_exp2.h that the device code calls.  Around them
// this file mirrors what zsum_dispatch does per pass, as tests/zsum_dead_segment_host.cpp does: the dead
// rule, the order all-dead -> zero -> clamp-free -> clamped split, the truncation end, the padding nodes
// of a runtime grid and the fma accumulate in node order; lzq_quad.h itself needs the HIP runtime, so
// its rule constants are restated (kUnroll, kDeadOct, kTruncOct).
//
// `defect` builds a deliberately broken dispatch, which the test must tell from the right one:
//   1  the tail's per-lane constants (held value; frozen t's entry and w) are formed at the grid's last
//      node nzp - 1, not at the last EXECUTED node kend - 1 the search compared with (they differ under
//      truncation);
//   2  k3 is the batch holding the first frozen NODE, i.e. rounded down instead of up;
//   3  the tail starts one batch before k3.
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

// one lane's pass: F's fma accumulate in node order, and a checksum over the bits of EVERY node's value.
// At the saturated end of the grid omega' is ~1e-10 of the sum, so a node value that is off by an ulp
// there vanishes in F's rounding; the checksum sees it.
struct Acc {
  double F = 0.0;
  uint64_t h = 0;
  void add(double om, int k, double v) {
    F = __builtin_fma(om, v, F);
    h += __builtin_bit_cast(uint64_t, v) * (uint64_t)(2 * k + 1);
  }
};

int padded_nodes(int nz) {
  const int n = nz > kUnroll ? nz : kUnroll;
  return (n + kUnroll - 1) / kUnroll * kUnroll;
}

// the dispatch's k3 (frozen_t: of t, else of s), with the defects
template <class Frozen>
int tail_start(Frozen frozen, const std::vector<double>& g, int kend, int defect) {
  int k3 = seg_first_batch(frozen, [&](int k) { return g[k]; }, kend, kUnroll);
  if (defect == 2) {
    int k = 0;
    while (k < kend && !frozen(g[k])) ++k;
    k3 = k / kUnroll * kUnroll;
  }
  if (defect == 3 && k3 >= kUnroll) k3 -= kUnroll;
  return k3;
}

// one pass; frozen = LZQ_FROZEN_SEG (0: the parent's dispatch, 1: frozen s, 2: both; -1: the single
// general loop); plan = {path, k2, kend, k3}, k3 = kend where no tail is taken
void pass(int frozen, int defect, bool truncate, const std::vector<double>& g, const std::vector<double>& om, int nz,
          const double* c2, double* F, uint64_t* V, int* plan) {
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
  int path, k2 = kend, k3 = kend;
  const double g_last = g[kend > 0 ? kend - 1 : 0];
  const double g_val = defect == 1 ? g[nzp - 1] : g_last;  // where the tail's per-lane constants are formed
  if (frozen < 0) {
    path = kPathGeneral;
    for (int l = 0; l < kLanes; ++l) {
      Acc acc;
      for (int k = 0; k < kend; ++k) acc.add(om[k], k, exp2_tab_scaled(c2e[l], g[k], tab));
      F[l] = acc.F, V[l] = acc.h;
    }
  } else {
    bool zero = true;
    for (int l = 0; l < kLanes; ++l) zero = zero && seg_zero(c2e[l], g_max, kTabMagic);
    if (all_dead) {
      path = kPathDead;
      k2 = 0;
      const double v0 = seg_node_dead(kSqA, seg_entry(tab, kTabMagic));
      for (int l = 0; l < kLanes; ++l) {
        Acc acc;
        for (int k = 0; k < kend; ++k) acc.add(om[k], k, v0);
        F[l] = acc.F, V[l] = acc.h;
      }
    } else if (zero) {
      path = kPathZero;
      k2 = 0;
      const double Ts = seg_entry(tab, kTabMagic);
      if (frozen >= 1)
        k3 = tail_start(
            [&](double gk) {
              bool c = true;
              for (int l = 0; l < kLanes; ++l) c = c && seg_frozen_s(c2e[l], gk, g_last, kSqA);
              return c;
            },
            g, kend, defect);
      for (int l = 0; l < kLanes; ++l) {
        Acc acc;
        for (int k = 0; k < k3; ++k) acc.add(om[k], k, seg_node_zero(c2e[l], g[k], kSqA, Ts));
        if (k3 < kend) {
          const double v = seg_value_frozen_s(c2e[l], g_val, kSqA, Ts);  // zsum_held
          for (int k = k3; k < kend; ++k) acc.add(om[k], k, v);
        }
        F[l] = acc.F, V[l] = acc.h;
      }
    } else if (small) {
      path = kPathFree;
      if (frozen >= 2)
        k3 = tail_start(
            [&](double gk) {
              bool c = true;
              for (int l = 0; l < kLanes; ++l) c = c && seg_frozen_t(c2e[l], gk, g_last, kTabMagic);
              return c;
            },
            g, kend, defect);
      for (int l = 0; l < kLanes; ++l) {
        Acc acc;
        for (int k = 0; k < k3; ++k) acc.add(om[k], k, node_free(c2e[l], g[k], tab));
        if (k3 < kend) {
          const double tl = __builtin_fma(c2e[l], g_val, kTabMagic);  // zsum_frozen_t
          const double Tl = seg_entry(tab, tl), wl = seg_frozen_w(tl);
          for (int k = k3; k < kend; ++k) acc.add(om[k], k, seg_node_frozen(c2e[l], g[k], wl, Tl));
        }
        F[l] = acc.F, V[l] = acc.h;
      }
    } else {
      path = kPathSplit;
      k2 = seg_first_batch(
          [&](double gk) {
            bool c = true;
            for (int l = 0; l < kLanes; ++l) c = c && seg_clamped(c2e[l], gk, kTabMagic);
            return c;
          },
          [&](int k) { return g[k]; }, kend, kUnroll);
      const double Ts = seg_entry(tab, kTabTClamp);
      for (int l = 0; l < kLanes; ++l) {
        Acc acc;
        for (int k = 0; k < k2; ++k) acc.add(om[k], k, exp2_tab_scaled(c2e[l], g[k], tab));
        for (int k = k2; k < kend; ++k) acc.add(om[k], k, seg_node(c2e[l], g[k], kTabMagic, Ts));
        F[l] = acc.F, V[l] = acc.h;
      }
    }
  }
  for (int l = 0; l < kLanes; ++l) F[l] = dead[l] ? 0.0 : F[l];
  if (plan) {
    plan[0] = path;
    plan[1] = k2;
    plan[2] = kend;
    plan[3] = k3;
  }
}

}  // namespace

extern "C" {

int zfrozen_zero(double c2N, double g_max) { return seg_zero(c2N, g_max, kTabMagic) ? 1 : 0; }
int zfrozen_dead(double c2N, double g_1) { return c2N * g_1 <= -(double)kTabN * kDeadOct ? 1 : 0; }
int zfrozen_small(double c2N, double g_max) { return c2N * g_max >= (double)kTabKMin ? 1 : 0; }

// n passes of 64 lanes each (see pass)
int zfrozen_passes(int frozen, int defect, int truncate, const double* g4, const double* omega, int nz, const double* c2,
                   long n, double* F, uint64_t* V, int* plan) {
  if (nz < 2 || !kSqForm || frozen < -1 || frozen > 2 || defect < 0 || defect > 3) return -1;
  build_tab();
  const int nzp = padded_nodes(nz);
  std::vector<double> g(nzp), om(nzp);
  for (int k = 0; k < nzp; ++k) {
    g[k] = k < nz ? g4[k] : g4[nz - 1];
    om[k] = k < nz ? ldexp(omega[k], -kOmegaBias) : 0.0;
  }
  for (long i = 0; i < n; ++i)
    pass(frozen, defect, truncate != 0, g, om, nz, c2 + i * kLanes, F + i * kLanes, V + i * kLanes,
         plan ? plan + 4 * i : nullptr);
  return 0;
}

// one lane, node by node over g4[n]: the loop's own s = fma(c2N, g, A) (kind 0) or t = fma(c2N, g, M)
// (kind 1), for the brute-force scan the test checks k3 against
int zfrozen_values(int kind, double c2N, const double* g4, int n, double* v) {
  for (int k = 0; k < n; ++k) v[k] = __builtin_fma(c2N, g4[k], kind ? kTabMagic : kSqA);
  return 0;
}

}  // extern "C"
