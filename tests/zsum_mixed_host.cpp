// Host restatement of the last branch of lzq::zsum_dispatch (csrc/lzq_quad.h) with the per-lane
// uniform-entry suffix of a clamped pass that holds dead lanes (LZQ_PASS_LEAN, zsum_uniform_lane), for
// ONE 64-lane wavefront; for tests/test_zsum_mixed_host.py (TEST INFRASTRUCTURE, compiled with
// g++ -ffp-contract=off).  The predicates (seg_zero, seg_clamped, seg_clamped_or_dead), the batch
// search (seg_first_batch), the table values (seg_entry, seg_entry_lane) and the nodes (seg_node,
// exp2_tab_scaled) are the LZQ_HD functions of csrc/lzq_exp2.h that the device code calls.  The other
// branches (all-dead, zero, clamp-free with their frozen tails) are tests/zsum_frozen_host.cpp's and are
// restated here only as far as their plan goes: the pass is classified with the dispatch's order
// all-dead -> zero -> clamp-free -> clamped, and a pass that is none of the first three runs
//   mode -1  the single general loop (exp2_tab_scaled at every node);
//   mode  0  the parent's split: k2 from seg_clamped over all 64 lanes, the wave-uniform entry;
//   mode  1  the new split: k2 from seg_clamped_or_dead, and where the wave holds a dead lane the suffix
//            with each lane's own entry.
// A pass of the first three kinds runs the general loop in every mode (its paths are pinned elsewhere)
// and reports its kind, so that the test can assert which passes the new branch takes.
//
// `defect` builds a deliberately broken new split, which the test must tell from the right one:
//   1  the per-lane entry is taken from the clamp constant for dead lanes too;
//   2  the suffix starts one batch before k2.
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

enum Path { kPathZero = 0, kPathFree = 1, kPathSplit = 2, kPathDead = 3, kPathMixed = 4 };

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

// plan = {path, k2, kend, number of dead lanes}; Fraw: F before the dead lanes are zeroed
void pass(int mode, int defect, bool truncate, const std::vector<double>& g, const std::vector<double>& om, int nz,
          const double* c2, double* Fraw, double* F, uint64_t* V, int* plan) {
  const int nzp = (int)g.size();
  const double g_1 = g[1], g_max = g[nz - 1];
  bool dead[kLanes], small = true, all_dead = true, any_dead = false, zero = true;
  double c2e[kLanes];
  int ndead = 0;
  for (int l = 0; l < kLanes; ++l) {
    dead[l] = c2[l] * g_1 <= -(double)kTabN * kDeadOct;
    c2e[l] = dead[l] ? 0.0 : c2[l];
    small = small && c2e[l] * g_max >= (double)kTabKMin;
    all_dead = all_dead && dead[l];
    any_dead = any_dead || dead[l];
    zero = zero && seg_zero(c2e[l], g_max, kTabMagic);
    ndead += dead[l] ? 1 : 0;
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
  int path, k2 = kend;
  const bool last_branch = !all_dead && !zero && !small;
  if (all_dead) path = kPathDead;
  else if (zero) path = kPathZero;
  else if (small) path = kPathFree;
  else path = kPathSplit;
  if (mode < 0 || !last_branch) {
    for (int l = 0; l < kLanes; ++l) {
      Acc acc;
      for (int k = 0; k < kend; ++k) acc.add(om[k], k, exp2_tab_scaled(c2e[l], g[k], tab));
      Fraw[l] = acc.F, V[l] = acc.h;
    }
  } else {
    const bool lean = mode == 1;
    const bool mixed = lean && any_dead;
    k2 = seg_first_batch(
        [&](double gk) {
          bool c = true;
          for (int l = 0; l < kLanes; ++l)
            c = c && (lean ? seg_clamped_or_dead(dead[l], c2e[l], gk, kTabMagic) : seg_clamped(c2e[l], gk, kTabMagic));
          return c;
        },
        [&](int k) { return g[k]; }, kend, kUnroll);
    if (mixed) path = kPathMixed;
    int ks = k2;  // where the suffix starts
    if (mixed && defect == 2 && ks >= kUnroll) ks -= kUnroll;
    for (int l = 0; l < kLanes; ++l) {
      const double Ts = mixed ? (defect == 1 ? seg_entry(tab, kTabTClamp) : seg_entry_lane(tab, dead[l]))
                              : seg_entry(tab, kTabTClamp);
      Acc acc;
      for (int k = 0; k < ks; ++k) acc.add(om[k], k, exp2_tab_scaled(c2e[l], g[k], tab));
      for (int k = ks; k < kend; ++k) acc.add(om[k], k, seg_node(c2e[l], g[k], kTabMagic, Ts));
      Fraw[l] = acc.F, V[l] = acc.h;
    }
  }
  for (int l = 0; l < kLanes; ++l) F[l] = dead[l] ? 0.0 : Fraw[l];
  if (plan) {
    plan[0] = path;
    plan[1] = k2;
    plan[2] = kend;
    plan[3] = ndead;
  }
}

}  // namespace

extern "C" {

// n passes of 64 lanes each (see pass)
int zmixed_passes(int mode, int defect, int truncate, const double* g4, const double* omega, int nz, const double* c2,
                  long n, double* Fraw, double* F, uint64_t* V, int* plan) {
  if (nz < 2 || !kSqForm || mode < -1 || mode > 1 || defect < 0 || defect > 2) return -1;
  build_tab();
  const int nzp = padded_nodes(nz);
  std::vector<double> g(nzp), om(nzp);
  for (int k = 0; k < nzp; ++k) {
    g[k] = k < nz ? g4[k] : g4[nz - 1];
    om[k] = k < nz ? ldexp(omega[k], -kOmegaBias) : 0.0;
  }
  for (long i = 0; i < n; ++i)
    pass(mode, defect, truncate != 0, g, om, nz, c2 + i * kLanes, Fraw + i * kLanes, F + i * kLanes, V + i * kLanes,
         plan ? plan + 4 * i : nullptr);
  return 0;
}

// one lane, node by node over g4[n]: the loop's own clamped magic sum max(fma(c2N, g, M), M + KMIN), for
// the brute-force scan the test checks k2 against
int zmixed_tc(double c2N, const double* g4, int n, double* v) {
  for (int k = 0; k < n; ++k) v[k] = __builtin_fmax(__builtin_fma(c2N, g4[k], kTabMagic), kTabTClamp);
  return 0;
}

double zmixed_tclamp() { return kTabTClamp; }
double zmixed_magic() { return kTabMagic; }

}  // extern "C"
