// Host restatement of the clamped argument (LZQ_CLAMP_ARG; csrc/lzq_exp2.h clamp_arg_s /
// exp2_tab_scaled_clamp_arg / clamp_arg_value / clamp_arg_rounds_away, csrc/lzq_quad.h zsum<.., CLAMP = true>
// and zsum_dispatch's clamped branch), for ONE 64-lane wavefront and for one lane; for
// tests/test_zsum_clamp_arg_host.py (TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off).  The
// predicates, the batch search, the table values and the nodes are the LZQ_HD functions of csrc/lzq_exp2.h
// that the device code calls.  The pass is classified with the dispatch's order all-dead -> zero ->
// clamp-free -> clamped (the first three are tests/zsum_frozen_host.cpp's and run the general loop here),
// and a pass of the last kind runs
//   mode -1  the general loop of LZQ_CLAMP_ARG=0 (exp2_tab_scaled at every node: the index clamped, s not);
//   mode  0  the new general loop (exp2_tab_scaled_clamp_arg at every node);
//   mode  1  the new dispatch: the new general loop up to k2 (seg_clamped_or_dead over the 64 lanes), then
//            F's accumulate alone with one value per lane -- v_c, or seg_node_dead on the lane's own entry
//            where the wave holds dead lanes.
//
// `defect` builds a deliberately broken mode 1, which the test must tell from the right one:
//   1  a wrong v_c: the suffix holds the value of the =0 node at k2 (its stray fractional part kept);
//   2  the suffix starts one batch before k2;
//   3  a lost node: the suffix's last node is not executed.
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
  int n = 0;
  void add(double om, int k, double v) {
    F = __builtin_fma(om, v, F);
    h += __builtin_bit_cast(uint64_t, v) * (uint64_t)(2 * k + 1);
    ++n;
  }
};

int padded_nodes(int nz) {
  const int n = nz > kUnroll ? nz : kUnroll;
  return (n + kUnroll - 1) / kUnroll * kUnroll;
}

double node_of(int mode, double c2N, double g, const double* tab) {
  return mode < 0 ? exp2_tab_scaled(c2N, g, tab) : exp2_tab_scaled_clamp_arg(c2N, g, tab);
}

// plan = {path, k2, kend, number of dead lanes, nodes executed per lane}; Fraw: F before the dead lanes are zeroed
void pass(int mode, int defect, bool truncate, const std::vector<double>& g, const std::vector<double>& om, int nz,
          const double* c2, double* Fraw, double* F, uint64_t* V, int* plan) {
  const int nzp = (int)g.size();
  const double g_1 = g[1], g_max = g[nz - 1];
  bool dead[kLanes], small = true, all_dead = true, any_dead = false, zero = true;
  double c2e[kLanes];
  int ndead = 0, executed = 0;
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
  else path = any_dead ? kPathMixed : kPathSplit;
  if (mode < 1 || !last_branch) {
    for (int l = 0; l < kLanes; ++l) {
      Acc acc;
      for (int k = 0; k < kend; ++k) acc.add(om[k], k, node_of(mode, c2e[l], g[k], tab));
      Fraw[l] = acc.F, V[l] = acc.h, executed = acc.n;
    }
    if (last_branch) {  // the plan's k2, for the brute-force scan, whatever loop ran
      k2 = seg_first_batch(
          [&](double gk) {
            bool c = true;
            for (int l = 0; l < kLanes; ++l) c = c && seg_clamped_or_dead(dead[l], c2e[l], gk, kTabMagic);
            return c;
          },
          [&](int k) { return g[k]; }, kend, kUnroll);
    }
  } else {
    k2 = seg_first_batch(
        [&](double gk) {
          bool c = true;
          for (int l = 0; l < kLanes; ++l) c = c && seg_clamped_or_dead(dead[l], c2e[l], gk, kTabMagic);
          return c;
        },
        [&](int k) { return g[k]; }, kend, kUnroll);
    int ks = k2;  // where the suffix starts
    if (defect == 2 && ks >= kUnroll) ks -= kUnroll;
    const int ke = defect == 3 && kend > ks ? kend - 1 : kend;
    const double Tc = seg_entry(tab, kTabTClamp);  // the uniform case's entry
    for (int l = 0; l < kLanes; ++l) {
      // zsum_dead's v0 from the entry of M + KMIN, or zsum_held's per-lane value from the lane's own entry
      double v = any_dead ? seg_node_dead(kSqA, seg_entry_lane(tab, dead[l])) : seg_node_dead(kSqA, Tc);
      if (defect == 1 && !dead[l] && ks < kend) v = exp2_tab_scaled(c2e[l], g[ks], tab);
      Acc acc;
      for (int k = 0; k < ks; ++k) acc.add(om[k], k, exp2_tab_scaled_clamp_arg(c2e[l], g[k], tab));
      for (int k = ks; k < ke; ++k) acc.add(om[k], k, v);
      Fraw[l] = acc.F, V[l] = acc.h, executed = acc.n;
    }
  }
  for (int l = 0; l < kLanes; ++l) F[l] = dead[l] ? 0.0 : Fraw[l];
  if (plan) {
    plan[0] = path;
    plan[1] = k2;
    plan[2] = kend;
    plan[3] = ndead;
    plan[4] = executed;
  }
}

}  // namespace

extern "C" {

// n passes of 64 lanes each (see pass)
int zca_passes(int mode, int defect, int truncate, const double* g4, const double* omega, int nz, const double* c2,
               long n, double* Fraw, double* F, uint64_t* V, int* plan) {
  if (nz < 2 || !kSqForm || mode < -1 || mode > 1 || defect < 0 || defect > 3) return -1;
  build_tab();
  const int nzp = padded_nodes(nz);
  std::vector<double> g(nzp), om(nzp);
  for (int k = 0; k < nzp; ++k) {
    g[k] = k < nz ? g4[k] : g4[nz - 1];
    om[k] = k < nz ? ldexp(omega[k], -kOmegaBias) : 0.0;
  }
  for (long i = 0; i < n; ++i)
    pass(mode, defect, truncate != 0, g, om, nz, c2 + i * kLanes, Fraw + i * kLanes, F + i * kLanes, V + i * kLanes,
         plan ? plan + 5 * i : nullptr);
  return 0;
}

// one lane at the n arguments (c2N[i], g4[i]): v[0][i] the =0 node, v[1][i] the new node, v[2][i] the magic sum t
int zca_nodes(const double* c2N, const double* g4, int n, double* v) {
  build_tab();
  for (int i = 0; i < n; ++i) {
    v[i] = exp2_tab_scaled(c2N[i], g4[i], g_tab);
    v[n + i] = exp2_tab_scaled_clamp_arg(c2N[i], g4[i], g_tab);
    v[2 * n + i] = __builtin_fma(c2N[i], g4[i], kTabMagic);
  }
  return 0;
}

// one lane's accumulate over the n nodes (g4[k], omega'[k]) -- omega' ALREADY scaled by 2^-512 -- with F
// entering as F0; mode -1 the =0 node, 0 the new node.  Returns F.
double zca_lane(int mode, double c2N, const double* g4, const double* omega_scaled, int n, double F0) {
  build_tab();
  double F = F0;
  for (int k = 0; k < n; ++k) F = __builtin_fma(omega_scaled[k], node_of(mode, c2N, g4[k], g_tab), F);
  return F;
}

double zca_vc() { return clamp_arg_value(); }
double zca_vc_from_table() {
  build_tab();
  return seg_node_dead(kSqA, seg_entry(g_tab, kTabTClamp));
}
double zca_tclamp() { return kTabTClamp; }
double zca_kmin() { return (double)kTabKMin; }
int zca_rounds_away(double omega_scaled, double v) { return clamp_arg_rounds_away(omega_scaled, v) ? 1 : 0; }
// the library's check of a grid's weights (omega as lzq_ztables returns it, unscaled)
int zca_grid_ok(const double* omega, int n) {
  return clamp_arg_grid_ok([&](int k) { return ldexp(omega[k], -kOmegaBias); }, n) ? 1 : 0;
}

}  // extern "C"
