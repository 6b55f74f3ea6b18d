// Host restatement of yb_wave's pass loop with grouped passes (csrc/lzq_quad.h yb_group / yb_group_run,
// LZQ_GROUP_SEG) for ONE point = one 64-lane wavefront; for tests/test_zsum_group_host.py and
// tools/uniform_segment_share.py (TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off).
//
// The single pass is tests/zsum_frozen_host.cpp's `pass` (included below: zsum_dispatch with the frozen
// tails, FROZEN = 2).  The group's classification is seg_group_slot / seg_group_kind of csrc/lzq_exp2.h,
// the LZQ_HD functions the device's yb_group calls; its values are seg_node_dead, seg_entry and
// seg_value_frozen_s, the ones zsum_dead and zsum_held take.  Around them this file mirrors yb_wave:
// the wave-uniform cue `grp`, the sizes tried at each base (gmax, then gmax / 2, full passes only, never
// under truncation), the G chains per lane each in node order from 0, the zeroing of dead lanes, and the
// y-integration acc = fma(w_j, F_j, acc) of the G passes in ascending pass order.  (The device multiplies
// F_j by the y-factors first; they do not depend on how F_j was summed, so the model's integrand is F_j.)
//
// `defect` builds a deliberately broken loop, which the test must tell from the right one:
//   1  the group test looks at slot 0 only;
//   2  the G passes of a group are integrated in descending pass order.
#include "zsum_frozen_host.cpp"

namespace {

// one lane's chain over all nodes with a fixed value
void chain(const std::vector<double>& om, int kend, double v, double* F, uint64_t* V) {
  Acc a;
  for (int k = 0; k < kend; ++k) a.add(om[k], k, v);
  *F = a.F, *V = a.h;
}

}  // namespace

extern "C" {

int zgroup_slot(double c2N, double g_0, double g_1, double g_last) {
  return seg_group_slot(c2N, g_0, g_1, g_last, kTabMagic, kSqA);
}

// One point: n y-nodes with c2N = c2[j] and integration weight wy[j], passes of 64 (tail lanes recompute
// the last node with weight 0, as yb_wave's do).  gmax = LZQ_GROUP_SEG (0, 2 or 4).  Out: F and V (node
// value checksum) per pass and lane, acc per lane, plan per pass = {size of the group the pass ran in
// (1: single), its path (zsum_frozen_host.cpp's Path; a held group is kPathZero, an all-dead one kPathDead),
// 1 if a group classification was made at this pass's base, the pass's k3 (0 in a group)}.
int zgroup_point(int gmax, int defect, int truncate, const double* g4, const double* omega, int nz, const double* c2,
                 const double* wy, long n, double* F, uint64_t* V, double* acc, int* plan) {
  if (nz < 2 || !kSqForm || (gmax != 0 && gmax != 2 && gmax != 4) || defect < 0 || defect > 2 || n < 1) return -1;
  build_tab();
  const int nzp = padded_nodes(nz);
  std::vector<double> g(nzp), om(nzp);
  for (int k = 0; k < nzp; ++k) {
    g[k] = k < nz ? g4[k] : g4[nz - 1];
    om[k] = k < nz ? ldexp(omega[k], -kOmegaBias) : 0.0;
  }
  const double g_0 = g[0], g_1 = g[1], g_last = g[nzp - 1];
  for (int l = 0; l < kLanes; ++l) acc[l] = 0.0;
  bool grp = true;
  for (long base = 0; base < n; base += kLanes) {
    const long p = base / kLanes;
    int attempted = 0;
    if (gmax >= 2 && grp && !truncate) {
      int G = 0;
      if (gmax >= 4 && base + 4 * kLanes <= n) G = 4;
      else if (base + 2 * kLanes <= n) G = 2;
      int ran = 0;
      bool all_dead = false;
      int cls[kLanes];
      if (G) {
        attempted = 1;
        for (int l = 0; l < kLanes; ++l) {
          cls[l] = 0;
          for (int b = 0; b < G; ++b) cls[l] |= seg_group_slot(c2[base + b * kLanes + l], g_0, g_1, g_last, kTabMagic, kSqA) << (2 * b);
        }
        for (int s = G; s >= 2 && !ran; s >>= 1) {
          bool dead = true, whole = true;
          for (int l = 0; l < kLanes; ++l) {
            const int kind = seg_group_kind(cls[l], defect == 1 ? 1 : s);
            dead = dead && (kind & kGrpDead);
            whole = whole && (kind & kGrpWhole);
          }
          if (dead || whole) ran = s, all_dead = dead;
        }
      }
      if (ran) {
        const double Ts0 = seg_entry(g_tab, kTabMagic);
        for (int b = 0; b < ran; ++b)
          for (int l = 0; l < kLanes; ++l) {
            const bool dead = (cls[l] >> (2 * b)) & kGrpDead;
            const double c2e = dead ? 0.0 : c2[base + b * kLanes + l];
            const double v = all_dead ? seg_node_dead(kSqA, Ts0) : seg_value_frozen_s(c2e, g_last, kSqA, Ts0);
            const long o = (p + b) * kLanes + l;
            chain(om, nzp, v, &F[o], &V[o]);
            if (dead) F[o] = 0.0;
          }
        for (int i = 0; i < ran; ++i) {
          const int b = defect == 2 ? ran - 1 - i : i;
          for (int l = 0; l < kLanes; ++l) {
            const long j = base + b * kLanes + l;
            acc[l] = __builtin_fma(wy[j], F[(p + b) * kLanes + l], acc[l]);
          }
          int* pl = plan + 4 * (p + b);
          pl[0] = ran, pl[1] = all_dead ? kPathDead : kPathZero, pl[2] = b == 0 ? 1 : 0, pl[3] = 0;
        }
        base += (long)(ran - 1) * kLanes;
        continue;
      }
      grp = false;
    }
    double c2p[kLanes];
    for (int l = 0; l < kLanes; ++l) c2p[l] = c2[base + l < n ? base + l : n - 1];
    int pp[4];
    pass(2, 0, truncate != 0, g, om, nz, c2p, F + p * kLanes, V + p * kLanes, pp);
    grp = pp[0] == kPathDead || (pp[0] == kPathZero && pp[3] == 0);
    for (int l = 0; l < kLanes; ++l) {
      const long j = base + l;
      acc[l] = __builtin_fma(j < n ? wy[j] : 0.0, F[p * kLanes + l], acc[l]);
    }
    int* pl = plan + 4 * p;
    pl[0] = 1, pl[1] = pp[0], pl[2] = attempted, pl[3] = pp[3];
  }
  return 0;
}

}  // extern "C"
