// Host restatement of yb_wave's pass loop with the accumulate-only loops fed from the packed omega' array
// of the grid's device image (csrc/lzq_quad.h acc_omega, LZQ_ACC_FEED; csrc/lzq_exp2.h zimage_doubles /
// zimage_pack / zimage_omega) for ONE point = one 64-lane wavefront; for tests/test_zsum_feed_host.py and
// tools/uniform_segment_share.py (TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off).
//
// The image is built as the library's three producers build it: nzp {g4, omega'} nodes (padding: the last
// g4, omega' = +0), then zimage_pack.  The pass loop is tests/zsum_group_host.cpp's zgroup_point (included
// below: the grouped passes and, per pass, tests/zsum_frozen_host.cpp's dispatch), run on the NODES' weights.
// With feed = 1 the three accumulate-only loops are then run again as the device runs them, on the weights
// zimage_omega hands out: the all-dead pass (zsum_dead), the held tail of a live zero pass from its k3
// (zsum_held; the nodes before k3 are zsum_uniform's and keep the node's own weight), and every chain of a
// grouped sweep.  Same values, same order; F, the checksum over every node's value AND weight, and acc must
// not move.  (The checksum of zsum_frozen_host.cpp covers the node values; `W` here covers the weights read.)
//
// `defect` builds a deliberately broken feed, which the test must tell from the right one:
//   1  the packed array is looked for behind the grid's nz real nodes, not its nzp padded ones (the same
//      place on a grid that needs no padding);
//   2  a held tail reads the packed array from its start, not from its own k3.
#include "zsum_group_host.cpp"

namespace {

struct Node {
  double g4, omega;
};

// one chain over nodes [kbeg, kend) with a fixed value, its weights from w[k - shift]
void feed_chain(const double* w, int kbeg, int kend, int shift, double v, double* F, uint64_t* W) {
  for (int k = kbeg; k < kend; ++k) {
    const double om = w[k - shift];
    *F = __builtin_fma(om, v, *F);
    *W += __builtin_bit_cast(uint64_t, om) * (uint64_t)(2 * k + 1);
  }
}

}  // namespace

extern "C" {

int zfeed_image_doubles(int nz) { return zimage_doubles(padded_nodes(nz)); }

// the device image of a grid: out[zfeed_image_doubles(nz)]
int zfeed_image(const double* g4, const double* omega, int nz, double* out) {
  if (nz < 2) return -1;
  const int nzp = padded_nodes(nz);
  Node* nodes = reinterpret_cast<Node*>(out);
  for (int k = 0; k < nzp; ++k) nodes[k] = k < nz ? Node{g4[k], ldexp(omega[k], -kOmegaBias)} : Node{g4[nz - 1], 0.0};
  zimage_pack(nodes, nzp);
  return 0;
}

// One point, as zgroup_point (same arguments and outputs), then with feed = 1 the accumulate-only loops
// again from the packed array.  W[pass * 64 + lane]: checksum over the weights the lane's accumulate-only
// nodes read (0 where the pass has none); fed[pass]: the pass's nodes that read the packed array.
int zfeed_point(int feed, int defect, int gmax, int truncate, const double* g4, const double* omega, int nz,
                const double* c2, const double* wy, long n, double* F, uint64_t* V, double* acc, int* plan, uint64_t* W,
                int* fed) {
  if (feed < 0 || feed > 1 || defect < 0 || defect > 2) return -1;
  const int rc = zgroup_point(gmax, 0, truncate, g4, omega, nz, c2, wy, n, F, V, acc, plan);
  if (rc) return rc;
  const int nzp = padded_nodes(nz);
  std::vector<double> image(zimage_doubles(nzp));
  zfeed_image(g4, omega, nz, image.data());
  const Node* nodes = reinterpret_cast<const Node*>(image.data());
  const double* packed = defect == 1 ? image.data() + 2 * nz : zimage_omega(nodes, nzp);
  std::vector<double> g(nzp), own(nzp);
  for (int k = 0; k < nzp; ++k) g[k] = nodes[k].g4, own[k] = nodes[k].omega;
  const double g_1 = g[1];
  const double Ts0 = seg_entry(g_tab, kTabMagic);
  const long npass = (n + kLanes - 1) / kLanes;
  for (long p = 0; p < npass; ++p) {
    const int* pl = plan + 4 * p;
    const bool group = pl[0] > 1;
    const bool accumulate_only = pl[1] == kPathDead || pl[1] == kPathZero;
    fed[p] = 0;
    for (int l = 0; l < kLanes; ++l) W[p * kLanes + l] = 0;
    if (!accumulate_only) continue;
    // the pass's end and tail start, as the dispatch finds them (zsum_frozen_host.cpp's pass)
    double c2p[kLanes];
    for (int l = 0; l < kLanes; ++l) c2p[l] = c2[p * kLanes + l < n ? p * kLanes + l : n - 1];
    int pp[4];
    std::vector<double> Fs(kLanes);
    std::vector<uint64_t> Vs(kLanes);
    pass(2, 0, truncate != 0, g, own, nz, c2p, Fs.data(), Vs.data(), pp);
    const int kend = pp[2], k3 = group ? 0 : (pl[1] == kPathDead ? 0 : pp[3]);
    if (k3 >= kend) continue;
    fed[p] = kend - k3;
    const double g_last = g[kend > 0 ? kend - 1 : 0];
    for (int l = 0; l < kLanes; ++l) {
      const bool dead = c2p[l] * g_1 <= -(double)kTabN * kDeadOct;
      const double c2e = dead ? 0.0 : c2p[l];
      // the head (zsum_uniform<1, true>): the node's own weight
      double Fl = 0.0;
      for (int k = 0; k < k3; ++k) Fl = __builtin_fma(own[k], seg_node_zero(c2e, g[k], kSqA, Ts0), Fl);
      // the accumulate-only stretch: an all-dead single pass or group has seg_node_dead's value, every other
      // the lane's held one
      const bool all_dead = pl[1] == kPathDead;
      const double v = all_dead ? seg_node_dead(kSqA, Ts0) : seg_value_frozen_s(c2e, g_last, kSqA, Ts0);
      uint64_t Wl = 0;
      feed_chain(feed ? packed : own.data(), k3, kend, feed && defect == 2 ? k3 : 0, v, &Fl, &Wl);
      F[p * kLanes + l] = dead ? 0.0 : Fl;
      W[p * kLanes + l] = Wl;
    }
  }
  // the y-integration again, in pass order, on the F just formed
  for (int l = 0; l < kLanes; ++l) acc[l] = 0.0;
  for (long p = 0; p < npass; ++p)
    for (int l = 0; l < kLanes; ++l) {
      const long j = p * kLanes + l;
      acc[l] = __builtin_fma(j < n ? wy[j] : 0.0, F[p * kLanes + l], acc[l]);
    }
  return 0;
}

}  // extern "C"
