// lzq_cont.hip -- A/V in the continuum limit of the z grid (lzq_cont.h): the node
// table's device image, the live-range z-sum kernels and the *_cont entry points of include/lzq.h.
//
// The continuum node table is a z table like a linspace grid's: its z-sums go through zsum_dispatch
// (lzq_quad.h), and the integration, window and solve kernels read the tables they fill (the host
// wrappers of lzq_kernels.hip with cont = true, lzq_internal.h).  New here is the table kernel.
//
// Live range.  gamma4 rises with z and the table ascends in z, so the nodes whose term
// omega 2^(c2 gamma4) is below 2^-1080 for every lane of a wavefront -- and which the accumulate's
// rounding discards, an exact +0 -- are the table's tail from a node kend on.  The lanes of a pass
// hold 64 consecutive y-nodes, a = -c within a factor e^(63 step) of each other, so kend is one
// wave-uniform number per pass (zsum_dispatch's truncation: a binary search over the node table on
// the scalar unit) and falls from the whole table for y < 7.7 (I_p = 0.34) to the panels below
// z ~ 1e-4 at y = 50, where the integrand's cut-off z_c = (4/a)^(1/4) is 1e-5: the live range is 144
// of the table's 528 nodes there and 82% of the nodes over the shipped y-grid (y from -48 to 50).
// The z-loops before kend are the linspace grids', node for node.
//
// The table kernel of the linspace grids gives a wavefront a whole table, 125 passes at n_y = 8000
// one after the other; a sweep has few tables (C4: 1000, an eighth of the device's wave slots).
// In table mode the passes are independent, so here a wavefront is one (table, pass) pair:
// 125 x the wavefronts, every one a single short z-loop, and the exp table staged once per block of
// 16 of them.  The node feed stays wave-uniform (scalar loads of {gamma4, omega'}, an SGPR operand of
// every FP64 instruction), the exponential's table stays in LDS.  F is bit for bit the every-node
// table's (LZQ_TUNE_CONT_SKIP = 0): the same y, c2 and zsum_dispatch on the same operands
// (tests/test_gpu_cont.py).
//
// Not built: replacing the leading nodes, where every lane's exponential returns its value at 0, by
// a precomputed running sum.  It is bit-identical only if the prefix sums are formed by the same
// fma chain from the same v = T''(0) (A^2 + beta), per exponential variant and per lane's frozen
// s; the zero-pass loops of zsum_dispatch (y < -9 at I_p = 0.34, 40% of the shipped y-grid's passes)
// already run those nodes as F's accumulate alone from the batch at which every lane's value stops
// changing (lzq_quad.h LZQ_FROZEN_SEG).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../include/lzq.h"
#include "lzq_quad.h"
#include "lzq_internal.h"
#include "lzq_cont.h"

namespace lzq {

int g_cont_skip = 1;

// fpy:158-165 on the continuum table, one lane per y value (aov_kernel's operations; truncate: the
// wavefront's live range)
template <int EXPV>
__global__ __launch_bounds__(kBlock) void aov_cont_kernel(ContKernel k, const double* __restrict__ ys, int64_t n,
                                                         const ZNode* __restrict__ zt, int32_t nzp,
                                                         const double* __restrict__ gtab, double* __restrict__ out,
                                                         int truncate) {
  __shared__ double lds_tab[kTabN];
  const double* tab = stage_table<EXPV>(gtab, lds_tab);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  const double y = live ? ys[i] : 0.0;
  const double pref0 = uniform(k.pref0), cneg = uniform(k.cneg);
  const double expy = exp_sc(pymax(pymin(y, 50.0), -50.0));
  double c2[1] = {((cneg * expy) * kLog2E) * c2_scale<EXPV>()}, F[1];
  zsum_dispatch<1, EXPV>(zt, nzp, tab, c2, F, truncate);
  if (live) out[i] = (y > 50.0) ? 0.0 : (pref0 * expy) * F[0];
}

// The live-range table kernel: wavefront (t, pass) writes the F of y-nodes [64 pass, 64 pass + 64) of
// table t, pass 0 its header too (ztable_wave's).  pts: table t is point pts[reps[t]]'s, else the
// grid's (table_rep).  An empty y range leaves the F values unwritten, as yb_wave does.
template <int EXPV>
__global__ __launch_bounds__(kBlock, LZQ_MIN_WAVES) void cont_ztable_kernel(
    lzq_point base, GridSpec grid, const lzq_point* __restrict__ pts, const int64_t* __restrict__ reps, int64_t n_tab,
    int32_t n_y, int32_t passes, int64_t tstride, const ZNode* __restrict__ zt, int32_t nzp, ZKey zk,
    const double* __restrict__ gtab, double* __restrict__ Fw) {
  __shared__ double lds_tab[kTabN];
  const double* tab = stage_table<EXPV>(gtab, lds_tab);
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + w;
  const int64_t t = wave / passes;
  if (t >= n_tab) return;  // wave-uniform
  const int pass = (int)(wave - t * passes);
  lzq_point pt;
  double P;
  if (pts) {
    pt = pts[reps[t]];
    P = pt.P_chi_to_B;
  } else {
    P = grid_point(base, grid, table_rep(grid, t), pt);
  }
  const QuadSetup qs = quad_setup(pt, P, pt.T_min_over_Tp * pt.T_p_GeV, pt.T_max_over_Tp * pt.T_p_GeV, n_y);
  double* F = Fw + t * tstride;
  if (pass == 0 && lane == 0) {
    F[0] = qs.y_lo;
    F[1] = qs.y_hi;
    F[2] = (double)qs.n;
    F[3] = qs.cneg;
    F[4] = zk.nz;
    F[5] = zk.z_max;
  }
  if (qs.empty) return;
  const int n = (int)qs.n;
  const int j = pass * kWaveSize + lane;
  const int jj = j < n ? j : n - 1;  // tail lanes recompute the last node
  const double y = y_node(qs, jj);
  const double ey = exp_sc(pymax(pymin(y, 50.0), -50.0));                   // fpy:161
  double c2[1] = {((qs.cneg * ey) * kLog2E) * c2_scale<EXPV>()}, Fv[1];  // fpy:163 c, log2 units
  zsum_dispatch<1, EXPV>(zt, nzp, tab, c2, Fv, 1);
  if (j < n) F[kTabHdr + j] = Fv[0];
}

}  // namespace lzq

namespace {

#define LZQ_HIP(call)                                                    \
  do {                                                                   \
    hipError_t e_ = (call);                                              \
    if (e_ != hipSuccess) {                                              \
      char m_[400];                                                      \
      snprintf(m_, sizeof(m_), "%s: %s", #call, hipGetErrorString(e_)); \
      return lzq_set_error(LZQ_EHIP, m_);                                \
    }                                                                    \
  } while (0)

int fail(int code, const char* fn, const char* what) {
  char m[400];
  snprintf(m, sizeof(m), "%s: %s", fn, what);
  return lzq_set_error(code, m);
}

std::mutex g_mu;
struct HostEntry {
  uint64_t zbits;
  lzq::ContTable t;
};
struct DevEntry {
  int dev;
  uint64_t zbits;
  lzq::ZNode* d;
  int32_t nzp;
};
std::vector<HostEntry*> g_host;  // one table per z_max, built once (guarded by g_mu)
std::vector<DevEntry> g_dev;     // uploaded on first use per (device, z_max)

// the host table of z_max (g_mu held)
int host_table(double z_max, const char* fn, const lzq::ContTable** out) {
  const uint64_t zb = __builtin_bit_cast(uint64_t, z_max);
  for (const HostEntry* e : g_host)
    if (e->zbits == zb) {
      *out = &e->t;
      return LZQ_OK;
    }
  HostEntry* e = new HostEntry{zb, {}};
  const char* why = lzq::cont_build(z_max, e->t);
  if (why) {
    delete e;
    char m[200];
    snprintf(m, sizeof(m), "z_max = %g: %s", z_max, why);
    return fail(LZQ_EINVAL, fn, m);
  }
  g_host.push_back(e);
  *out = &e->t;
  return LZQ_OK;
}

// The A/V kernel's fields of *pt with aov's over them (lzq_aov_batch's rule).
int kernel_of(const lzq_point* pt, const lzq_aov_params* aov, const char* fn, lzq::ContKernel& k) {
  if (!pt && !aov) return fail(LZQ_EINVAL, fn, "bad arguments");
  lzq_aov_params a;
  if (aov) a = *aov;
  else a = lzq_aov_params{pt->I_p, pt->beta_over_H, pt->T_p_GeV, pt->v_w, pt->g_star};
  k = lzq::cont_kernel(a.I_p, a.beta_over_H, a.T_p_GeV, a.v_w, a.g_star);
  return LZQ_OK;
}

}  // namespace

// Device image: a leading (gamma4 = 0, omega = 0) node -- a linspace grid's node 0, which the dead-lane
// rule and the padding of zsum_dispatch are keyed on -- the N nodes with omega 2^-512, then the padding
// to the unroll (the last gamma4 again, omega = 0).
int lzq::cont_grid_for(int dev, double z_max, const ZNode** zt, int32_t* nzp) {
  const uint64_t zb = __builtin_bit_cast(uint64_t, z_max);
  std::lock_guard<std::mutex> lk(g_mu);
  for (const DevEntry& e : g_dev)
    if (e.dev == dev && e.zbits == zb) {
      *zt = e.d;
      *nzp = e.nzp;
      return LZQ_OK;
    }
  const ContTable* t;
  int rc = host_table(z_max, "continuum z rule", &t);
  if (rc) return rc;
  const int32_t n = (int32_t)t->z.size() + 1;
  const int32_t np = (n + kKUnroll - 1) / kKUnroll * kKUnroll;
  // (the image of every z grid: the nodes, then their weights packed -- zimage_pack, lzq_exp2.h)
  static_assert(sizeof(ZNode) == 2 * sizeof(double), "ZNode layout");
  std::vector<double> image(zimage_doubles(np));
  ZNode* host = reinterpret_cast<ZNode*>(image.data());
  host[0] = ZNode{0.0, 0.0};
  for (int32_t k = 1; k < np; ++k)
    host[k] = k < n ? ZNode{t->g4[k - 1], ldexp(t->omega[k - 1], -kOmegaBias)} : ZNode{t->g4[n - 2], 0.0};
  zimage_pack(host, np);
  void* dv = nullptr;
  LZQ_HIP(hipMalloc(&dv, image.size() * sizeof(double)));
  LZQ_HIP(hipMemcpy(dv, image.data(), image.size() * sizeof(double), hipMemcpyHostToDevice));
  ZNode* d = static_cast<ZNode*>(dv);
  g_dev.push_back(DevEntry{dev, zb, d, np});
  *zt = d;
  *nzp = np;
  return LZQ_OK;
}

int lzq::launch_cont_ztables(int exp_variant, const lzq_point* base, const GridSpec* grid, const lzq_point* pts,
                             const int64_t* reps, int64_t n_tab, int32_t n_y, int64_t tstride, const ZNode* zt,
                             int32_t nzp, double key_z_max, const double* gtab, double* d_work, hipStream_t s) {
  if (n_tab == 0) return LZQ_OK;
  const int32_t n = n_y > LZQ_NY_MIN ? n_y : LZQ_NY_MIN;
  const int32_t passes = (n + kWaveSize - 1) / kWaveSize;
  if (n_tab > INT64_MAX / passes) return fail(LZQ_EINVAL, "continuum z-sum tables", "too large for one launch");
  const int64_t nb = (n_tab * passes + kWavesPerBlock - 1) / kWavesPerBlock;
  if (nb > 2147483647LL) return fail(LZQ_EINVAL, "continuum z-sum tables", "too large for one launch");
  lzq_point b;
  GridSpec g;
  memset(&b, 0, sizeof(b));
  memset(&g, 0, sizeof(g));
  if (!pts) {
    b = *base;
    g = *grid;
  }
  const ZKey zk{kContKeyNz, key_z_max};
  if (exp_variant == kExpTable)
    hipLaunchKernelGGL((cont_ztable_kernel<kExpTable>), dim3((unsigned)nb), dim3(kBlock), 0, s, b, g, pts, reps, n_tab,
                       n_y, passes, tstride, zt, nzp, zk, gtab, d_work);
  else
    hipLaunchKernelGGL((cont_ztable_kernel<kExpPoly11>), dim3((unsigned)nb), dim3(kBlock), 0, s, b, g, pts, reps, n_tab,
                       n_y, passes, tstride, zt, nzp, zk, gtab, d_work);
  LZQ_HIP(hipGetLastError());
  return LZQ_OK;
}

extern "C" {

int lzq_cont_tables(double z_max, double* z, double* gamma4, double* omega, int32_t* n) {
  std::lock_guard<std::mutex> lk(g_mu);
  const lzq::ContTable* t;
  const int rc = host_table(z_max, "lzq_cont_tables", &t);
  if (rc) return rc;
  const size_t bytes = sizeof(double) * t->z.size();
  if (n) *n = (int32_t)t->z.size();
  if (z) memcpy(z, t->z.data(), bytes);
  if (gamma4) memcpy(gamma4, t->g4.data(), bytes);
  if (omega) memcpy(omega, t->omega.data(), bytes);
  return LZQ_OK;
}

int lzq_aov_cont_host(const lzq_point* pt, const lzq_aov_params* aov, const double* y, int64_t n, double z_max,
                      double* out) {
  const char* fn = "lzq_aov_cont_host";
  if (n < 0 || (n > 0 && (!y || !out))) return fail(LZQ_EINVAL, fn, "bad arguments");
  lzq::ContKernel k;
  int rc = kernel_of(pt, aov, fn, k);
  if (rc) return rc;
  const lzq::ContTable* t;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    rc = host_table(z_max, fn, &t);  // entries are never freed or moved
  }
  if (rc) return rc;
  for (int64_t i = 0; i < n; ++i)
    out[i] = lzq::cont_aov(k, y[i], t->g4.data(), t->omega.data(), (int32_t)t->z.size(), [](double x) { return exp(x); });
  return LZQ_OK;
}

int lzq_aov_batch_cont(const lzq_point* pt, const lzq_aov_params* aov, const double* d_y, int64_t n, double z_max,
                       double* d_out, void* stream) {
  const char* fn = "lzq_aov_batch_cont";
  if (n < 0 || (n > 0 && (!d_y || !d_out))) return fail(LZQ_EINVAL, fn, "bad arguments");
  lzq::ContKernel k;
  int rc = kernel_of(pt, aov, fn, k);
  if (rc) return rc;
  if (!(z_max > 0.0) || !(z_max <= 0x1.fffffffffffffp1023)) return fail(LZQ_EINVAL, fn, "z_max must be finite and > 0");
  if (n == 0) return LZQ_OK;
  int dev, exp_variant;
  const double* gtab;
  rc = lzq::device_exp_table(&dev, &gtab, &exp_variant);
  if (rc) return rc;
  const lzq::ZNode* zt;
  int32_t nzp;
  rc = lzq::cont_grid_for(dev, z_max, &zt, &nzp);
  if (rc) return rc;
  const int64_t nb = (n + lzq::kBlock - 1) / lzq::kBlock;
  if (nb > 2147483647LL) return fail(LZQ_EINVAL, fn, "n too large");
  if (exp_variant == lzq::kExpTable)
    hipLaunchKernelGGL(lzq::aov_cont_kernel<lzq::kExpTable>, dim3((unsigned)nb), dim3(lzq::kBlock), 0,
                       (hipStream_t)stream, k, d_y, n, zt, nzp, gtab, d_out, lzq::g_cont_skip);
  else
    hipLaunchKernelGGL(lzq::aov_cont_kernel<lzq::kExpPoly11>, dim3((unsigned)nb), dim3(lzq::kBlock), 0,
                       (hipStream_t)stream, k, d_y, n, zt, nzp, gtab, d_out, lzq::g_cont_skip);
  LZQ_HIP(hipGetLastError());
  return LZQ_OK;
}

int lzq_sweep_grid_ztables_cont(const lzq_point* base, const lzq_axis* axes, int32_t n_axes, int32_t n_y, double z_max,
                                double* d_work, int64_t work_doubles, void* stream) {
  return lzq::sweep_grid_reuse_parts(base, axes, n_axes, 0, 0, n_y, 0, z_max, nullptr, d_work, work_doubles, nullptr,
                                     stream, 1, "lzq_sweep_grid_ztables_cont", true, nullptr, nullptr, true);
}

int lzq_sweep_grid_from_ztables_cont(const lzq_point* base, const lzq_window* base_win, const lzq_axis* axes,
                                     int32_t n_axes, int64_t start, int64_t count, int32_t n_y, double z_max,
                                     const double* d_P, const double* d_work, int64_t work_doubles,
                                     const lzq_window_tables* d_tables, lzq_yield* d_out, void* stream) {
  return lzq::sweep_grid_reuse_parts(base, axes, n_axes, start, count, n_y, 0, z_max, d_P, const_cast<double*>(d_work),
                                     work_doubles, d_out, stream, 2, "lzq_sweep_grid_from_ztables_cont",
                                     base_win != nullptr, base_win, d_tables, true);
}

int lzq_sweep_grid_cont(const lzq_point* base, const lzq_window* base_win, const lzq_axis* axes, int32_t n_axes,
                        int64_t start, int64_t count, int32_t n_y, double z_max, const double* d_P, double* d_work,
                        int64_t work_doubles, const lzq_window_tables* d_tables, lzq_yield* d_out, void* stream) {
  // an empty range validates only, as lzq_sweep_grid_reuse (parts = 2 builds nothing)
  return lzq::sweep_grid_reuse_parts(base, axes, n_axes, start, count, n_y, 0, z_max, d_P, d_work, work_doubles, d_out,
                                     stream, count == 0 ? 2 : 3, "lzq_sweep_grid_cont", base_win != nullptr, base_win,
                                     d_tables, true);
}

int lzq_yields_batch_cont(const lzq_point* d_points, int64_t n, int32_t n_y, double z_max, const double* d_P,
                          const int64_t* d_rep, const int32_t* d_table_index, int64_t n_tables, double* d_work,
                          int64_t work_doubles, const lzq_window* d_win, const lzq_window_tables* d_tables,
                          lzq_yield* d_out, void* stream) {
  const char* fn = "lzq_yields_batch_cont";
  lzq_window_tables wt = {0, 0, nullptr, nullptr};
  if (d_win) {
    const int rc = lzq::window_tables_arg(d_tables, fn, wt);
    if (rc) return rc;
  }
  return lzq::yields_batch_reuse(d_points, n, n_y, 0, z_max, d_P, d_rep, d_table_index, n_tables, d_work, work_doubles,
                                 d_win, &wt, d_out, stream, true, fn);
}

int lzq_sweep_grid_solve_cont(const lzq_point* base, const lzq_window* base_win, const lzq_axis* axes, int32_t n_axes,
                              const lzq_solve* solve, int64_t start, int64_t count, int32_t n_y, double z_max,
                              const double* d_P, const double* d_work, int64_t work_doubles,
                              const lzq_window_tables* d_tables, lzq_yield* d_out, lzq_solve_result* d_sol,
                              void* stream) {
  return lzq::sweep_grid_solve(base, base_win, axes, n_axes, solve, start, count, n_y, 0, z_max, d_P, d_work,
                               work_doubles, d_tables, d_out, d_sol, stream, true, "lzq_sweep_grid_solve_cont");
}

}  // extern "C"
