// lzq_fk.hip -- the momentum-averaged Landau-Zener probability inside the Y_B quadrature (lzq_fk.h;
// include/lzq.h "momentum-averaged LZ probability"): the node table's device image, the
// R-table kernel, the integration kernel and the lzq_fk_* entry points.
//
// R tables.  P-bar depends on a point through mu_j = m/T(y_j), its statistics, delta_0 and its block;
// points equal in those form a class and share one table R_j = P-bar(mu_j).  A wavefront of
// fk_pbar_table_kernel is one (class, 64 y-nodes) pair, one lane per y-node: y_j, the denominator, its
// reciprocal square root and T are y_factors' operations (lzq_quad.h), mu = m/T, then fk_pbar's node
// loop.  The node table comes in by wave-uniform scalar loads (a kernel argument pointer indexed by the
// loop counter), as the z tables do; every lane of a wavefront has the same p, so the p = 0 loop without
// log and exp is a scalar branch.  One more lane past the grid's last node takes mu = m/T_p: the
// P_used of the class's records, by the same fk_pbar.
//
// Integration.  One wavefront per point, its own y-loop over y_factors (lzq_quad.h is not edited and
// yb_wave is not instantiated): the passes, the tail-lane rule, the per-lane fma chain, the butterfly
// and the epilogue are the reuse mode's (yb_wave kYbReuse, reuse_wave), with P = 1 and the window factor
// W(y_j) R_j.  Nothing is held across a z-loop here, so the setup stays in scalar registers and only a
// point's window block is parked in LDS, as window_W reads it.
//
// Not built: skipping the nodes whose weight can no longer change either sum.  Unlike the z-sum's
// tail, where a term below the accumulator's last bit is an exact +0 for every lane at once, the
// weights t (t + 2 mu) W e^-t fall below 2^-53 of the sums only past t ~ 45 (1 of the 25 panels), and
// the cut depends on mu through the sums themselves; bit-identity would have to be shown per class.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <vector>

#define LZQ_QUAD_CONST_LINKAGE static
#include "lzq_quad.h"
#include "lzq_internal.h"
#include "lzq_quad_window.h"  // window_W, WinParams
#include "lzq_fk.h"

namespace lzq {

constexpr int kFkBlock = 256;
constexpr int kFkWaves = kFkBlock / kWaveSize;

// T(y) by the operations of y_factors (denom, rsqrt_pos, T = Tp * rs)
__device__ __forceinline__ double fk_T_of_y(const QuadSetup& s, double y) {
  const double denom = pymax(1.0 + 2.0 * y / s.Bc, 1e-12);  // fpy:252-253
  return s.Tp * rsqrt_pos(denom);                           // fpy:254
}

// lzq_fk_pbar_batch: one lane per (mu, delta_0) pair, one block for all
__global__ __launch_bounds__(kFkBlock) void fk_pbar_eval_kernel(lzq_fk blk, int32_t stats,
                                                                const double* __restrict__ mu,
                                                                const double* __restrict__ delta0, int64_t n,
                                                                const FkNode* __restrict__ tab, int32_t n_nodes,
                                                                double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kFkBlock + threadIdx.x;
  const bool live = i < n;
  const double m = live ? mu[i] : 0.0, d = live ? delta0[i] : 0.0;
  const double r = fk_pbar(m, fk_delta_ok(d) ? fk_g(d) : __builtin_nan(""), blk, stats, tab, n_nodes);
  if (live) out[i] = r;
}

// lzq_fk_tables: wavefront (c, pass) writes R of y-nodes [64 pass, 64 pass + 64) of class c -- node n is
// mu = m/T_p -- and pass 0 the header.  passes = ceil((n + 1) / 64).
__global__ __launch_bounds__(kFkBlock) void fk_pbar_table_kernel(const lzq_point* __restrict__ pts,
                                                                 const double* __restrict__ delta0,
                                                                 const lzq_fk* __restrict__ fk,
                                                                 const int64_t* __restrict__ reps, int64_t n_classes,
                                                                 int32_t n_y, int32_t passes, int64_t rstride,
                                                                 const FkNode* __restrict__ tab, int32_t n_nodes,
                                                                 double* __restrict__ Rw, double* __restrict__ mu_out) {
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wave = (int64_t)blockIdx.x * kFkWaves + w;
  const int64_t c = wave / passes;
  if (c >= n_classes) return;  // wave-uniform
  const int pass = (int)(wave - c * passes);
  const int64_t rep = reps[c];
  const lzq_point pt = pts[rep];
  const lzq_fk blk = fk[rep];
  const double d0 = delta0[rep];
  const QuadSetup qs = quad_setup(pt, 1.0, pt.T_min_over_Tp * pt.T_p_GeV, pt.T_max_over_Tp * pt.T_p_GeV, n_y);
  const int n = (int)qs.n;
  const double g = fk_delta_ok(d0) ? fk_g(d0) : __builtin_nan("");
  double* R = Rw + c * rstride;
  if (pass == 0 && lane == 0) {
    const FkKey key = fk_key(qs.y_lo, qs.y_hi, qs.n, qs.Tp, qs.Bc, qs.m, pt.stats, g, blk);
#pragma unroll
    for (int i = 0; i < kFkHdr; ++i) R[i] = key.k[i];
  }
  const int j = pass * kWaveSize + lane;
  if (j > n) return;  // past the P_used slot
  // (an empty y range has no nodes to integrate; its R_j are formed all the same, from a grid that
  // runs backwards -- finite values nobody reads)
  const double T = j < n ? fk_T_of_y(qs, y_node(qs, j)) : qs.Tp;
  const double mu = qs.m / T;
  R[kFkHdr + j] = fk_pbar(mu, g, blk, pt.stats, tab, n_nodes);
  if (mu_out) mu_out[c * (int64_t)(n + 1) + j] = mu;
}

struct FkWaveSlot {
  WinParams win;
};

// lzq_yields_batch_reuse_fk
__global__ __launch_bounds__(kBlock) void points_reuse_fk_kernel(
    const lzq_point* __restrict__ pts, const double* __restrict__ delta0, const lzq_fk* __restrict__ fk,
    const lzq_window* __restrict__ win, lzq_window_tables wt, int64_t n_pts, int32_t n_y, double key_nz,
    double key_z_max, const int32_t* __restrict__ tidx, const double* __restrict__ Fw, int64_t tstride,
    int64_t n_tables, const int32_t* __restrict__ cidx, const double* __restrict__ Rw, int64_t rstride,
    int64_t n_classes, lzq_yield* __restrict__ out) {
  __shared__ FkWaveSlot slots[kWavesPerBlock];
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t idx = (int64_t)blockIdx.x * kWavesPerBlock + w;
  if (idx >= n_pts) return;  // wave-uniform
  const lzq_point pt = pts[idx];
  const lzq_fk blk = fk[idx];
  const double d0 = delta0[idx];
  const bool has_win = win != nullptr;
  if (has_win) {
    if (lane == 0) slots[w].win = window_params(win[idx], wt.n_tables, wt.n_knots, wt.u, wt.W);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  const QuadSetup qs = quad_setup(pt, 1.0, pt.T_min_over_Tp * pt.T_p_GeV, pt.T_max_over_Tp * pt.T_p_GeV, n_y);
  const bool usable = fk_block_error(blk) == kFkOk && fk_delta_ok(d0);
  const int64_t ti = tidx[idx], ci = cidx[idx];
  const bool in_range = ti >= 0 && ti < n_tables && ci >= 0 && ci < n_classes;
  bool match = false;
  const double* F = Fw;
  const double* R = Rw;
  if (usable && in_range) {  // (wave-uniform) a refused point reads no table
    F = Fw + ti * tstride;
    R = Rw + ci * rstride;
    const FkKey key = fk_key(qs.y_lo, qs.y_hi, qs.n, qs.Tp, qs.Bc, qs.m, pt.stats, fk_g(d0), blk);
    match = fk_key_match(key, R) &&
            (qs.empty || (F[0] == qs.y_lo && F[1] == qs.y_hi && F[2] == (double)qs.n && F[3] == qs.cneg &&
                          F[4] == key_nz && F[5] == key_z_max));
  }
  const int n = (int)qs.n;
  double Y_B = 0.0;
  if (match && !qs.empty) {
    const double* Fv = F + kTabHdr;
    const double* Rv = R + kFkHdr;
    const int32_t wkind = has_win ? __builtin_amdgcn_readfirstlane(slots[w].win.kind) : 0;
    double acc = 0.0;
    for (int base = 0; base < n; base += kWaveSize) {
      const int j = base + lane;
      const int jj = j < n ? j : n - 1;  // tail lanes recompute the last node with weight 0
      const double Fj = Fv[jj], Rj = Rv[jj];
      const double y = y_node(qs, jj);
      const double ey = exp_y<false>(y);
      const double wgt = j < n ? y_weight(qs, jj, y) : 0.0;
      const YFactors f = y_factors(qs, y, ey, wgt, [&](double yy) {
        const double W = has_win ? window_W(slots[w].win, wkind, yy) : gauss_window(qs, yy);
        return W * Rj;
      });
      acc = __builtin_fma(f.w, integrand_from(f, Fj), acc);
    }
    Y_B = wave_sum(acc);
  }
  if (lane == 0) {
    const double P_used = match ? R[kFkHdr + n] : __builtin_nan("");
    lzq_yield o = epilogue_finish(epilogue_pre(pt, P_used), Y_B);
    if (!match) o.Y_B = o.rho_B_kg_m3 = o.DM_over_B = __builtin_nan("");
    out[idx] = o;
  }
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

int fail(const char* fn, const char* what) {
  char m[400];
  snprintf(m, sizeof(m), "%s: %s", fn, what);
  return lzq_set_error(LZQ_EINVAL, m);
}

std::mutex g_mu;
struct DevEntry {
  int dev;
  lzq::FkNode* d;
};
std::vector<DevEntry> g_dev;  // the node table, uploaded on first use per device (guarded by g_mu)

const std::vector<lzq::FkNode>& host_nodes() {
  static const std::vector<lzq::FkNode> t = [] {
    std::vector<lzq::FkNode> v;
    lzq::fk_build(v);
    return v;
  }();
  return t;
}

int device_nodes(const lzq::FkNode** tab, int32_t* n) {
  int dev = 0;
  LZQ_HIP(hipGetDevice(&dev));
  const std::vector<lzq::FkNode>& h = host_nodes();
  *n = (int32_t)h.size();
  std::lock_guard<std::mutex> lk(g_mu);
  for (const DevEntry& e : g_dev)
    if (e.dev == dev) {
      *tab = e.d;
      return LZQ_OK;
    }
  lzq::FkNode* d = nullptr;
  LZQ_HIP(hipMalloc(&d, h.size() * sizeof(lzq::FkNode)));
  LZQ_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(lzq::FkNode), hipMemcpyHostToDevice));
  g_dev.push_back(DevEntry{dev, d});
  *tab = d;
  return LZQ_OK;
}

int check_block(const lzq_fk& b, int64_t i) {
  char msg[200];
  switch (lzq::fk_block_error(b)) {
    case lzq::kFkOk: return LZQ_OK;
    case lzq::kFkKind: snprintf(msg, sizeof(msg), "fk block %lld: unknown kind %d", (long long)i, b.kind); break;
    case lzq::kFkP:
      snprintf(msg, sizeof(msg), "fk block %lld: p = %g outside [0, %g]", (long long)i, b.p, LZQ_FK_P_MAX);
      break;
    default: snprintf(msg, sizeof(msg), "fk block %lld: v_ref = %g outside (0, 1]", (long long)i, b.v_ref);
  }
  return lzq_set_error(LZQ_EINVAL, msg);
}

int check_delta(double d, int64_t i) {
  if (lzq::fk_delta_ok(d)) return LZQ_OK;
  char msg[200];
  snprintf(msg, sizeof(msg), "fk point %lld: delta0 = %g must be >= 0", (long long)i, d);
  return lzq_set_error(LZQ_EINVAL, msg);
}

int64_t n_of(int32_t n_y) { return n_y > LZQ_NY_MIN ? n_y : LZQ_NY_MIN; }

}  // namespace

extern "C" {

int lzq_fk_check_host(const lzq_fk* fk, const double* delta0, int64_t n) {
  if (n < 0 || (n > 0 && !fk)) return fail("lzq_fk_check_host", "bad arguments");
  for (int64_t i = 0; i < n; ++i) {
    int rc = check_block(fk[i], i);
    if (rc) return rc;
    if (delta0 && (rc = check_delta(delta0[i], i))) return rc;
  }
  return LZQ_OK;
}

int lzq_fk_nodes(double* t, double* w_exp, double* e, int32_t* n) {
  const std::vector<lzq::FkNode>& h = host_nodes();
  if (n) *n = (int32_t)h.size();
  for (size_t i = 0; i < h.size(); ++i) {
    if (t) t[i] = h[i].t;
    if (w_exp) w_exp[i] = h[i].we;
    if (e) e[i] = h[i].e;
  }
  return LZQ_OK;
}

int lzq_fk_pbar_host(const lzq_fk* fk, int32_t stats, const double* mu, const double* delta0, int64_t n, double* out) {
  const char* fn = "lzq_fk_pbar_host";
  if (!fk || n < 0 || (n > 0 && (!mu || !delta0 || !out))) return fail(fn, "bad arguments");
  int rc = check_block(*fk, 0);
  if (rc) return rc;
  for (int64_t i = 0; i < n; ++i) {
    if ((rc = check_delta(delta0[i], i))) return rc;
    if (!(mu[i] >= 0.0)) {
      char msg[200];
      snprintf(msg, sizeof(msg), "lzq_fk_pbar_host: mu[%lld] = %g must be >= 0", (long long)i, mu[i]);
      return lzq_set_error(LZQ_EINVAL, msg);
    }
  }
  const std::vector<lzq::FkNode>& h = host_nodes();
  for (int64_t i = 0; i < n; ++i)
    out[i] = lzq::fk_pbar(mu[i], lzq::fk_g(delta0[i]), *fk, stats, h.data(), (int32_t)h.size());
  return LZQ_OK;
}

int lzq_fk_pbar_batch(const lzq_fk* fk, int32_t stats, const double* d_mu, const double* d_delta0, int64_t n,
                      double* d_out, void* stream) {
  const char* fn = "lzq_fk_pbar_batch";
  if (!fk || n < 0 || (n > 0 && (!d_mu || !d_delta0 || !d_out))) return fail(fn, "bad arguments");
  int rc = check_block(*fk, 0);
  if (rc) return rc;
  if (n == 0) return LZQ_OK;
  const lzq::FkNode* tab;
  int32_t nn;
  rc = device_nodes(&tab, &nn);
  if (rc) return rc;
  const int64_t nb = (n + lzq::kFkBlock - 1) / lzq::kFkBlock;
  if (nb > 2147483647LL) return fail(fn, "n too large");
  hipLaunchKernelGGL(lzq::fk_pbar_eval_kernel, dim3((unsigned)nb), dim3(lzq::kFkBlock), 0, (hipStream_t)stream, *fk,
                     stats, d_mu, d_delta0, n, tab, nn, d_out);
  LZQ_HIP(hipGetLastError());
  return LZQ_OK;
}

int64_t lzq_fk_table_stride(int32_t n_y) { return n_of(n_y) + 1 + LZQ_FK_TABLE_HEADER; }

int lzq_fk_tables(const lzq_point* d_points, const double* d_delta0, const lzq_fk* d_fk, const int64_t* d_rep,
                  int64_t n_classes, int32_t n_y, double* d_R, int64_t r_doubles, double* d_mu, void* stream) {
  const char* fn = "lzq_fk_tables";
  if (n_classes < 0 || (n_classes > 0 && (!d_points || !d_delta0 || !d_fk || !d_rep || !d_R)))
    return fail(fn, "bad arguments");
  const int64_t stride = lzq_fk_table_stride(n_y);
  if (n_classes > INT64_MAX / stride) return fail(fn, "too many classes");
  if (r_doubles < n_classes * stride) {
    char msg[200];
    snprintf(msg, sizeof(msg), "lzq_fk_tables: R workspace of %lld doubles < %lld needed", (long long)r_doubles,
             (long long)(n_classes * stride));
    return lzq_set_error(LZQ_EINVAL, msg);
  }
  if (n_classes == 0) return LZQ_OK;
  const lzq::FkNode* tab;
  int32_t nn;
  const int rc = device_nodes(&tab, &nn);
  if (rc) return rc;
  const int32_t passes = (int32_t)((n_of(n_y) + 1 + lzq::kWaveSize - 1) / lzq::kWaveSize);
  const int64_t nb = (n_classes * passes + lzq::kFkWaves - 1) / lzq::kFkWaves;
  if (nb > 2147483647LL) return fail(fn, "too large for one launch");
  hipLaunchKernelGGL(lzq::fk_pbar_table_kernel, dim3((unsigned)nb), dim3(lzq::kFkBlock), 0, (hipStream_t)stream,
                     d_points, d_delta0, d_fk, d_rep, n_classes, n_y, passes, stride, tab, nn, d_R, d_mu);
  LZQ_HIP(hipGetLastError());
  return LZQ_OK;
}

int lzq_yields_batch_reuse_fk(const lzq_point* d_points, int64_t n, int32_t n_y, int32_t nz, double z_max,
                              const double* d_delta0, const lzq_fk* d_fk, const int32_t* d_table_index,
                              const double* d_work, int64_t work_doubles, const int32_t* d_class, const double* d_R,
                              int64_t r_doubles, const lzq_window* d_win, const lzq_window_tables* d_tables,
                              lzq_yield* d_out, void* stream) {
  const char* fn = "lzq_yields_batch_reuse_fk";
  if (n < 0 || work_doubles < 0 || r_doubles < 0 ||
      (n > 0 && (!d_points || !d_delta0 || !d_fk || !d_table_index || !d_work || !d_class || !d_R || !d_out)))
    return fail(fn, "bad arguments");
  if (nz < 0 && nz != LZQ_FK_NZ_CONT) return fail(fn, "nz < 0 (LZQ_FK_NZ_CONT names the continuum rule)");
  lzq_window_tables wt = {0, 0, nullptr, nullptr};
  if (d_win) {
    const int rc = lzq::window_tables_arg(d_tables, fn, wt);
    if (rc) return rc;
  }
  if (n == 0) return LZQ_OK;
  const int64_t tstride = n_of(n_y) + lzq::kTabHdr, rstride = lzq_fk_table_stride(n_y);
  const int64_t n_tables = work_doubles / tstride, n_classes = r_doubles / rstride;  // whole tables only
  const int64_t nb = (n + lzq::kWavesPerBlock - 1) / lzq::kWavesPerBlock;
  if (nb > 2147483647LL) return fail(fn, "n too large for one launch");
  const double key_nz = nz == LZQ_FK_NZ_CONT ? lzq::kContKeyNz : (double)nz;
  hipLaunchKernelGGL(lzq::points_reuse_fk_kernel, dim3((unsigned)nb), dim3(lzq::kBlock), 0, (hipStream_t)stream,
                     d_points, d_delta0, d_fk, d_win, wt, n, n_y, key_nz, z_max, d_table_index, d_work, tstride,
                     n_tables, d_class, d_R, rstride, n_classes, d_out);
  LZQ_HIP(hipGetLastError());
  return LZQ_OK;
}

}  // extern "C"
