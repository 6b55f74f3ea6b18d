// lzq_wash.hip -- wash-out and source depletion on the y-grid quadrature (lzq_wash.h; include/lzq.h
// "wash-out and source depletion"): omega alone, the three integration kernels (explicit
// points, grid, per-point root solve) and the lzq_*_wash entry points.
//
// Each kernel is one wavefront per point on its own y-loop over y_factors (lzq_quad.h is not edited and
// yb_wave is not instantiated), modelled on points_reuse_fk_kernel (lzq_fk.hip): the passes, the
// tail-lane rule, the per-lane fma chain, the butterfly and the epilogue are the reuse mode's (yb_wave
// kYbReuse), and the z-sum tables are the ones lzq_sweep_grid_ztables[_window|_cont] /
// lzq_yields_batch_reuse build, their header checked as the reuse kernels check it.  The per-node
// factor is W(y_j) omega(T_j): W the point's Gaussian or its lzq_window block, T_j by the operations
// y_factors forms it with.  With depletion a second accumulator sums the unwashed terms in the same
// order, and Y_chi = Y_chi0 - Y_B0 is one IEEE subtraction ahead of the epilogue, which then runs on
// (Y_B, Y_chi) unchanged.  Gamma = 0 and no depletion give the reuse kernels' bits.
//
// Nothing is held across a z-loop here, so the setup stays in scalar registers; only a point's window
// block (and the solve's state and bracket records) is parked in LDS.
//
// Its own translation unit: no existing code object changes.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#define LZQ_QUAD_CONST_LINKAGE static
#include "lzq_quad.h"
#include "lzq_internal.h"
#include "lzq_quad_window.h"  // window_W, WinParams
#include "lzq_solve.h"
#include "lzq_wash.h"

namespace lzq {

// T(y) by the operations of y_factors (denom, rsqrt_pos, T = Tp * rs): the same bits
__device__ __forceinline__ double wash_T_of_y(double Tp, double Bc, double y) {
  const double denom = pymax(1.0 + 2.0 * y / Bc, 1e-12);  // fpy:252-253
  return Tp * rsqrt_pos(denom);                           // fpy:254
}

// omega(T) on the device; gamma is wave-uniform
__device__ __forceinline__ double wash_omega(double gamma, double T_lo, double T) {
  return gamma != 0.0 ? exp_sc(wash_exponent(gamma, T_lo, T)) : 1.0;
}

// lzq_wash_factor_batch: omega(T(y)) of one point and block, one lane per y
__global__ __launch_bounds__(256) void wash_factor_kernel(lzq_point pt, lzq_ode_params ode,
                                                          const double* __restrict__ ys, int64_t n,
                                                          double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const WashParams wp = wash_params(pt, ode);
  const double T = wash_T_of_y(pt.T_p_GeV, pymax(pt.beta_over_H, 1e-30), ys[i]);
  out[i] = wp.ok ? wash_omega(wp.gamma, wp.T_lo, T) : __builtin_nan("");
}

struct WashSums {
  double Y_B;   // sum_j w_j g_j omega_j
  double Y_B0;  // sum_j w_j g_j  (deplete only; else 0)
};

// The y-loop of one point on its z-sum table values Fv[0..n): the reuse mode's passes (yb_wave
// kYbReuse) with the window factor W(y_j) omega(T_j) and, where deplete, the unwashed sum next to it.
// win: the point's block in the wave's LDS slot (has_win), else the point's Gaussian.
__device__ __forceinline__ WashSums wash_wave(const QuadSetup& qs, const double* __restrict__ Fv, bool has_win,
                                              const WinParams& win, double gamma, double T_lo, bool deplete,
                                              int lane) {
  const int n = (int)qs.n;
  const int32_t wkind = has_win ? __builtin_amdgcn_readfirstlane(win.kind) : 0;
  double acc = 0.0, acc0 = 0.0;
  for (int base = 0; base < n; base += kWaveSize) {
    const int j = base + lane;
    const int jj = j < n ? j : n - 1;  // tail lanes recompute the last node with weight 0
    const double Fj = Fv[jj];
    const double y = y_node(qs, jj);
    const double ey = exp_y<false>(y);
    const double wgt = j < n ? y_weight(qs, jj, y) : 0.0;
    double W0;
    const YFactors f = y_factors(qs, y, ey, wgt, [&](double yy) {
      W0 = has_win ? window_W(win, wkind, yy) : gauss_window(qs, yy);
      return gamma != 0.0 ? W0 * wash_omega(gamma, T_lo, wash_T_of_y(qs.Tp, qs.Bc, yy)) : W0;
    });
    acc = __builtin_fma(f.w, integrand_from(f, Fj), acc);
    if (deplete) {
      YFactors f0 = f;
      f0.W = W0;
      acc0 = __builtin_fma(f0.w, integrand_from(f0, Fj), acc0);
    }
  }
  WashSums s;
  s.Y_B = wave_sum(acc);
  s.Y_B0 = deplete ? wave_sum(acc0) : 0.0;
  return s;
}

// The epilogue on (Y_B, Y_chi), split around the y-loop as lzq_quad.h splits its own, so that the point
// record need not stay live across the loop: wash_epi_pre is epilogue_pre and the factor rho_DM is
// re-formed with; wash_finish takes Y_chi0 less the unwashed sum where deplete (rho_DM from it by
// epilogue_pre's operations, fpy:414-416), then epilogue_finish.  match: the table was the point's;
// wp.ok: the block was not a refusal.
struct WashEpi {
  EpiPre e;
  double mkg;  // m_chi in kg
};

__device__ __forceinline__ WashEpi wash_epi_pre(const lzq_point& pt, double P) {
  WashEpi w;
  w.e = epilogue_pre(pt, P);
  w.mkg = pt.m_chi_GeV * kGeVToKg;
  return w;
}

__device__ __forceinline__ lzq_yield wash_finish(WashEpi w, const WashParams& wp, const WashSums& s, bool match) {
  if (wp.deplete) {
    const double Ychi = w.e.o.Y_chi - s.Y_B0;
    const double nDM0 = Ychi * kS0M3;
    w.e.o.Y_chi = Ychi;
    w.e.o.rho_DM_kg_m3 = nDM0 * w.mkg;
  }
  lzq_yield o = epilogue_finish(w.e, s.Y_B);
  if (!match || !wp.ok) o.Y_B = o.rho_B_kg_m3 = o.DM_over_B = __builtin_nan("");
  if ((!match && wp.deplete) || !wp.ok) o.Y_chi = o.rho_DM_kg_m3 = __builtin_nan("");
  return o;
}

__device__ __forceinline__ bool wash_table_match(const QuadSetup& qs, const double* F, double key_nz,
                                                 double key_z_max) {
  return qs.empty || (F[0] == qs.y_lo && F[1] == qs.y_hi && F[2] == (double)qs.n && F[3] == qs.cneg &&
                      F[4] == key_nz && F[5] == key_z_max);
}

struct WashWaveSlot {
  WinParams win;
};

__device__ __forceinline__ void park_block(WinParams& dst, const WinParams& src, int lane) {
  if (lane == 0) dst = src;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// wave-uniform block -> scalar registers
__device__ __forceinline__ WashParams wash_uniform(WashParams p) {
  p.gamma = uniform(p.gamma);
  p.T_lo = uniform(p.T_lo);
  p.deplete = __builtin_amdgcn_readfirstlane(p.deplete);
  p.ok = __builtin_amdgcn_readfirstlane(p.ok);
  return p;
}

// lzq_yields_batch_reuse_wash
__global__ __launch_bounds__(kBlock) void points_reuse_wash_kernel(
    const lzq_point* __restrict__ pts, const lzq_ode_params* __restrict__ ode, const lzq_window* __restrict__ win,
    lzq_window_tables wt, int64_t n_pts, int32_t n_y, const double* __restrict__ Pov, double key_nz, double key_z_max,
    const int32_t* __restrict__ tidx, const double* __restrict__ Fw, int64_t tstride, int64_t n_tables,
    lzq_yield* __restrict__ out) {
  __shared__ WashWaveSlot slots[kWavesPerBlock];
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t idx = (int64_t)blockIdx.x * kWavesPerBlock + w;
  if (idx >= n_pts) return;  // wave-uniform
  const lzq_point pt = pts[idx];
  const double P = Pov ? Pov[idx] : pt.P_chi_to_B;
  const WashParams wp = wash_uniform(wash_params(pt, ode[idx]));
  const bool has_win = win != nullptr;
  if (has_win) park_block(slots[w].win, window_params(win[idx], wt.n_tables, wt.n_knots, wt.u, wt.W), lane);
  const QuadSetup qs = quad_setup(pt, P, pt.T_min_over_Tp * pt.T_p_GeV, pt.T_max_over_Tp * pt.T_p_GeV, n_y);
  const WashEpi epi = wash_epi_pre(pt, P);
  const int64_t ti = tidx[idx];
  bool match = false;
  const double* F = Fw;
  if (wp.ok && ti >= 0 && ti < n_tables) {  // (wave-uniform) a refused point reads no table
    F = Fw + ti * tstride;
    match = wash_table_match(qs, F, key_nz, key_z_max);
  }
  WashSums s = {0.0, 0.0};
  if (match && !qs.empty) s = wash_wave(qs, F + kTabHdr, has_win, slots[w].win, wp.gamma, wp.T_lo, wp.deplete, lane);
  if (lane == 0) out[idx] = wash_finish(epi, wp, s, match);
}

// lzq_sweep_grid_from_ztables_wash: the point (grid_point), its window block (window_grid_block), its
// wash block (wash_grid_block) and its table index decoded from the flat index
__global__ __launch_bounds__(kBlock) void grid_reuse_wash_kernel(
    lzq_point base, lzq_ode_params base_ode, lzq_window base_win, int has_win_i, GridSpec grid, lzq_window_tables wt,
    int64_t start, int64_t count, int32_t n_y, const double* __restrict__ Pov, double key_nz, double key_z_max,
    const double* __restrict__ Fw, int64_t tstride, lzq_yield* __restrict__ out) {
  __shared__ WashWaveSlot slots[kWavesPerBlock];
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t local = (int64_t)blockIdx.x * kWavesPerBlock + w;
  if (local >= count) return;  // wave-uniform
  const bool has_win = has_win_i != 0;
  lzq_point pt;
  const double Pg = grid_point(base, grid, start + local, pt);
  const double P = Pov ? Pov[local] : Pg;
  const WashParams wp = wash_uniform(wash_params(pt, wash_grid_block(base_ode, grid, start + local)));
  if (has_win) {
    const lzq_window blk = window_grid_block(base_win, grid, start + local);
    park_block(slots[w].win, window_params(blk, wt.n_tables, wt.n_knots, wt.u, wt.W), lane);
  }
  const QuadSetup qs = quad_setup(pt, P, pt.T_min_over_Tp * pt.T_p_GeV, pt.T_max_over_Tp * pt.T_p_GeV, n_y);
  const WashEpi epi = wash_epi_pre(pt, P);
  const double* F = Fw + win_table_of(grid, start + local) * tstride;
  const bool match = wash_table_match(qs, F, key_nz, key_z_max);  // wave-uniform
  WashSums s = {0.0, 0.0};
  if (match && wp.ok && !qs.empty)
    s = wash_wave(qs, F + kTabHdr, has_win, slots[w].win, wp.gamma, wp.T_lo, wp.deplete, lane);
  if (lane == 0) out[local] = wash_finish(epi, wp, s, match);
}

// What the solve keeps between evaluations (lzq_solve.hip SolveWaveSlot, less yb_wave's slot).
struct WashSolveSlot {
  WinParams win;
  WashEpi epi;       // the evaluation's epilogue inputs, parked across its y-loop
  WashParams wp;
  SolveState st;     // the rule's state
  lzq_yield rec[2];  // the records of the bracket's lower and upper end
};

__device__ __forceinline__ double wash_yield_field(const lzq_yield& o, int32_t f) {
  switch (f) {
    case 0: return o.Y_B;
    case 1: return o.Y_chi;
    case 2: return o.rho_B_kg_m3;
    case 3: return o.rho_DM_kg_m3;
    case 4: return o.DM_over_B;
    default: return o.P_used;
  }
}

// The rule's state out of the slot into scalar registers (it is wave-uniform).
__device__ __forceinline__ SolveState wash_load_state(const SolveState& m) {
  SolveState s;
  s.a = uniform(m.a), s.b = uniform(m.b), s.fa = uniform(m.fa), s.fb = uniform(m.fb);
  s.ga = uniform(m.ga), s.gb = uniform(m.gb), s.w = uniform(m.w), s.w1 = uniform(m.w1), s.w2 = uniform(m.w2);
  s.lo = uniform(m.lo), s.hi = uniform(m.hi), s.xtol = uniform(m.xtol);
  s.evals = __builtin_amdgcn_readfirstlane(m.evals), s.max_evals = __builtin_amdgcn_readfirstlane(m.max_evals);
  s.side = __builtin_amdgcn_readfirstlane(m.side), s.force = __builtin_amdgcn_readfirstlane(m.force);
  s.status = __builtin_amdgcn_readfirstlane(m.status), s.done = __builtin_amdgcn_readfirstlane(m.done);
  return s;
}

// lzq_sweep_grid_solve_wash: grid_solve_kernel (lzq_solve.hip) -- the same decode of the point at x, the
// same rule, the same records -- with every evaluation one point of grid_reuse_wash_kernel, and
// LZQ_F_GAMMA_WASH one more field x can be written into.
__global__ __launch_bounds__(kBlock) void grid_solve_wash_kernel(
    lzq_point base, lzq_ode_params base_ode, lzq_window base_win, int has_win_i, GridSpec grid, lzq_window_tables wt,
    lzq_solve sv, int64_t start, int64_t count, int32_t n_y, const double* __restrict__ Pov, double key_nz,
    double key_z_max, const double* __restrict__ Fw, int64_t tstride, lzq_yield* __restrict__ out,
    lzq_solve_result* __restrict__ sol) {
  __shared__ WashSolveSlot slots[kWavesPerBlock];
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t local = (int64_t)blockIdx.x * kWavesPerBlock + w;
  if (local >= count) return;  // wave-uniform
  const bool has_win = has_win_i != 0;
  {
    const SolveState st0 = solve_init(sv.lo, sv.hi, sv.xtol, sv.max_evals);
    if (lane == 0) slots[w].st = st0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  const double* F = Fw + win_table_of(grid, start + local) * tstride;
  bool bad_table = false;
  for (int it = 0; it < kSolveMaxEvals; ++it) {
    int wi = w;
    asm volatile("" : "+s"(wi));  // the slot is re-read, not carried in registers
    SolveState st = wash_load_state(slots[wi].st);
    double x;
    const bool more = solve_next(st, x);
    if (!__builtin_amdgcn_readfirstlane((int)more)) break;
    x = uniform(x);
    // the point at x, as grid_solve_kernel forms it
    int64_t idx = start + local;
    asm volatile("" : "+s"(idx));  // (the decode is not hoisted out of the loop into registers)
    lzq_point pt;
    const double Pg = grid_point(base, grid, idx, pt);
    double P = Pov ? Pov[local] : Pg;
    double m_mix = __builtin_nan(""), dprime = __builtin_nan("");
    bool ax_mix = false;  // an m_mix axis: grid_point forms P from m_mix, dprime and the point's v_w
    if (sv.field == LZQ_F_M_MIX || sv.field == LZQ_F_DPRIME || sv.field == LZQ_F_V_W)
      for (int a = 0; a < grid.n_axes; ++a) {  // the LZ axes' values, which grid_point folds into P
        if (grid.field[a] != LZQ_F_M_MIX && grid.field[a] != LZQ_F_DPRIME) continue;
        const double v = grid.values[a][(idx / grid.stride[a]) % grid.n[a]];
        if (grid.field[a] == LZQ_F_M_MIX) m_mix = v, ax_mix = true;
        else dprime = v;
      }
    if (sv.field == LZQ_F_DELTA_LZ) {
      P = p_closed_form(x);  // fpy:183-184
    } else if (sv.field == LZQ_F_M_MIX) {
      P = p_closed_form(x * x / (2.0 * pymax(pt.v_w, 1e-12) * fabs(dprime)));  // PAPER eq.(8)
    } else if (sv.field == LZQ_F_DPRIME) {
      P = p_closed_form(m_mix * m_mix / (2.0 * pymax(pt.v_w, 1e-12) * fabs(x)));
    } else if (!window_field(sv.field) && !wash_field(sv.field)) {
      double d0, d1, d2;
      set_field(pt, sv.field, x, d0, d1, d2);
      if (sv.field == LZQ_F_P) P = x;
      if (sv.field == LZQ_F_V_W && ax_mix) {
        pt.P_chi_to_B = p_closed_form(m_mix * m_mix / (2.0 * pymax(pt.v_w, 1e-12) * fabs(dprime)));
        if (!Pov) P = pt.P_chi_to_B;
      }
    }
    if (sv.field == LZQ_F_DELTA_LZ || sv.field == LZQ_F_M_MIX || sv.field == LZQ_F_DPRIME) pt.P_chi_to_B = P;
    lzq_ode_params ob = wash_grid_block(base_ode, grid, idx);
    wash_set_field(ob, sv.field, x);  // (a field of the point or its window: not written)
    const WashParams wp = wash_uniform(wash_params(pt, ob));
    const QuadSetup qs = quad_setup(pt, P, pt.T_min_over_Tp * pt.T_p_GeV, pt.T_max_over_Tp * pt.T_p_GeV, n_y);
    if (it == 0 && !wash_table_match(qs, F, key_nz, key_z_max)) {  // no allowed field moves the y-grid
      bad_table = true;
      break;
    }
    if (has_win) {
      lzq_window blk = window_grid_block(base_win, grid, idx);
      window_set_field(blk, sv.field, x);  // (a field of the point or its wash block: not written)
      park_block(slots[w].win, window_params(blk, wt.n_tables, wt.n_knots, wt.u, wt.W), lane);
    }
    {
      const WashEpi epi = wash_epi_pre(pt, P);
      if (lane == 0) {
        slots[w].epi = epi;
        slots[w].wp = wp;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    WashSums s = {0.0, 0.0};
    if (wp.ok && !qs.empty) s = wash_wave(qs, F + kTabHdr, has_win, slots[w].win, wp.gamma, wp.T_lo, wp.deplete, lane);
    int wr = w;
    asm volatile("" : "+s"(wr));  // the slot is re-read, not carried in registers
    const lzq_yield o = wash_finish(slots[wr].epi, wash_uniform(slots[wr].wp), s, true);
    const double f = uniform(wash_yield_field(o, sv.target_field) - sv.target);
    st = wash_load_state(slots[wr].st);
    const int32_t mask = __builtin_amdgcn_readfirstlane(solve_feed(st, x, f));
    if (lane == 0) {
      slots[w].st = st;
      if (mask & 1) slots[w].rec[0] = o;
      if (mask & 2) slots[w].rec[1] = o;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
    lzq_yield o;
    lzq_solve_result r;
    int32_t slot = -1;
    if (bad_table) r = solve_refused(sv.lo, sv.hi, LZQ_SOLVE_BAD_TABLE, 0);
    else r = solve_result(slots[w].st, &slot);
    if (slot >= 0) {
      o = slots[w].rec[slot];
    } else {
      o.Y_B = o.Y_chi = o.rho_B_kg_m3 = o.rho_DM_kg_m3 = o.DM_over_B = o.P_used = __builtin_nan("");
    }
    out[local] = o;
    sol[local] = r;
  }
}

}  // namespace lzq

namespace {

int fail(int code, const char* msg) { return lzq_set_error(code, msg); }

template <class A0, class... A>
int fail(int code, const char* fmt, A0 a0, A... a) {
  char msg[320];
  snprintf(msg, sizeof(msg), fmt, a0, a...);
  return lzq_set_error(code, msg);
}

int hip_ok(const char* fn) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? LZQ_OK : fail(LZQ_EHIP, "%s: %s", fn, hipGetErrorString(e));
}

constexpr int64_t kMaxGrid = 2147483647LL;

int check_block(const lzq_ode_params& o, const char* who, long long i) {
  switch (lzq::wash_error(o)) {
    case lzq::kWashOk: return LZQ_OK;
    case lzq::kWashNaNSigma: return fail(LZQ_EINVAL, "%s %lld: sigma_v_chi_GeV_m2 is NaN", who, i);
    case lzq::kWashNaNGamma: return fail(LZQ_EINVAL, "%s %lld: Gamma_wash_over_H is NaN", who, i);
    default:
      return fail(LZQ_EUNSUPPORTED,
                  "%s %lld: sigma_v_chi_GeV_m2 = %g > 0 leaves the linear system (fpy:279, 283): the ODE entry "
                  "points take it", who, i, o.sigma_v_chi_GeV_m2);
  }
}

int64_t n_of(int32_t n_y) { return n_y > LZQ_NY_MIN ? n_y : LZQ_NY_MIN; }

// the z grid as a table's header stores it
int z_key(int32_t nz, double z_max, const char* fn, double& key_nz) {
  if (nz < 0 && nz != LZQ_WASH_NZ_CONT) return fail(LZQ_EINVAL, "%s: nz < 0 (LZQ_WASH_NZ_CONT names the continuum rule)", fn);
  key_nz = nz == LZQ_WASH_NZ_CONT ? lzq::kContKeyNz : (double)nz;
  (void)z_max;
  return LZQ_OK;
}

bool ztable_field(int32_t f) {
  return f == LZQ_F_I_P || f == LZQ_F_BETA_OVER_H || f == LZQ_F_T_P || f == LZQ_F_T_MIN_OVER_TP ||
         f == LZQ_F_T_MAX_OVER_TP;
}

// lzq_kernels.hip's make_grid with the wash fields known: the axes as the kernels read them (C order
// strides, table strides of the z-sum fields), every check of lzq_sweep_grid_from_ztables[_window], two
// axes writing one wash field refused.  *n_tab: the tables of the axis list (the wash axes give none).
int make_wash_grid(const lzq_point* base, const lzq_ode_params* base_ode, const lzq_axis* axes, int32_t n_axes,
                   int64_t start, int64_t count, const void* d_out, const char* who, bool window_axes,
                   int32_t solve_field, lzq::GridSpec& g, int64_t* n_tab) {
  if (!base || !base_ode || n_axes < 0 || n_axes > LZQ_MAX_AXES || (n_axes > 0 && !axes) || start < 0 || count < 0 ||
      (count > 0 && !d_out))
    return fail(LZQ_EINVAL, "%s: bad arguments", who);
  memset(&g, 0, sizeof(g));
  g.n_axes = n_axes;
  int64_t total = 1, ts = 1;
  bool mix = solve_field == LZQ_F_M_MIX, dpr = solve_field == LZQ_F_DPRIME;  // (a solve stands for its axis)
  bool ax_gamma = false, ax_dep = false;
  for (int a = n_axes - 1; a >= 0; --a) {
    const int32_t f = axes[a].field;
    if (!((f >= 0 && f <= 14) || f == LZQ_F_DELTA_LZ || f == LZQ_F_M_MIX || f == LZQ_F_DPRIME || lzq::wash_field(f) ||
          (window_axes && lzq::window_field(f))))
      return fail(LZQ_EINVAL, "%s: axis %d has unknown field %d", who, a, f);
    if (axes[a].n <= 0 || !axes[a].values) return fail(LZQ_EINVAL, "%s: axis %d is empty", who, a);
    if ((f == LZQ_F_GAMMA_WASH && ax_gamma) || (f == LZQ_F_DEPLETE && ax_dep))
      return fail(LZQ_EINVAL, "%s: axis %d (field %d) writes a wash field that another axis writes", who, a, f);
    ax_gamma |= f == LZQ_F_GAMMA_WASH;
    ax_dep |= f == LZQ_F_DEPLETE;
    mix |= f == LZQ_F_M_MIX;
    dpr |= f == LZQ_F_DPRIME;
    g.field[a] = f;
    g.n[a] = axes[a].n;
    g.values[a] = axes[a].values;
    g.stride[a] = total;
    if (total > INT64_MAX / axes[a].n) return fail(LZQ_EINVAL, "%s: grid too large", who);
    total *= axes[a].n;
    if (ztable_field(f)) {
      g.tstride[a] = ts;
      if (ts > INT64_MAX / 16 / axes[a].n) return fail(LZQ_EINVAL, "%s: too many tables", who);
      ts *= axes[a].n;
    }
  }
  *n_tab = ts;
  if (mix != dpr) return fail(LZQ_EINVAL, "%s: LZQ_F_M_MIX and LZQ_F_DPRIME must be swept together", who);
  if (start > total || count > total - start)
    return fail(LZQ_EINVAL, "%s: range [%lld, %lld) outside grid of %lld points", who, (long long)start,
                (long long)(start + count), (long long)total);
  if (base->regime != LZQ_THERMAL && base->regime != LZQ_NONTHERMAL)
    return fail(LZQ_EUNSUPPORTED, "%s: regime must be thermal or nonthermal (fpy:376-384)", who);
  const int rc = check_block(*base_ode, who, 0);  // (axis values live on the device: a refusal there is NaN yields)
  if (rc) return rc;
  return window_axes ? lzq::window_axes_check(axes, n_axes, who) : LZQ_OK;
}

int workspace_ok(int64_t n_tab, int32_t n_y, const double* d_work, int64_t work_doubles, const char* fn) {
  const int64_t stride = n_of(n_y) + lzq::kTabHdr;
  if (n_tab > INT64_MAX / stride) return fail(LZQ_EINVAL, "%s: too many tables", fn);
  if (!d_work || work_doubles < n_tab * stride)
    return fail(LZQ_EINVAL, "%s: workspace of %lld doubles < %lld needed", fn, (long long)work_doubles,
                (long long)(n_tab * stride));
  return LZQ_OK;
}

bool lz_field(int32_t f) { return f == LZQ_F_DELTA_LZ || f == LZQ_F_M_MIX || f == LZQ_F_DPRIME; }

}  // namespace

extern "C" {

int lzq_wash_check_host(const lzq_ode_params* ode, int64_t n) {
  if (n < 0 || (n > 0 && !ode)) return fail(LZQ_EINVAL, "lzq_wash_check_host: bad arguments");
  for (int64_t i = 0; i < n; ++i) {
    const int rc = check_block(ode[i], "wash block", (long long)i);
    if (rc) return rc;
  }
  return LZQ_OK;
}

int lzq_wash_factor_host(const lzq_point* pt, const lzq_ode_params* ode, const double* y, int64_t n, double* out) {
  if (!pt || !ode || n < 0 || (n > 0 && (!y || !out))) return fail(LZQ_EINVAL, "lzq_wash_factor_host: bad arguments");
  const int rc = check_block(*ode, "wash block", 0);
  if (rc) return rc;
  const lzq::WashParams wp = lzq::wash_params(*pt, *ode);
  for (int64_t i = 0; i < n; ++i)
    out[i] = wp.gamma != 0.0 ? exp(lzq::wash_exponent(wp.gamma, wp.T_lo, lzq::wash_T_of_y_host(*pt, y[i]))) : 1.0;
  return LZQ_OK;
}

int lzq_wash_factor_batch(const lzq_point* pt, const lzq_ode_params* ode, const double* d_y, int64_t n, double* d_out,
                          void* stream) {
  const char* fn = "lzq_wash_factor_batch";
  if (!pt || !ode || n < 0 || (n > 0 && (!d_y || !d_out))) return fail(LZQ_EINVAL, "%s: bad arguments", fn);
  const int rc = check_block(*ode, "wash block", 0);
  if (rc) return rc;
  if (n == 0) return LZQ_OK;
  const int64_t nb = (n + 255) / 256;
  if (nb > kMaxGrid) return fail(LZQ_EINVAL, "%s: n too large", fn);
  hipLaunchKernelGGL(lzq::wash_factor_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, *pt, *ode, d_y, n,
                     d_out);
  return hip_ok(fn);
}

int lzq_yields_batch_reuse_wash(const lzq_point* d_points, int64_t n, int32_t n_y, int32_t nz, double z_max,
                                const double* d_P, const int64_t* d_rep, const int32_t* d_table_index,
                                int64_t n_tables, double* d_work, int64_t work_doubles, const lzq_window* d_win,
                                const lzq_window_tables* d_tables, const lzq_ode_params* d_ode, lzq_yield* d_out,
                                void* stream) {
  const char* fn = "lzq_yields_batch_reuse_wash";
  if (n < 0 || n_tables < 0 || (n > 0 && (!d_points || !d_ode || !d_out || !d_rep || !d_table_index || n_tables == 0)))
    return fail(LZQ_EINVAL, "%s: bad arguments", fn);
  double key_nz;
  int rc = z_key(nz, z_max, fn, key_nz);
  if (rc) return rc;
  lzq_window_tables wt = {0, 0, nullptr, nullptr};
  if (d_win && (rc = lzq::window_tables_arg(d_tables, fn, wt))) return rc;
  if (n == 0) return LZQ_OK;
  if ((rc = workspace_ok(n_tables, n_y, d_work, work_doubles, fn))) return rc;
  const int64_t nb = (n + lzq::kWavesPerBlock - 1) / lzq::kWavesPerBlock;
  if (nb > kMaxGrid) return fail(LZQ_EINVAL, "%s: n too large for one launch", fn);
  // The tables are lzq_yields_batch_reuse's: its table kernel runs for all n_tables whatever the number
  // of points, so it is called for point 0 alone, whose record this call's own kernel then overwrites.
  rc = lzq::yields_batch_reuse(d_points, 1, n_y, nz, z_max, d_P, d_rep, d_table_index, n_tables, d_work, work_doubles,
                               nullptr, nullptr, d_out, stream, nz == LZQ_WASH_NZ_CONT, fn);
  if (rc) return rc;
  hipLaunchKernelGGL(lzq::points_reuse_wash_kernel, dim3((unsigned)nb), dim3(lzq::kBlock), 0, (hipStream_t)stream,
                     d_points, d_ode, d_win, wt, n, n_y, d_P, key_nz, z_max, d_table_index, d_work,
                     n_of(n_y) + lzq::kTabHdr, n_tables, d_out);
  return hip_ok(fn);
}

int lzq_sweep_grid_from_ztables_wash(const lzq_point* base, const lzq_window* base_win, const lzq_ode_params* base_ode,
                                     const lzq_axis* axes, int32_t n_axes, int64_t start, int64_t count, int32_t n_y,
                                     int32_t nz, double z_max, const double* d_P, const double* d_work,
                                     int64_t work_doubles, const lzq_window_tables* d_tables, lzq_yield* d_out,
                                     void* stream) {
  const char* fn = "lzq_sweep_grid_from_ztables_wash";
  lzq::GridSpec gs;
  int64_t n_tab;
  int rc = make_wash_grid(base, base_ode, axes, n_axes, start, count, d_out, fn, base_win != nullptr, -1, gs, &n_tab);
  if (rc) return rc;
  double key_nz;
  if ((rc = z_key(nz, z_max, fn, key_nz))) return rc;
  lzq_window_tables wt = {0, 0, nullptr, nullptr};
  if (base_win && (rc = lzq::window_tables_arg(d_tables, fn, wt))) return rc;
  if (count == 0) return LZQ_OK;
  if ((rc = workspace_ok(n_tab, n_y, d_work, work_doubles, fn))) return rc;
  const int64_t nb = (count + lzq::kWavesPerBlock - 1) / lzq::kWavesPerBlock;
  if (nb > kMaxGrid) return fail(LZQ_EINVAL, "%s: too large for one launch", fn);
  hipLaunchKernelGGL(lzq::grid_reuse_wash_kernel, dim3((unsigned)nb), dim3(lzq::kBlock), 0, (hipStream_t)stream, *base,
                     *base_ode, base_win ? *base_win : lzq_window(), base_win ? 1 : 0, gs, wt, start, count, n_y, d_P,
                     key_nz, z_max, d_work, n_of(n_y) + lzq::kTabHdr, d_out);
  return hip_ok(fn);
}

int lzq_solve_check_host_wash(const lzq_solve* solve, const lzq_window* base_win, const lzq_ode_params* base_ode,
                              const lzq_axis* axes, int32_t n_axes) {
  if (!base_ode) return lzq_solve_check_host(solve, base_win, axes, n_axes);  // the list allowed without a block
  if (!solve || n_axes < 0 || n_axes > LZQ_MAX_AXES || (n_axes > 0 && !axes))
    return lzq_set_error(LZQ_EINVAL, "lzq_solve: bad arguments");
  int rc = check_block(*base_ode, "lzq_solve: base wash block", 0);
  if (rc) return rc;
  if (solve->field != LZQ_F_GAMMA_WASH) {
    if (solve->field == LZQ_F_DEPLETE)
      return fail(LZQ_EINVAL, "lzq_solve: deplete_DM_from_source (field %d) is a switch, not a solve field",
                  (int)solve->field);
    // every other field: the checks it has today, on the axis list without the wash axes
    lzq_axis rest[LZQ_MAX_AXES];
    int32_t n_rest = 0;
    for (int a = 0; a < n_axes; ++a)
      if (!lzq::wash_field(axes[a].field)) rest[n_rest++] = axes[a];
    return lzq_solve_check_host(solve, base_win, rest, n_rest);
  }
  if (solve->target_field < 0 || solve->target_field > 5)
    return fail(LZQ_EINVAL, "lzq_solve: target field %lld outside [0, 5]", (long long)solve->target_field);
  if (!lzq::solve_finite(solve->lo) || !lzq::solve_finite(solve->hi))
    return fail(LZQ_EINVAL, "lzq_solve: bounds lo = %g, hi = %g must be finite", solve->lo, solve->hi);
  if (!(solve->lo < solve->hi))
    return fail(LZQ_EINVAL, "lzq_solve: bounds need lo < hi (lo = %g, hi = %g)", solve->lo, solve->hi);
  if (solve->lo < 0.0)
    return fail(LZQ_EINVAL, "lzq_solve: Gamma_wash_over_H is read as max(., 0) (fpy:284): lo = %g < 0 leaves the "
                            "field flat below 0", solve->lo);
  if (!lzq::solve_finite(solve->target)) return fail(LZQ_EINVAL, "lzq_solve: target = %g must be finite", solve->target);
  if (!(solve->xtol >= 0.0 && solve->xtol < 1.0)) return fail(LZQ_EINVAL, "lzq_solve: xtol = %g outside [0, 1)", solve->xtol);
  for (int a = 0; a < n_axes; ++a)
    if (axes[a].field == LZQ_F_GAMMA_WASH) return fail(LZQ_EINVAL, "lzq_solve: axis %lld writes the solve field", (long long)a);
  return LZQ_OK;
}

int lzq_sweep_grid_solve_wash(const lzq_point* base, const lzq_window* base_win, const lzq_ode_params* base_ode,
                              const lzq_axis* axes, int32_t n_axes, const lzq_solve* solve, int64_t start,
                              int64_t count, int32_t n_y, int32_t nz, double z_max, const double* d_P,
                              const double* d_work, int64_t work_doubles, const lzq_window_tables* d_tables,
                              lzq_yield* d_out, lzq_solve_result* d_sol, void* stream) {
  const char* fn = "lzq_sweep_grid_solve_wash";
  if (!solve || !base_ode || (count > 0 && !d_sol)) return fail(LZQ_EINVAL, "%s: bad arguments", fn);
  int rc = lzq_solve_check_host_wash(solve, base_win, base_ode, axes, n_axes);
  if (rc) return rc;
  const int32_t sf = solve->field;
  if (d_P && (sf == LZQ_F_P || lz_field(sf)))
    return fail(LZQ_EINVAL, "%s: a per-point P override (d_P) together with a solve for P or an LZ field", fn);
  lzq::GridSpec gs;
  int64_t n_tab;
  rc = make_wash_grid(base, base_ode, axes, n_axes, start, count, d_out, fn, base_win != nullptr, sf, gs, &n_tab);
  if (rc) return rc;
  double key_nz;
  if ((rc = z_key(nz, z_max, fn, key_nz))) return rc;
  lzq_window_tables wt = {0, 0, nullptr, nullptr};
  if (base_win && (rc = lzq::window_tables_arg(d_tables, fn, wt))) return rc;
  if (count == 0) return LZQ_OK;
  if ((rc = workspace_ok(n_tab, n_y, d_work, work_doubles, fn))) return rc;
  const int64_t nb = (count + lzq::kWavesPerBlock - 1) / lzq::kWavesPerBlock;
  if (nb > kMaxGrid) return fail(LZQ_EINVAL, "%s: too large for one launch", fn);
  lzq_solve sv = *solve;
  sv.max_evals = lzq::solve_clamp_evals(sv.max_evals);
  hipLaunchKernelGGL(lzq::grid_solve_wash_kernel, dim3((unsigned)nb), dim3(lzq::kBlock), 0, (hipStream_t)stream, *base,
                     *base_ode, base_win ? *base_win : lzq_window(), base_win ? 1 : 0, gs, wt, sv, start, count, n_y,
                     d_P, key_nz, z_max, d_work, n_of(n_y) + lzq::kTabHdr, d_out, d_sol);
  return hip_ok(fn);
}

}  // extern "C"
