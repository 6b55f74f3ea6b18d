// lzq_solve.hip -- lzq_sweep_grid_solve: one parameter per grid point solved for a target value of
// a yield field, on the device (include/lzq.h; the rule is csrc/lzq_solve.h, one definition for host
// and device).
//
// One wavefront per grid point, built like grid_reuse_kernel / grid_reuse_window_kernel: the point
// (and its window block) are decoded from the flat index; each evaluation of f(x) = field(x) - target
// writes x into the solve field, and is then one
// reuse-mode point -- quad_setup, epilogue_pre, park, yb_wave<kYbReuse> on the point's z-sum table,
// epilogue_finish.  The allowed solve fields cannot change the y-grid or c, so every evaluation reads
// the same table (its header is matched once, at lo) and the solve builds no z-sum of its own.
//
// Every lane holds the same butterfly sum, so x, f and every decision of the rule are wave-uniform;
// f goes through uniform() and the loop control through readfirstlane, so it is scalar.  The rule's
// state and the records of the two bracket ends live in the slot, not in registers: nothing but
// yb_wave's own state is live across it, as in the other quadrature kernels.  The record stored for
// a point is the evaluation's own at x*, not a re-evaluation.  The loop is bounded by
// kSolveMaxEvals whatever the host passed.
//
// Its own translation unit: no existing code object changes.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#define LZQ_QUAD_CONST_LINKAGE static
#include "lzq_quad.h"
#include "lzq_internal.h"
#include "lzq_quad_window.h"
#include "lzq_solve.h"
#include "lzq_window.h"

namespace lzq {

// WinWaveSlot extended by what the solve keeps between evaluations.
struct SolveWaveSlot {
  QuadSetup s;
  EpiPre e;
  double acc[kWaveSize];
  WinParams win;
  SolveState st;     // the rule's state
  lzq_yield rec[2];  // the records of the bracket's lower and upper end
};

__device__ __forceinline__ double yield_field(const lzq_yield& o, int32_t f) {
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
__device__ __forceinline__ SolveState load_state(const SolveState& m) {
  SolveState s;
  s.a = uniform(m.a), s.b = uniform(m.b), s.fa = uniform(m.fa), s.fb = uniform(m.fb);
  s.ga = uniform(m.ga), s.gb = uniform(m.gb), s.w = uniform(m.w), s.w1 = uniform(m.w1), s.w2 = uniform(m.w2);
  s.lo = uniform(m.lo), s.hi = uniform(m.hi), s.xtol = uniform(m.xtol);
  s.evals = __builtin_amdgcn_readfirstlane(m.evals), s.max_evals = __builtin_amdgcn_readfirstlane(m.max_evals);
  s.side = __builtin_amdgcn_readfirstlane(m.side), s.force = __builtin_amdgcn_readfirstlane(m.force), s.status = __builtin_amdgcn_readfirstlane(m.status);
  s.done = __builtin_amdgcn_readfirstlane(m.done);
  return s;
}

// WIN: the window of the point's block (SlotWindow), else the point's Gaussian (SlotGaussWindow)
template <bool WIN>
__global__ __launch_bounds__(kBlock, LZQ_REUSE_MIN_WAVES) void grid_solve_kernel(
    lzq_point base, lzq_window base_win, GridSpec grid, lzq_window_tables wt, lzq_solve sv, int64_t start,
    int64_t count, int32_t n_y, const double* __restrict__ Pov, double key_nz, double key_z_max,
    const double* __restrict__ Fw, int64_t tstride, lzq_yield* __restrict__ out,
    lzq_solve_result* __restrict__ sol) {
  __shared__ SolveWaveSlot slots[kWavesPerBlock];
  const int lane = threadIdx.x & (kWaveSize - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t local = (int64_t)blockIdx.x * kWavesPerBlock + w;
  if (local >= count) return;  // wave-uniform
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
    SolveState st = load_state(slots[wi].st);
    double x;
    const bool more = solve_next(st, x);
    if (!__builtin_amdgcn_readfirstlane((int)more)) break;
    x = uniform(x);
    // the point at x: decoded from the flat index as in grid_reuse_kernel (scalar loads, every
    // evaluation anew: nothing of it is live across yb_wave), then the solve field written as an
    // axis of the one value x would write it
    int64_t idx = start + local;
    asm volatile("" : "+s"(idx));  // (not hoisted out of the loop into registers)
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
    } else if (!window_field(sv.field)) {
      double d0, d1, d2;
      set_field(pt, sv.field, x, d0, d1, d2);
      if (sv.field == LZQ_F_P) P = x;
      if (sv.field == LZQ_F_V_W && ax_mix) {
        // v_w enters eq.(8): the P of the m_mix / dprime axes is re-formed with v_w = x, as grid_point
        // forms it when v_w is an axis (a per-point override still takes precedence)
        pt.P_chi_to_B = p_closed_form(m_mix * m_mix / (2.0 * pymax(pt.v_w, 1e-12) * fabs(dprime)));
        if (!Pov) P = pt.P_chi_to_B;
      }
    }
    if (sv.field == LZQ_F_DELTA_LZ || sv.field == LZQ_F_M_MIX || sv.field == LZQ_F_DPRIME) pt.P_chi_to_B = P;
    const QuadSetup qs = quad_setup(pt, P, pt.T_min_over_Tp * pt.T_p_GeV, pt.T_max_over_Tp * pt.T_p_GeV, n_y);
    if (it == 0) {
      // match is wave-uniform: every lane formed the same setup; no allowed field moves the y-grid
      const bool match = qs.empty || (F[0] == qs.y_lo && F[1] == qs.y_hi && F[2] == (double)qs.n &&
                                      F[3] == qs.cneg && F[4] == key_nz && F[5] == key_z_max);
      if (!match) {
        bad_table = true;
        break;
      }
    }
    double Y_B;
    if constexpr (WIN) {
      lzq_window blk = window_grid_block(base_win, grid, idx);
      window_set_field(blk, sv.field, x);  // (a field of the point: not written)
      park_window(slots[w], qs, epilogue_pre(pt, P), window_params(blk, wt.n_tables, wt.n_knots, wt.u, wt.W), lane);
      // inlined at this call: yb_wave keeps its wave index in a scalar register, which only the
      // kernel's own (readfirstlane) w can supply
      [[clang::always_inline]] Y_B = yb_wave<kYB, kExpTable, kYbReuse, 0, SlotWindow>(slots, w, nullptr, 0, nullptr, 0,
                                                                                        F + LZQ_REUSE_TABLE_HEADER);
    } else {
      if (lane == 0) {
        slots[w].s = qs;
        slots[w].e = epilogue_pre(pt, P);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      [[clang::always_inline]] Y_B = yb_wave<kYB, kExpTable, kYbReuse, 0, SlotGaussWindow>(
          slots, w, nullptr, 0, nullptr, 0, F + LZQ_REUSE_TABLE_HEADER);
    }
    int wr = w;
    asm volatile("" : "+s"(wr));
    const lzq_yield o = epilogue_finish(slots[wr].e, Y_B);
    const double f = uniform(yield_field(o, sv.target_field) - sv.target);
    st = load_state(slots[wr].st);
    const int32_t mask = __builtin_amdgcn_readfirstlane(solve_feed(st, x, f));
    if (lane == 0) {
      slots[wr].st = st;
      if (mask & 1) slots[wr].rec[0] = o;
      if (mask & 2) slots[wr].rec[1] = o;
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

int lzq::launch_grid_solve(const lzq_point& base, const lzq_window* base_win, const GridSpec& grid,
                           const lzq_window_tables& wt, const lzq_solve& solve, int64_t start, int64_t count,
                           int32_t n_y, const double* d_P, double key_nz, double key_z_max, const double* d_work,
                           int64_t stride, lzq_yield* d_out, lzq_solve_result* d_sol, hipStream_t s) {
  const int64_t nb = (count + kWavesPerBlock - 1) / kWavesPerBlock;
  lzq_solve sv = solve;
  sv.max_evals = solve_clamp_evals(sv.max_evals);
  if (base_win)
    hipLaunchKernelGGL(grid_solve_kernel<true>, dim3((unsigned)nb), dim3(kBlock), 0, s, base, *base_win, grid, wt, sv,
                       start, count, n_y, d_P, key_nz, key_z_max, d_work, stride, d_out, d_sol);
  else
    hipLaunchKernelGGL(grid_solve_kernel<false>, dim3((unsigned)nb), dim3(kBlock), 0, s, base, lzq_window(), grid, wt,
                       sv, start, count, n_y, d_P, key_nz, key_z_max, d_work, stride, d_out, d_sol);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? LZQ_OK : lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
}

namespace {

template <class... A>
int solve_fail(const char* fmt, A... a) {
  char msg[256];
  snprintf(msg, sizeof(msg), fmt, a...);
  return lzq_set_error(LZQ_EINVAL, msg);
}

bool lz_field(int32_t f) { return f == LZQ_F_DELTA_LZ || f == LZQ_F_M_MIX || f == LZQ_F_DPRIME; }

}  // namespace

extern "C" int lzq_solve_check_host(const lzq_solve* solve, const lzq_window* base_win, const lzq_axis* axes,
                                    int32_t n_axes) {
  if (!solve || n_axes < 0 || n_axes > LZQ_MAX_AXES || (n_axes > 0 && !axes))
    return lzq_set_error(LZQ_EINVAL, "lzq_solve: bad arguments");
  const int32_t f = solve->field;
  if (f == LZQ_F_I_P || f == LZQ_F_BETA_OVER_H || f == LZQ_F_T_P || f == LZQ_F_T_MIN_OVER_TP ||
      f == LZQ_F_T_MAX_OVER_TP)
    return solve_fail("lzq_solve: field %lld changes the z-sum tables (I_p, beta_over_H, T_p, T_min/T_max_over_Tp): "
                      "not a solve field", (long long)f);
  if (f == LZQ_F_WIN_TABLE) return solve_fail("lzq_solve: the window table index (field %lld) is not a solve field", (long long)f);
  const bool win = lzq::window_field(f);
  if (!((f >= LZQ_F_M_CHI && f <= LZQ_F_N_CHI_AT_TP) || lz_field(f) || win)) return solve_fail("lzq_solve: unknown solve field %lld", (long long)f);
  if (win && !base_win) return solve_fail("lzq_solve: window field %lld needs a window block", (long long)f);
  if (f == LZQ_F_SIGMA_Y && base_win)
    return lzq_set_error(LZQ_EINVAL, "lzq_solve: source_shape_sigma_y is not read when the point has a window block: "
                                     "solve a window field (LZQ_F_WIN_SIGMA) instead");
  if (solve->target_field < 0 || solve->target_field > 5)
    return solve_fail("lzq_solve: target field %lld outside [0, 5]", (long long)solve->target_field);
  if (!lzq::solve_finite(solve->lo) || !lzq::solve_finite(solve->hi))
    return solve_fail("lzq_solve: bounds lo = %g, hi = %g must be finite", solve->lo, solve->hi);
  if (!(solve->lo < solve->hi))
    return solve_fail("lzq_solve: bounds need lo < hi (lo = %g, hi = %g)", solve->lo, solve->hi);
  if (!lzq::solve_finite(solve->target)) return solve_fail("lzq_solve: target = %g must be finite", solve->target);
  if (!(solve->xtol >= 0.0 && solve->xtol < 1.0))
    return solve_fail("lzq_solve: xtol = %g outside [0, 1)", solve->xtol);
  bool ax_mix = false, ax_dpr = false, ax_delta = false;
  for (int a = 0; a < n_axes; ++a) {
    const int32_t g = axes[a].field;
    ax_mix |= g == LZQ_F_M_MIX;
    ax_dpr |= g == LZQ_F_DPRIME;
    ax_delta |= g == LZQ_F_DELTA_LZ;
    const bool same = win ? (lzq::window_field_mask(f) & lzq::window_field_mask(g)) != 0 : g == f;
    if (same) return solve_fail("lzq_solve: axis %lld writes the solve field", (long long)a);
  }
  // P is what the LZ fields set (grid_point): one source for it
  if (f == LZQ_F_P && (ax_mix || ax_dpr || ax_delta))
    return lzq_set_error(LZQ_EINVAL, "lzq_solve: an LZ axis writes P, the solve field");
  if (f == LZQ_F_DELTA_LZ && (ax_mix || ax_dpr))
    return lzq_set_error(LZQ_EINVAL, "lzq_solve: m_mix / dprime axes write delta_LZ, the solve field");
  if (f == LZQ_F_M_MIX && (!ax_dpr || ax_delta))
    return lzq_set_error(LZQ_EINVAL, "lzq_solve: a solve for m_mix needs a dprime axis and no delta_LZ axis");
  if (f == LZQ_F_DPRIME && (!ax_mix || ax_delta))
    return lzq_set_error(LZQ_EINVAL, "lzq_solve: a solve for dprime needs an m_mix axis and no delta_LZ axis");
  return LZQ_OK;
}
