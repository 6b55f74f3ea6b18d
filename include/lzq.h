/*
 * lzq.h -- C ABI of the MI355X-native bounce-sourced Landau-Zener yield engine.
 *
 * Drop-in boundary for the hot path of /root/reference/first_principles_yields.py ("fpy"):
 *
 *   fpy:141-165  AoverVKernel(..., z_max, nz) / A_over_V_y -> lzq_aov_batch (any z grid: nz, z_max)
 *   fpy:231-267  integrate_YB_by_quadrature           -> lzq_yields_batch (out->Y_B), lzq_sweep_grid
 *   fpy:372-384, fpy:413-417  Y_chi + densities        -> lzq_yields_batch / lzq_sweep_grid epilogue
 *   fpy:170-187  LZ plug-in closed form (fpy:183-184)  -> lzq_p_closed_form
 *   fpy:222-223 + fpy:122-123  J_chi (diagnostics)     -> lzq_jchi_batch
 *   (no reference counterpart; north_star (1))        -> lzq_lz_propagate
 *   fpy:200-219, 270-286, 385-417  ODE fallback        -> lzq_ode_tables / _integrate / _batch,
 *                                                         lzq_ode_integrate_shared, lzq_ode_quadrature,
 *                                                         lzq_ode_aov_T, lzq_ode_rhs
 *
 * Conventions (all entry points):
 *   - plain C types only; device buffers are raw device pointers, `stream` is a hipStream_t
 *     passed as void* (NULL = the null stream) and must belong to the current HIP device;
 *   - the caller owns every buffer; the library never frees caller memory; launches are
 *     asynchronous on `stream` (no host synchronisation inside the launch functions once
 *     lzq_init has run for the device);
 *   - return 0 on success, a negative LZQ_E* code on failure; lzq_last_error() returns a
 *     thread-local message for the last failure on the calling thread; no C++ exception
 *     crosses the boundary;
 *   - results are deterministic: each point is reduced by one wavefront in a fixed order, so
 *     they do not depend on launch geometry, batch composition or the number of GPUs.
 */
#ifndef LZQ_H
#define LZQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LZQ_ABI_VERSION 3   /* 3: optional lzq_aov_params on the A/V-evaluating entry points */
#define LZQ_NZ 1200          /* fpy:142 nz default, used unchanged at fpy:197 */
#define LZQ_Z_MAX 30.0       /* fpy:142 z_max default */
#define LZQ_NZ_MAX (1 << 22) /* largest z grid accepted (64 MB of device nodes) */
#define LZQ_NY_MAIN 8000     /* fpy:374 */
#define LZQ_NY_MIN 2000      /* fpy:246 */

enum lzq_status {
  LZQ_OK = 0,
  LZQ_EINVAL = -1,       /* bad argument (null pointer, n < 0, unknown field, ...)        */
  LZQ_EHIP = -2,         /* a HIP runtime call failed (message has the HIP error string)  */
  LZQ_EUNSUPPORTED = -3, /* configuration outside the fast quadrature path (fpy:372)       */
  LZQ_ENODEVICE = -4
};

/* chi statistics (fpy:96: str(stats).lower().startswith("ferm")) */
enum lzq_stats { LZQ_FERMION = 0, LZQ_BOSON = 1 };
/* regime (fpy:376-384); LZQ_REGIME_OTHER ("auto") has no branch in the reference, which
 * raises UnboundLocalError; the engine returns NaN yields for such points. */
enum lzq_regime { LZQ_THERMAL = 0, LZQ_NONTHERMAL = 1, LZQ_REGIME_OTHER = 2 };

/* One parameter point: the fpy `Config` fields (fpy:44-79) read by the fast path.
 * Optional[float] fields carry has_* flags.  136 bytes, 8-byte aligned. */
typedef struct lzq_point {
  double m_chi_GeV;            /* field  0 */
  double g_chi;                /* field  1 (int in fpy; used as a float factor) */
  double T_p_GeV;              /* field  2 */
  double beta_over_H;          /* field  3 */
  double v_w;                  /* field  4 */
  double I_p;                  /* field  5 */
  double g_star;               /* field  6 */
  double g_star_s;             /* field  7 */
  double P_chi_to_B;           /* field  8 */
  double source_shape_sigma_y; /* field  9 */
  double incident_flux_scale;  /* field 10 */
  double T_max_over_Tp;        /* field 11 */
  double T_min_over_Tp;        /* field 12 */
  double Y_chi_init;           /* field 13 (valid iff has_Y_chi_init) */
  double n_chi_at_Tp_GeV3;     /* field 14 (valid iff has_n_chi_at_Tp) */
  int32_t stats;               /* enum lzq_stats  */
  int32_t regime;              /* enum lzq_regime */
  int32_t has_Y_chi_init;
  int32_t has_n_chi_at_Tp;
} lzq_point;

/* The A/V kernel's own parameters: AoverVKernel(I_p, beta_over_H, T_p, v_w, g_star, z_max, nz)
 * (fpy:141-151).  BoltzmannSystem builds self.aov from cfg (fpy:197), but it is a separate public
 * object: integrate_YB_by_quadrature (fpy:261), build_tables (fpy:211) and S_B_T (fpy:228) take
 * A/V from self.aov while the y-grid, T(y), H, s, J and window come from self.cfg (fpy:234-262).
 * Entry points that take an optional lzq_aov_params block use it for the A/V constants
 * pref0 = (I_p/2)(beta/max(v_w, 1e-12)), beta = beta_over_H H_std(T_p, g_star), and c = -I_p/6
 * (fpy:146-151, 162-163); NULL = the point's own fields (self.aov built from cfg).  40 bytes. */
typedef struct lzq_aov_params {
  double I_p;          /* fpy:143 */
  double beta_over_H;  /* fpy:144 */
  double T_p_GeV;      /* fpy:145 (AoverVKernel's T_p) */
  double v_w;          /* fpy:146 (max(., 1e-12) applied) */
  double g_star;       /* fpy:147 */
} lzq_aov_params;

/* Per-point yield record: the `final` block of yields_out.json (fpy:425-427) + P_used
 * (fpy:424).  48 bytes; tables of these are what the multi-GPU all-gather moves. */
typedef struct lzq_yield {
  double Y_B, Y_chi, rho_B_kg_m3, rho_DM_kg_m3, DM_over_B, P_used;
} lzq_yield;

/* Sweep axis fields.  0..14 address the double fields of lzq_point in declaration order.
 * Derived LZ fields set P_chi_to_B through the closed form (fpy:183-184, PAPER eq.(9)):
 *   LZQ_F_DELTA_LZ           : P = clamp(1 - exp(-2 pi max(delta, 0)), 0, 1)
 *   LZQ_F_M_MIX, LZQ_F_DPRIME: delta = m_mix^2 / (2 max(v_w,1e-12) |Delta'|) (PAPER eq.(8), F = 1)
 * Axis values live in device memory. */
enum lzq_field {
  LZQ_F_M_CHI = 0, LZQ_F_G_CHI = 1, LZQ_F_T_P = 2, LZQ_F_BETA_OVER_H = 3, LZQ_F_V_W = 4,
  LZQ_F_I_P = 5, LZQ_F_G_STAR = 6, LZQ_F_G_STAR_S = 7, LZQ_F_P = 8, LZQ_F_SIGMA_Y = 9,
  LZQ_F_FLUX = 10, LZQ_F_T_MAX_OVER_TP = 11, LZQ_F_T_MIN_OVER_TP = 12, LZQ_F_Y_CHI_INIT = 13,
  LZQ_F_N_CHI_AT_TP = 14,
  LZQ_F_DELTA_LZ = 32, LZQ_F_M_MIX = 33, LZQ_F_DPRIME = 34,
  /* fields of the point's window block (lzq_window below), accepted only by the *_window grid
   * entry points; every other one refuses them as unknown fields */
  LZQ_F_WIN_Y0 = 64, LZQ_F_WIN_HALF_WIDTH = 65, LZQ_F_WIN_SIGMA_LO = 66, LZQ_F_WIN_SIGMA_HI = 67,
  LZQ_F_WIN_SIGMA = 68 /* sigma_lo and sigma_hi */, LZQ_F_WIN_SCALE = 69,
  LZQ_F_WIN_TABLE = 70 /* table, from a double holding an integer */,
  /* fields of the point's lzq_ode_params block, accepted only by the *_wash grid entry points ("wash-out
   * and source depletion" below); every other one refuses them as unknown fields */
  LZQ_F_GAMMA_WASH = 96 /* Gamma_wash_over_H */,
  LZQ_F_DEPLETE = 97 /* deplete_DM_from_source: value != 0 */
};

#define LZQ_MAX_AXES 8
typedef struct lzq_axis {
  int32_t field;          /* enum lzq_field */
  int32_t n;              /* number of values (> 0) */
  const double* values;   /* device pointer, n doubles */
} lzq_axis;

/* ---- library / device management ---------------------------------------------------- */
int lzq_abi_version(void);
const char* lzq_last_error(void);
/* The z grid.  Every entry point that evaluates A/V (fpy:158-165) takes the grid of the
 * reference operator AoverVKernel(I_p, beta_over_H, T_p, v_w, g_star, z_max=30.0, nz=1200)
 * (fpy:141-156) as (int32 nz, double z_max): z = linspace(0, z_max, nz), the cancelling gamma4
 * of fpy:156 verbatim, the trapezoid of fpy:164.  (LZQ_NZ, LZQ_Z_MAX) is the grid main() uses
 * (fpy:197) and runs the compile-time-sized headline kernels; any other grid is built on the
 * host and uploaded once per (device, nz, z_max) on first use (a synchronous copy), then kept.
 * 0 <= nz <= LZQ_NZ_MAX (nz < 0 is numpy's ValueError) and 0 <= z_max < inf; nz <= 1 or z_max = 0
 * give A/V = 0 exactly, as numpy's trapezoid of <= 1 node / zero width does.  Refused with
 * LZQ_EINVAL although numpy accepts them (documented parity gaps):
 *   - z_max < 0: linspace(0, z_max, nz) runs backwards and the trapezoid of fpy:164 changes sign;
 *   - a grid so fine that the cancelling gamma4 of fpy:156 rounds below 0 (the reference then
 *     exponentiates positive arguments) or stops being non-decreasing (rounding noise of a few ulp
 *     of 6.0 at the first nodes): z_1 below ~1e-3, i.e. nz >~ 2e4 on [0, 1] or >~ 1e5 on [0, 30]. */
/* Builds and uploads the default z tables (fpy:154-156) and the exp table for `device`.  Called
 * lazily by every entry point; call it up front before capturing launches into a graph. */
int lzq_init(int device);
/* The same for the grid (nz, z_max) (lzq_init = lzq_zgrid_init(device, LZQ_NZ, LZQ_Z_MAX)). */
int lzq_zgrid_init(int device, int32_t nz, double z_max);
/* Host copies of the z tables of the grid (nz, z_max): z (fpy:154), gamma4 (fpy:156) and the
 * quadrature weights omega_k = z_k^2 e^{-z_k} * (trapezoid weight of node k); nz entries each
 * (any pointer may be NULL). */
int lzq_ztables(int32_t nz, double z_max, double* z, double* gamma4, double* omega);

/* Tuning knobs for ablations (process-wide, not thread-safe against concurrent launches).
 * LZQ_TUNE_EXP selects the inner-loop exponential: LZQ_EXP_TABLE (default; 2^(j/N) LDS table,
 * N = 2^LZQ_TABBITS = 8192, + degree-2 minimax polynomial in completed-square form, <= 1.73e-14 relative) or
 * LZQ_EXP_POLY11 (degree-11 minimax polynomial, 0.6 ulp).  Results agree to ~1e-14 relative.
 * Returns the previous value. */
/* LZQ_TUNE_TRUNCATE (0 = dense, the default; 1 = on): stop each wave's z-sum at the first
 * node beyond which every lane's term is below 2^-1080, where it can no longer change the
 * FP64 accumulator.  Results are bit-identical to the dense sum; fewer nodes are executed.
 * The headline benchmark is dense and reports this mode separately. */
/* LZQ_TUNE_ODE_COOP (1 = on, the default; 0 = off): the ODE integrator's cooperative mode,
 * where a full wavefront of points that differ only in P, flux, sigma_v, Gamma_wash, deplete
 * and the initial state evaluates each step's stage ingredients once for the whole wavefront.
 * Results are bit-identical either way (tests/test_gpu_ode.py). */
/* LZQ_TUNE_ODE_LAUNCH_STEPS (value = log2 of the steps per launch, 6..40; default 24): the ODE
 * integrator runs a batch as continuation launches of at most 2^value fixed Radau steps each,
 * ceil(max_steps / 2^value) launches (<= 65536), the per-point state carried between them in
 * stream-ordered scratch (64 B per point), so any window the reference accepts completes in
 * bounded launches.  Results are bit-identical for every value (tests/test_gpu_ode.py). */
/* LZQ_TUNE_PROFILE_FLAT (1 = on; 0 = off, the default): lzq_lz_propagate_profile's flattened
 * propagation (the step rule for all of a point's knot intervals ahead of the propagation, then one
 * loop of Magnus steps per lane, a lane entering its next interval while the others step) or the
 * interval-by-interval loop in keyed launch order (measured faster).  P is
 * bit-identical either way (tests/test_gpu_profile.py). */
/* LZQ_TUNE_ODE_TP_INTERVAL (steps, a multiple of 64 in [64, 2^20]; default 64): the interval length of
 * lzq_ode_integrate_tp's multiple shooting (longer for a point whose window would need over 65536
 * intervals). */
/* LZQ_TUNE_ODE_TABLE_WIDE (bit mask, default 3 = both; 0 = off): lzq_ode_tables for few tables
 * (<= 4096) spreads each table wide -- bit 0: the A/V knots over 64-knot wavefronts instead of one
 * wavefront per table; bit 1: the spline's per-knot work over a wavefront's lanes around its two
 * recurrences instead of one lane per table.  The tables are bit-identical either way
 * (tests/test_gpu_ode_tp.py). */
/* LZQ_TUNE_CONT_SKIP (1 = on, the default; 0 = off): the z-sum tables of the continuum z rule (the
 * *_cont entry points below) from the live-range kernel -- one wavefront per (table, 64 y-nodes), each
 * stopping at the first node beyond which every lane's term underflows -- or, off, from the table
 * kernel of the linspace grids at every node.  The tables are bit-identical either way
 * (tests/test_gpu_cont.py). */
enum lzq_tune_key { LZQ_TUNE_EXP = 0, LZQ_TUNE_TRUNCATE = 1, LZQ_TUNE_ODE_COOP = 2, LZQ_TUNE_ODE_LAUNCH_STEPS = 3,
                    LZQ_TUNE_PROFILE_FLAT = 4, LZQ_TUNE_ODE_TP_INTERVAL = 5, LZQ_TUNE_ODE_TABLE_WIDE = 6,
                    LZQ_TUNE_CONT_SKIP = 7 };
enum lzq_exp_variant { LZQ_EXP_POLY11 = 0, LZQ_EXP_TABLE = 1 };
int lzq_tune(int32_t key, int32_t value);

/* ---- hot path -------------------------------------------------------------------------- */
/* fpy:158-165: out[i] = A_over_V_y(y[i]) for the kernel AoverVKernel(I_p, beta_over_H, T_p, v_w,
 * g_star, z_max, nz): aov (host struct) if non-NULL, else point *pt's fields (pt may then be NULL
 * only if aov is not; no other field of *pt is read). */
int lzq_aov_batch(const lzq_point* pt, const lzq_aov_params* aov, const double* d_y, int64_t n, int32_t nz,
                  double z_max, double* d_out, void* stream);

/* fpy:222-223: out[i] = BoltzmannSystem.J_chi(T[i]) for point *pt (diagnostics table). */
int lzq_jchi_batch(const lzq_point* pt, const double* d_T, int64_t n, double* d_out, void* stream);

/* fpy:231-267 + fpy:372-384 + fpy:413-417 for n explicit points (device AoS array).
 * d_T_lo / d_T_hi: optional per-point integration range (NULL: main()'s
 * T_lo = T_min_over_Tp*T_p, T_hi = T_max_over_Tp*T_p, fpy:367-369).
 * d_P: optional per-point P override (NULL: point.P_chi_to_B), e.g. lzq_lz_propagate output.
 * n_y: y-grid size as passed to integrate_YB_by_quadrature (fpy:374 uses 8000; raised to
 * LZQ_NY_MIN as fpy:246).  (nz, z_max): the A/V kernel's z grid (fpy:141-142; main(): LZQ_NZ,
 * LZQ_Z_MAX).  d_aov: optional [n] device lzq_aov_params, point i's A/V kernel (bs.aov replaced,
 * fpy:261); NULL = each point's own fields (fpy:197), the headline kernels. */
int lzq_yields_batch(const lzq_point* d_points, int64_t n, int32_t n_y, int32_t nz, double z_max,
                     const double* d_T_lo, const double* d_T_hi, const double* d_P, const lzq_aov_params* d_aov,
                     lzq_yield* d_out, void* stream);

/* Cartesian sweep: points [start, start+count) of the grid base x axes[0] x ... x
 * axes[n_axes-1] (C order: last axis fastest), generated on device from the flat index.
 * d_P: optional [count] per-point P override (e.g. lzq_lz_propagate output for multi-crossing
 * profiles, config C5); it takes precedence over P_chi_to_B and the LZ axes. */
int lzq_sweep_grid(const lzq_point* base, const lzq_axis* axes, int32_t n_axes,
                   int64_t start, int64_t count, int32_t n_y, int32_t nz, double z_max, const double* d_P,
                   lzq_yield* d_out, void* stream);

/* lzq_sweep_grid with the z-sums shared -- a separate mode, NOT the dense headline path
 * (SURVEY §8d allows separable reuse only as such).  The z-sums F(y_j) = sum_k omega_k
 * exp(c(y_j) gamma4_k) of fpy:160-165 depend on a point only through I_p, beta_over_H, T_p_GeV,
 * T_min_over_Tp, T_max_over_Tp (its y-grid and c, fpy:141-156, 234-247) and n_y: they are
 * computed once per combination of the grid's values of those fields (each table = the dense
 * kernel's passes for the combination's first grid point, into d_work), then every point of
 * [start, start+count) is integrated from its table.  Yields are bit-identical to
 * lzq_sweep_grid (same operations, same lane order).  d_work: >= lzq_sweep_grid_reuse_workspace
 * doubles (tables x (max(n_y, LZQ_NY_MIN) + LZQ_REUSE_TABLE_HEADER)); a negative return is an
 * error code.  A table's header records the y grid, c and the z grid (nz, z_max) it was made
 * for: a point integrated from a table of another setup or z grid gets NaN yields. */
#define LZQ_REUSE_TABLE_HEADER 6
int64_t lzq_sweep_grid_reuse_workspace(const lzq_axis* axes, int32_t n_axes, int32_t n_y);
/* The same for n explicit points: d_rep[n_tables] (int64) names one point per table, whose
 * I_p, beta_over_H, T_p_GeV, T_min_over_Tp, T_max_over_Tp the table is made for;
 * d_table_index[n] (int32) gives each point's table.  main()'s window only (no T_lo/T_hi
 * overrides).  d_work >= n_tables * (max(n_y, LZQ_NY_MIN) + LZQ_REUSE_TABLE_HEADER) doubles.  A point
 * whose y-grid or c differs from its table's gets NaN yields.  Bit-identical to lzq_yields_batch. */
int lzq_yields_batch_reuse(const lzq_point* d_points, int64_t n, int32_t n_y, int32_t nz, double z_max,
                           const double* d_P, const int64_t* d_rep, const int32_t* d_table_index, int64_t n_tables,
                           double* d_work, int64_t work_doubles, lzq_yield* d_out, void* stream);
int lzq_sweep_grid_reuse(const lzq_point* base, const lzq_axis* axes, int32_t n_axes, int64_t start, int64_t count,
                         int32_t n_y, int32_t nz, double z_max, const double* d_P, double* d_work,
                         int64_t work_doubles, lzq_yield* d_out, void* stream);

/* lzq_sweep_grid_reuse in two halves, so a sweep evaluated in chunks (or shards) builds its
 * z-sum tables once: lzq_sweep_grid_ztables writes every table of the grid into d_work (the
 * whole grid's, independent of any range); lzq_sweep_grid_from_ztables integrates points
 * [start, start+count) from tables built by it for the same base, axes and n_y (and exponential
 * variant).  Together they are lzq_sweep_grid_reuse, bit for bit. */
int lzq_sweep_grid_ztables(const lzq_point* base, const lzq_axis* axes, int32_t n_axes, int32_t n_y, int32_t nz,
                           double z_max, double* d_work, int64_t work_doubles, void* stream);
int lzq_sweep_grid_from_ztables(const lzq_point* base, const lzq_axis* axes, int32_t n_axes, int64_t start,
                                int64_t count, int32_t n_y, int32_t nz, double z_max, const double* d_P,
                                const double* d_work, int64_t work_doubles, lzq_yield* d_out, void* stream);

/* fpy:183-184: P[i] = clamp(1 - exp(-2 pi max(lambda[i], 0)), 0, 1) (naive 1-exp kept). */
int lzq_p_closed_form(const double* d_lambda, int64_t n, double* d_P, void* stream);

/* ---- source activity window W(y) (fpy:262; PAPER §10 step 4) --------------------------- */
/* The reference's window is the Gaussian proxy exp(-(y/sigma_y)^2 / 2) of fpy:262, one per-y factor
 * of the integrand, independent of the z-sums.  The entry points below take the window of each
 * point from a block of its own instead (csrc/lzq_window.h holds the one definition that the host
 * and the device build).  In the first two kinds W = exp(-q q / 2), q formed by the IEEE
 * operations listed, one rounding each:
 *   LZQ_WIN_GAUSS    q = y r,  r = 1/max(sigma_hi, 1e-6): the operations of the headline kernels;
 *   LZQ_WIN_PLATEAU  u = y - y0,  d = max(|u| - half_width, 0),  sigma = sigma_lo if u < 0 else
 *                    sigma_hi,  q = d (1/max(sigma, 1e-6)): a shifted Gaussian, a two-sided one, a
 *                    flat top with Gaussian shoulders, in the limit a top-hat;
 *   LZQ_WIN_TABLE    v = (y - y0)/scale,  W = W_k + (v - u_k)((W_{k+1} - W_k)/(u_{k+1} - u_k)) on the
 *                    knot interval u_k <= v < u_{k+1} (found by binary search), W_0 for v < u_0 and
 *                    W_last for v >= u_last; no exponential is taken.
 * A block is refused (LZQ_EINVAL and a message from the host-side checks; NaN yields from a kernel
 * that meets one in device memory) when any field is NaN, a sigma or the scale is <= 0 or not
 * finite, half_width < 0, the kind is unknown or, for LZQ_WIN_TABLE, the table index is outside
 * [0, n_tables).  Every field is checked whatever the kind (neutral values: y0 = 0, half_width = 0,
 * sigmas = scale = 1, table = 0).  48 bytes. */
enum lzq_window_kind { LZQ_WIN_GAUSS = 0, LZQ_WIN_PLATEAU = 1, LZQ_WIN_TABLE = 2 };
typedef struct lzq_window {
  int32_t kind;  /* enum lzq_window_kind */
  int32_t table; /* LZQ_WIN_TABLE: row of lzq_window_tables.W */
  double y0, half_width, sigma_lo, sigma_hi, scale;
} lzq_window;
/* Tabulated profiles shared by a batch: n_tables rows W[t][0..n_knots) over one ascending knot
 * vector u[0..n_knots).  2 <= n_knots <= LZQ_WIN_MAX_KNOTS, 0 <= n_tables <= LZQ_WIN_MAX_TABLES
 * (0: no table kind in the batch; u and W may then be NULL).  Knots must be finite and strictly
 * ascending, every W_k finite and >= 0: lzq_window_check_host checks a host copy, which a caller
 * does before uploading one -- the launches read the device arrays unchecked.  24 bytes. */
#define LZQ_WIN_MAX_KNOTS 4096
#define LZQ_WIN_MAX_TABLES 1024
typedef struct lzq_window_tables {
  int32_t n_tables, n_knots;
  const double* u; /* [n_knots] */
  const double* W; /* [n_tables][n_knots] */
} lzq_window_tables;

/* Host-side check of n blocks (host array) and of tables whose u / W are HOST arrays (tables may
 * be NULL when no block is of the table kind): every refusal listed above.  No GPU. */
int lzq_window_check_host(const lzq_window* win, int64_t n, const lzq_window_tables* host_tables);
/* The host build of the window: for one block and n host values of y, q_or_v[i] = q (the v of a
 * table kind) and W[i] with libm's exp (the interpolated W of a table kind); either output may be
 * NULL.  host_tables as for lzq_window_check_host, whose checks run first.  No GPU. */
int lzq_window_eval_host(const lzq_window* win, const lzq_window_tables* host_tables, const double* y, int64_t n,
                         double* q_or_v, double* W);
/* The device build: d_W[i] = W(d_y[i]) for one host-side block; d_tables' u / W are device arrays
 * (NULL for the other kinds).  The exponential is the quadrature kernels' (<= 1 ulp). */
int lzq_window_batch(const lzq_window* win, const lzq_window_tables* d_tables, const double* d_y, int64_t n,
                     double* d_W, void* stream);
/* lzq_yields_batch (without an A/V block) with point i's window taken from d_win[i] (device
 * array) instead of its source_shape_sigma_y, which is then not read.  A LZQ_WIN_GAUSS block whose
 * sigma_hi is the point's source_shape_sigma_y gives lzq_yields_batch's bits. */
int lzq_yields_batch_window(const lzq_point* d_points, int64_t n, int32_t n_y, int32_t nz, double z_max,
                            const double* d_T_lo, const double* d_T_hi, const double* d_P, const lzq_window* d_win,
                            const lzq_window_tables* d_tables, lzq_yield* d_out, void* stream);
/* lzq_yields_batch_reuse likewise: the z-sum tables do not depend on the window, so points that
 * differ only in their windows share one.  Bit-identical to lzq_yields_batch_window. */
int lzq_yields_batch_reuse_window(const lzq_point* d_points, int64_t n, int32_t n_y, int32_t nz, double z_max,
                                  const double* d_P, const int64_t* d_rep, const int32_t* d_table_index,
                                  int64_t n_tables, double* d_work, int64_t work_doubles, const lzq_window* d_win,
                                  const lzq_window_tables* d_tables, lzq_yield* d_out, void* stream);
/* Cartesian sweeps whose points carry a window: lzq_sweep_grid and the shared-z-sum entry points
 * with point i's window = *base_win (a host struct) with the values of the grid's window axes
 * (LZQ_F_WIN_*) written into it, decoded from the flat index inside the kernel like the point's
 * own fields (csrc/lzq_window.h window_grid_block: the one definition host and device build); the
 * point's source_shape_sigma_y is not read.  LZQ_F_WIN_SIGMA writes sigma_lo and sigma_hi;
 * LZQ_F_WIN_TABLE takes a double that must hold an integer (tested as a double before it is
 * converted; anything else gives table = -1, which a table-kind block is refused for).  Two axes
 * that write the same block field (a duplicate, or LZQ_F_WIN_SIGMA next to _SIGMA_LO / _SIGMA_HI)
 * are LZQ_EINVAL; every other argument check is lzq_sweep_grid's.  Axis values live in device
 * memory and are not checked at launch: a point whose decoded block is one of the refusals above
 * gets NaN yields and reads no table (check host copies first with lzq_window_grid_check_host).
 * With no window axis and a LZQ_WIN_GAUSS base block whose sigma_hi is the point's
 * source_shape_sigma_y the yields are lzq_sweep_grid's bits; for any axes they are those of
 * lzq_yields_batch_window on the decoded points and blocks.
 * The z-sum tables do not depend on the window: window axes contribute no table
 * (lzq_sweep_grid_reuse_workspace counts none for them), and lzq_sweep_grid_ztables_window is
 * lzq_sweep_grid_ztables accepting (and skipping) the window fields, so that a table's index is
 * formed from the strides of the whole axis list, as lzq_sweep_grid_from_ztables_window forms it. */
int lzq_sweep_grid_window(const lzq_point* base, const lzq_window* base_win, const lzq_axis* axes, int32_t n_axes,
                          int64_t start, int64_t count, int32_t n_y, int32_t nz, double z_max, const double* d_P,
                          const lzq_window_tables* d_tables, lzq_yield* d_out, void* stream);
int lzq_sweep_grid_reuse_window(const lzq_point* base, const lzq_window* base_win, const lzq_axis* axes,
                                int32_t n_axes, int64_t start, int64_t count, int32_t n_y, int32_t nz, double z_max,
                                const double* d_P, double* d_work, int64_t work_doubles,
                                const lzq_window_tables* d_tables, lzq_yield* d_out, void* stream);
int lzq_sweep_grid_ztables_window(const lzq_point* base, const lzq_axis* axes, int32_t n_axes, int32_t n_y,
                                  int32_t nz, double z_max, double* d_work, int64_t work_doubles, void* stream);
int lzq_sweep_grid_from_ztables_window(const lzq_point* base, const lzq_window* base_win, const lzq_axis* axes,
                                       int32_t n_axes, int64_t start, int64_t count, int32_t n_y, int32_t nz,
                                       double z_max, const double* d_P, const double* d_work, int64_t work_doubles,
                                       const lzq_window_tables* d_tables, lzq_yield* d_out, void* stream);
/* The host build of that decode: out_blocks[i] = the block of flat grid index start + i, i < count
 * (64-bit throughout).  axes[a].values are HOST arrays here and are read only for the window
 * axes (the others need their n alone).  No GPU. */
int lzq_window_grid_blocks_host(const lzq_window* base_win, const lzq_axis* axes, int32_t n_axes, int64_t start,
                                int64_t count, lzq_window* out_blocks);
/* Host-side check of a window grid (HOST axis values): lzq_window_check_host on *base_win and the
 * tables, then every value of every window axis substituted into *base_win on its own -- a block's
 * refusals are per field, so this covers every block of the grid without a pass over it.  The
 * message names the axis (its position in axes) and the value. */
int lzq_window_grid_check_host(const lzq_window* base_win, const lzq_axis* axes, int32_t n_axes,
                               const lzq_window_tables* host_tables);
/* ---- one parameter per grid point solved for a target yield (PAPER eqs.(22)-(24), §10) ---- */
/* The inverse of a sweep: for every point of a grid, the value x of ONE parameter in [lo, hi] at
 * which a yield field takes a target value (e.g. the P_eff at which DM_over_B = 5.357, PAPER
 * eq.(24)), found on the device by a bracketing root solve of f(x) = field(x) - target (one IEEE
 * subtraction).  csrc/lzq_solve.h holds the stepping rule, one definition that the host and the
 * device build: f(lo), then f(hi); then regula-falsi points (a fb - b fa)/(fb - fa) with the
 * Anderson-Bjorck scaling of a twice-retained end's f, replaced by the midpoint a + (b - a)/2 when
 * they do not fall strictly inside the bracket or when the width would otherwise not have halved
 * over three evaluations.  Guarantees: the bracket [x_lo, x_hi]
 * keeps a strict sign change of f; its width at least halves every three evaluations; evals <=
 * max_evals (clamped to [2, 256] on the host and again in the kernel); the result is a pure function
 * of (point, block, solve), independent of the range, chunk or shard it is computed in.  The solve
 * stops when x_hi - x_lo <= xtol max(|x_lo|, |x_hi|), when no double lies strictly between the
 * ends, at an exact zero of f (then x_lo = x = x_hi), or after max_evals evaluations
 * (LZQ_SOLVE_MAX_EVALS: the bracket is still valid and returned).  x is the end with the smaller
 * |f| (ties: the lower one), residual = f(x) as evaluated there.
 *
 * Allowed solve fields are those that contribute no z-sum table, so that every evaluation is one
 * point integrated from the grid's shared tables: m_chi, g_chi, v_w, g_star, g_star_s, P, sigma_y,
 * flux, Y_chi_init, n_chi_at_Tp; the LZ fields delta_LZ, m_mix, dprime (the other one of m_mix /
 * dprime must then be an axis; a solve for v_w on a grid with m_mix / dprime axes re-forms their P
 * with v_w = x, PAPER eq.(8), as the forward sweep does with v_w as an axis); with a block,
 * LZQ_F_WIN_Y0, _HALF_WIDTH, _SIGMA_LO, _SIGMA_HI, _SIGMA, _SCALE.  LZQ_EINVAL with a message
 * (lzq_solve_check_host: the same checks without a GPU) for: a table field (I_p, beta_over_H, T_p, T_min / T_max_over_Tp); LZQ_F_WIN_TABLE; a window field
 * without a block; sigma_y with a block (the block replaces it); a field that an axis also writes
 * (for window fields: whose masks meet, as for two axes; P counts as written by every LZ axis, delta_LZ by m_mix / dprime axes); lo >= hi or
 * non-finite bounds or target; xtol outside [0, 1); target_field outside [0, 5]; d_P together with a
 * solve for P or an LZ field.
 *
 * d_work: the tables of lzq_sweep_grid_ztables (base_win NULL) or lzq_sweep_grid_ztables_window for
 * the same base, axes and n_y; the solve builds none.  (For a solve of m_mix or dprime the axis list
 * holds the other one alone, which the table entry points refuse: build the tables from the list
 * without its LZ axes -- they contribute no table, so the workspace is the same.)
 * d_out[i]: the yield record at x, the
 * evaluation's own -- bit for bit what lzq_sweep_grid_from_ztables[_window] returns for that grid
 * point with the solve field set to x.  d_sol[i]: six doubles, so a table of results travels like a
 * table of records.  For LZQ_SOLVE_NO_BRACKET (f(lo) and f(hi) of one strict sign), LZQ_SOLVE_NAN (a
 * non-finite f, at an end or inside; also a point whose decoded window block is a refusal, which
 * reads no window table) and LZQ_SOLVE_BAD_TABLE (the table's header does not match the point's
 * y-grid, c or z grid; tested once, at lo) all six yields, x and residual are NaN and x_lo, x_hi
 * are the given bounds. */
enum lzq_solve_status { LZQ_SOLVE_OK = 0, LZQ_SOLVE_MAX_EVALS = 1, LZQ_SOLVE_NO_BRACKET = 2,
                        LZQ_SOLVE_NAN = 3, LZQ_SOLVE_BAD_TABLE = 4 };
typedef struct lzq_solve {          /* host struct, 48 bytes */
  int32_t field;        /* enum lzq_field: the parameter solved for */
  int32_t target_field; /* 0..5: index into lzq_yield */
  double lo, hi, target, xtol;
  int32_t max_evals;    /* clamped to [2, 256] */
} lzq_solve;
typedef struct lzq_solve_result {   /* 48 bytes */
  double x, x_lo, x_hi, residual, evals, status;
} lzq_solve_result;
int lzq_sweep_grid_solve(const lzq_point* base, const lzq_window* base_win /* NULL: the point's Gaussian */,
                         const lzq_axis* axes, int32_t n_axes, const lzq_solve* solve, int64_t start, int64_t count,
                         int32_t n_y, int32_t nz, double z_max, const double* d_P, const double* d_work,
                         int64_t work_doubles, const lzq_window_tables* d_tables,
                         lzq_yield* d_out, lzq_solve_result* d_sol, void* stream);
/* The solve's host-side refusals (all of the above but d_P's).  Axis values are not read.  No GPU. */
int lzq_solve_check_host(const lzq_solve* solve, const lzq_window* base_win, const lzq_axis* axes, int32_t n_axes);

/* ---- A/V in the continuum limit of the z grid --------------------------- */
/* Every yield above inherits the reference's z grid -- linspace(0, z_max, nz), trapezoid weights, the
 * cancelling gamma4 of fpy:156 -- in which Y_B is not converged, and no finer linspace
 * grid reaches the limit (see lzq_init).  The entry points below replace the z-sum alone by a
 * converged z-integral on a fixed node rule of their own (csrc/lzq_cont.h holds the one definition
 * that the host and the device build):
 *
 *   A/V_cont(y) = 0 for y > 50, else pref0 e^yh F_cont(c),  yh = clip(y, +-50), c = -(I_p/6) e^yh
 *   F_cont(c)   = sum_k omega_k exp(c gamma4_k)   over the rule's nodes, ascending in z
 *   omega_k     = z_k^2 e^{-z_k} w_k,  gamma4_k = gamma(4, z_k) without the cancellation of fpy:156
 *
 * pref0, the clip, the y > 50 zero and everything outside the z-integral stay the reference's
 * (fpy:158-165, 231-267).  The rule: 20-point Gauss-Legendre on panels geometric in z (edges
 * z_max 2^-j down to the first at or below 1e-6, plus the panel from 0); z_max = 30 gives 520 nodes and
 * a rule error of 1.7e-16 relative, below the inner loop's exponential.  z_max stays a parameter; there
 * is no nz.  z_max not finite or <= 0 is LZQ_EINVAL (as is one so small that the first node's weight
 * leaves the inner loop's range, z_max below ~1e-49).  An opt-in mode: no default changes.
 *
 * The yields always go through shared z-sum tables (lzq_sweep_grid_reuse's format).  A continuum
 * table's header carries a z grid no linspace grid can have (nz slot -1, z_max slot z_max), so a
 * linspace entry point given a continuum table, or the reverse, returns NaN yields.  The tables come
 * from the live-range kernel (LZQ_TUNE_CONT_SKIP); the integration, window and solve kernels are the
 * linspace grids'.  Each entry point is its namesake without the _cont suffix less the nz argument;
 * base_win / d_win / d_tables are optional (NULL: the point's Gaussian), and with a window the axes
 * may carry the window fields (the table half skips them). */
/* Host copies of the rule's tables for z_max: *n nodes (set whenever non-NULL), ascending in
 * (0, z_max); z, gamma4, omega may be NULL (call once for *n, then with arrays of *n doubles).  No GPU. */
int lzq_cont_tables(double z_max, double* z, double* gamma4, double* omega, int32_t* n);
/* The host build of the definition: out[i] = A/V_cont(y[i]) for the kernel of aov (else of *pt, as
 * lzq_aov_batch), a plain left-to-right FP64 sum with libm's exp.  No GPU. */
int lzq_aov_cont_host(const lzq_point* pt, const lzq_aov_params* aov, const double* y, int64_t n, double z_max,
                      double* out);
int lzq_aov_batch_cont(const lzq_point* pt, const lzq_aov_params* aov, const double* d_y, int64_t n, double z_max,
                       double* d_out, void* stream);
int lzq_sweep_grid_ztables_cont(const lzq_point* base, const lzq_axis* axes, int32_t n_axes, int32_t n_y, double z_max,
                                double* d_work, int64_t work_doubles, void* stream);
int lzq_sweep_grid_from_ztables_cont(const lzq_point* base, const lzq_window* base_win, const lzq_axis* axes,
                                     int32_t n_axes, int64_t start, int64_t count, int32_t n_y, double z_max,
                                     const double* d_P, const double* d_work, int64_t work_doubles,
                                     const lzq_window_tables* d_tables, lzq_yield* d_out, void* stream);
/* both halves in one call (an empty range validates only) */
int lzq_sweep_grid_cont(const lzq_point* base, const lzq_window* base_win, const lzq_axis* axes, int32_t n_axes,
                        int64_t start, int64_t count, int32_t n_y, double z_max, const double* d_P, double* d_work,
                        int64_t work_doubles, const lzq_window_tables* d_tables, lzq_yield* d_out, void* stream);
/* explicit points, as lzq_yields_batch_reuse[_window] */
int lzq_yields_batch_cont(const lzq_point* d_points, int64_t n, int32_t n_y, double z_max, const double* d_P,
                          const int64_t* d_rep, const int32_t* d_table_index, int64_t n_tables, double* d_work,
                          int64_t work_doubles, const lzq_window* d_win, const lzq_window_tables* d_tables,
                          lzq_yield* d_out, void* stream);
int lzq_sweep_grid_solve_cont(const lzq_point* base, const lzq_window* base_win, const lzq_axis* axes, int32_t n_axes,
                              const lzq_solve* solve, int64_t start, int64_t count, int32_t n_y, double z_max,
                              const double* d_P, const double* d_work, int64_t work_doubles,
                              const lzq_window_tables* d_tables, lzq_yield* d_out, lzq_solve_result* d_sol,
                              void* stream);

/* ---- momentum-averaged LZ probability P-bar(T) from F(k) (PAPER §10 step 1) ---- */
/* Everywhere above P_chi_to_B is one number per point that multiplies the quadrature from outside:
 * PAPER eq. (8) with the placeholder F(k) = 1.  With a momentum kernel F the conversion probability
 * depends on the particle's speed v = k/E in the plasma frame, and its average over the thermal flux
 * on m/T, so it belongs inside the y-integral, Y_B = int g(y) P-bar(y) dy (csrc/lzq_fk.h holds the one
 * definition that the host and the device build):
 *
 *   mu = m_chi/T(y), T(y) as the quadrature forms it;  t = (E - m)/T,  v = sqrt(t (t + 2 mu))/(t + mu)
 *   omega(t)  = t (t + 2 mu) e^-t / (1 +- e^-mu e^-t)        + LZQ_FERMION, - LZQ_BOSON
 *   P-bar(mu) = int omega(t) [-expm1(-2 pi delta_0 F(v))] dt / int omega(t) dt
 *   F(v)      = (v_ref / v)^p                                 LZQ_FK_POWER; p = 0 is F = 1
 *
 * delta_0 >= 0 is eq. (8) at F = 1, one per point.  J(T), its relativistic / non-relativistic branch
 * included, stays the reference's: only the constant P is replaced by the normalised average, so
 * p = 0 gives P = 1 - e^(-2 pi delta_0) back up to rounding.  The t-integrals run on one fixed node
 * table (350 nodes, rule error 3.6e-14 relative; numerator and denominator in node order with the same
 * weights: delta_0 = +inf gives exactly 1 and delta_0 = 0 exactly +0).
 * A block is refused (LZQ_EINVAL and a message from the host-side checks; NaN from a kernel that meets
 * one in device memory) when its kind is unknown, p is NaN, < 0 or > LZQ_FK_P_MAX, or v_ref is NaN,
 * <= 0 or > 1; a point when its delta_0 is NaN or < 0.  24 bytes. */
enum lzq_fk_kind { LZQ_FK_POWER = 0 };
#define LZQ_FK_P_MAX 8.0
typedef struct lzq_fk {
  int32_t kind; /* enum lzq_fk_kind */
  int32_t pad;
  double p, v_ref;
} lzq_fk;
/* Host-side check of n blocks and (delta0 non-NULL) n values of delta_0: every refusal above, the
 * message naming the field.  No GPU. */
int lzq_fk_check_host(const lzq_fk* fk, const double* delta0, int64_t n);
/* The host build of the definition: out[i] = P-bar(mu[i]) at delta0[i] for one block and statistics
 * (libm's exp, log, expm1).  mu NaN or < 0 is LZQ_EINVAL.  No GPU. */
int lzq_fk_pbar_host(const lzq_fk* fk, int32_t stats, const double* mu, const double* delta0, int64_t n, double* out);
/* Its device twin (device arrays; the device library's exp, log, expm1, <= 1 ulp each).  The block
 * is checked on the host; a mu or delta_0 in device memory that is NaN or < 0 gives NaN. */
int lzq_fk_pbar_batch(const lzq_fk* fk, int32_t stats, const double* d_mu, const double* d_delta0, int64_t n,
                      double* d_out, void* stream);
/* The host copy of the node table: *n nodes (set whenever non-NULL); t, w_exp = W e^-t, e = e^-t may
 * be NULL (call once for *n).  No GPU. */
int lzq_fk_nodes(double* t, double* w_exp, double* e, int32_t* n);
/* R tables.  Points that agree in T_p_GeV, beta_over_H, T_min_over_Tp, T_max_over_Tp (the y-grid and
 * T(y)), m_chi_GeV, stats, delta_0 and their block form a class and share one table of
 * R_j = P-bar(m/T(y_j)), j < n = max(n_y, LZQ_NY_MIN): table c is made for point d_rep[c] (int64) with
 * d_delta0[d_rep[c]] and d_fk[d_rep[c]], one wavefront per 64 y-nodes.  Layout: LZQ_FK_TABLE_HEADER
 * key doubles, the n values R_j, then P-bar(m/T_p), the P_used of the class's records;
 * d_R >= n_classes * lzq_fk_table_stride(n_y) doubles.  A class whose block or delta_0 is refused has
 * NaN throughout.  d_mu (optional, same layout less the header: n_classes * (n + 1) doubles) receives
 * the mu_j the kernel formed. */
#define LZQ_FK_TABLE_HEADER 6
int64_t lzq_fk_table_stride(int32_t n_y);
int lzq_fk_tables(const lzq_point* d_points, const double* d_delta0, const lzq_fk* d_fk, const int64_t* d_rep,
                  int64_t n_classes, int32_t n_y, double* d_R, int64_t r_doubles, double* d_mu, void* stream);
/* Y_B = int g(y) P-bar(y) dy from shared tables: point i is integrated from its z-sum table
 * d_table_index[i] of d_work (tables built for the same n_y and z grid by lzq_yields_batch_reuse,
 * lzq_sweep_grid_ztables or their _cont forms; nz = LZQ_FK_NZ_CONT: the continuum rule of z_max) and
 * from R table d_class[i] of d_R, both int32.  The per-y work is lzq_yields_batch_reuse's with P = 1
 * and the window factor W(y_j) R_j; W is point i's block d_win[i] (d_tables as for
 * lzq_yields_batch_window), or with d_win = NULL the point's Gaussian.  P_chi_to_B is not read;
 * P_used is P-bar(m/T_p).  A point whose own y-grid, c, z grid, m, stats, delta_0 or block differ from
 * its tables' headers gets NaN yields; a refused block or delta_0 gives NaN Y_B, rho_B, DM_over_B and
 * P_used and reads no table. */
#define LZQ_FK_NZ_CONT (-1)
int lzq_yields_batch_reuse_fk(const lzq_point* d_points, int64_t n, int32_t n_y, int32_t nz, double z_max,
                              const double* d_delta0, const lzq_fk* d_fk, const int32_t* d_table_index,
                              const double* d_work, int64_t work_doubles, const int32_t* d_class, const double* d_R,
                              int64_t r_doubles, const lzq_window* d_win, const lzq_window_tables* d_tables,
                              lzq_yield* d_out, void* stream);

/* The ODE entry points below take no window: their source term keeps the reference's Gaussian
 * (fpy:226-228).  Engine.ode and the facade's ODE operators raise when given another one.  Nor do they
 * take the continuum rule: lzq_ode_tables stays on the linspace grids. */

/* ---- ODE fallback (fpy:200-219, 270-286, 385-417) -------------------------------------- */
/* Configurations with sigma_v != 0, Gamma_wash != 0 or depletion leave the fast path
 * (fpy:372) for the reference's Boltzmann ODE.  These three Config fields ride next to the
 * lzq_point of each point. */
typedef struct lzq_ode_params {
  double sigma_v_chi_GeV_m2;       /* fpy:279 (max(., 0) applied) */
  double Gamma_wash_over_H;        /* fpy:284 (max(., 0) applied) */
  int32_t deplete_DM_from_source;  /* fpy:282 */
  int32_t reserved;                /* 0 */
} lzq_ode_params;                  /* 24 bytes */

/* ---- wash-out and source depletion on the y-grid quadrature (PAPER §10 step 5) ---- */
/* With sigma_v = 0 the system of fpy:270-286 is linear: Y_B has the integrating factor
 * (x/x_1)^Gamma = (T_lo/T)^Gamma and the depletion term is the unwashed source, so on the fast path's
 * own y-grid, with g its integrand (fpy:264-265) and w its trapezoid weights,
 *
 *   Y_B   = sum_j w_j g_j omega(T_j),     omega(T) = exp(-Gamma log(T / T_lo))
 *   Y_chi = Y_chi0 - [deplete] sum_j w_j g_j          (one IEEE subtraction; nothing is clamped)
 *
 * Gamma = max(Gamma_wash_over_H, 0) (fpy:284), deplete = (deplete_DM_from_source != 0), T_lo =
 * max(T_min_over_Tp T_p, 1e-30) (fpy:369, 389), Y_chi0 the fast path's Y_chi (fpy:376-384 = 389-399);
 * the epilogue (fpy:413-417) then runs on (Y_B, Y_chi).  csrc/lzq_wash.h holds the one definition that
 * the host and the device build.  Gamma = 0 takes neither the logarithm nor the exponential: omega is
 * exactly 1, and with deplete = 0 every entry point below returns its namesake's bits.  The entry
 * points read the z-sum tables of the shared-table mode, linspace or continuum (nz = LZQ_WASH_NZ_CONT
 * names the continuum rule; the header is checked as the reuse kernels check it), and combine with a
 * window block (base_win / d_win NULL: the point's Gaussian).  An opt-in mode: no default changes, and
 * the ODE entry points below are untouched.
 * Refused: sigma_v_chi_GeV_m2 > 0 after its max(., 0) (LZQ_EUNSUPPORTED) or a NaN in sigma_v or
 * Gamma (LZQ_EINVAL), with a message naming the field, from the host-side checks; NaN yields from a
 * kernel that meets such a block in device memory.  A regime that is neither thermal nor nonthermal
 * starts thermal in the reference's ODE branch (fpy:399-400) but has no Y_chi on its fast path: here it
 * is the fast path's rule (LZQ_EUNSUPPORTED from the grid entry points, NaN yields from explicit
 * records), so such a point differs from what lzq_ode_* return for it.  Not built: sigma_v != 0, a momentum kernel F(k)
 * together with wash-out, the dense (unshared) form, fractional depletion. */
#define LZQ_WASH_NZ_CONT (-1)
int lzq_wash_check_host(const lzq_ode_params* ode, int64_t n);
/* The host build of omega: out[i] = omega(T(y[i])) with T(y) = T_p / sqrt(max(1 + 2y / max(beta_over_H,
 * 1e-30), 1e-12)) (fpy:252-254) and libm's log and exp.  lzq_wash_check_host runs first.  No GPU. */
int lzq_wash_factor_host(const lzq_point* pt, const lzq_ode_params* ode, const double* y, int64_t n, double* out);
/* The device build: T(y) by the quadrature kernels' operations, their exponential (<= 1 ulp). */
int lzq_wash_factor_batch(const lzq_point* pt, const lzq_ode_params* ode, const double* d_y, int64_t n, double* d_out,
                          void* stream);
/* lzq_yields_batch_reuse_window (d_win NULL: lzq_yields_batch_reuse) with point i's block d_ode[i]. */
int lzq_yields_batch_reuse_wash(const lzq_point* d_points, int64_t n, int32_t n_y, int32_t nz, double z_max,
                                const double* d_P, const int64_t* d_rep, const int32_t* d_table_index,
                                int64_t n_tables, double* d_work, int64_t work_doubles, const lzq_window* d_win,
                                const lzq_window_tables* d_tables, const lzq_ode_params* d_ode, lzq_yield* d_out,
                                void* stream);
/* lzq_sweep_grid_from_ztables[_window|_cont] with point i's block = *base_ode (a host struct) with the
 * values of the grid's wash axes (LZQ_F_GAMMA_WASH, LZQ_F_DEPLETE) written into it, decoded from the
 * flat index in the kernel beside the point and window fields.  Neither field contributes a z-sum
 * table: d_work is what lzq_sweep_grid_ztables[_window|_cont] builds for the axis list WITHOUT them
 * (the strides of the table fields do not depend on the axes between them).  Two axes writing one wash
 * field are LZQ_EINVAL.  The records are those of lzq_yields_batch_reuse_wash on the decoded points
 * and blocks, bit for bit. */
int lzq_sweep_grid_from_ztables_wash(const lzq_point* base, const lzq_window* base_win, const lzq_ode_params* base_ode,
                                     const lzq_axis* axes, int32_t n_axes, int64_t start, int64_t count, int32_t n_y,
                                     int32_t nz, double z_max, const double* d_P, const double* d_work,
                                     int64_t work_doubles, const lzq_window_tables* d_tables, lzq_yield* d_out,
                                     void* stream);
/* lzq_sweep_grid_solve: the same contract and stepping rule (csrc/lzq_solve.h), each evaluation one
 * point of lzq_sweep_grid_from_ztables_wash.  LZQ_F_GAMMA_WASH is an allowed solve field next to every
 * field allowed today (the DM_over_B = 5.357 question of PAPER §10 step 5).  New refusals
 * (lzq_solve_check_host_wash; base_ode NULL there: lzq_solve_check_host, unchanged): Gamma solved and
 * also an axis; lo < 0 for Gamma; LZQ_F_DEPLETE as the solve field; sigma_v != 0 or a NaN in the base block. */
int lzq_sweep_grid_solve_wash(const lzq_point* base, const lzq_window* base_win, const lzq_ode_params* base_ode,
                              const lzq_axis* axes, int32_t n_axes, const lzq_solve* solve, int64_t start,
                              int64_t count, int32_t n_y, int32_t nz, double z_max, const double* d_P,
                              const double* d_work, int64_t work_doubles, const lzq_window_tables* d_tables,
                              lzq_yield* d_out, lzq_solve_result* d_sol, void* stream);
int lzq_solve_check_host_wash(const lzq_solve* solve, const lzq_window* base_win, const lzq_ode_params* base_ode,
                              const lzq_axis* axes, int32_t n_axes);

#define LZQ_ODE_NT 800             /* fpy:207 build_tables(n=800), the n main() uses (fpy:387) */
#define LZQ_ODE_WS_PER_POINT 3200  /* workspace doubles per point (spline coefficients): 4 x LZQ_ODE_NT */
#define LZQ_ODE_NT_MAX (1 << 20)   /* largest build_tables n accepted */
enum lzq_ode_status {
  LZQ_ODE_OK = 0,
  LZQ_ODE_BAD_GRID = 1,       /* T grid not strictly increasing: CubicSpline raises ValueError */
  LZQ_ODE_BAD_STEP = 2,       /* max_step <= 0 (zero-width x range): solve_ivp raises ValueError */
  LZQ_ODE_TOO_MANY_STEPS = 3, /* more than max_steps integration steps: not attempted */
  LZQ_ODE_NOT_LINEAR = 5,     /* internal to lzq_ode_quadrature: Y_chi still to be stepped */
  LZQ_ODE_BAD_TABLE = 7,      /* the point's spline table was not built by lzq_ode_tables with
                                 nt = LZQ_ODE_NT (the integrators' knot count; NaN yields) */
  LZQ_ODE_UNRESOLVED = 6,     /* lzq_ode_quadrature: a knot interval needs more than 4096
                                 Gauss sub-intervals to resolve its scales (NaN yields) */
  LZQ_ODE_NEWTON = 4          /* a Radau stage system did not converge: the yields are the
                                 state at the start of the failed step (fpy:408-410 reports
                                 sol.y[:, -1] after a failed solve) */
};

/* BoltzmannSystem.build_tables(T_lo, T_hi, n=nt) (fpy:207-212) with self.aov = AoverVKernel(...,
 * z_max, nz) for n points, at per-point windows d_T_lo/d_T_hi ([n] each) or, both NULL, main()'s
 * window T_lo = T_min_over_Tp T_p, T_hi = T_max_over_Tp T_p (fpy:368-369, what lzq_ode_integrate
 * needs): A/V at linspace(T_lo, T_hi, nt) (the quadrature kernels' z-sum on the grid (nz, z_max))
 * and its not-a-knot cubic spline (scipy CubicSpline), into d_work[i * 4 nt ...] (work_doubles >=
 * n * 4 nt; 4 <= nt <= LZQ_ODE_NT_MAX).  The integrators (lzq_ode_integrate*, lzq_ode_quadrature)
 * read tables of nt = LZQ_ODE_NT knots, main()'s build_tables (fpy:387), on any z grid: a table
 * records its nt in its last 4 (spare) doubles, and a point whose table holds another nt gets
 * LZQ_ODE_BAD_TABLE (NaN yields) from them.
 * d_status (optional, [n] int32): LZQ_ODE_BAD_GRID for a window CubicSpline rejects.  d_aov:
 * optional [n] device lzq_aov_params, the A/V kernel of each point's table (bs.aov replaced:
 * y(T) from the point, A/V from the block, fpy:211); NULL = the point's own fields. */
int lzq_ode_tables(const lzq_point* d_points, int64_t n, const double* d_T_lo, const double* d_T_hi, int32_t nt,
                   int32_t nz, double z_max, const lzq_aov_params* d_aov, double* d_work, int64_t work_doubles,
                   int32_t* d_status, void* stream);

/* fpy:385-417 on built tables: Y_chi(x1), Y_B(x1) of rhs (fpy:270-286) from x0 = m/T_hi to
 * x1 = m/max(T_lo, 1e-30), Y(x0) = (Y_chi0 of fpy:389-399, 0), by the reference's method
 * (3-stage Radau IIA) on uniform steps h = (x1 - x0)/ceil(|x1 - x0|/max_step) <= max_step of
 * fpy:404, one point per lane; then the densities epilogue.  The steps run as continuation
 * launches of <= 2^24 steps (LZQ_TUNE_ODE_LAUNCH_STEPS), so max_steps only caps the work: points
 * needing more than max_steps steps are not integrated (status LZQ_ODE_TOO_MANY_STEPS, NaN
 * yields; max_steps <= 65536 x the launch size); so are
 * points whose T grid CubicSpline would reject (LZQ_ODE_BAD_GRID).  A Newton failure
 * (LZQ_ODE_NEWTON) stops the point and reports the state reached.  d_status: optional [n]
 * int32 output (enum lzq_ode_status). */
int lzq_ode_integrate(const lzq_point* d_points, const lzq_ode_params* d_ode, int64_t n, const double* d_work,
                      int64_t work_doubles, int64_t max_steps, lzq_yield* d_out, int32_t* d_status,
                      void* stream);

/* lzq_ode_integrate with tables shared between points: point i reads the spline table at
 * d_work[d_table_index[i] * LZQ_ODE_WS_PER_POINT] (0 <= d_table_index[i] < n_tables, the
 * caller's contract; work_doubles >= n_tables * LZQ_ODE_WS_PER_POINT).  A table depends only
 * on the A/V kernel and the window of fpy:141-156, 207-212 -- (I_p, beta_over_H, T_p_GeV, v_w,
 * g_star, T_min_over_Tp, T_max_over_Tp) -- so points equal in those fields (a sweep over P,
 * flux, sigma_v, Gamma_wash, m_chi, ...) share one lzq_ode_tables row; the results are
 * bit-identical to lzq_ode_integrate with per-point tables. */
int lzq_ode_integrate_shared(const lzq_point* d_points, const lzq_ode_params* d_ode, int64_t n,
                             const int32_t* d_table_index, int64_t n_tables, const double* d_work,
                             int64_t work_doubles, int64_t max_steps, lzq_yield* d_out, int32_t* d_status,
                             void* stream);

/* Shared step-row tables for linear sweeps (sigma_v = 0, no depletion; round 6; no reference
 * counterpart -- a re-use of fpy:270-286's per-step quantities across points).  A run is a set
 * of points equal in everything Y_B's Radau step map reads but P and the flux: the stage fields
 * of the A/V spline, m_chi, g_chi, g_star_s, source_shape_sigma_y, stats, the table and
 * Gamma_wash.  lzq_ode_rows writes run q's N_q step maps (c, d: Y_B' = c Y_B + P flux d, 16 B a
 * step) from its representative point d_run_rep[q] into d_rows (as doubles) from row
 * d_row_off[q] on, N_q = d_row_off[q + 1] - d_row_off[q] = the point's step count (ceil(|x1 -
 * x0| / max_step), fpy:403-404); max_run_rows >= every N_q; rows past rows_doubles / 2 are not
 * written.  lzq_ode_integrate_rows is lzq_ode_integrate_shared whose linear wavefronts read their
 * run's rows (d_run_of[i]: point i's run, -1 none) instead of forming their own -- only after
 * checking, per wavefront, that it is one run whose representative equals each point in all the
 * rows depend on, bit for bit, and whose row count is the point's step count (otherwise, and for
 * every other wavefront, lzq_ode_integrate_shared's path).  Results are bit-identical to
 * lzq_ode_integrate_shared. */
int lzq_ode_rows(const lzq_point* d_points, const lzq_ode_params* d_ode, int64_t n, const int32_t* d_table_index,
                 int64_t n_tables, const double* d_work, int64_t work_doubles, const int64_t* d_run_rep,
                 const int64_t* d_row_off, int64_t n_runs, int64_t max_run_rows, double* d_rows,
                 int64_t rows_doubles, void* stream);
int lzq_ode_integrate_rows(const lzq_point* d_points, const lzq_ode_params* d_ode, int64_t n,
                           const int32_t* d_table_index, int64_t n_tables, const double* d_work,
                           int64_t work_doubles, int64_t max_steps, const int32_t* d_run_of,
                           const int64_t* d_run_rep, const int64_t* d_row_off, int64_t n_runs,
                           const double* d_rows, int64_t rows_doubles, lzq_yield* d_out, int32_t* d_status,
                           void* stream);

/* lzq_ode_integrate / lzq_ode_integrate_shared (d_table_index NULL: table i for point i) for a
 * FEW points on long windows -- the CLI's single point -- integrated parallel in time: each
 * point's N fixed steps are cut into intervals of LZQ_TUNE_ODE_TP_INTERVAL steps, every interval
 * is integrated from a guess of its start state on its own lane (the same per-step operations),
 * and Newton's method on the interval boundaries (multiple shooting; the corrections by a scan of
 * the intervals' linearised maps) iterates the guesses to within a few ulps of the sequential
 * trajectory; then every interval is integrated from the candidate starts around its converged
 * node and the exact chains are followed through those tables from the exact initial state (no
 * integrator uses the predictor on the first step of a 64-step block, so an interval's end is a
 * function of its start values alone).  A point's latency drops from N serial steps to (a few
 * iterations + the candidate pass) x (one interval), and its result is lzq_ode_integrate's, BIT FOR
 * BIT (tests/test_gpu_ode_tp.py).  A point whose iteration does not converge to 1e-14 within 32
 * updates, whose exact chain leaves the candidate windows (+-256 ulps), or whose status is not OK,
 * takes the sequential integration (the same bits again, at the sequential cost); so does every
 * point of a batch of more than 64.  d_iters (optional, [n] int32): the Newton updates of a point
 * that was stitched; 0: not iterated, -k: iterated k updates, then integrated sequentially.
 * Blocks nothing: the iteration count is fixed (32 rounds of two launches; a converged point's
 * later launches return at once), so the call is stream-ordered like lzq_ode_integrate.
 * Scratch (stream-ordered, hipMallocAsync, freed by the call): with L = LZQ_TUNE_ODE_TP_INTERVAL
 * and M = min(ceil(max_steps / L), 65536) intervals per point, about n M (72 + 32 (2J + 1)) bytes
 * for the nodes, ends, scans and the two chains' candidate tables, J = 256 when those fit 1 GiB
 * (else 32), plus n M L 88 bytes of the regular steps' stage rows when they fit 2 GiB (else the
 * stages are formed inline).  max_steps only sizes it: pass the batch's longest step count
 * (Engine.ode does), not a generous cap -- e.g. n = 64 with max_steps = 2^22 asks ~4.7 GB. */
int lzq_ode_integrate_tp(const lzq_point* d_points, const lzq_ode_params* d_ode, int64_t n,
                         const int32_t* d_table_index, int64_t n_tables, const double* d_work, int64_t work_doubles,
                         int64_t max_steps, lzq_yield* d_out, int32_t* d_status, int32_t* d_iters, void* stream);

/* Quadrature form of the fallback (opt-in; not the reference's method).  Y_B's equation of
 * fpy:270-286 is linear with integrating factor (x/x1)^Gamma_wash for every sigma_v, so
 * Y_B(x1) = int alpha(x) (x/x1)^Gamma_wash dx, alpha = (SB/s)/(H x), exactly; with
 * sigma_v = 0 so is Y_chi's: Y_chi(x1) = Y_chi(x0) - [deplete] int alpha(x) dx.  Both are
 * integrated over the built spline tables (knot intervals split at T = m/3 and into
 * sub-intervals below the window / integrating-factor / Boltzmann scales, 8-point
 * Gauss-Legendre), one wavefront per point: the converged solution of the reference's
 * equations (the reference's own rtol-1e-8 Radau sits up to ~2e-8 from it on wide windows).
 * For sigma_v != 0 points Y_chi's Riccati equation is then stepped alone by the Radau
 * integrator (max_steps as lzq_ode_integrate; without a source term its stages need neither
 * the spline nor the window).  d_table_index: optional shared tables as in
 * lzq_ode_integrate_shared (NULL: table i for point i). */
int lzq_ode_quadrature(const lzq_point* d_points, const lzq_ode_params* d_ode, int64_t n,
                       const int32_t* d_table_index, int64_t n_tables, const double* d_work, int64_t work_doubles,
                       int64_t max_steps, lzq_yield* d_out, int32_t* d_status, void* stream);

/* lzq_ode_tables (nt = LZQ_ODE_NT, main()'s window, the z grid (nz, z_max), d_aov as there) +
 * lzq_ode_integrate (d_status may be NULL). */
int lzq_ode_batch(const lzq_point* d_points, const lzq_ode_params* d_ode, int64_t n, int32_t nz, double z_max,
                  const lzq_aov_params* d_aov, double* d_work, int64_t work_doubles, int64_t max_steps,
                  lzq_yield* d_out, int32_t* d_status, void* stream);

/* BoltzmannSystem.A_over_V_T (fpy:214-218) and .rhs (fpy:270-286) of ONE point (host structs)
 * whose nt-knot tables for the window (T_lo, T_hi) are at d_work_point (4 nt doubles, from
 * lzq_ode_tables): out_Av[i] = A_over_V_T(T[i]); out_dY[2i..2i+1] = rhs(x[i], (Y[2i], Y[2i+1])). */
int lzq_ode_aov_T(const lzq_point* pt, double T_lo, double T_hi, int32_t nt, const double* d_work_point,
                  const double* d_T, int64_t n, double* d_out_Av, void* stream);
int lzq_ode_rhs(const lzq_point* pt, const lzq_ode_params* ode, double T_lo, double T_hi, int32_t nt,
                const double* d_work_point, const double* d_x, const double* d_Y, int64_t n, double* d_out_dY,
                void* stream);

/* ---- Landau-Zener propagator (north_star (1); no reference counterpart) --------------- */
/* Coherent two-level propagation through n_cross sequential linear avoided crossings per
 * point: i dpsi/dt = H(t) psi, H = [[D(xi), m_c],[m_c, -D(xi)]], xi = v_w t, D piecewise linear
 * with slope (-1)^c |Delta'_c| through crossing c at xi_c (continuous at the turning points
 * between crossings).  The outer half-windows are window_lz LZ lengths of the first/last
 * crossing (L = sqrt(v_w/|Delta'|) max(1, sqrt(delta))).  Each cell with delta <= 16 takes
 * max(steps_per_crossing, 6 x the adiabatic phase in radians of its core) eighth-order Magnus
 * steps (exact SU(2) exponentials) on a core around its crossing (~5-7 LZ lengths: out to where
 * the first neglected angle of the order-10 superadiabatic frame falls to 1e-11) and follows the
 * state in that frame outside it, so the step count is bounded for any crossing spacing; cells
 * with delta > 16 are propagated in closed form.  Arrays are [n][n_cross] row-major device
 * buffers (xi increasing per point).  0 < window_lz <= 200, 0 < steps_per_crossing <= 1e6 (else
 * LZQ_EINVAL); a point whose inputs are not finite gets P = NaN.  Output d_P[n]: conversion
 * probability 1 - |<chi-like dressed state | psi_end>|^2, psi_start = chi-like dressed state,
 * where "dressed" = second-order superadiabatic state of the outer cell (the adiabatic state
 * carried in from / out to infinity).  For one crossing this is 1 - exp(-2 pi delta)
 * (fpy:183-184, PAPER eq.(9)) to <= 1e-8 relative at window_lz = 20 for any steps_per_crossing;
 * DESIGN.md §4.4 states the window / step tolerances (the C5 default is steps_per_crossing = 64).
 * Scratch from hipMallocAsync on `stream`, freed stream-ordered: 80 bytes per (point, crossing)
 * for the follow matrices (lz_follow_kernel; batches beyond 2^23 pairs run in slices) and, for
 * n >= 16384 points, 8n bytes for the longest-first launch order (points binned by their step
 * count, a counting sort in three small kernels); d_P is bit-identical to index order.
 * n < 2^31. */
int lzq_lz_propagate(const double* d_m_mix, const double* d_dprime, const double* d_xi,
                     int64_t n, int32_t n_cross, double v_w, double window_lz,
                     int32_t steps_per_crossing, double* d_P, void* stream);

/* lzq_lz_propagate with a per-point wall speed d_v_w[n] (sweeps over v_w with crossings); a
 * point whose v_w is not > 0 gets P = NaN. */
int lzq_lz_propagate_v(const double* d_m_mix, const double* d_dprime, const double* d_xi, const double* d_v_w,
                       int64_t n, int32_t n_cross, double window_lz, int32_t steps_per_crossing, double* d_P,
                       void* stream);

/* ---- bounce-profile LZ path (PAPER p.3 §3 eqs.(5)-(9); the absent modules of fpy:173) ---- */
/* The reference's hook (fpy:170-187) imports `transport_from_profile` and calls
 * compute_prob_from_profile(csv, v_w) / compute_lambda_eff_from_profile(csv) (fpy:178-184);
 * that module is absent from the reference, so these entry points implement the paper's
 * definition of it.  A profile SHAPE is the bounce's two background fields phi(xi), Phi(xi)
 * on n_knots knots xi_0 < ... < xi_{n_knots-1} (xi = r - R_0), each a not-a-knot cubic spline
 * (scipy CubicSpline, the interpolant fpy:212 uses).  Coefficient rows: d_coef[shape][j][8] =
 * (phi c0..c3, Phi c0..c3) with value c0 + c1 t + c2 t^2 + c3 t^3, t = xi - xi_j on
 * [xi_j, xi_{j+1}].  A POINT is a shape plus the couplings of eqs.(5)-(8):
 *   Delta = y_B phi - y_chi Phi (eq.5), Delta'* (eq.6), m_mix = lambda_tr_eff phi (eq.7),
 *   delta_LZ = m_mix(xi*)^2 / (2 v_w |Delta'*|) (eq.8, F = 1), P = 1 - exp(-2 pi delta) (eq.9). */
typedef struct lzq_profile_point {
  double y_B;            /* eq.(5) */
  double y_chi;          /* eq.(5) */
  double lambda_tr_eff;  /* eq.(7) */
  double v_w;            /* eq.(8); the propagation's xi = v_w t */
  int32_t shape;         /* 0 <= shape < n_shapes (else: NaN P / count -1) */
  int32_t reserved;      /* 0 */
} lzq_profile_point;     /* 40 bytes */

/* The not-a-knot splines of n_shapes shapes: d_knots/d_phi/d_Phi [n_shapes][n_knots] (device),
 * n_knots >= 4, into d_coef [n_shapes][n_knots-1][8].  d_bad[n_shapes] (int32): 1 for a shape
 * whose knots are not strictly increasing (CubicSpline raises ValueError; its rows are not
 * written), else 0. */
int lzq_profile_splines(const double* d_knots, const double* d_phi, const double* d_Phi, int32_t n_shapes,
                        int32_t n_knots, double* d_coef, int32_t* d_bad, void* stream);

/* eqs.(5)-(8) per point: every sign change of Delta in [xi_0, xi_{n_knots-1}) (a cubic per knot
 * interval, split at its stationary points; each root by safeguarded Newton to full precision).
 * Delta has one value per knot (an interior knot's: the next row's c0), so a sign flip across a
 * knot is one crossing, reported at the knot, and the count's parity matches Delta's signs at the
 * two ends; a zero exactly on an interior knot, or a whole zero interval, is one crossing (at the
 * first zero met) iff the signs around it differ; zeros on the first or last knot are none.
 * Up to max_cross crossings per point, in increasing xi, into d_xi / d_dprime (signed Delta'*) /
 * d_m_mix / d_delta_lz [n][max_cross]; d_count[n] = the number found (which may exceed
 * max_cross: the rest are not written; -1 for a bad shape index). */
int lzq_profile_crossings(const double* d_knots, const double* d_coef, int32_t n_shapes, int32_t n_knots,
                          const lzq_profile_point* d_points, int64_t n, int32_t max_cross, double* d_xi,
                          double* d_dprime, double* d_m_mix, double* d_delta_lz, int32_t* d_count, void* stream);

/* Time-ordered propagation through the whole profile (beyond the minimal estimator of eq.(8):
 * the crossings' energy dependence and their interference are kept): i dpsi/dt = H psi,
 * H = Delta(xi) sigma_z + m_mix(xi) sigma_x, xi = v_w t, from xi_0 to xi_{n_knots-1}.  psi starts
 * in the chi-like second-order dressed (superadiabatic) state of H at xi_0; d_P[n] =
 * 1 - |<chi-like dressed state at the far end | psi>|^2.  Sixth-order Magnus (three
 * Gauss-Legendre nodes, exact SU(2) exponentials), on knot interval j
 * max(min_steps, ceil(steps_per_radian x duration x max(E, 4 sqrt|dH/dt|))) uniform steps.
 * 0.5 <= steps_per_radian <= 1000 and 1 <= min_steps <= 1e6 (else LZQ_EINVAL); a point with
 * v_w <= 0, a bad shape index or more than 2^24 steps in one interval gets P = NaN.  For one
 * linear crossing in a wide window P -> eq.(9).  Accuracy: the error falls as
 * steps_per_radian^-6; at 3 it is within 9.2e-10 of the exact (Weber) solutions of
 * lzq_lz_propagate's piecewise-linear model and up to ~1e-8 on coarse smooth profiles, at 4 (the
 * package default) <= ~1e-9. 
 * n < 2^31. */
int lzq_lz_propagate_profile(const double* d_knots, const double* d_coef, int32_t n_shapes, int32_t n_knots,
                             const lzq_profile_point* d_points, int64_t n, double steps_per_radian,
                             int32_t min_steps, double* d_P, void* stream);

/* ---- sweep fits (no reference counterpart: a sweep's records reduced where they are) ------ */
/* A fit folds lzq_yield records into a small device-resident state, chunk by chunk, on the
 * caller's stream.  chi2 of a row: for each term in order d = (x - target) /
 * sigma (IEEE division), q = d * d; chi2 = q0, then chi2 + q1, ... left to right, each operation
 * rounded on its own (numpy's float64 expression gives the same bits).  A row is VALID iff its
 * chi2 is finite; every other row counts in n_invalid and takes part in nothing else but the
 * column statistics.  Everything kept is independent of the order rows arrive in (integer counts
 * and integer atomic minima only), so the state is the same bit for bit however the rows are
 * split into chunks, shards or ranks.
 *
 * The state is an array of 64-bit words:
 *   [0] n_valid   [1] n_invalid   [2..5] n_within[l]: valid rows with chi2 <= levels[l]
 *   [6] smallest chi2 (a double's bits; +inf with no valid row)   [7] the lowest flat grid index
 *       attaining it (int64; -1 with no valid row)
 *   [8..13] / [14..19] per lzq_yield column the min / max over its finite values, as the
 *       order-preserving key k(x) = bits(x) ^ (x < 0 ? ~0 : 1 << 63) (min ~0 / max 0: no finite value)
 *   [20..25] per column the count of non-finite values
 *   [26] rows selected so far by lzq_fit_select   [27..31] reserved (0)
 *   then per map, in order: chi2_min[cells] (doubles; +inf: empty cell), argmin[cells] (int64; -1).
 * A map projects onto one or two grid axes: the cell of flat index i is i_a = (i / stride[a]) %
 * len[a] (the C-order decode of lzq_sweep_grid: stride = the product of the later axes' lengths),
 * and (i_0, i_1) -> i_0 * len[1] + i_1 for two axes, in the order the map names them. */
#define LZQ_FIT_MAX_TERMS 4
#define LZQ_FIT_MAX_LEVELS 4
#define LZQ_FIT_MAX_MAPS 4
#define LZQ_FIT_MAX_CELLS (1 << 24) /* per map */
#define LZQ_FIT_HEADER_WORDS 32
#define LZQ_FIT_MAX_INDEX ((int64_t)1 << 62) /* start + count and every stride stay at or below this */
typedef struct lzq_fit_term {
  int32_t field;    /* 0..5: the doubles of lzq_yield in declaration order */
  int32_t reserved; /* 0 */
  double target;    /* finite */
  double sigma;     /* finite, > 0 */
} lzq_fit_term;     /* 24 bytes */
typedef struct lzq_fit_map {
  int32_t n_axes;    /* 1 or 2 */
  int32_t reserved;  /* 0 */
  int64_t stride[2]; /* 1 .. LZQ_FIT_MAX_INDEX */
  int64_t len[2];    /* >= 1; len[0] * len[1] <= LZQ_FIT_MAX_CELLS */
} lzq_fit_map;       /* 40 bytes */

/* Terms, levels and maps are host arrays.  LZQ_EINVAL (with a message) for more than
 * LZQ_FIT_MAX_TERMS / _LEVELS / _MAPS entries (or no term), an unknown field, sigma <= 0 or a
 * non-finite sigma or target, levels that are not ascending, and a map of more than
 * LZQ_FIT_MAX_CELLS cells. */
/* Bytes of the state for these maps (LZQ_FIT_HEADER_WORDS + 2 cells per map, 8 B each); negative:
 * an error code. */
int64_t lzq_fit_state_bytes(const lzq_fit_map* maps, int32_t n_maps);
/* The empty state (no row seen). */
int lzq_fit_reset(const lzq_fit_map* maps, int32_t n_maps, void* d_state, void* stream);
/* Fold records d_yields[count] of flat grid indices [start, start + count) into the state: two
 * streaming passes (minima, then the lowest index attaining each), maps of up to 4096 cells in all
 * block-private in LDS, larger ones straight to global memory; the result does not depend on the
 * path.  Asynchronous on `stream`; calls on one stream (or otherwise ordered) may come in any order
 * of start. */
int lzq_fit_update(const lzq_fit_term* terms, int32_t n_terms, const double* levels, int32_t n_levels,
                   const lzq_fit_map* maps, int32_t n_maps, const lzq_yield* d_yields, int64_t start, int64_t count,
                   void* d_state, void* stream);
/* Append the flat indices of the valid rows with chi2 <= level, ascending, to d_selected at the
 * state's running offset (word 26, which advances by the exact number selected); entries at or
 * beyond cap are dropped.  Count, scan, scatter on `stream` with no host synchronisation (scratch:
 * 8 B per 2048 rows, stream-ordered); chunks fed in ascending order of start on one stream leave
 * the list ascending. */
int lzq_fit_select(const lzq_fit_term* terms, int32_t n_terms, double level, const lzq_yield* d_yields, int64_t start,
                   int64_t count, void* d_state, int64_t* d_selected, int64_t cap, void* stream);
/* d_dst <- d_dst merged with d_src (two states of these maps over disjoint rows): counts add,
 * extrema by value, a cell takes the smaller chi2 and on a tie the lower index.  The cross-rank
 * combine of a sharded sweep. */
int lzq_fit_merge(const lzq_fit_map* maps, int32_t n_maps, void* d_dst, const void* d_src, void* stream);

/* ---- sweep posteriors: the likelihood-weighted half of a fit -------------- */
/* The weight of a row with chi2 c (the fit's expression; the row is valid iff c is finite), for an
 * offset (finite, >= 0) that is a parameter of the state: a = c - offset;
 *   a < 0: the row is "above": counted in n_above, it carries no weight (with offset = the sweep's
 *          best chi2 no valid row is above);
 *   else   w = exp(-a/2) in (0, 1], computed as 2^(a K), K = -log2(e)/2: u = a K, kd = rint(u),
 *          r = fma(a, K, -kd), w = ldexp(p(r), (int)kd) with p the degree-11 polynomial of 2^r
 *          (0.63 ulp), every operation rounded on its own; q = min(trunc(w 2^62), 2^62) is the
 *          weight in fixed point, units of 2^-62.  Rows with q = 0 (a >~ 124 ln 2 = 85.95) count in
 *          n_zero; a >= 2048 is q = 0 without the evaluation (exp(-a/2) is no double from 1490 on,
 *          and the reduction only holds while |u| < 2^52).
 * Only IEEE operations and an exact truncation are used: host and device give the same q.
 *
 * Every accumulator is a PAIR of unsigned 64-bit words (hi, lo) = (sum of q >> 31, sum of
 * q & 0x7fffffff), its value hi * 2^31 + lo in units of 2^-62.  All additions are integer, so the
 * state is the same bit for bit for every order, chunking, sharding and merge tree -- exactly, as
 * long as a state has been fed at most LZQ_POST_MAX_ROWS = 2^32 rows in all (merged states count
 * together): each word then stays below 2^32 * 2^31 = 2^63.  The library cannot see that total
 * across calls; the caller counts (the Python Engine does, and raises).
 *
 * The state is an array of 64-bit words, all 0 when empty:
 *   [0] n_used: valid rows with a >= 0 and q > 0   [1] n_zero   [2] n_above   [3] n_invalid
 *   [4,5] Z, the total weight   [6 + 2l, 7 + 2l] the weight of the rows with c <= levels[l], l < 4
 *   [14..31] reserved (0)
 *   [32 + 2b, 33 + 2b], b < LZQ_POST_BINS: the weight of the rows with min(2047, (int)(a * 16)) = b,
 *       a histogram of weight by a in bins of 1/16 (the last bin takes everything beyond 127.94);
 *       its sum is Z, and credible thresholds are read from it
 *   then per map, in order, `cells` pairs: the marginal weight of each cell (lzq_fit_map's decode). */
#define LZQ_POST_HEADER_WORDS 32
#define LZQ_POST_BINS 2048
#define LZQ_POST_MAX_ROWS ((int64_t)1 << 32) /* rows folded into one state, merges included */
/* q of n HOST rows into q_out: ~0 for an invalid row, ~0 - 1 for a row above, else the weight.  A
 * plain host function (no GPU work): the definition the kernels are compared with. */
int lzq_post_weights_host(const lzq_fit_term* terms, int32_t n_terms, double offset, const lzq_yield* rows, int64_t n,
                          uint64_t* q_out);
/* Bytes of the state for these maps ((LZQ_POST_HEADER_WORDS + 2 LZQ_POST_BINS + 2 cells per map)
 * words of 8 B); negative: an error code.  Arguments are validated as lzq_fit_* validates them,
 * with LZQ_EINVAL and a message before any GPU work; an offset that is negative or not finite is
 * LZQ_EINVAL too. */
int64_t lzq_post_state_bytes(const lzq_fit_map* maps, int32_t n_maps);
/* The empty state (all words 0), asynchronously on `stream`. */
int lzq_post_reset(const lzq_fit_map* maps, int32_t n_maps, void* d_state, void* stream);
/* Fold records d_yields[count] of flat grid indices [start, start + count) into the state: one
 * streaming pass; sums are taken inside a wave first, the histogram and maps of up to 1024 cells
 * in all are block-private in LDS, larger maps go straight to global memory; the result does not
 * depend on the path.  Every call on one state must pass the same offset.  Asynchronous on
 * `stream`, no host synchronisation; count <= LZQ_POST_MAX_ROWS. */
int lzq_post_update(const lzq_fit_term* terms, int32_t n_terms, const double* levels, int32_t n_levels,
                    const lzq_fit_map* maps, int32_t n_maps, double offset, const lzq_yield* d_yields, int64_t start,
                    int64_t count, void* d_state, void* stream);
/* d_dst <- d_dst + d_src, word by word (two states of these maps and one offset over disjoint
 * rows): the same result whatever the order of merges. */
int lzq_post_merge(const lzq_fit_map* maps, int32_t n_maps, void* d_dst, const void* d_src, void* stream);

/* ---- sweep observables: histograms of a fit over yield fields ------------- */
/* The fit and posterior states are indexed by the sweep's input axes; an OBSERVABLE is a histogram
 * over one or two lzq_yield fields, folded from the same records on the same stream.  Per cell it
 * keeps the number of valid rows, their smallest chi2 (a profile likelihood of the field) and, on
 * a weighted call, their posterior weight q (lzq_post_update's, for the call's offset).
 *
 * The bin of a finite value x on an axis -- integer and IEEE operations only, each rounded on its
 * own, so host and device agree:
 *   LZQ_OBS_LINEAR (lo < hi finite, bins >= 1, inv = bins / (hi - lo) in float64, which must be
 *     finite and > 0): below if x < lo, above if x >= hi, else min(bins - 1, (int64)((x - lo) * inv)).
 *   LZQ_OBS_LOG2 (0 < lo < hi finite, 2^log2_sub sub-bins per octave, log2_sub in 0..8):
 *     key(x) = bits(x) >> (52 - log2_sub) for x > 0 (sub-bins are linear inside an octave; no
 *     logarithm is taken); bins = key(hi) - key(lo) >= 1; the bin is key(x) - key(lo); below if
 *     x <= 0 or key(x) < key(lo), above if key(x) >= key(hi).  Edge e is the double with bits
 *     (key(lo) + e) << (52 - log2_sub): the effective range is [lo, hi) rounded down to sub-bin edges.
 * Every VALID row (finite chi2) falls into one class per observable: NONFINITE if one of the
 * observable's fields is NaN or +-inf; else OUT if one is below or above; else IN cell b0, or
 * b0 * bins1 + b1 for two axes.  Invalid rows touch nothing (the fit counts them).
 *
 * The state is an array of 64-bit words; per observable, in order:
 *   4 header words: n_in, n_out, n_nonfinite, reserved (0)
 *   2 * cells words: the weight of each cell as a pair (hi, lo) = (sum of q >> 31, sum of
 *       q & 0x7fffffff), exactly the posterior state's pairs; added only on a weighted call and only
 *       for rows that carry weight (1 <= q <= 2^62)
 *   cells words: the count of valid rows in the cell (weightless and "above" rows included)
 *   cells words: the smallest chi2 in the cell as a double's bits (+inf: empty), again over every
 *       valid row of the cell
 * There is no argmin: it would take the fit's second pass, and lzq_fit_select already lists the
 * points.  All sums are integer and the minimum is an integer minimum (chi2 >= 0 orders like its
 * bits), so the state is the same bit for bit for every order, chunking, sharding and merge tree,
 * up to LZQ_POST_MAX_ROWS rows a state, merges included (the caller counts, as for the posterior). */
#define LZQ_OBS_MAX 4
#define LZQ_OBS_MAX_CELLS (1 << 20) /* per observable */
#define LZQ_OBS_LDS_CELLS 1536      /* observables of up to this many cells IN ALL stay block-private in LDS */
#define LZQ_OBS_HEADER_WORDS 4
#define LZQ_OBS_LINEAR 0
#define LZQ_OBS_LOG2 1
typedef struct lzq_obs_axis {
  int32_t field;    /* 0..5: the doubles of lzq_yield in declaration order */
  int32_t kind;     /* LZQ_OBS_LINEAR or LZQ_OBS_LOG2 */
  double lo, hi;
  int32_t bins;     /* LZQ_OBS_LINEAR: the number of bins; LZQ_OBS_LOG2: ignored */
  int32_t log2_sub; /* LZQ_OBS_LOG2: 0..8; LZQ_OBS_LINEAR: ignored */
} lzq_obs_axis;     /* 32 bytes */
typedef struct lzq_obs {
  int32_t n_axes;   /* 1 or 2, over different fields */
  int32_t reserved; /* 0 */
  lzq_obs_axis axes[2];
} lzq_obs;          /* 72 bytes */

/* Observables are host arrays.  LZQ_EINVAL (with a message, before any GPU work) for more than
 * LZQ_OBS_MAX observables, an axis count other than 1 or 2, an unknown field or kind, two axes over
 * one field, a range or bin count outside the rules above, and more than LZQ_OBS_MAX_CELLS cells. */
/* Bytes of the state ((4 + 4 cells) words of 8 B per observable); negative: an error code. */
int64_t lzq_obs_state_bytes(const lzq_obs* obs, int32_t n_obs);
/* The empty state (zeros, +inf in the chi2 words), asynchronously on `stream`. */
int lzq_obs_reset(const lzq_obs* obs, int32_t n_obs, void* d_state, void* stream);
/* Fold records d_yields[count] into the state: one streaming pass.  weighted != 0 adds the rows'
 * weights for `offset` (finite, >= 0; the same for every weighted call on a state); weighted == 0
 * leaves the weight words alone and ignores offset.  Nothing depends on a row's flat index, so
 * there is no `start`.  The lanes of a wave that share a cell are combined before anything leaves
 * the wave; observables of up to LZQ_OBS_LDS_CELLS cells in all are block-private in LDS, larger
 * ones go straight to global memory; the result does not depend on the path.  Asynchronous on
 * `stream`, no host synchronisation; count <= LZQ_POST_MAX_ROWS. */
int lzq_obs_update(const lzq_fit_term* terms, int32_t n_terms, const lzq_obs* obs, int32_t n_obs, int32_t weighted,
                   double offset, const lzq_yield* d_yields, int64_t count, void* d_state, void* stream);
/* d_dst <- d_dst merged with d_src (two states of these observables over disjoint rows): words
 * add, the chi2 words take the minimum. */
int lzq_obs_merge(const lzq_obs* obs, int32_t n_obs, void* d_dst, const void* d_src, void* stream);
/* The class of n HOST rows in observable k into cell_out: the cell, -1 for OUT, -2 for NONFINITE
 * (validity is not looked at: there are no terms).  A plain host function (no GPU work): the
 * definition the kernel is compared with. */
int lzq_obs_cells_host(const lzq_obs* obs, int32_t n_obs, int32_t k, const lzq_yield* rows, int64_t n,
                       int32_t* cell_out);

/* ---- ranked points: the n rows of smallest chi2 with their records -------- */
/* The fit keeps one best point and lzq_fit_select lists indices within a level in index order; a
 * RANKED state keeps the n best rows themselves, in order.  The key of a row is (bits of its chi2
 * as an unsigned 64-bit word, its flat index): chi2 is the fit's expression, a row is valid iff it
 * is finite, and as a sum of squares it is never negative and never -0, so it orders like its bits.
 * Row a ranks before row b iff chi2(a) < chi2(b), or they are equal and index(a) < index(b).  Flat
 * indices are distinct, so this is a strict total order and "the n first rows" is one fixed list
 * however the rows are cut into chunks, shards or ranks and in whatever order states are merged.
 *
 * The state for capacity n (1 .. LZQ_RANK_MAX_N) is LZQ_RANK_HEADER_WORDS + 8 n 64-bit words:
 *   [0] n  [1] entries filled = min(n, valid rows seen)  [2] valid rows seen  [3] invalid rows seen
 *   [4..7] reserved, 0 ([4] counts a call's candidates while the call runs on its stream)
 *   then n entries of 8 words in rank order: chi2 bits, flat index (int64), the six doubles of the
 *   row's lzq_yield record as bits.  An unfilled entry is (+inf bits, -1, 0, 0, 0, 0, 0, 0).
 * Two states that saw the same set of rows are equal word for word.  Indices obey
 * LZQ_FIT_MAX_INDEX; nothing is summed, so there is no limit on the number of rows. */
#define LZQ_RANK_MAX_N 4096 /* a list's 16-byte keys fit one block's 64 KB of LDS */
#define LZQ_RANK_HEADER_WORDS 8
/* Bytes of the state, 8 * (8 + 8 n); negative: an error code (n out of range). */
int64_t lzq_rank_state_bytes(int32_t n);
/* The empty state, asynchronously on `stream`. */
int lzq_rank_reset(int32_t n, void* d_state, void* stream);
/* Fold records d_yields[count] of flat indices [start, start + count), none of which the state has
 * seen, into the state.  One streaming pass appends the keys of the rows that rank before the
 * list's last entry (every valid row while the list is not full) to scratch; one block then sorts
 * them with the list (a radix select over the 128-bit key first, when there are more than fit its
 * LDS) and rewrites the list.  A chunk without such a row -- a sweep's steady state -- writes two
 * counters.  Terms and errors as lzq_fit_update's, plus n outside 1 .. LZQ_RANK_MAX_N; count == 0
 * is a no-op.  Scratch (16 B a row of the chunk + 64 B an entry) is allocated and freed in stream
 * order inside the call.  Asynchronous on `stream`, no host synchronisation. */
int lzq_rank_update(const lzq_fit_term* terms, int32_t n_terms, int32_t n, const lzq_yield* d_yields, int64_t start,
                    int64_t count, void* d_state, void* stream);
/* d_dst <- the n first of d_dst and d_src, two states of capacity n over disjoint rows; words [2]
 * and [3] add. */
int lzq_rank_merge(int32_t n, void* d_dst, const void* d_src, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LZQ_H */
