// lzq_internal.h -- declarations shared between the library's translation units (not ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lzq.h"

namespace lzq {

constexpr int kOdeNT = LZQ_ODE_NT;           // fpy:207 build_tables(n=800)
constexpr int kOdeWS = LZQ_ODE_WS_PER_POINT;  // workspace doubles per point

// Per-point workspace layout (doubles): w[4k + 0..3] = PPoly c0..c3 of interval k < 799
// (value c0 s^3 + c1 s^2 + c2 s + c3, s = T - T_k); w[kOdeWS - 1] holds A/V at the last knot
// while the spline is built.

// A/V at the nt T-knots of every point (z grid (nz, z_max)) into w[4k + 3] / w[4 nt - 1] of its
// 4 nt doubles (lzq_kernels.hip: the quadrature kernels' z-sum, one wavefront per point).
// Host-side launch; sets lzq_last_error.
// d_aov (optional, [n]): the A/V kernel's own parameters per point (lzq_aov.hip).
int launch_ode_aov_tables(const lzq_point* d_points, int64_t n, const double* d_T_lo, const double* d_T_hi,
                          int32_t nt, int32_t nz, double z_max, const lzq_aov_params* d_aov, double* d_work,
                          hipStream_t stream);

// lzq_aov.hip: the quadrature / build_tables kernels with the A/V constants of a per-point
// lzq_aov_params block (fpy:141-151, 197, 211, 261), on a resolved z grid (zt, nzp; default_grid:
// the compile-time LZQ_NZ kernels) and exp table gtab.  Set lzq_last_error on failure.
struct ZNode;  // lzq_quad.h
int launch_yields_points_aov(int exp_variant, bool default_grid, const lzq_point* d_points,
                             const lzq_aov_params* d_aov, int64_t n, int32_t n_y, const double* d_T_lo,
                             const double* d_T_hi, const double* d_P, const ZNode* zt, int32_t nzp, const double* gtab,
                             lzq_yield* d_out, int truncate, hipStream_t s);
int launch_ode_aov_tables_aov(int exp_variant, const lzq_point* d_points, const lzq_aov_params* d_aov, int64_t n,
                              int32_t nt, const ZNode* zt, int32_t nzp, const double* gtab, const double* d_T_lo,
                              const double* d_T_hi, double* d_work, int truncate, hipStream_t s, int chunks = 1);

// lzq_window.hip: the quadrature kernels with the window of a per-point lzq_window block, dense and
// from z-sum tables written by points_ztable_kernel (key_nz, key_z_max: the z grid as a table's
// header stores it).  window_tables_arg: *d_tables (NULL: none) with its limits checked.
int window_tables_arg(const lzq_window_tables* d_tables, const char* who, lzq_window_tables& out);
int launch_yields_points_window(int exp_variant, bool default_grid, const lzq_point* d_points,
                                const lzq_window* d_win, const lzq_window_tables& wt, int64_t n, int32_t n_y,
                                const double* d_T_lo, const double* d_T_hi, const double* d_P, const ZNode* zt,
                                int32_t nzp, const double* gtab, lzq_yield* d_out, int truncate, hipStream_t s);
int launch_points_reuse_window(const lzq_point* d_points, const lzq_window* d_win, const lzq_window_tables& wt,
                               int64_t n, int32_t n_y, const double* d_P, double key_nz, double key_z_max,
                               const int32_t* d_table_index, const double* d_work, int64_t stride, lzq_yield* d_out,
                               hipStream_t s);

// The grid forms (lzq_sweep_grid_window, lzq_sweep_grid_from_ztables_window): point, block and table
// index decoded from the flat index in the kernel; grid: make_grid's GridSpec (lzq_kernels.hip), with
// tstride set for the reuse kernel.  window_axes_check: LZQ_EINVAL when two axes write the same
// field of the window block.
struct GridSpec;  // lzq_quad.h
int window_axes_check(const lzq_axis* axes, int32_t n_axes, const char* who);
int launch_yields_grid_window(int exp_variant, bool default_grid, const lzq_point& base, const lzq_window& base_win,
                              const GridSpec& grid, const lzq_window_tables& wt, int64_t start, int64_t count,
                              int32_t n_y, const double* d_P, const ZNode* zt, int32_t nzp, const double* gtab,
                              lzq_yield* d_out, int truncate, hipStream_t s);
int launch_grid_reuse_window(const lzq_point& base, const lzq_window& base_win, const GridSpec& grid,
                             const lzq_window_tables& wt, int64_t start, int64_t count, int32_t n_y, const double* d_P,
                             double key_nz, double key_z_max, const double* d_work, int64_t stride, lzq_yield* d_out,
                             hipStream_t s);

// lzq_solve.hip: lzq_sweep_grid_solve's kernel, one wavefront per grid point on the z-sum tables of
// lzq_sweep_grid_ztables[_window] (grid with tstride set); base_win NULL: the point's Gaussian.
int launch_grid_solve(const lzq_point& base, const lzq_window* base_win, const GridSpec& grid,
                      const lzq_window_tables& wt, const lzq_solve& solve, int64_t start, int64_t count, int32_t n_y,
                      const double* d_P, double key_nz, double key_z_max, const double* d_work, int64_t stride,
                      lzq_yield* d_out, lzq_solve_result* d_sol, hipStream_t s);

// lzq_cont.hip: the continuum z rule (lzq_cont.h).  Its node table goes through the z-sum table,
// integration, window and solve kernels of the linspace grids, so the *_cont entry points are the
// host wrappers below (lzq_kernels.hip) with cont = true: the z grid is then cont_grid_for's and nz
// is not read.  cont = false is the public entry point of the same name, unchanged.
constexpr double kContKeyNz = -1.0;  // a continuum table's header nz slot: no linspace grid has it
extern int g_cont_skip;              // lzq_tune(LZQ_TUNE_CONT_SKIP)
// the device image of z_max's table on device dev (built and uploaded once per (device, z_max))
int cont_grid_for(int dev, double z_max, const ZNode** zt, int32_t* nzp);
// the current device's exp table and the tuned variant, its tables initialised (lzq_kernels.hip)
int device_exp_table(int* dev, const double** gtab, int* exp_variant);
// The live-range z-sum table kernel: table t of the grid (pts NULL) or of point pts[reps[t]].
int launch_cont_ztables(int exp_variant, const lzq_point* base, const GridSpec* grid, const lzq_point* pts,
                        const int64_t* reps, int64_t n_tab, int32_t n_y, int64_t tstride, const ZNode* zt, int32_t nzp,
                        double key_z_max, const double* gtab, double* d_work, hipStream_t s);
int yields_batch_reuse(const lzq_point* d_points, int64_t n, int32_t n_y, int32_t nz, double z_max, const double* d_P,
                       const int64_t* d_rep, const int32_t* d_table_index, int64_t n_tables, double* d_work,
                       int64_t work_doubles, const lzq_window* d_win, const lzq_window_tables* wt, lzq_yield* d_out,
                       void* stream, bool cont, const char* fn);
int sweep_grid_reuse_parts(const lzq_point* base, const lzq_axis* axes, int32_t n_axes, int64_t start, int64_t count,
                           int32_t n_y, int32_t nz, double z_max, const double* d_P, double* d_work,
                           int64_t work_doubles, lzq_yield* d_out, void* stream, int parts, const char* fn,
                           bool window_axes, const lzq_window* base_win, const lzq_window_tables* d_tables, bool cont);
int sweep_grid_solve(const lzq_point* base, const lzq_window* base_win, const lzq_axis* axes, int32_t n_axes,
                     const lzq_solve* solve, int64_t start, int64_t count, int32_t n_y, int32_t nz, double z_max,
                     const double* d_P, const double* d_work, int64_t work_doubles, const lzq_window_tables* d_tables,
                     lzq_yield* d_out, lzq_solve_result* d_sol, void* stream, bool cont, const char* fn);

// Longest-first launch order (lzq_propagator.hip): cost bins per point (0 = costliest, kCostBins
// of them) and their histogram -> offs (kCostBins scratch) and order[n] (a counting sort: one
// scan, one scatter; stable across bins, atomics order within one).  Sets lzq_last_error.
constexpr int kCostBins = 128;  // 4 bins per octave of a point's step count
int launch_bin_order(const int32_t* bins, const int32_t* hist, int32_t* offs, int64_t n, int32_t* order,
                     hipStream_t st);

// lzq_tune(LZQ_TUNE_ODE_COOP) / (LZQ_TUNE_ODE_LAUNCH_STEPS) state, read by lzq_ode.hip's launches
extern int g_ode_coop;
extern int g_ode_launch_log2;
extern int g_ode_tp_interval;  // lzq_tune(LZQ_TUNE_ODE_TP_INTERVAL): steps per lzq_ode_integrate_tp interval
extern int g_ode_table_wide;   // lzq_tune(LZQ_TUNE_ODE_TABLE_WIDE): few ODE tables built a wavefront wide
// lzq_tune(LZQ_TUNE_PROFILE_FLAT) state, read by lzq_profile.hip's launch
extern int g_profile_flat;

}  // namespace lzq

// lzq_kernels.hip's error plumbing (thread-local message behind lzq_last_error)
int lzq_set_error(int code, const char* msg);
