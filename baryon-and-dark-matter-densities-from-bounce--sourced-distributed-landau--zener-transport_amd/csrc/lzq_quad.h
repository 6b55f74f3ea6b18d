// lzq_quad.h -- device side of the dense Y_B quadrature (fpy:158-165, 231-267, 372-417): the
// per-point setup, the z-sum inner loop, the one-wavefront-per-point y-loop and the epilogue,
// shared by the translation units that launch it (lzq_kernels.hip: the headline kernels;
// lzq_aov.hip: the kernels whose A/V kernel has parameters of its own, fpy:141-151, 197).
// Not ABI.  The design notes are in lzq_kernels.hip's header comment and DESIGN.md §4.1.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/lzq.h"
#include "lzq_exp2.h"
#include "lzq_physics.h"
#include "lzq_ynode.h"

// linkage of the header's __constant__ tables: external in lzq_kernels.hip (the headline's code
// object is unchanged by the split), internal in any other translation unit that includes it
#ifndef LZQ_QUAD_CONST_LINKAGE
#define LZQ_QUAD_CONST_LINKAGE
#endif

namespace lzq {

// The seven fast-path levels of the dense z-sum and y-loop.  Each is a switch only because a host test
// builds it with =0 and pins the result to the recorded machine code of the commit before it; the full
// account of every level is DESIGN.md §4.1.  A level whose "needs" are not at their defaults is off.
//
//   switch            values   what the level adds                                        needs
//   LZQ_ZERO_SEG      0, 1     zero passes (round(u) = 0 in every lane) skip the range    --
//                              reduction: four FP64 operations per node, not six
//   LZQ_DEAD_SEG      0, 1     all-dead zero passes form the node value once: the node    ZERO_SEG
//                              is F's accumulate alone (zsum_dead)
//   LZQ_FROZEN_SEG    0, 1, 2  1: a zero pass's tail with s frozen is the accumulate      ZERO_SEG, DEAD_SEG
//                              alone (zsum_held); 2: also a clamp-free pass's tail with
//                              t frozen runs without the lookup (zsum_frozen_t)
//   LZQ_GROUP_SEG     0, 2, 4  up to that many consecutive accumulate-only passes are     FROZEN_SEG >= 1
//                              swept through z together (yb_group)
//   LZQ_PASS_LEAN     0, 1     y, e^y and the weight stay live across the loops that      all four at their
//                              have room; clamp-free exp_sc; interior y-nodes; the        defaults
//                              dead/clamped mixed pass (zsum_uniform_lane)
//   LZQ_ACC_FEED      0, 1     the accumulate-only loops (zsum_dead, zsum_held, single    all five at their
//                              and grouped) read omega' from the image's packed array:    defaults
//                              one 64-byte line per 8-node batch, not two
//   LZQ_CLAMP_ARG     0, 1     a clamped node is evaluated at the clamped argument        all six at their
//                              u = KMIN (s = A), so its value is one number, and a        defaults
//                              clamped pass runs as F's accumulate alone from the batch
//                              at which its last live lane clamps
#ifndef LZQ_ZERO_SEG
#define LZQ_ZERO_SEG 1
#endif
#ifndef LZQ_DEAD_SEG
#define LZQ_DEAD_SEG 1
#endif
#ifndef LZQ_FROZEN_SEG
#define LZQ_FROZEN_SEG 2
#endif
#ifndef LZQ_GROUP_SEG
#define LZQ_GROUP_SEG 4
#endif
#ifndef LZQ_PASS_LEAN
#define LZQ_PASS_LEAN 1
#endif
#ifndef LZQ_ACC_FEED
#define LZQ_ACC_FEED 1
#endif
#ifndef LZQ_CLAMP_ARG
#define LZQ_CLAMP_ARG 1
#endif
static_assert(LZQ_GROUP_SEG == 0 || LZQ_GROUP_SEG == 2 || LZQ_GROUP_SEG == 4, "LZQ_GROUP_SEG is 0, 2 or 4");
static_assert(LZQ_PASS_LEAN == 0 || LZQ_PASS_LEAN == 1, "LZQ_PASS_LEAN is 0 or 1");
static_assert(LZQ_ACC_FEED == 0 || LZQ_ACC_FEED == 1, "LZQ_ACC_FEED is 0 or 1");
static_assert(LZQ_CLAMP_ARG == 0 || LZQ_CLAMP_ARG == 1, "LZQ_CLAMP_ARG is 0 or 1");
constexpr int kFrozenSeg = (LZQ_ZERO_SEG != 0 && LZQ_DEAD_SEG != 0) ? LZQ_FROZEN_SEG : 0;
constexpr int kGroupSeg = kFrozenSeg >= 1 ? LZQ_GROUP_SEG : 0;
constexpr bool kLean = LZQ_ZERO_SEG == 1 && LZQ_DEAD_SEG == 1 && LZQ_FROZEN_SEG == 2 && LZQ_GROUP_SEG == 4 &&
                       LZQ_PASS_LEAN == 1;
constexpr bool kAccFeed = kLean && LZQ_ACC_FEED == 1;
constexpr bool kClampArg = kAccFeed && LZQ_CLAMP_ARG == 1;
// the per-point dense kernels: on wherever the kernel keeps its 64 VGPRs without scratch with it
// (tools/kernel_resources.py; tests/test_zsum_clamp_arg_host.py)
template <int NZ>
constexpr bool kClampArgFits = kClampArg && NZ == 0;

constexpr int kNZ = LZQ_NZ;
constexpr int kWaveSize = 64;
// The block is sized so that the LDS copies of the exp table that fit in a CU's 160 KB carry
// the waves: 64-KB table (default) -> two 1024-thread blocks per CU = 8 waves per SIMD, with
// LZQ_MIN_WAVES = 8 capping the kernel at 64 VGPRs (its few spills sit outside the z-loop;
// +2.2% over 4 waves/SIMD, tools/ablate_builds.py).
#ifndef LZQ_BLOCK
#define LZQ_BLOCK ((8 << LZQ_TABBITS) > 81920 ? 1024 : (8 << LZQ_TABBITS) > 40960 ? 1024 : 256)
#endif
constexpr int kBlock = LZQ_BLOCK;
constexpr int kWavesPerBlock = kBlock / kWaveSize;
#ifndef LZQ_KUNROLL
#define LZQ_KUNROLL 8
#endif
#ifndef LZQ_YB
#define LZQ_YB 1
#endif
// __launch_bounds__ second argument = minimum waves per SIMD (8: <= 64 VGPRs; see LZQ_BLOCK)
#ifndef LZQ_MIN_WAVES
#define LZQ_MIN_WAVES 8
#endif
// the same for the table-reuse kernels (grid_reuse, points_reuse, their window forms and grid_solve):
// 8 waves/SIMD (SGPRs capped, a few spilled to VGPR lanes): +12% over 7 (tools/ablate_builds.py ... reuse)
#ifndef LZQ_REUSE_MIN_WAVES
#define LZQ_REUSE_MIN_WAVES 8
#endif
constexpr int kKUnroll = LZQ_KUNROLL;  // z-nodes per scalar-load batch (must divide 1200)
constexpr int kYB = LZQ_YB;            // y-nodes per lane per pass (independent chains)
static_assert(kNZ % kKUnroll == 0, "z unroll must divide nz");

struct ZNode {
  double g4;     // fpy:156 gamma4(z_k), verbatim cancelling form
  double omega;  // z_k^2 e^{-z_k} * trapezoid weight of node k
};

// omega'_k of the accumulate-only loops.  FEED (LZQ_ACC_FEED): from the packed array behind the grid's nzp
// nodes (zimage_omega, lzq_exp2.h) -- the node's own bits, one 64-byte line per batch -- else from the node
// itself.  FEED is the dense, untruncated pass's and the A/V kernels'; the truncated passes and the table
// mode keep reading the nodes, so the on-device controls of the dense kernels do not share the array.
template <bool FEED>
__device__ __forceinline__ double acc_omega(const ZNode* __restrict__ zt, int nzp, int k) {
  if constexpr (FEED) return zimage_omega(zt, nzp)[k];
  else return zt[k].omega;
}

// ---------------------------------------------------------------------------------------
// per-point quadrature setup (wave-uniform values)
// ---------------------------------------------------------------------------------------
struct QuadSetup {
  double y_lo, y_hi, step, delta;  // ys = linspace(y_lo, y_hi, n)    fpy:247
  int64_t n;
  bool empty;                      // y_hi <= y_lo -> Y_B = 0         fpy:242-243
  double pref0;                    // (I_p/2)(beta/v_w)               fpy:162
  double cneg;                     // -(I_p/6)                        fpy:163
  double Bc, Tp, dT0, sig, m, m3, flux, P, g_star, g_star_s;
  double H0;      // 1.66 sqrt(g*) / M_Pl             fpy:85
  double s0;      // (2 pi^2/45) g*s                   fpy:88
  double c_rel;   // g * 3 zeta3/(4 pi^2) | g zeta3/pi^2   fpy:96-99
  double c_nr;    // g (m/2pi)^1.5                     fpy:104
  double v0;      // pi * max(m, 1e-20)                fpy:117
  double isig;    // 1/sig: y_factors multiplies instead of dividing
};

// Move a wave-uniform double into SGPRs (two v_readfirstlane_b32): the per-point constants
// then occupy scalar registers instead of ~44 VGPRs across the z-loop.
__device__ __forceinline__ double uniform(double x) {
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// x**1.5 as x*sqrt(x) (<= 2 ulp from pow; the device pow is ~100 VALU and ~40 VGPRs)
__device__ __forceinline__ double pow15(double x) { return x * sqrt(x); }

__device__ __forceinline__ QuadSetup quad_setup(const lzq_point& pt, double P, double T_lo, double T_hi,
                                                int32_t n_y) {
  QuadSetup s;
  const double B = pt.beta_over_H, Tp = pt.T_p_GeV;
  // fpy:234-243
  double y_lo = pymax(y_of_T(T_hi, Tp, B), -80.0);
  double y_hi = pymin(y_of_T(T_lo, Tp, B), +50.0);
  s.empty = !(y_hi > y_lo);
  s.y_lo = y_lo;
  s.y_hi = y_hi;
  s.n = n_y > LZQ_NY_MIN ? n_y : LZQ_NY_MIN;  // fpy:246
  s.delta = y_hi - y_lo;
  s.step = s.delta / (double)(s.n - 1);
  // AoverVKernel constants fpy:146-151
  double v_w = pymax(pt.v_w, 1e-12);
  double H_p = H_std(Tp, pt.g_star);
  double beta = B * H_p;
  s.pref0 = (pt.I_p / 2.0) * (beta / v_w);
  s.cneg = -(pt.I_p / 6.0);
  // fpy:250-262
  s.Bc = pymax(B, 1e-30);
  s.Tp = Tp;
  s.dT0 = -(Tp / s.Bc);
  s.sig = pymax(pt.source_shape_sigma_y, 1e-6);
  s.m = pt.m_chi_GeV;
  s.m3 = pt.m_chi_GeV / 3.0;
  s.flux = pt.incident_flux_scale;
  s.P = P;
  s.g_star = pt.g_star;
  s.g_star_s = pt.g_star_s;
  s.H0 = 1.66 * sqrt(pt.g_star);
  s.s0 = (2.0 * (kPi * kPi) / 45.0) * pt.g_star_s;
  s.c_rel = (pt.stats == 0) ? pt.g_chi * (3.0 * kZeta3 / (4.0 * (kPi * kPi))) : pt.g_chi * (kZeta3 / (kPi * kPi));
  s.c_nr = pt.g_chi * pow15(pt.m_chi_GeV / (2.0 * kPi));
  s.v0 = kPi * pymax(pt.m_chi_GeV, 1e-20);
  s.isig = 1.0 / s.sig;
  double* f[] = {&s.y_lo, &s.y_hi, &s.step, &s.delta, &s.pref0, &s.cneg, &s.Bc, &s.Tp, &s.dT0, &s.sig, &s.m,
                 &s.m3, &s.flux, &s.P, &s.g_star, &s.g_star_s, &s.H0, &s.s0, &s.c_rel, &s.c_nr, &s.v0,
                 &s.isig};
#pragma unroll
  for (double* v : f) *v = uniform(*v);
  return s;
}

// A loop-invariant double materialised once in a VGPR (opaque to re-materialisation).
__device__ __forceinline__ double vgpr_const(double x) {
  double v;
  asm volatile("v_mov_b64 %0, %1" : "=v"(v) : "s"(x));
  return v;
}

// e^x for the per-y factors (<= 1 ulp, like the device libm exp).  Cody-Waite reduction
// x = k ln2 + r, |r| <= ln2/2, Taylor series to r^13 (truncation < 5e-18), ldexp.  The 15
// constants are read from constant memory through an offset made opaque per call, so they
// come in by scalar loads where needed: the libm exp's coefficients were hoisted out of the
// y-loop into VGPRs and spilled to scratch across the z-loop (which needs ~60 of 64 VGPRs).
LZQ_QUAD_CONST_LINKAGE __constant__ double kExpC[15] = {
    0x1.6124613a86d09p-33, 0x1.1eed8eff8d898p-29, 0x1.ae64567f544e4p-26, 0x1.27e4fb7789f5cp-22,
    0x1.71de3a556c734p-19, 0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-13, 0x1.6c16c16c16c17p-10,
    0x1.1111111111111p-7,  0x1.5555555555555p-5,  0x1.5555555555555p-3,  0x1.0p-1,  // 1/13! .. 1/2!
    0x1.71547652b82fep+0,                                                           // 1/ln2
    0x1.62e42fefa39efp-1,  0x1.abc9e3b39803fp-56};                                  // ln2 hi, lo
//
// The argument is clamped to [-1100, 710] first.  A caller that has shown more takes less of the clamp
// (LZQ_PASS_LEAN): kExpIn for an argument already inside the range, kExpLow for one that is <= 0 or NaN.
enum ExpClamp { kExpIn = 0, kExpLow = 1, kExpBoth = 3 };
template <int CLAMP = kExpBoth>
__device__ __forceinline__ double exp_sc(double x) {
  int o = 0;
  asm volatile("" : "+s"(o));
  const double* c = kExpC + o;
  if constexpr ((CLAMP & 1) != 0) x = x < -1100.0 ? -1100.0 : x;  // NaN passes through both
  if constexpr ((CLAMP & 2) != 0) x = x > 710.0 ? 710.0 : x;
  const double k = __builtin_rint(x * c[12]);
  double r = __builtin_fma(-k, c[13], x);
  r = __builtin_fma(-k, c[14], r);
  double p = c[0];
#pragma unroll
  for (int i = 1; i < 12; ++i) p = fma_vvs(p, r, c[i]);  // the coefficient as the fma's SGPR operand
  p = __builtin_fma(p, r, 1.0);  // (e^r - 1) / r
  p = __builtin_fma(p, r, 1.0);  // e^r
  return __builtin_ldexp(p, (int)k);
}

// numpy.linspace element (handles numpy's step == 0 branch as well)
__device__ __forceinline__ double y_node(const QuadSetup& s, int j) {  // n_y is int32
  return y_node_general(s, j);
}

// e^y of the A/V prefactor, fpy:161: exp(clip(y, -50, 50)).  LEAN (LZQ_PASS_LEAN; y is a finite linspace
// element, never NaN): the clip is one max and one min, and exp_sc runs without the clamp of its own that
// cannot fire behind it -- the same argument, the same bits.
template <bool LEAN>
__device__ __forceinline__ double exp_y(double y) {
  if constexpr (LEAN) return exp_sc<kExpIn>(__builtin_fmin(__builtin_fmax(y, -50.0), 50.0));
  else return exp_sc(pymax(pymin(y, 50.0), -50.0));
}

// Per-y factors of the integrand of fpy:264-265 that do not depend on F, computed BEFORE the
// z-loop so that only these 7 doubles (not the whole QuadSetup) stay live across it.  The
// post-loop combination keeps the reference's rounding order:
//   SB = ((P*J)*Av)*W,  integrand = SB/((s*H)*T)*|dT/dy|,  Av = (pref0*expy)*F.
struct YFactors {
  double PJ;     // P * J(T)                        fpy:260,264
  double W;      // window                          fpy:262
  double sHT;    // (s*H)*T                         fpy:258-259,265
  double adTdy;  // |dT/dy|                         fpy:255,265
  double pexp;   // pref0 * expy  (A/V prefactor)   fpy:162
  double w;      // trapezoid weight of the node    fpy:267
  double live;   // 1 if y <= 50 (fpy:159), else 0
};

// 1/sqrt(d) for a positive normal d: v_rsq_f64, then the Goldschmidt iteration that the
// compiler's correctly rounded sqrt uses (g -> sqrt(d), h -> 1/(2 sqrt(d))); <= 2 ulp.
__device__ __forceinline__ double rsqrt_pos(double d) {
  const double r = __builtin_amdgcn_rsq(d);
  double g = d * r, h = 0.5 * r;
  double e = __builtin_fma(-g, h, 0.5);
  g = __builtin_fma(g, e, g);
  h = __builtin_fma(h, e, h);
  e = __builtin_fma(-g, h, 0.5);
  h = __builtin_fma(h, e, h);
  return 2.0 * h;
}

// The fixed-exponent powers of numpy's `**` (SVML pow, <= 1 ulp) are evaluated with products
// (<= 3 ulp): denom**-0.5 and denom**-1.5 from one reciprocal square root, T**3 = (T*T)*T,
// T**1.5 = T sqrt T; the quotients by per-point constants (y/sigma, H's 1/M_Pl) are products
// with their reciprocals.  This keeps the per-y work small (the device pow(double) is
// ~100 VALU and ~40 VGPRs; a division or a sqrt ~10-16) and moves results by ~1e-16 relative
// (tests: worst golden error unchanged at 1e-13).
//
// The window W(y) is the caller's: wf(y) is evaluated where the reference's Gaussian proxy stands
// (gauss_window below, the default); lzq_window.hip passes the window of a point's own block.
template <typename WinF>
__device__ __forceinline__ YFactors y_factors(const QuadSetup& s, double y, double expy, double wt, const WinF& wf) {
  YFactors f;
  // 2y/B stays a correctly rounded division: near y = -B/2 (T_max/T_p large) 1 + 2y/B cancels,
  // and the product with a rounded 2/B moved Y_B by 6.7e-13 on a golden point (diag_golden.py)
  const double denom = pymax(1.0 + 2.0 * y / s.Bc, 1e-12);  // fpy:252-253
  const double rs = rsqrt_pos(denom);
  const double T = s.Tp * rs;                               // fpy:254
  const double dTdy = s.dT0 * ((rs * rs) * rs);             // fpy:255  denom**(-1.5)
  const double H = s.H0 * T * T * (1.0 / kMplGeV);          // fpy:258 via fpy:85
  double T3 = (T * T) * T;
  double sE = s.s0 * T3;                                  // fpy:259 via fpy:88
  double n_eq, vbar;                                      // fpy:90-120, strict T > m/3 branch
  if (T > s.m3) {
    n_eq = s.c_rel * T3;
    vbar = 1.0;
  } else {
    n_eq = s.c_nr * (T * sqrt(T)) * exp_sc(-s.m / pymax(T, 1e-30));
    vbar = sqrt(pymax(8.0 * T / s.v0, 0.0));
  }
  double J = s.flux * 0.25 * n_eq * vbar;                 // fpy:260
  f.W = wf(y);                                             // fpy:262
  f.PJ = s.P * J;
  f.sHT = sE * H * T;
  f.adTdy = fabs(dTdy);
  f.pexp = s.pref0 * expy;
  f.w = wt;
  f.live = (y > 50.0) ? 0.0 : 1.0;
  return f;
}

// fpy:262: the reference's window, exp(-(y/sigma_y)^2 / 2)
// (LEAN, LZQ_PASS_LEAN: the argument is <= 0 or NaN, so exp_sc's upper clamp cannot fire and is left out)
template <bool LEAN = false>
__device__ __forceinline__ double gauss_window(const QuadSetup& s, double y) {
  const double q = y * s.isig;
  return exp_sc<LEAN ? kExpLow : kExpBoth>(-0.5 * (q * q));
}

__device__ __forceinline__ YFactors y_factors(const QuadSetup& s, double y, double expy, double wt) {
  return y_factors(s, y, expy, wt, [&](double yy) { return gauss_window(s, yy); });
}

// yb_wave's window: W(y) of the point parked in a wave's slot.  The default is the reference's.
struct SlotGaussWindow {
  template <typename Slot>
  static __device__ __forceinline__ double eval(const Slot& slot, double y) { return gauss_window(slot.s, y); }
};

// Win::eval; the default window in its lean form where LEAN (LZQ_PASS_LEAN)
template <bool LEAN, typename Win, typename Slot>
__device__ __forceinline__ double win_eval(const Slot& slot, double y) {
  if constexpr (LEAN && __is_same(Win, SlotGaussWindow)) return gauss_window<true>(slot.s, y);
  else return Win::eval(slot, y);
}

__device__ __forceinline__ double integrand_from(const YFactors& f, double F) {
  double Av = f.live != 0.0 ? f.pexp * F : 0.0;           // fpy:159-165
  double SB = f.PJ * Av * f.W;                            // fpy:264
  return SB / f.sHT * f.adTdy;                            // fpy:265
}

// trapezoid weight of y-node j: (d_{j-1} + d_j)/2 with d = diff(ys)      fpy:267
__device__ __forceinline__ double y_weight(const QuadSetup& s, int j, double y) {
  return y_weight_general(s, j, y);
}

// y, e^y and the trapezoid weight of y-node j of a pass, as yb_wave and yb_group form them.  `interior`
// (wave-uniform; LZQ_PASS_LEAN only): the pass touches neither end of the y-grid (y_pass_interior,
// lzq_ynode.h) and takes the forms without the end-of-grid selects; otherwise j may lie past the grid
// (a tail lane of the last pass), which recomputes the last node with weight 0.
template <bool LEAN>
__device__ __forceinline__ void y_triple(const QuadSetup& s, int j, int n, bool interior, double& y, double& ey,
                                         double& wt) {
  if (LEAN && interior) {
    y = y_node_interior(s.y_lo, s.step, j);
    wt = y_weight_interior(s.y_lo, s.step, j, y);
  } else {
    const int jj = j < n ? j : n - 1;
    y = y_node(s, jj);
    wt = j < n ? y_weight(s, jj, y) : 0.0;
  }
  ey = exp_y<LEAN>(y);  // (one copy behind the branch: the code is what a launch fetches from HBM)
}

// exp variants of the inner loop (lzq_tune(LZQ_TUNE_EXP, ...))
enum ExpVariant { kExpPoly11 = 0, kExpTable = 1 };

// Scale of c2 expected by the variant (2^(c2*g) for poly11, 2^(c2N*g/256) for the table).
template <int EXPV>
__device__ __forceinline__ double c2_scale() { return EXPV == kExpTable ? (double)kTabN : 1.0; }

// F(c2) = sum_k omega_k 2^(c2 g4_k) for YB independent y-nodes per lane.
//
// The loop is VALU-issue bound: an FP64 instruction costs 4.4 cycles per wave64 on gfx950 and an
// integer / FP32 one ~2.5 (tools/ubench_valu.hip, pure streams); in this kernel a node's 8.48
// VALU instructions take 30.9 SIMD-cycles, 79% of them in the 6.1 FP64 FMA/MUL/ADD
// (profiles/round2/pmc_summary.json).  So the loop is built to minimise the instruction count,
// FP64 first.  Table variant, per (y, z) node:
//
//   t  = fma(c2, g, M)          M = 1.5*2^52: t = M + round(u), u = c2*g in 1/N-octave units
//   kd = t - M                  exact
//   r  = fma(c2, g, -kd)        u - round(u) in [-1/2, 1/2], one rounding
//   tc = max(t, M + KMIN)       clamp to e >= -1534 octaves (also keeps lo32 in int range)
//   a  = (lo32(tc) & (N-1))*8   LDS byte address: ONE v_lshlrev_b16 for N = 8192
//   T' = lds[a]                 T'.hi = hi(2^(j/N)) - (j << S) + (512 << 20), S = 20 - BITS
//   T'.hi += lo32(tc) << S      ONE v_lshl_add_u32: T' = 2^(j/N) * 2^(e+512), e = floor(k/N)
//   q  = r*(B1 + r*B2)          2 FP64
//   v  = fma(T', q, T')         = 2^(u/N) * 2^512, always a normal double (e+512 >= -1022)
//   F  = fma(omega', v, F)      omega' = omega * 2^-512 (z table), so omega'*v = omega*2^u
//
// = 10 VALU per node (round-1 kernel: 12.5).  The default completed-square form (kSqForm,
// lzq_exp2.h) replaces kd, r, q and the T*(1+q) fma by
//   w  = (M + A) - t            exact (M + A an integer below 2^53)
//   s  = fma(c2, g, w)          r + A, one rounding
//   v  = T'' * fma(s, s, beta)  T'' = C * 2^(j/N) * 2^(e+512) from the same lookup + insert
// = 9 VALU per node, 8 on clamp-free passes.  The last fma rounds the exact product omega*2^u
// once, so gradual underflow is exact; clamped nodes (u < -1534 octaves) contribute
// omega*2^-1534*(...) which rounds away exactly like the underflowed 0 it stands for.
// For |u| < 2^51 (every non-dead lane, checked on the host) t is exact; dead lanes (whose
// every node k >= 1 underflows) run with c2 = 0 and are zeroed, so no input reaches the
// loop with |u| >= 2^51.
//
// CLAMP = false drops the max (9 VALU/node) on passes whose lanes all satisfy |c2N|*g_max <=
// N*1534 (no node can leave the clamp range); zsum_dispatch picks it per pass.
//
// Where every lane of the wave would read ONE entry at every node -- tc = M on a pass whose lanes
// all have round(u) = 0 or are dead, tc = M + KMIN from the node at which the last lane clamps --
// the lookup (address, ds_read, insert, and the max) returns what it returned at the node before.
// zsum_dispatch finds those stretches per pass with the loop's own t and runs them through
// zsum_uniform below: the same six FP64 operations per node on the same operands, the entry fetched
// once (80.3% of the C2 workload's nodes, tools/uniform_segment_share.py).  On the
// first kind of stretch (t = M at every node, 64.0% of the nodes) two of the six are known before
// the loop starts -- t = M, and w = (M + A) - M = A exactly -- and the node runs the other four:
// s = fma(c2, g, A), q, v and F's fma, on the operands the six-operation node hands them
// (LZQ_ZERO_SEG).  Where all 64 lanes of such a pass are dead (c2 = +0.0 in every lane, 24.8% of the
// nodes) s = A as well, so q and v are one number for the pass and the node runs F's fma alone
// (LZQ_DEAD_SEG, zsum_dead).  gamma4 saturates, so on the live zero passes every lane's s, and on the
// clamp-free passes every lane's t, reaches the value it has at the last executed node well before
// the pass ends: from that batch on, what depends on it is formed once per lane -- v on a zero pass,
// whose node is then F's fma alone (18.0% of the nodes), the table entry and w on a clamp-free one,
// whose node is then s, q, v and F's fma (6.4%) (LZQ_FROZEN_SEG, zsum_held, zsum_frozen_t).  No node
// is skipped and the bits are the general loop's
// (tests/test_zsum_segments_host.py, tests/test_zsum_zero_segment_host.py,
// tests/test_zsum_dead_segment_host.py, tests/test_zsum_frozen_host.py, tests/test_gpu_zsum_segments.py,
// tests/test_gpu_zsum_zero_segment.py, tests/test_gpu_zsum_dead_segment.py, tests/test_gpu_zsum_frozen.py).
// Those accumulate-only nodes (42.8%) are bound by the feed of omega', not by their one instruction: where
// consecutive passes are accumulate-only from node 0, yb_wave sweeps up to four of them through z together
// (LZQ_GROUP_SEG, yb_group below; tests/test_zsum_group_host.py, tests/test_gpu_zsum_group.py), and all of
// them, grouped or not, read omega' from the packed array of the grid's image, one line per 8-node batch
// instead of two (LZQ_ACC_FEED, acc_omega; tests/test_zsum_feed_host.py, tests/test_gpu_zsum_feed.py).
template <int YB, int EXPV, bool CLAMP = true, bool CARG = kClampArg>
__device__ __forceinline__ void zsum(const ZNode* __restrict__ zt, const double* tab, const double (&c2)[YB],
                                     double (&F)[YB], int kend) {
#pragma unroll
  for (int b = 0; b < YB; ++b) F[b] = 0.0;
  if constexpr (EXPV == kExpTable) {
    constexpr double kMagic = 0x1.8p52;
    constexpr double kTClamp = kMagic + (double)kTabKMin;  // exact
    const double Mv = vgpr_const(kMagic);
    const double MAv = kMagic + kSqA;  // exact (an integer below 2^53)
    // plain form: polynomial coefficients, B1 pinned in a VGPR for the whole loop (see tab_q_with)
    double Bv[kPolyDeg];
#pragma unroll
    for (int i = 0; i < kPolyDeg; ++i) Bv[i] = TabPoly<kTabBits, kPolyDeg>::B[i];
    if constexpr (!kSqForm) Bv[0] = vgpr_const(Bv[0]);
    const char* tabb = reinterpret_cast<const char*>(tab);
    // (LZQ_CLAMP_ARG: A's high word for the clamped lanes' select, in a VGPR for this loop alone)
    [[maybe_unused]] uint32_t Ah = 0;
    if constexpr (CLAMP && CARG && kSqForm) Ah = clamp_arg_hi();
    for (int k = 0; k < kend; k += kKUnroll) {
      double g4[kKUnroll], om[kKUnroll];
#pragma unroll
      for (int kk = 0; kk < kKUnroll; ++kk) {
        g4[kk] = zt[k + kk].g4;
        om[kk] = zt[k + kk].omega;
      }
      // phases: reduction + addresses for the whole batch, then the lookups (in flight
      // together), then polynomial + accumulate.  (LZQ_CLAMP_ARG: the clamped loop runs the phases on the two
      // halves of the batch in turn -- with the select's masks and A's high word beside it, eight nodes in
      // flight are a register more than the kernel has)
      constexpr int kPh = (CLAMP && CARG && kSqForm && kKUnroll % 2 == 0) ? kKUnroll / 2 : kKUnroll;
#pragma unroll
      for (int h = 0; h < kKUnroll; h += kPh) {
        double r[YB][kPh], T[YB][kPh];
        uint32_t kc[YB][kPh], a[YB][kPh];
#pragma unroll
        for (int kk = 0; kk < kPh; ++kk)
#pragma unroll
          for (int b = 0; b < YB; ++b) {
            const double t = __builtin_fma(c2[b], g4[h + kk], Mv);
            if constexpr (kSqForm) {
              r[b][kk] = __builtin_fma(c2[b], g4[h + kk], MAv - t);  // s = r + A (lzq_exp2.h)
              // (LZQ_CLAMP_ARG: a clamped lane takes the clamped argument's s = A, on the max's own comparison)
              if constexpr (CLAMP && CARG) r[b][kk] = clamp_arg_s(t, r[b][kk], Ah);
            } else {
              const double kd = t - Mv;
              r[b][kk] = __builtin_fma(c2[b], g4[h + kk], -kd);
            }
            const double tc = CLAMP ? __builtin_fmax(t, kTClamp) : t;
            kc[b][kk] = (uint32_t)__builtin_bit_cast(uint64_t, tc);
            a[b][kk] = tab_byte_addr(kc[b][kk]);
          }
#pragma unroll
        for (int kk = 0; kk < kPh; ++kk)
#pragma unroll
          for (int b = 0; b < YB; ++b) T[b][kk] = *reinterpret_cast<const double*>(tabb + a[b][kk]);
#pragma unroll
        for (int kk = 0; kk < kPh; ++kk)
#pragma unroll
          for (int b = 0; b < YB; ++b) {
            const double Ts = tab_scale(T[b][kk], kc[b][kk]);
            if constexpr (kSqForm) {
              F[b] = __builtin_fma(om[h + kk], Ts * __builtin_fma(r[b][kk], r[b][kk], kSqBeta), F[b]);
            } else {
              const double q = tab_q_with<kPolyDeg>(r[b][kk], Bv);
              F[b] = __builtin_fma(om[h + kk], __builtin_fma(Ts, q, Ts), F[b]);
            }
          }
      }
    }
  } else {
    for (int k = 0; k < kend; k += kKUnroll) {
#pragma unroll
      for (int kk = 0; kk < kKUnroll; ++kk) {
        const double g = zt[k + kk].g4, om = zt[k + kk].omega;
#pragma unroll
        for (int b = 0; b < YB; ++b) F[b] = __builtin_fma(om, exp2_nonpos(c2[b], g, kOmegaBias), F[b]);
      }
    }
  }
}

// The uniform-entry loop: nodes kbeg .. kend of a pass on which every lane's
// clamped magic sum tc is one constant at every node, so all 64 lanes would fetch the same entry
// with the same exponent, node after node.  Ts is that entry as the general loop forms it
// (seg_entry), wave-uniform, an SGPR pair; a node is then exactly the general node's six FP64
// operations on the same operands in the same order (seg_node: t, w, s, q, v, and F's fma) --
// no max, no address, no ds_read, no insert.  Every node is executed; F carries on from kbeg in
// node order like the general loop's.
//
// ZERO (LZQ_ZERO_SEG; the caller has shown t = M for every lane at g_max, hence at every node):
// t and w are not recomputed -- w is A exactly, so s = fma(c2, g, A) is the same instruction on the
// same operand (seg_node_zero) -- and a node is four FP64 operations: s, q, v, and F's fma.  A takes
// the loop's one pinned VGPR pair, where M sits otherwise: g, beta, Ts and omega' are scalar
// operands already and a VOP3 instruction reads one, so a scalar A would cost a v_mov per node.
template <int YB, bool ZERO = false>
__device__ __forceinline__ void zsum_uniform(const ZNode* __restrict__ zt, double Ts, const double (&c2)[YB],
                                             double (&F)[YB], int kend, int kbeg) {
  if (kbeg == 0) {
#pragma unroll
    for (int b = 0; b < YB; ++b) F[b] = 0.0;
  }
  const double Pv = vgpr_const(ZERO ? kSqA : kTabMagic);  // the pinned pair: A, or M
  for (int k = kbeg; k < kend; k += kKUnroll) {
    double g4[kKUnroll], om[kKUnroll];
#pragma unroll
    for (int kk = 0; kk < kKUnroll; ++kk) {
      g4[kk] = zt[k + kk].g4;
      om[kk] = zt[k + kk].omega;
    }
#pragma unroll
    for (int kk = 0; kk < kKUnroll; ++kk)
#pragma unroll
      for (int b = 0; b < YB; ++b) {
        const double v = ZERO ? seg_node_zero(c2[b], g4[kk], Pv, Ts) : seg_node(c2[b], g4[kk], Pv, Ts);
        F[b] = __builtin_fma(om[kk], v, F[b]);
      }
  }
}

// The uniform-entry loop with the entry held per lane (LZQ_PASS_LEAN): nodes kbeg .. kend of a clamped
// pass that holds dead lanes, from the batch at which every LIVE lane is clamped.  A dead lane runs with
// c2e = +0.0, so its t is M at every node and max(M, M + KMIN) = M: it reads T''[0] with nothing inserted
// throughout, while a live lane reads the entry of M + KMIN.  Each lane's clamped magic sum is therefore
// one constant from kbeg on -- not the same one in every lane -- and Ts[b] is its entry as the general
// loop forms it (seg_entry on M for a dead lane, on M + KMIN for the others), a VGPR pair.  The node is
// zsum_uniform's: seg_node's six FP64 operations on the general node's operands, every node executed.
template <int YB>
__device__ __forceinline__ void zsum_uniform_lane(const ZNode* __restrict__ zt, const double (&Ts)[YB],
                                                  const double (&c2)[YB], double (&F)[YB], int kend, int kbeg) {
  if (kbeg == 0) {
#pragma unroll
    for (int b = 0; b < YB; ++b) F[b] = 0.0;
  }
  const double Mv = vgpr_const(kTabMagic);
  for (int k = kbeg; k < kend; k += kKUnroll) {
    double g4[kKUnroll], om[kKUnroll];
#pragma unroll
    for (int kk = 0; kk < kKUnroll; ++kk) {
      g4[kk] = zt[k + kk].g4;
      om[kk] = zt[k + kk].omega;
    }
#pragma unroll
    for (int kk = 0; kk < kKUnroll; ++kk)
#pragma unroll
      for (int b = 0; b < YB; ++b) F[b] = __builtin_fma(om[kk], seg_node(c2[b], g4[kk], Mv, Ts[b]), F[b]);
  }
}

// The all-dead loop (LZQ_DEAD_SEG): a zero pass whose 64 lanes are all dead, so every lane runs with
// c2e = +0.0.  Then s = fma(+0 * g, A) = A at every node, and q = fma(A, A, beta) and v = T''[0] * q
// are the same two numbers at each of them (seg_node_dead): they are formed once, and a node is F's
// accumulate alone, F = fma(omega'_k, v0, F), on the operands zsum_uniform<YB, true> hands it, in node
// order from F = 0.  No node is skipped.  v0 takes the loop's one pinned VGPR pair; omega' is the
// instruction's scalar operand, and g4 is not read.  FEED (LZQ_ACC_FEED): omega' comes from the packed
// array behind the grid's nzp nodes (acc_omega), the same bits out of one 64-byte line per batch.
// kbeg > 0 (LZQ_CLAMP_ARG): the clamped suffix of a pass without dead lanes, nodes kbeg .. kend with Ts the
// entry of M + KMIN, so that v0 is the clamped argument's value v_c; F carries on from the prefix.
template <int YB, bool FEED = false>
__device__ __forceinline__ void zsum_dead(const ZNode* __restrict__ zt, int nzp, double Ts, double (&F)[YB], int kend,
                                          int kbeg = 0) {
  if (kbeg == 0) {
#pragma unroll
    for (int b = 0; b < YB; ++b) F[b] = 0.0;
    // (YB > 1: the chains start from the same 0 and add the same terms; opaque starts keep them YB
    // chains of YB fma per node -- dense work -- instead of one chain the compiler copies)
    if constexpr (YB > 1) {
#pragma unroll
      for (int b = 0; b < YB; ++b) asm volatile("" : "+v"(F[b]));
    }
  }
  const double v0 = seg_node_dead(vgpr_const(kSqA), Ts);
  for (int k = kbeg; k < kend; k += kKUnroll) {
    double om[kKUnroll];
#pragma unroll
    for (int kk = 0; kk < kKUnroll; ++kk) om[kk] = acc_omega<FEED>(zt, nzp, k + kk);
#pragma unroll
    for (int kk = 0; kk < kKUnroll; ++kk)
#pragma unroll
      for (int b = 0; b < YB; ++b) F[b] = __builtin_fma(om[kk], v0, F[b]);
  }
}

// The held-value loop (LZQ_FROZEN_SEG >= 1): nodes kbeg .. kend of a zero pass on which every lane's
// s = fma(c2, g, A) already has the value it has at the last executed node, so each lane's v is one
// number on all of them (v[b]: seg_node_zero at that node, formed by the caller).  A node is F's
// accumulate alone, F = fma(omega'_k, v, F), in node order, carrying on from kbeg: zsum_dead's loop
// with a per-lane value, and these lanes are live, so F is kept.  No node is skipped.  (FEED: as zsum_dead.)
template <int YB, bool FEED = false>
__device__ __forceinline__ void zsum_held(const ZNode* __restrict__ zt, int nzp, const double (&v)[YB], double (&F)[YB],
                                          int kend, int kbeg) {
  if (kbeg == 0) {
#pragma unroll
    for (int b = 0; b < YB; ++b) F[b] = 0.0;
  }
  for (int k = kbeg; k < kend; k += kKUnroll) {
    double om[kKUnroll];
#pragma unroll
    for (int kk = 0; kk < kKUnroll; ++kk) om[kk] = acc_omega<FEED>(zt, nzp, k + kk);
#pragma unroll
    for (int kk = 0; kk < kKUnroll; ++kk)
#pragma unroll
      for (int b = 0; b < YB; ++b) F[b] = __builtin_fma(om[kk], v[b], F[b]);
  }
}

// The frozen-t loop (LZQ_FROZEN_SEG >= 2): nodes kbeg .. kend of a clamp-free pass on which every
// lane's t = fma(c2, g, M) already has the value it has at the last executed node.  What the general
// node derives from t alone is then fixed per lane -- the address, the ds_read and the exponent
// insert (Ts[b]) and w = (M + A) - t (w[b]); the caller forms both with the general path's own
// functions -- and a node is the general node's other four operations on the same operands in the
// same order: s = fma(c2, g, w), q, v = Ts * q, and F's fma.  No node is skipped.
template <int YB>
__device__ __forceinline__ void zsum_frozen_t(const ZNode* __restrict__ zt, const double (&Ts)[YB], const double (&w)[YB],
                                              const double (&c2)[YB], double (&F)[YB], int kend, int kbeg) {
  if (kbeg == 0) {
#pragma unroll
    for (int b = 0; b < YB; ++b) F[b] = 0.0;
  }
  for (int k = kbeg; k < kend; k += kKUnroll) {
    double g4[kKUnroll], om[kKUnroll];
#pragma unroll
    for (int kk = 0; kk < kKUnroll; ++kk) {
      g4[kk] = zt[k + kk].g4;
      om[kk] = zt[k + kk].omega;
    }
#pragma unroll
    for (int kk = 0; kk < kKUnroll; ++kk)
#pragma unroll
      for (int b = 0; b < YB; ++b) F[b] = __builtin_fma(om[kk], seg_node_frozen(c2[b], g4[kk], w[b], Ts[b]), F[b]);
  }
}

// The zero stretch's magic sum M as seg_entry's argument.  PINNED (the frozen paths are compiled in):
// the dispatch's pinned VGPR copy of M, whose low word is the lookup's k = 0 -- as a literal, that 0
// took a VGPR pair across the y-loop, and with the frozen paths' registers beside it, a spill.
template <bool PINNED>
__device__ __forceinline__ double zero_magic(double Mv) {
  if constexpr (PINNED) return Mv;
  else return kTabMagic;
}

// __shfl_xor over the 64 lanes with the lane index re-derived where it is used (two v_mbcnt; volatile).
// __shfl_xor's own is hoisted out of the y-loop and held in a VGPR across every z-loop, which the values
// the lean passes keep live there have no room for (LZQ_PASS_LEAN).
__device__ __forceinline__ double shfl_xor_rederived(double v, int off) {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  const int a = (l ^ off) << 2;
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)(uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// Pass-level wrapper: "dead" lanes, c2 * g4_1 <= -N*1077 (every node k >= 1 underflows to
// exactly 0: g4 is increasing and omega_0 = 0), run the loop with c2 = 0 and are zeroed
// afterwards -- the same instruction stream, the exact zero.
//
// The z grid: NZ > 0 is the compile-time node count of the reference's default grid
// (fpy:142, LZQ_NZ = 1200: the headline kernels); NZ = 0 reads the padded node count nzp of a
// runtime (nz, z_max) grid (AoverVKernel(..., z_max, nz), fpy:141-156).  Padding nodes repeat the
// last g4 with omega = 0: each adds an exact +0, so F is the sum over the nz real nodes.  On a
// fine grid (small g4_1) a live lane can reach |u| >= 2^51 at later nodes, where the magic-
// constant reduction is inexact; every such node has u < KMIN, takes the clamped path (the
// clamp-free test below sees it), and its term omega' * T''(KMIN) * ((A + O(|u| 2^-52))^2 + beta)
// stays below 2^-1074 for |u| < 2^200, so it rounds away exactly like the underflow it stands
// for; build_ztable bounds |u| by that on the host.  Pinned by tests/test_gpu_zsum.py: A/V on the
// (2400, 30) and (12000, 30) grids, whose live lanes reach |u| >= 2^51, against mpmath up to the
// dead threshold, and equal bits for equal y whatever the wave holds (dead, clamped, clamp-free).
//
// truncate != 0 (lzq_tune LZQ_TUNE_TRUNCATE; NOT used by the headline bench, which is dense
// per SURVEY §8d): the pass stops at kend, the first z-node (rounded up to the unroll) beyond
// which every live lane has c2*g4_k < -1080 octaves.  Those nodes add omega*2^u < 2^-1080 to
// F, which the accumulate's rounding discards exactly, so F is bit-identical to the dense sum
// (tests/test_zsum_host.py in a one-lane model, every regime and padded grids; on the device
// tests/test_gpu_zsum.py: truncated tables against dense kernels, per value and through Y_B).
// (Needs g4 non-decreasing over the grid: the host passes truncate = 0 for a grid whose
// rounded g4 is not.)
//
// Returns whether the pass ran as F's accumulate alone from node 0 (all lanes dead, or a zero pass with
// k3 = 0): what yb_wave's pass grouping (LZQ_GROUP_SEG) takes as its cue to try a group next.
//
// FEEDOK (LZQ_ACC_FEED): the accumulate-only loops of an untruncated pass may read the packed omega' array;
// false for the table mode, which like the truncated pass stays on the nodes (the dense kernels' controls).
//
// CARG (LZQ_CLAMP_ARG, per kernel): the clamped argument.  A template parameter beside the switch because the
// per-point kernels on the default grid (yields_points_kernel and yields_points_aov_kernel with NZ = 1200) do
// not fit 64 VGPRs with it -- 12 bytes of scratch, outside the z-loops -- and run without (kClampArgFits);
// F's bits are the same either way.
//
// after_general (LZQ_PASS_LEAN; yb_wave's): called at the end of the branches that ran the table-lookup
// loop zsum<>, and of no other.  What the caller keeps in registers across the lean loops it re-forms
// there, so that on the control-flow graph those values are dead through zsum<>, which has no room for
// them (a flag tested after the branches rejoin would keep them live through it).  The default does nothing.
struct NoAfterGeneral {
  __device__ __forceinline__ void operator()() const {}
};

template <int YB, int EXPV, int NZ = 0, bool FEEDOK = true, bool CARG = kClampArg, typename After = NoAfterGeneral>
__device__ __forceinline__ bool zsum_dispatch(const ZNode* __restrict__ zt, int nzp, const double* tab,
                                              const double (&c2)[YB], double (&F)[YB], int truncate = 0,
                                              const After& after_general = After()) {
  const int nz = NZ > 0 ? NZ : nzp;
  const double g_1 = zt[1].g4, g_max = zt[nz - 1].g4;
  bool dead[YB], small = true;
  double c2e[YB];
#pragma unroll
  for (int b = 0; b < YB; ++b) {
    dead[b] = c2[b] * g_1 <= -c2_scale<EXPV>() * 1077.0;
    c2e[b] = dead[b] ? 0.0 : c2[b];
    small = small && c2e[b] * g_max >= (double)kTabKMin;  // every node stays >= KMIN
  }
  int kend = nz;
  bool acc_only = false;
  if (truncate) {
    // largest per-lane threshold g_thr = -1080 N / c2 (live lanes; dead lanes impose none,
    // c2 = 0 lanes never underflow)
    double thr = 0.0;
#pragma unroll
    for (int b = 0; b < YB; ++b) {
      const double tb = dead[b] ? 0.0 : (c2e[b] < 0.0 ? (-1080.0 * c2_scale<EXPV>()) / c2e[b] : __builtin_inf());
      thr = pymax(thr, tb);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      if constexpr (kLean) thr = pymax(thr, shfl_xor_rederived(thr, off));
      else thr = pymax(thr, __shfl_xor(thr, off, kWaveSize));
    }
    thr = uniform(thr);
    // first k with g4_k > thr (g4 increasing): scalar binary search over the z table
    int lo = 0, hi = nz;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (zt[mid].g4 > thr) hi = mid;
      else lo = mid + 1;
    }
    kend = (lo + kKUnroll - 1) / kKUnroll * kKUnroll;
  }
  if constexpr (EXPV == kExpTable && kSqForm) {
    // Uniform-entry segments, decided per pass with the loop's own t = fma(c2, g, M) (lzq_exp2.h):
    //   every lane has t = M at g_max (small |c2|, or dead: c2e = 0): t = M at every node (g4 runs
    //     from >= 0 up to g_max, padding nodes repeat g_max), the whole pass reads T''[0] with
    //     nothing inserted and, with LZQ_ZERO_SEG, forms s from w = A without recomputing t; if
    //     every lane is dead as well (LZQ_DEAD_SEG), s = A too and the node is F's fma alone;
    //   else, on a pass that can clamp: from the first batch k2 at whose first node every lane
    //     has t <= M + KMIN, every lane reads the entry of M + KMIN (t only falls with k); the
    //     nodes before k2 run the clamped general loop.  A wave-uniform binary search.
    const double Mv = vgpr_const(kTabMagic);
    bool zero = true;
#pragma unroll
    for (int b = 0; b < YB; ++b) zero = zero && seg_zero(c2e[b], g_max, Mv);
    // every lane dead (tested first: dead lanes pass the zero test): the zero pass whose node value
    // is fixed as well (zsum_dead); a pass holding one live lane takes the paths below
    bool all_dead = LZQ_ZERO_SEG != 0 && LZQ_DEAD_SEG != 0;
#pragma unroll
    for (int b = 0; b < YB; ++b) all_dead = all_dead && dead[b];
    if (LZQ_ZERO_SEG != 0 && LZQ_DEAD_SEG != 0 && __all(all_dead)) {
      const double Ts0 = uniform(seg_entry(tab, zero_magic<(kFrozenSeg > 0)>(Mv)));
      if (kAccFeed && FEEDOK && !truncate) zsum_dead<YB, kAccFeed && FEEDOK>(zt, nz, Ts0, F, kend);
      else zsum_dead<YB>(zt, nz, Ts0, F, kend);
      acc_only = true;
    } else if (__all(zero)) {
      const double Ts0 = uniform(seg_entry(tab, zero_magic<(kFrozenSeg > 0)>(Mv)));
      if constexpr (kFrozenSeg >= 1) {
        // frozen s: from the first batch k3 at whose first node every lane's s equals its s at the
        // last executed node, v is a per-lane constant (s is monotone in g, g4 non-decreasing); the
        // nodes before k3 run the zero node, the rest F's accumulate alone.  k3 = 0: the whole pass
        const double Av = vgpr_const(kSqA);
        const double g_last = zt[kend > 0 ? kend - 1 : 0].g4;
        const int k3 = seg_first_batch(
            [&](double g) {
              bool c = true;
#pragma unroll
              for (int b = 0; b < YB; ++b) c = c && seg_frozen_s(c2e[b], g, g_last, Av);
              return __all(c) != 0;
            },
            [&](int k) { return zt[k].g4; }, kend, kKUnroll);
        acc_only = k3 == 0;
        zsum_uniform<YB, true>(zt, Ts0, c2e, F, k3, 0);
        if (k3 < kend) {
          double v[YB];
#pragma unroll
          for (int b = 0; b < YB; ++b) v[b] = seg_value_frozen_s(c2e[b], g_last, Av, Ts0);
          if (kAccFeed && FEEDOK && !truncate) zsum_held<YB, kAccFeed && FEEDOK>(zt, nz, v, F, kend, k3);
          else zsum_held<YB>(zt, nz, v, F, kend, k3);
        }
      } else {
        zsum_uniform<YB, LZQ_ZERO_SEG != 0>(zt, Ts0, c2e, F, kend, 0);
      }
    } else if (__all(small)) {
      if constexpr (kFrozenSeg >= 2) {
        // frozen t: from the first batch k3 at whose first node every lane's t equals its t at the
        // last executed node, the lookup and w are per-lane constants; the nodes before k3 run the
        // clamp-free general loop, the rest the four-operation node
        const double g_last = zt[kend > 0 ? kend - 1 : 0].g4;
        const int k3 = seg_first_batch(
            [&](double g) {
              bool c = true;
#pragma unroll
              for (int b = 0; b < YB; ++b) c = c && seg_frozen_t(c2e[b], g, g_last, Mv);
              return __all(c) != 0;
            },
            [&](int k) { return zt[k].g4; }, kend, kKUnroll);
        zsum<YB, EXPV, false>(zt, tab, c2e, F, k3);
        if (k3 < kend) {
          // (M pinned afresh: the copy above, kept live across the general loop, costs it a spill)
          const double Mt = vgpr_const(kTabMagic);
          double Tl[YB], wl[YB];
#pragma unroll
          for (int b = 0; b < YB; ++b) {
            const double tl = __builtin_fma(c2e[b], g_last, Mt);
            Tl[b] = seg_entry(tab, tl);  // per lane: the general path's address, load and insert
            wl[b] = seg_frozen_w(tl);
          }
          zsum_frozen_t<YB>(zt, Tl, wl, c2e, F, kend, k3);
        }
      } else {
        zsum<YB, EXPV, false>(zt, tab, c2e, F, kend);
      }
      after_general();
    } else {
      // Dead lanes among clamped ones (LZQ_PASS_LEAN): a dead lane (c2e = +0.0, t = M) never passes
      // seg_clamped, but its clamped magic sum is the constant M at every node.  So the search asks for
      // the first batch at which every LIVE lane is clamped (dead does not depend on k: still monotone;
      // without dead lanes it is the test it was), and from there a pass that holds dead lanes runs the
      // uniform node with each lane's own entry, the others with the one entry in SGPRs as before.
      if constexpr (kLean) {
        bool any_dead = false;
#pragma unroll
        for (int b = 0; b < YB; ++b) any_dead = any_dead || dead[b];
        const bool mixed = __any(any_dead) != 0;  // wave-uniform
        const int k2 = seg_first_batch(
            [&](double g) {
              bool c = true;
#pragma unroll
              for (int b = 0; b < YB; ++b) c = c && seg_clamped_or_dead(dead[b], c2e[b], g, Mv);
              return __all(c) != 0;
            },
            [&](int k) { return zt[k].g4; }, kend, kKUnroll);
        if (k2 > 0) zsum<YB, EXPV, true, CARG>(zt, tab, c2e, F, k2);
        if constexpr (CARG) {
          // The clamped argument (LZQ_CLAMP_ARG): from k2 on every live lane's node is evaluated at u = KMIN
          // (s = A) and a dead lane's s is A already, so each lane's node value is one number -- the entry
          // times fma(A, A, beta) -- and the suffix is F's accumulate alone, in node order, carrying F from
          // the prefix: zsum_dead's loop from k2 with v_c, or zsum_held with the value of each lane's own entry
          if (mixed) {
            const double Av = vgpr_const(kSqA);
            double v[YB];
#pragma unroll
            for (int b = 0; b < YB; ++b) v[b] = seg_node_dead(Av, seg_entry_lane(tab, dead[b]));
            if (kAccFeed && FEEDOK && !truncate) zsum_held<YB, kAccFeed && FEEDOK>(zt, nz, v, F, kend, k2);
            else zsum_held<YB>(zt, nz, v, F, kend, k2);
          } else {
            const double Tc = uniform(seg_entry(tab, kTabTClamp));
            if (kAccFeed && FEEDOK && !truncate) zsum_dead<YB, kAccFeed && FEEDOK>(zt, nz, Tc, F, kend, k2);
            else zsum_dead<YB>(zt, nz, Tc, F, kend, k2);
          }
        } else if (mixed) {
          double Tl[YB];
#pragma unroll
          for (int b = 0; b < YB; ++b) Tl[b] = seg_entry_lane(tab, dead[b]);
          zsum_uniform_lane<YB>(zt, Tl, c2e, F, kend, k2);
        } else {
          zsum_uniform<YB>(zt, uniform(seg_entry(tab, kTabTClamp)), c2e, F, kend, k2);
        }
      } else {
        const int k2 = seg_first_batch(
            [&](double g) {
              bool c = true;
#pragma unroll
              for (int b = 0; b < YB; ++b) c = c && seg_clamped(c2e[b], g, Mv);
              return __all(c) != 0;
            },
            [&](int k) { return zt[k].g4; }, kend, kKUnroll);
        if (k2 > 0) zsum<YB, EXPV, true>(zt, tab, c2e, F, k2);
        zsum_uniform<YB>(zt, uniform(seg_entry(tab, kTabTClamp)), c2e, F, kend, k2);
      }
      after_general();
    }
  } else if (EXPV == kExpTable && __all(small)) {
    zsum<YB, EXPV, false>(zt, tab, c2e, F, kend);
  } else {
    zsum<YB, EXPV, true>(zt, tab, c2e, F, kend);
  }
#pragma unroll
  for (int b = 0; b < YB; ++b) F[b] = dead[b] ? 0.0 : F[b];
  return acc_only;
}

// Stage the exp table (N doubles, see lzq_exp2.h) in LDS (every thread of the block must call this).
template <int EXPV>
__device__ __forceinline__ const double* stage_table(const double* __restrict__ gtab, double* lds) {
  if (EXPV != kExpTable) return nullptr;
  for (int i = threadIdx.x; i < kTabN; i += blockDim.x) lds[i] = gtab[i];
  __syncthreads();
  return lds;
}

// Fixed-order xor butterfly over the 64 lanes (every lane ends with the same sum).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWaveSize);
  return v;
}
// (LZQ_PASS_LEAN: the same butterfly through shfl_xor_rederived)
__device__ __forceinline__ double wave_sum_rederived(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += shfl_xor_rederived(v, off);
  return v;
}

// Lane index 0..63, re-derived where it is used (v_mbcnt; volatile, so it is not kept live).
__device__ __forceinline__ int lane_id() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// Grouped passes (LZQ_GROUP_SEG): up to G consecutive full, untruncated passes of yb_wave from y-node
// `base`, swept through z together where every one of them would run as F's accumulate alone from node 0.
//
// yb_group forms c2 of the passes exactly as the single pass does, classifies every lane and slot with
// the single pass's own rules (seg_group_slot, lzq_exp2.h) and runs the largest of G, G/2, .. 2 leading
// passes that fit the y-grid (`fit`: the full passes left from base, >= 2) and qualify.  The all-dead
// group is zsum_dead<g>, the other zsum_held<g> from node 0 with each slot's held value; a dead lane
// among live ones runs with c2e = +0.0 and is zeroed, as in zsum_dispatch: g chains per lane, each in
// node order from 0.  The g passes are then integrated in ascending pass order with the single pass's
// post-loop code (one unrolled copy per slot, shared by the group sizes: the code is what a launch
// fetches from HBM besides its 48 B per point).  Returns the number of passes run and integrated;
// 0: none qualifies, nothing was touched, and the caller runs the single pass.
//
// LEAN (LZQ_PASS_LEAN): y and e^y of the slots stay live from the classification to the integration --
// the accumulate-only loops have the room -- instead of being formed again, and a group whose G slots
// touch neither end of the y-grid (y_pass_interior on n_lin, lzq_ynode.h) forms y and the weight
// without the end-of-grid selects.
template <int G, int NZ, typename Win, bool LEAN, typename Slot>
__device__ __forceinline__ int yb_group(Slot* slots, int w, const ZNode* __restrict__ zt, int nzp, const double* tab,
                                        int base, int fit, int n_lin) {
  const int nz = NZ > 0 ? NZ : nzp;
  double c2g[G];
  [[maybe_unused]] double yk[G], ek[G];  // LEAN: y and e^y of the slots, kept across the sweep
  [[maybe_unused]] const bool interior = LEAN && y_pass_interior(base, G * kWaveSize, n_lin);
  int cls = 0;
  {
    const int lane = lane_id();
    int wo = w;
    asm volatile("" : "+s"(wo));
    const QuadSetup& s = slots[wo].s;
    const double g_0 = zt[0].g4, g_1 = zt[1].g4, g_last = zt[nz - 1].g4;
    const double Mv = vgpr_const(kTabMagic), Av = vgpr_const(kSqA);
#pragma unroll
    for (int b = 0; b < G; ++b) {
      // (a slot past `fit` is formed too -- y_node is arithmetic on j -- and never looked at)
      const int j = base + b * kWaveSize + lane;
      const double yv = interior ? y_node_interior(s.y_lo, s.step, j) : y_node(s, j);
      const double ey = exp_y<LEAN>(yv);                                     // fpy:161
      yk[b] = yv, ek[b] = ey;
      c2g[b] = ((s.cneg * ey) * kLog2E) * c2_scale<kExpTable>();             // fpy:163, as in yb_wave
      cls |= seg_group_slot(c2g[b], g_0, g_1, g_last, Mv, Av) << (2 * b);
    }
  }
  int ran = 0;
  bool all_dead = false;
  if constexpr (G >= 4) {
    if (fit >= 4) {
      const int k4 = seg_group_kind(cls, 4);
      all_dead = __all(k4 & kGrpDead) != 0;
      if (all_dead || __all(k4 & kGrpWhole) != 0) ran = 4;
    }
  }
  if (ran == 0) {
    const int k2 = seg_group_kind(cls, 2);
    all_dead = __all(k2 & kGrpDead) != 0;
    if (all_dead || __all(k2 & kGrpWhole) != 0) ran = 2;
  }
  if (ran == 0) return 0;
  double F[G];
  {
    const double Mv = vgpr_const(kTabMagic);
    const double Ts0 = uniform(seg_entry(tab, Mv));
    const double Av = vgpr_const(kSqA);
    const double g_last = zt[nz - 1].g4;
    double v[G] = {};
    if (!all_dead) {
#pragma unroll
      for (int b = 0; b < G; ++b)
        v[b] = seg_value_frozen_s(((cls >> (2 * b)) & kGrpDead) ? 0.0 : c2g[b], g_last, Av, Ts0);
    }
    if (G >= 4 && ran == 4) {
      if (all_dead) zsum_dead<G, kAccFeed>(zt, nz, Ts0, F, nz);
      else zsum_held<G, kAccFeed>(zt, nz, v, F, nz, 0);
    } else {
      double F2[2];
      const double v2[2] = {v[0], v[1]};
      if (all_dead) zsum_dead<2, kAccFeed>(zt, nz, Ts0, F2, nz);
      else zsum_held<2, kAccFeed>(zt, nz, v2, F2, nz, 0);
#pragma unroll
      for (int b = 0; b < G; ++b) F[b] = b < 2 ? F2[b] : 0.0;
    }
  }
  // (unrolled: rolled into one copy with F rotating down, the loop's hoisted constants spill)
#pragma unroll
  for (int b = 0; b < G; ++b) {
    if (b < ran) {
      const double Fb = ((cls >> (2 * b)) & kGrpDead) ? 0.0 : F[b];
      int wr = w;
      asm volatile("" : "+s"(wr));
      const int lane2 = lane_id();
      const QuadSetup& sr = slots[wr].s;
      const int j = base + b * kWaveSize + lane2;  // < n: the group's passes are full
      const double yv = LEAN ? yk[b] : y_node(sr, j);
      const double ey = LEAN ? ek[b] : exp_y<false>(yv);
      const double wt = interior ? y_weight_interior(sr.y_lo, sr.step, j, yv) : y_weight(sr, j, yv);
      const YFactors f =
          y_factors(slots[wr].s, yv, ey, wt, [&](double yy) { return win_eval<LEAN, Win>(slots[wr], yy); });
      slots[wr].acc[lane2] = __builtin_fma(f.w, integrand_from(f, Fb), slots[wr].acc[lane2]);
    }
  }
  return ran;
}

// Y_B of one point by one wavefront.  fpy:231-267
//
// Nothing but the z-loop's own state is held in registers across the z-loop (which needs ~60
// of the 64 VGPRs at 8 waves/SIMD):
//   * the point's QuadSetup lives in the wave's LDS slot (~44 SGPRs otherwise); each pass
//     re-reads the fields it needs with broadcast ds_reads, through a slot index made opaque
//     per pass so that the reads are not hoisted back out of the y-loop;
//   * y, e^y and the weight are re-formed after the z-loop (same operations, same bits) -- after
//     the table-lookup loop zsum<> only, in the dense mode (LZQ_PASS_LEAN): the other z-loops have
//     room for them, and a pass that ran zsum<> re-forms them on its own branch of zsum_dispatch;
//   * the lane's running sum over its y-nodes sits in the slot.
// Without this the kernel spilled ~200 B/lane to scratch around every z-loop.
// MODE (see lzq_sweep_grid_reuse): kYbDense computes every F(y_j) = sum_k omega_k 2^(c2_j g_k)
// itself (the headline); kYbTable computes them the same way and stores them to Fout instead of
// integrating; kYbReuse reads them from Fin (a table written by kYbTable for a point with the
// same y-grid and A/V kernel) and integrates.  The F values and the integration are the same
// operations in the same lane order in every mode, so Y_B is bit-identical.
enum YbMode { kYbDense = 0, kYbReuse = 1, kYbTable = 2 };

template <int YB, int EXPV, int MODE = kYbDense, int NZ = 0, typename Win = SlotGaussWindow, bool CARG = kClampArg,
          typename Slot>
__device__ double yb_wave(Slot* slots, int w, const ZNode* __restrict__ zt, int nzp, const double* tab, int truncate,
                          const double* __restrict__ Fin = nullptr, double* __restrict__ Fout = nullptr) {
  if (slots[w].s.empty) return 0.0;
  // y-node counts are int32 (n_y of the C ABI): 32-bit loop bounds save the SGPRs that
  // would otherwise spill around the z-loop
  const int n = (int)__builtin_bit_cast(int64_t, uniform(__builtin_bit_cast(double, slots[w].s.n)));  // SGPR
  const int per_pass = kWaveSize * YB;
  slots[w].acc[lane_id()] = 0.0;
  // grouped passes (LZQ_GROUP_SEG): the dense mode only -- the table and reuse modes are its controls.
  // grp (wave-uniform): the pass before ran as the accumulate alone from node 0, or this is the first;
  // only then is a group tried, so a point pays for a handful of classifications that fail
  constexpr bool kGroupHere = kGroupSeg >= 2 && MODE == kYbDense && EXPV == kExpTable && YB == 1 && kSqForm;
  // a window of the point's own (lzq_window.hip) groups two passes at most: with four, the F of the
  // passes still to be integrated and the window's evaluation do not fit the 64 VGPRs (4 spilled)
  constexpr int kGroupMax = __is_same(Win, SlotGaussWindow) ? kGroupSeg : (kGroupSeg < 2 ? kGroupSeg : 2);
  // the lean per-pass work (LZQ_PASS_LEAN): where the grouping is, and for its reason
  constexpr bool kLeanHere = kLean && kGroupHere;
  // n where the grid is (double)j * step + y_lo, 0 where numpy's step == 0 branch is taken: an SGPR
  [[maybe_unused]] const int n_lin = kLeanHere ? __builtin_amdgcn_readfirstlane(y_lin_count(slots[w].s.step, n)) : 0;
  [[maybe_unused]] bool grp = true;
  for (int base = 0; base < n; base += per_pass) {
    if constexpr (kGroupHere) {
      // under truncation kend differs from pass to pass and a dead pass is 8 nodes long: never grouped
      if (grp && !truncate) {
        int ran = 0;
        const int fit = (n - base) / kWaveSize;  // the full passes left
        if (fit >= 2) ran = yb_group<kGroupMax, NZ, Win, kLeanHere>(slots, w, zt, nzp, tab, base, fit, n_lin);
        if (ran) {
          base += (ran - 1) * per_pass;
          continue;
        }
        grp = false;
      }
    }
    // at most y, e^y and the weight stay live across the z-loop; the y-factors are formed after it
    double yv[YB], ey[YB], wt[YB];
    double F[YB];
    if constexpr (MODE == kYbReuse) {
      const int lane = lane_id();
#pragma unroll
      for (int b = 0; b < YB; ++b) {
        const int j = base + b * kWaveSize + lane;
        F[b] = Fin[j < n ? j : n - 1];
      }
    } else {
      const int lane = lane_id();
      int wo = w;
      asm volatile("" : "+s"(wo));
      const QuadSetup& s = slots[wo].s;
      double c2[YB];
      [[maybe_unused]] const bool interior = kLeanHere && y_pass_interior(base, per_pass, n_lin);
#pragma unroll
      for (int b = 0; b < YB; ++b) {
        const int j = base + b * kWaveSize + lane;
        // (the pass that re-forms the triple after the z-loop needs e^y alone here)
        if constexpr (kLeanHere) y_triple<true>(s, j, n, interior, yv[b], ey[b], wt[b]);
        else ey[b] = exp_y<false>(y_node(s, j < n ? j : n - 1));                // fpy:161
        c2[b] = ((s.cneg * ey[b]) * kLog2E) * c2_scale<EXPV>();                 // fpy:163 c, log2 units
      }
      if constexpr (kLeanHere) {
        // y, e^y and the weight stay live through the lean loops; a pass that ran the table-lookup loop
        // re-forms them on its own branch (zsum_dispatch's after_general), as every pass did before
        grp = zsum_dispatch<YB, EXPV, NZ, MODE == kYbDense, CARG>(zt, nzp, tab, c2, F, truncate, [&]() {
          int wa = w;
          asm volatile("" : "+s"(wa));
          const int la = lane_id();
#pragma unroll
          for (int b = 0; b < YB; ++b)
            y_triple<true>(slots[wa].s, base + b * kWaveSize + la, n, interior, yv[b], ey[b], wt[b]);
        });
      } else {
        grp = zsum_dispatch<YB, EXPV, NZ, MODE == kYbDense, CARG>(zt, nzp, tab, c2, F, truncate);
      }
      if constexpr (MODE == kYbTable) {
#pragma unroll
        for (int b = 0; b < YB; ++b) {
          const int j = base + b * kWaveSize + lane;
          if (j < n) Fout[j] = F[b];
        }
        continue;
      }
    }
    int wr = w;
    asm volatile("" : "+s"(wr));
    const int lane2 = lane_id();
    if constexpr (!kLeanHere) {
      // (y_triple<false> written out: with the weight formed before e^y the compiler schedules otherwise)
      const QuadSetup& sr = slots[wr].s;
#pragma unroll
      for (int b = 0; b < YB; ++b) {
        const int j = base + b * kWaveSize + lane2;
        const int jj = j < n ? j : n - 1;  // tail lanes recompute the last node with weight 0
        yv[b] = y_node(sr, jj);
        ey[b] = exp_y<false>(yv[b]);
        wt[b] = j < n ? y_weight(sr, jj, yv[b]) : 0.0;
      }
    }
    double acc = slots[wr].acc[lane2];
#pragma unroll
    for (int b = 0; b < YB; ++b) {
      const YFactors f =
          y_factors(slots[wr].s, yv[b], ey[b], wt[b], [&](double yy) { return win_eval<kLeanHere, Win>(slots[wr], yy); });
      acc = __builtin_fma(f.w, integrand_from(f, F[b]), acc);
    }
    slots[wr].acc[lane2] = acc;
  }
  if constexpr (kLeanHere) return wave_sum_rederived(slots[w].acc[lane_id()]);
  else return wave_sum(slots[w].acc[lane_id()]);
}

// fpy:372-384 (fast path) + fpy:413-417, split around the quadrature: epilogue_pre forms every
// field that does not depend on Y_B before the z-loops (so the point record need not stay live
// across them), epilogue_finish adds Y_B with the same operations and rounding order.
struct EpiPre {
  lzq_yield o;  // Y_chi, rho_DM_kg_m3, P_used set
  int valid;    // regime is thermal / nonthermal
};

__device__ __forceinline__ EpiPre epilogue_pre(const lzq_point& pt, double P) {
  const double T_p = pt.T_p_GeV;
  const double T_hi = pt.T_max_over_Tp * T_p;
  double Ychi;
  if (pt.regime == LZQ_THERMAL) {
    Ychi = n_chi_eq(T_hi, pt.m_chi_GeV, pt.g_chi, pt.stats) / s_entropy(T_hi, pt.g_star_s);
  } else if (pt.regime == LZQ_NONTHERMAL) {
    if (pt.has_Y_chi_init) Ychi = pt.Y_chi_init;
    else if (pt.has_n_chi_at_Tp) Ychi = pt.n_chi_at_Tp_GeV3 / pymax(s_entropy(T_p, pt.g_star_s), 1e-300);
    else Ychi = 1.0e-12;
  } else {
    Ychi = __builtin_nan("");  // reference: UnboundLocalError
  }
  EpiPre e;
  const double nDM0 = Ychi * kS0M3;
  e.o.Y_B = 0.0;
  e.o.rho_B_kg_m3 = 0.0;
  e.o.DM_over_B = 0.0;
  e.o.Y_chi = Ychi;
  e.o.rho_DM_kg_m3 = nDM0 * (pt.m_chi_GeV * kGeVToKg);
  e.o.P_used = P;
  e.valid = pt.regime == LZQ_THERMAL || pt.regime == LZQ_NONTHERMAL;
  return e;
}

__device__ __forceinline__ lzq_yield epilogue_finish(const EpiPre& e, double YB) {
  lzq_yield o = e.o;
  const double nB0 = YB * kS0M3;
  o.Y_B = YB;
  o.rho_B_kg_m3 = nB0 * kMProtonKg;
  o.DM_over_B = o.rho_DM_kg_m3 / pymax(o.rho_B_kg_m3, 1e-300);
  if (!e.valid) o.Y_B = o.rho_B_kg_m3 = o.rho_DM_kg_m3 = o.DM_over_B = __builtin_nan("");
  return o;
}

// Per-wave LDS slot of the quadrature kernels (one point per wavefront).
struct WaveSlot {
  QuadSetup s;
  EpiPre e;
  double acc[kWaveSize];  // per-lane running sums of yb_wave
};

// Park the (wave-uniform) setup and epilogue inputs in the wave's slot.  Lane 0 writes; LDS
// operations of one wavefront complete in order, the fence makes that formal for the compiler.
__device__ __forceinline__ void park(WaveSlot& slot, const QuadSetup& s, const EpiPre& e, int lane) {
  if (lane == 0) {
    slot.s = s;
    slot.e = e;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Quadrature of the parked point, then lane 0 stores its yields.  (CARG: LZQ_CLAMP_ARG for this kernel.)
template <int YB, int EXPV, int NZ, bool CARG = kClampArg>
__device__ __forceinline__ void point_yields(WaveSlot* slots, int w, const ZNode* __restrict__ zt, int nzp,
                                             const double* tab, int lane, int truncate, lzq_yield* out) {
  const double Y_B = yb_wave<YB, EXPV, kYbDense, NZ, SlotGaussWindow, CARG>(slots, w, zt, nzp, tab, truncate);
  if (lane == 0) *out = epilogue_finish(slots[w].e, Y_B);
}

// ---------------------------------------------------------------------------------------
// point sources
// ---------------------------------------------------------------------------------------
struct GridSpec {
  int32_t n_axes;
  int32_t field[LZQ_MAX_AXES];
  int64_t n[LZQ_MAX_AXES];
  int64_t stride[LZQ_MAX_AXES];
  const double* values[LZQ_MAX_AXES];
  int64_t tstride[LZQ_MAX_AXES];  // lzq_sweep_grid_reuse: stride in the z-sum table index (0: axis not in it)
};

__device__ __forceinline__ void set_field(lzq_point& p, int32_t f, double v, double& delta, double& m_mix,
                                          double& dprime) {
  switch (f) {  // explicit switch: a runtime-indexed store would push the struct to scratch
    case LZQ_F_M_CHI: p.m_chi_GeV = v; break;
    case LZQ_F_G_CHI: p.g_chi = v; break;
    case LZQ_F_T_P: p.T_p_GeV = v; break;
    case LZQ_F_BETA_OVER_H: p.beta_over_H = v; break;
    case LZQ_F_V_W: p.v_w = v; break;
    case LZQ_F_I_P: p.I_p = v; break;
    case LZQ_F_G_STAR: p.g_star = v; break;
    case LZQ_F_G_STAR_S: p.g_star_s = v; break;
    case LZQ_F_P: p.P_chi_to_B = v; break;
    case LZQ_F_SIGMA_Y: p.source_shape_sigma_y = v; break;
    case LZQ_F_FLUX: p.incident_flux_scale = v; break;
    case LZQ_F_T_MAX_OVER_TP: p.T_max_over_Tp = v; break;
    case LZQ_F_T_MIN_OVER_TP: p.T_min_over_Tp = v; break;
    case LZQ_F_Y_CHI_INIT: p.Y_chi_init = v; p.has_Y_chi_init = 1; break;
    case LZQ_F_N_CHI_AT_TP: p.n_chi_at_Tp_GeV3 = v; p.has_n_chi_at_Tp = 1; break;
    case LZQ_F_DELTA_LZ: delta = v; break;
    case LZQ_F_M_MIX: m_mix = v; break;
    case LZQ_F_DPRIME: dprime = v; break;
    default: break;
  }
}

// Materialise grid point `idx`; returns P after the LZ closed form if an LZ axis is swept.
__device__ __forceinline__ double grid_point(const lzq_point& base, const GridSpec& g, int64_t idx, lzq_point& p) {
  p = base;
  double delta = __builtin_nan(""), m_mix = __builtin_nan(""), dprime = __builtin_nan("");
  bool has_delta = false, has_mix = false;
  for (int a = 0; a < g.n_axes; ++a) {
    int64_t c = (idx / g.stride[a]) % g.n[a];
    double v = g.values[a][c];
    set_field(p, g.field[a], v, delta, m_mix, dprime);
    has_delta |= g.field[a] == LZQ_F_DELTA_LZ;
    has_mix |= g.field[a] == LZQ_F_M_MIX;
  }
  if (has_mix) delta = m_mix * m_mix / (2.0 * pymax(p.v_w, 1e-12) * fabs(dprime));  // PAPER eq.(8)
  if (has_mix || has_delta) p.P_chi_to_B = p_closed_form(delta);                     // fpy:183-184
  return p.P_chi_to_B;
}

// ---------------------------------------------------------------------------------------
// z-sum tables (lzq_sweep_grid_reuse; the kernels are lzq_kernels.hip's and lzq_cont.hip's)
// ---------------------------------------------------------------------------------------
constexpr int kTabHdr = 6;
static_assert(kTabHdr == LZQ_REUSE_TABLE_HEADER, "include/lzq.h");

// The z grid a table is made for, as its header stores it.
struct ZKey {
  double nz, z_max;
};

__device__ __forceinline__ int64_t table_of(const GridSpec& g, int64_t idx) {
  int64_t t = 0;
  for (int a = 0; a < g.n_axes; ++a) t += ((idx / g.stride[a]) % g.n[a]) * g.tstride[a];
  return t;
}

// flat grid index of table t's representative (every other axis at its first value)
__device__ __forceinline__ int64_t table_rep(const GridSpec& g, int64_t t) {
  int64_t idx = 0;
  for (int a = 0; a < g.n_axes; ++a)
    if (g.tstride[a]) idx += ((t / g.tstride[a]) % g.n[a]) * g.stride[a];
  return idx;
}

}  // namespace lzq
