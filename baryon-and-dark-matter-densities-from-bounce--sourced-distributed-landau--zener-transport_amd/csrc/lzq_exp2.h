// lzq_exp2.h -- the FP64 exponential of the KJMA inner loop (fpy:163), CDNA4 form.
//
// The reference evaluates, per (y, z_k) node, exp(c * g4_k) with c = -(I_p/6) e^y <= 0
// (fpy:163).  The kernel evaluates the same quantity as 2^(c2 * g4_k) with c2 = c*log2(e)
// rounded once per y-node (not per z-node), in 17 FP64 VALU issue slots per node instead
// of the ~23 of the generic ROCm exp(double):
//
//   u  = c2*g            v_mul_f64
//   kd = rint(u)         v_rndne_f64
//   r  = fma(c2,g,-kd)   v_fma_f64     r in [-1/2, 1/2], one rounding
//   k  = (int)kd         v_cvt_i32_f64 saturating: |u| >= 2^31 gives INT_MIN -> result 0
//   p  = 1 + r*q(r)      11 x v_fma_f64, degree-11 minimax (tools/exp2_poly.py): 0.63 ulp
//   2^u = ldexp(p, k)    v_ldexp_f64   exact scaling, gradual underflow to 0 like libm
//
// No overflow / NaN / positive-argument handling is needed: g4_k >= 0 (checked when the
// table is built) and c2 < 0, so u <= 0.  For |u| >= 2^52 the reduction is meaningless
// but p stays finite (|r| < 2^30) and ldexp(p, INT_MIN) is 0, the exact answer.
// Accuracy vs the libm exp of the oracle: the rounding of c2 costs |u|*2^-53 relative,
// i.e. < 1e-13 even where u ~ -1000 (and those nodes are ~1e-300 of the sum).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LZQ_HD __host__ __device__ __forceinline__
#else
#define LZQ_HD static inline
#endif

namespace lzq {

// 2^r = 1 + r*(A1 + r*(A2 + ... + r*A11)) on [-1/2, 1/2]; tools/exp2_poly.py 11
constexpr double kExp2A1 = 0x1.62e42fefa39efp-1;
constexpr double kExp2A2 = 0x1.ebfbdff82c5a4p-3;
constexpr double kExp2A3 = 0x1.c6b08d7049fe8p-5;
constexpr double kExp2A4 = 0x1.3b2ab6fba0119p-7;
constexpr double kExp2A5 = 0x1.5d87fe78cd6d4p-10;
constexpr double kExp2A6 = 0x1.4309130ed8da0p-13;
constexpr double kExp2A7 = 0x1.ffcbfba97fab8p-17;
constexpr double kExp2A8 = 0x1.62bfc79d2fa58p-20;
constexpr double kExp2A9 = 0x1.b5267ce2583c7p-24;
constexpr double kExp2A10 = 0x1.e61b4fc4ab239p-28;
constexpr double kExp2A11 = 0x1.e79bb37875897p-32;
constexpr double kLog2E = 0x1.71547652b82fep0;  // log2(e) rounded to nearest

// fma(a, b, c) with the addend c in an SGPR pair: one VOP3 v_fma_f64 on the device.  Left to
// itself the compiler keeps Horner coefficients in VGPRs (hoisted out of loops: 2 VGPRs each)
// and emits v_mov_b64 + v_fmac_f64 (addend = destination) per step, 2 VALU instead of 1.
LZQ_HD double fma_vvs(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
  return r;
#else
  return __builtin_fma(a, b, c);
#endif
}

LZQ_HD double exp2_poly(double r) {
  double q = __builtin_fma(r, kExp2A11, kExp2A10);
  q = __builtin_fma(r, q, kExp2A9);
  q = __builtin_fma(r, q, kExp2A8);
  q = __builtin_fma(r, q, kExp2A7);
  q = __builtin_fma(r, q, kExp2A6);
  q = __builtin_fma(r, q, kExp2A5);
  q = __builtin_fma(r, q, kExp2A4);
  q = __builtin_fma(r, q, kExp2A3);
  q = __builtin_fma(r, q, kExp2A2);
  q = __builtin_fma(r, q, kExp2A1);
  return __builtin_fma(r, q, 1.0);
}

// Saturating double -> int32 (v_cvt_i32_f64 semantics: out-of-range clamps, NaN -> 0).
LZQ_HD int32_t cvt_i32_sat(double kd) {
#if defined(__HIP_DEVICE_COMPILE__)
  int32_t k;
  asm("v_cvt_i32_f64 %0, %1" : "=v"(k) : "v"(kd));
  return k;
#else
  if (kd != kd) return 0;
  if (kd <= -2147483648.0) return INT32_MIN;
  if (kd >= 2147483647.0) return INT32_MAX;
  return (int32_t)kd;
#endif
}

// 2^(c2*g + bias) for c2*g <= 0 (see header comment); bias = kOmegaBias when the caller's
// weights are the scaled omega' = omega * 2^-512 of the z table.
LZQ_HD double exp2_nonpos(double c2, double g, int32_t bias = 0) {
  double u = c2 * g;
  double kd = __builtin_rint(u);
  double r = __builtin_fma(c2, g, -kd);
  int32_t k = cvt_i32_sat(kd);  // INT_MIN + bias stays hugely negative -> 0
  return __builtin_ldexp(exp2_poly(r), k + bias);
}

// ---------------------------------------------------------------------------------------
// Table-driven variant (default).  2^(u/N) for u = c2N*g <= 0 (u in 1/N-octave units):
//   u = N e + j + r,  k = N e + j = round(u),  |r| <= 1/2,
//   2^(u/N) = 2^e * T[j] * (1 + q(r)),  T[j] = 2^(j/N),  q(r) = r*(B1 + r*(B2 + ...)),
// q a minimax polynomial of degree LZQ_POLYDEG in r (tools/exp2_tab_poly.py; absolute error
// |dq| of q is the relative error of T*(1+q)).  The kernel (lzq_kernels.hip, zsum) never
// forms 2^e with ldexp: the LDS table stores T'[j] with its high word pre-biased so that ONE
// integer add of (k << S), S = 20 - BITS, gives T[j] * 2^(e + 512) (tab_scale), and the z
// table's weights carry the compensating 2^-512 (kOmegaBias).  k is clamped to
// KMIN = -1534 N so that e + 512 >= -1022 keeps that product a normal double.
//
//   BITS DEG  LDS/block  |dq| (minimax)     VALU/node  C2 points/s (1 GPU)
//     8   4     2 KB     1.9e-17 (0.1 ulp)   12.5       3.17e5  (round-1 kernel: ldexp path)
//    12   2    32 KB     2.5e-14 (114 ulp)   11.4       3.54e5  (ldexp path, 2-op address)
//    13   2    64 KB     3.2e-15 (14 ulp)    10         4.64e5  (LZQ_SQFORM=0)
//    13   2sq  64 KB     1.73e-14 (78 ulp)   9          5.25e5  (default: completed square, below)
// The 13-bit address is ONE v_lshlrev_b16 ((k << 3) mod 2^16 = 8*(k mod 8192)).  The default's
// 1.73e-14 bound moves Y_B by at most that much (relative), 6e5 x inside the north_star 1e-8
// gate; tests/test_exp2_host.py pins every row against mpmath on the host, and
// tests/test_gpu_zsum.py the device's sums F and A/V (LDS table, SDWA address, exponent insert)
// against a 60-digit sum with a tolerance built on that bound.
#ifndef LZQ_TABBITS
#define LZQ_TABBITS 13
#endif
#ifndef LZQ_POLYDEG
#define LZQ_POLYDEG 2
#endif

template <int BITS, int DEG>
struct TabPoly;  // coefficients B1..B_DEG of 2^(r/2^BITS) - 1 ~= r*(B1 + r*(B2 + ...))
template <>
struct TabPoly<8, 4> {  // Taylor: (ln2/256)^i / i!
  static constexpr double B[4] = {0x1.62e42fefa39efp-9, 0x1.ebfbdff82c58fp-19, 0x1.c6b08d704a0c0p-29,
                                  0x1.3b2ab6fba4e77p-39};
};
template <>
struct TabPoly<10, 3> {
  static constexpr double B[3] = {0x1.62e42fefa39efp-11, 0x1.ebfbe03972542p-23, 0x1.c6b08dae13771p-35};
};
template <>
struct TabPoly<12, 2> {
  static constexpr double B[2] = {0x1.62e42ff4f7b0ap-13, 0x1.ebfbdffcafed4p-27};
};
template <>
struct TabPoly<12, 3> {
  static constexpr double B[3] = {0x1.62e42fefa39efp-13, 0x1.ebfbdffc40b8ap-27, 0x1.c6b08d7426a2bp-41};
};
template <>
struct TabPoly<13, 2> {
  static constexpr double B[2] = {0x1.62e42ff0f8a36p-14, 0x1.ebfbdff94d3e0p-29};
};
template <>
struct TabPoly<14, 2> {
  static constexpr double B[2] = {0x1.62e42feff8e01p-15, 0x1.ebfbdff874923p-31};
};
template <>
struct TabPoly<14, 3> {
  static constexpr double B[3] = {0x1.62e42fefa39efp-15, 0x1.ebfbdff86d9eep-31, 0x1.c6b08d7087d56p-47};
};

// Completed-square form of the degree-2 step (LZQ_SQFORM, default on for 13 bits / degree 2):
//   2^(r/N) ~= C * ((r + A)^2 + beta),  A an INTEGER,
// so that s = r + A comes out of the reduction at no extra cost (w = (M + A) - t is exact
// because M + A is, then s = fma(c2N, g, w) rounds once), the polynomial is ONE fma
// q = fma(s, s, beta), and C is folded into the table, T''[j] = C * 2^(j/N).  The node is then
//   t, w, s, address, exponent insert, q, v = T'' * q, F += omega' * v  = 8 VALU (was 9).
// A = N/ln2 would be Taylor's centre (11818.47); the nearest integers cost accuracy: the
// minimax (C, beta) at A = 11819 leaves |2^(r/N) - p(r)| <= 1.73e-14 relative on [-1/2, 1/2]
// (A = 11818: 2.16e-14) -- 6e5 x inside the north_star 1e-8 gate (tests/test_exp2_host.py
// pins it against mpmath).  C ~ 2^-27.06 lowers the table's exponents by 28, so KMIN is
// -1506 N (e + 512 - 28 >= -1022 keeps T''*2^(e+512) normal); those clamped nodes still
// contribute omega*2^u with u < -1506 octaves, which rounds away exactly (clamp onset sampled
// densely against mpmath in tests/test_gpu_zsum.py; a clamp constant that leaves the normal range
// is one of the defects tests/test_zsum_host.py shows that comparison to reject).
#ifndef LZQ_SQFORM
#define LZQ_SQFORM 1
#endif

constexpr int kTabBits = LZQ_TABBITS;
constexpr int kTabN = 1 << kTabBits;
constexpr int kPolyDeg = LZQ_POLYDEG;
constexpr bool kSqForm = LZQ_SQFORM && kTabBits == 13 && kPolyDeg == 2;
constexpr double kSqA = 11819.0;
constexpr double kSqBeta = 139678307.60123383601;  // tools/exp2_tab_poly.py --sq 11819
constexpr long double kSqC = 3.5795199663544010274e-9L;
constexpr int kTabShift = 20 - kTabBits;          // (k << S) = (e << 20) + (j << S)
constexpr int32_t kOmegaBias = 512;               // T' carries 2^512, omega' carries 2^-512
constexpr int32_t kTabKMin = (kSqForm ? -1506 : -1534) * kTabN;  // T'*2^(e+512) stays normal
static_assert(kTabBits >= 8 && kTabBits <= 16, "table bits");
static_assert((int64_t)kTabKMin * (1 << kTabShift) >= INT32_MIN, "k << S must not overflow");

// q(r) = r*(B1 + r*(B2 + ...)): DEG-1 fma + 1 mul, coefficients passed in (so that a caller
// can hold B1 in a VGPR across its loop: a VOP3 op reads at most one SGPR on gfx950, and the
// compiler otherwise re-materialises the copy every iteration)
template <int DEG>
LZQ_HD double tab_q_with(double r, const double (&B)[DEG]) {
  double acc = B[DEG - 1];
#pragma unroll
  for (int i = DEG - 2; i >= 0; --i) acc = __builtin_fma(r, acc, B[i]);
  return r * acc;
}

// Exact value of table entry j before its one rounding (host side): 2^(j/N), times C in the
// completed-square form.
static inline long double tab_exact(int32_t j) {
  const long double T = exp2l((long double)j / (long double)kTabN);
  return kSqForm ? T * kSqC : T;
}

// Table entry j as stored (host side): tab_exact(j) rounded once, high word pre-biased by
// (512 << 20) - (j << S) (mod 2^32).
static inline uint64_t tab_entry_bits(long double T_exact, int32_t j) {
  const uint64_t b = __builtin_bit_cast(uint64_t, (double)T_exact);
  const uint32_t hi = (uint32_t)(b >> 32) + ((uint32_t)kOmegaBias << 20) - ((uint32_t)j << kTabShift);
  return ((uint64_t)hi << 32) | (b & 0xffffffffu);
}

// LDS byte address of entry (k mod N) from the low word k of the clamped magic sum.
LZQ_HD uint32_t tab_byte_addr(uint32_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (kTabBits == 13) {
    uint32_t a;  // 16-bit shift, upper half zeroed: (k << 3) & 0xffff = 8 * (k & 8191)
    asm("v_lshlrev_b16_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
        : "=v"(a) : "v"(k));
    return a;
  }
#endif
  return (k & (uint32_t)(kTabN - 1)) << 3;
}

// T'[j] with its high word advanced by k << S:  T[j] * 2^(e + 512).
// (written on a 2 x u32 vector so that the compiler emits one v_lshl_add_u32 on the high
// VGPR of the pair, not a 64-bit add)
typedef uint32_t lzq_u32x2 __attribute__((vector_size(8)));
LZQ_HD double tab_scale(double Tp, uint32_t k) {
  lzq_u32x2 w = __builtin_bit_cast(lzq_u32x2, Tp);
  w[1] = w[1] + (k << kTabShift);
  return __builtin_bit_cast(double, w);
}

// Host/device reference of one table-variant node: returns 2^(u/N) * 2^512 exactly as the
// kernel forms it (the kernel multiplies by omega' = omega * 2^-512 inside its accumulate).
// tabp = table as stored (tab_entry_bits).  c2N*g <= 0, |c2N*g| < 2^51.
LZQ_HD double exp2_tab_scaled(double c2N, double g, const double* tabp) {
  constexpr double kMagic = 0x1.8p52;
  const double t = __builtin_fma(c2N, g, kMagic);
  const double tc = __builtin_fmax(t, kMagic + (double)kTabKMin);
  const uint32_t k = (uint32_t)__builtin_bit_cast(uint64_t, tc);
  const double Ts = tab_scale(tabp[tab_byte_addr(k) >> 3], k);
  if constexpr (kSqForm) {
    const double s = __builtin_fma(c2N, g, (kMagic + kSqA) - t);  // r + A, one rounding
    return Ts * __builtin_fma(s, s, kSqBeta);
  }
  const double kd = t - kMagic;
  const double r = __builtin_fma(c2N, g, -kd);
  const double q = tab_q_with<kPolyDeg>(r, TabPoly<kTabBits, kPolyDeg>::B);
  return __builtin_fma(Ts, q, Ts);
}

// ---------------------------------------------------------------------------------------
// Uniform-entry segments of a z-sum pass (zsum_dispatch in lzq_quad.h calls these; the host
// test tests/zsum_segments_host.cpp compiles the same source).  g4 is non-decreasing over the
// grid and starts at >= 0, so t_k = fma(c2N, g4_k, M) moves one way with k, and two stretches of
// a pass read ONE table entry at every node:
//   zero:    t at g_max equals M  ->  t_k = M at every node (round(u) = 0: the entry T''[0], the
//            insert adds 0), with or without the clamp;
//   clamped: t_k <= M + KMIN      ->  max(t_k, M + KMIN) = M + KMIN from node k on.
// Both tests evaluate the loop's own expression, so they are exact.  When every lane of a wave
// passes one, the node's lookup (address, LDS read, exponent insert, and the max) returns the
// value of the node before: seg_entry fetches it once, seg_node is the rest of the node.
// On a zero stretch the range reduction is known as well: t_k = M at every node, so the node's
// w = (M + A) - t_k is (M + A) - M = A exactly (both integers below 2^53), and s = fma(c2N, g, w)
// is fma(c2N, g, A) -- seg_node_zero forms s from that operand directly and drops t and w; the
// rest of the node (q, v) is seg_node's, so the bits are.  (The invariant is the zero test's:
// t_k = M  =>  w = A.  It does not hold on the clamped stretch, whose unclamped t still moves.)
// A dead lane runs the zero stretch with c2N = +0.0, and then s = fma(+0 * g, A) = A whatever g is:
// q and v are fixed too, seg_node_dead forms them without c2N or g, and only F's accumulate is left
// per node (lzq_quad.h runs it that way where all 64 lanes are dead).
constexpr double kTabMagic = 0x1.8p52;
constexpr double kTabTClamp = kTabMagic + (double)kTabKMin;  // exact

// (Mv = kTabMagic here and in seg_node: a parameter so that the device can pin it in a VGPR where
// it is used, instead of the compiler keeping a copy live across the y-loop)
LZQ_HD bool seg_zero(double c2N, double g_max, double Mv) { return __builtin_fma(c2N, g_max, Mv) == kTabMagic; }
LZQ_HD bool seg_clamped(double c2N, double g, double Mv) { return __builtin_fma(c2N, g, Mv) <= kTabTClamp; }

// the scaled table value every node of a segment with the constant (clamped) magic sum tc reads:
// the general path's address, load and insert, so its bits
LZQ_HD double seg_entry(const double* tabp, double tc) {
  const uint32_t k = (uint32_t)__builtin_bit_cast(uint64_t, tc);
  return tab_scale(tabp[tab_byte_addr(k) >> 3], k);
}

// one node of a uniform-entry segment (completed-square form): v = Ts * ((r + A)^2 + beta), the
// operands and operations of exp2_tab_scaled with Ts given.
LZQ_HD double seg_node(double c2N, double g, double Mv, double Ts) {
  const double t = __builtin_fma(c2N, g, Mv);
  const double s = __builtin_fma(c2N, g, (kTabMagic + kSqA) - t);  // the unclamped t, as in the general node
  return Ts * __builtin_fma(s, s, kSqBeta);
}

// one node of a zero stretch (seg_zero held for this lane at g_max, 0 <= g <= g_max): seg_node with
// t = M and w = A known, i.e. its s, q and v on the same operands.  (Av = kSqA: a parameter so that
// the device can pin it in a VGPR, as Mv above.)
LZQ_HD double seg_node_zero(double c2N, double g, double Av, double Ts) {
  const double s = __builtin_fma(c2N, g, Av);
  return Ts * __builtin_fma(s, s, kSqBeta);
}

// one node of a zero stretch on a dead lane, whose c2N is the literal +0.0 (zsum_dispatch's c2e):
// s = fma(+0 * g, A) is A exactly for every finite g >= 0, so the node is seg_node_zero(0.0, g, A, Ts)
// whatever g is -- one value for the whole pass, formed once.  Only for that +0.0: a c2N of -0.0 or a
// subnormal also leaves s = A, but the dispatch never hands one over as "dead", and any c2N whose
// product with g can reach half an ulp of A does move s.  (Av = kSqA, as in seg_node_zero.  beta is
// handed over as the fma's scalar operand: it is one already, in the loops of the other paths, and
// a VGPR copy of it was kept live across the y-loop, at the cost of a spill.)
LZQ_HD double seg_node_dead(double Av, double Ts) { return Ts * fma_vvs(Av, Av, kSqBeta); }

// A clamped pass that holds dead lanes (LZQ_PASS_LEAN; zsum_dispatch's last branch, zsum_uniform_lane in
// lzq_quad.h).  A dead lane runs with c2N = +0.0: t = M at every node, so it never passes seg_clamped,
// and its clamped magic sum max(M, M + KMIN) is the constant M.  From the first node at which every
// live lane is clamped, every lane reads one entry of its own at every node -- the uniform-entry
// argument with the entry held per lane: T''[0] with nothing inserted for a dead lane (seg_entry on
// M), the entry of M + KMIN for the others.  `dead` does not depend on the node, so the test stays
// monotone in k.
LZQ_HD bool seg_clamped_or_dead(bool dead, double c2N, double g, double Mv) { return dead || seg_clamped(c2N, g, Mv); }
LZQ_HD double seg_entry_lane(const double* tabp, bool dead) { return seg_entry(tabp, dead ? kTabMagic : kTabTClamp); }

// The clamped argument (LZQ_CLAMP_ARG, lzq_quad.h).  The max above clamps the magic sum, that is the table
// index; exp2_tab_scaled's s still comes from the unclamped t, so an underflowed node's stand-in value is
// T''(KMIN) * ((r_k + A)^2 + beta) with a fractional part r_k that moves at every node and does no work: the
// node's term omega' * v ~ omega * 2^-1506 is discarded by the accumulate's rounding whatever r_k is.  With
// the argument itself clamped, a node with t <= M + KMIN is evaluated AT u = KMIN: r = 0, s = A, and its
// value is the one number
//   v_c = T''(KMIN) * fma(A, A, beta) = seg_node_dead(A, seg_entry(tab, M + KMIN))
// (clamp_arg_s: a select on the comparison the max already makes; exp2_tab_scaled_clamp_arg: the general
// clamped node with it; a node above the clamp keeps exp2_tab_scaled's bits).  t only falls with k, so from
// the first node at which every live lane is clamped the node value is fixed by the pass test and the rest
// of the pass is F's accumulate alone (zsum_dispatch's clamped branch).  A dead lane (c2N = +0.0, t = M)
// is never clamped and keeps its s = fma(+0 * g, A) = A: seg_node_dead on T''[0], as before.
//
// F's bits do not move: either stand-in's term is below half the smallest subnormal, omega'_k v_c < 2^-1075,
// so fma(omega'_k, v, F) returns F whether F is +0, subnormal or normal.  That bound is a condition on the
// grid's weights; clamp_arg_rounds_away states it and every producer of a grid checks it on the host.
//
// The select is a compare and two v_cndmask_b32 on the halves of s, in place: three VALU per node.  A's low
// word is 0, an inline constant; its high word a_hi is handed over by the caller, which on the device holds it
// in a VGPR filled once per loop (clamp_arg_hi: opaque, so that the compiler neither hoists it out of the
// y-loop, where it is one register more than the kernel has, nor re-forms it per node).
constexpr uint32_t kSqAHi = (uint32_t)(__builtin_bit_cast(uint64_t, kSqA) >> 32);
static_assert((uint32_t)__builtin_bit_cast(uint64_t, kSqA) == 0u, "A's low word is 0");
LZQ_HD uint32_t clamp_arg_hi() {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t a;
  asm volatile("v_mov_b32 %0, %1" : "=v"(a) : "i"(kSqAHi));
  return a;
#else
  return kSqAHi;
#endif
}
LZQ_HD double clamp_arg_s(double t, double s, uint32_t a_hi = kSqAHi) {
  const bool clamped = t <= kTabTClamp;
  lzq_u32x2 w = __builtin_bit_cast(lzq_u32x2, s);
  w[0] = clamped ? 0u : w[0];
  w[1] = clamped ? a_hi : w[1];
  return __builtin_bit_cast(double, w);
}
LZQ_HD double exp2_tab_scaled_clamp_arg(double c2N, double g, const double* tabp) {
  const double t = __builtin_fma(c2N, g, kTabMagic);
  const double tc = __builtin_fmax(t, kTabTClamp);
  const uint32_t k = (uint32_t)__builtin_bit_cast(uint64_t, tc);
  const double Ts = tab_scale(tabp[tab_byte_addr(k) >> 3], k);
  const double s = clamp_arg_s(t, __builtin_fma(c2N, g, (kTabMagic + kSqA) - t));
  return Ts * __builtin_fma(s, s, kSqBeta);
}
// v_c on the host, from the one entry it reads (KMIN is a whole number of octaves: entry 0)
static_assert(kTabKMin % kTabN == 0, "the clamp constant reads entry 0");
static inline double clamp_arg_value() {
  const double T0 = __builtin_bit_cast(double, tab_entry_bits(tab_exact(0), 0));
  return seg_node_dead(kSqA, seg_entry(&T0, kTabTClamp));
}
// whether omega' * v_c < 2^-1075 for a scaled weight omega' = omega * 2^-512 >= 0, decided on the binary
// exponents (omega' < 2^(a+1) and v_c < 2^(b+1), so the product is below 2^(a+b+2)): no product is formed
static inline bool clamp_arg_rounds_away(double omega_scaled, double v_c) {
  if (!(omega_scaled > 0.0)) return omega_scaled == 0.0;
  if (!(omega_scaled <= 0x1.fffffffffffffp1023) || !(v_c > 0.0)) return false;
  return ilogb(omega_scaled) + ilogb(v_c) + 2 <= -1075;
}
template <class Omega>
static inline bool clamp_arg_grid_ok(Omega omega_scaled, int n) {
  const double v_c = clamp_arg_value();
  for (int k = 0; k < n; ++k)
    if (!clamp_arg_rounds_away(omega_scaled(k), v_c)) return false;
  return true;
}

// Frozen stretches.  gamma4 saturates, so g4_k moves ever less with k, and a lane's rounded
// intermediate -- s = fma(c2N, g, A) on a zero pass, t = fma(c2N, g, M) on a clamp-free one -- stops
// changing long before the pass ends (on small |c2N| it never changes).  Both are correctly rounded
// and monotone in g for either sign of c2N, and g4 is non-decreasing up to the last executed node
// g_last, so a lane whose value at g equals its value at g_last holds that value at every node in
// between.  The tests evaluate the loop's own expression, so they are exact:
//   frozen s (zero pass):  s, q = fma(s, s, beta) and v = T''[0] * q are per-lane constants from that
//            node on -- seg_node_zero at g_last is their value, and a node is F's accumulate alone;
//   frozen t (clamp-free pass):  t is, and with it the lookup (address, read, insert: seg_entry at
//            that t) and w = (M + A) - t (seg_frozen_w); seg_node_frozen is the rest of the node, the
//            general node's s, q and v on the same operands.
LZQ_HD bool seg_frozen_s(double c2N, double g, double g_last, double Av) {
  return __builtin_fma(c2N, g, Av) == __builtin_fma(c2N, g_last, Av);
}
LZQ_HD bool seg_frozen_t(double c2N, double g, double g_last, double Mv) {
  return __builtin_fma(c2N, g, Mv) == __builtin_fma(c2N, g_last, Mv);
}
// a lane's held value on a frozen-s stretch: seg_node_zero at g_last, its instructions on its operands.
// (beta is handed over as the fma's scalar operand, as in seg_node_dead and for its reason: formed
// once per pass, a VGPR copy of beta was kept live across the y-loop and spilled.)
LZQ_HD double seg_value_frozen_s(double c2N, double g_last, double Av, double Ts) {
  const double s = __builtin_fma(c2N, g_last, Av);
  return Ts * fma_vvs(s, s, kSqBeta);
}
LZQ_HD double seg_frozen_w(double t) { return (kTabMagic + kSqA) - t; }  // exact, as in the general node
LZQ_HD double seg_node_frozen(double c2N, double g, double w, double Ts) {
  const double s = __builtin_fma(c2N, g, w);
  return Ts * __builtin_fma(s, s, kSqBeta);
}

// Grouped passes (LZQ_GROUP_SEG; yb_group in lzq_quad.h).  A pass whose every node is F's accumulate
// alone from node 0 -- all 64 lanes dead (zsum_dead), or a zero pass with k3 = 0 (zsum_held from the
// first node) -- can share its sweep through z with its neighbours of the same kind.  seg_group_slot
// classifies one lane of one untruncated pass with the single pass's own rules (g_0, g_1, g_last: g4 of
// nodes 0, 1 and nz - 1, the last executed node, which is g_max):
//   kGrpDead   the dispatch's dead rule, c2N g4_1 <= -N * 1077;
//   kGrpWhole  with c2e = +0.0 on a dead lane as in the dispatch: the zero test at g_max and s frozen
//              at the FIRST node, which is what makes the batch search return k3 = 0 (the predicate is
//              monotone in k).  A dead lane passes both, so kGrpDead implies kGrpWhole.
// seg_group_kind combines a lane's slots: the bits every one of its first g slots has.  A wave runs the
// group as all-dead if every lane has kGrpDead, else as held if every lane has kGrpWhole, else not at all.
constexpr int kGrpDead = 1, kGrpWhole = 2;
constexpr double kDeadOctaves = 1077.0;  // zsum_dispatch's dead rule
LZQ_HD int seg_group_slot(double c2N, double g_0, double g_1, double g_last, double Mv, double Av) {
  const bool dead = c2N * g_1 <= -(double)kTabN * kDeadOctaves;
  const double c2e = dead ? 0.0 : c2N;
  const bool whole = seg_zero(c2e, g_last, Mv) && seg_frozen_s(c2e, g_0, g_last, Av);
  return (dead ? kGrpDead : 0) | (whole ? kGrpWhole : 0);
}
// the classes of up to four slots packed two bits each (slot b in bits 2b, 2b + 1): AND over slots 0..g-1
LZQ_HD int seg_group_kind(int packed, int g) {
  int m = kGrpDead | kGrpWhole;
  for (int b = 0; b < g; ++b) m &= packed >> (2 * b);
  return m;
}

// The packed omega' array of a z grid's device image (LZQ_ACC_FEED; lzq_quad.h's zsum_dead and zsum_held
// read it).  The image of a grid of nzp padded nodes is nzp {g4, omega'} pairs, then the same nzp weights
// once more as contiguous doubles: a loop that needs omega' alone touches one 64-byte line per 8-node
// batch there, not the two of the interleaved pairs.  One layout for every producer (the default grid,
// whose exp table follows the packed array; a runtime grid; the continuum grid), so the array sits at a
// fixed place seen from the nodes and no kernel takes an argument for it.  zimage_doubles: the image's
// size; zimage_pack: fills the packed part from the nodes, the weights' own bits, padding +0 included.
LZQ_HD int zimage_doubles(int nzp) { return 3 * nzp; }
LZQ_HD const double* zimage_omega(const void* nodes, int nzp) { return static_cast<const double*>(nodes) + 2 * nzp; }
template <class Node>
static inline void zimage_pack(Node* nodes, int nzp) {
  double* packed = reinterpret_cast<double*>(nodes) + 2 * nzp;
  for (int k = 0; k < nzp; ++k) packed[k] = nodes[k].omega;
}

// First node k2 in [0, kend], a multiple of `unroll` (which divides kend), with pred(g4(k2)); pred
// must be monotone in k (false ... false true ... true); kend if it holds at no batch start.
template <class Pred, class G4>
LZQ_HD int seg_first_batch(Pred pred, G4 g4, int kend, int unroll) {
  int lo = 0, hi = kend / unroll;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pred(g4(mid * unroll))) hi = mid;
    else lo = mid + 1;
  }
  return lo * unroll;
}

}  // namespace lzq
