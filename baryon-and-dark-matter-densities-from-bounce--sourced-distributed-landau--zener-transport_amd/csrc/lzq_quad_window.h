// lzq_quad_window.h -- device helpers of the quadrature kernels whose window W(y) is a per-point
// block (lzq_window.h), shared by the translation units that launch such kernels (lzq_window.hip:
// the yields; lzq_solve.hip: the per-point root solve).  Not ABI.
#pragma once
#include "lzq_quad.h"
#include "lzq_window.h"

namespace lzq {

// W(y) on the device: the table kind interpolates, the others take the quadrature's exponential
// of -q^2/2.  kind is wave-uniform (one block per wavefront / per launch).
__device__ __forceinline__ double window_W(const WinParams& p, int32_t kind, double y) {
  if (kind == LZQ_WIN_TABLE) return window_table_W(p, window_v(p, y));
  if (kind == kWinBad) return __builtin_nan("");
  const double q = window_q(p, kind, y);
  return exp_sc(-0.5 * (q * q));
}

// WaveSlot (lzq_quad.h) extended by the point's window.
struct WinWaveSlot {
  QuadSetup s;
  EpiPre e;
  double acc[kWaveSize];
  WinParams win;
};

// yb_wave's window: the block parked in the wave's slot (any slot with a `win` member)
struct SlotWindow {
  template <typename Slot>
  static __device__ __forceinline__ double eval(const Slot& slot, double y) {
    return window_W(slot.win, __builtin_amdgcn_readfirstlane(slot.win.kind), y);
  }
};

template <typename Slot>
__device__ __forceinline__ void park_window(Slot& slot, const QuadSetup& s, const EpiPre& e, const WinParams& win,
                                            int lane) {
  if (lane == 0) {
    slot.s = s;
    slot.e = e;
    slot.win = win;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// a grid point's z-sum table (lzq_kernels.hip table_of: the table axes' coordinates by tstride;
// window axes lie between them with tstride 0)
__device__ __forceinline__ int64_t win_table_of(const GridSpec& g, int64_t idx) {
  int64_t t = 0;
  for (int a = 0; a < g.n_axes; ++a) t += ((idx / g.stride[a]) % g.n[a]) * g.tstride[a];
  return t;
}

}  // namespace lzq
