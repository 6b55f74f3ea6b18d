// lzq_fit_common.h -- what the fit kernels (lzq_fit.hip) and the posterior kernels (lzq_post.hip)
// share: the parameter block, the row load, chi2, the incremental cell decode and the wave /
// block reductions.  Not ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/lzq.h"
#include "lzq_exp2.h"   // LZQ_HD

namespace lzq {

constexpr int kFitBlock = 256;
constexpr int kFitWaves = kFitBlock / 64;
constexpr int kFitGrid = 512;          // blocks of the update passes (grid-stride beyond)

struct FitMapDev {
  int64_t stride0, len0, stride1, len1;
  int64_t off;       // word offset of the map's first cell in the state
  int32_t cells;
  int32_t lds_off;   // first cell in the block-private LDS image, or -1: straight to global memory
};

struct FitParams {
  int32_t n_terms, n_levels, n_maps, lds_cells;
  int32_t field[LZQ_FIT_MAX_TERMS];
  double target[LZQ_FIT_MAX_TERMS], sigma[LZQ_FIT_MAX_TERMS], level[LZQ_FIT_MAX_LEVELS];
  FitMapDev map[LZQ_FIT_MAX_MAPS];
};

template <bool A16>
__device__ __forceinline__ void fit_load_row(const lzq_yield* rows, int64_t r, double x[6]) {
  if (A16) {   // 48-B records on a 16-B aligned base: three 16-B loads
    const double2* q = reinterpret_cast<const double2*>(rows + r);
    const double2 a = q[0], b = q[1], c = q[2];
    x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y; x[4] = c.x; x[5] = c.y;
  } else {
    const double* q = reinterpret_cast<const double*>(rows + r);
#pragma unroll
    for (int j = 0; j < 6; ++j) x[j] = q[j];
  }
}

LZQ_HD double fit_pick(const double x[6], int f) {
  return f == 0 ? x[0] : f == 1 ? x[1] : f == 2 ? x[2] : f == 3 ? x[3] : f == 4 ? x[4] : x[5];
}

LZQ_HD double fit_chi2(const FitParams& P, const double x[6]) {
  double c = 0.0;
  for (int t = 0; t < P.n_terms; ++t) {
    const double d = (fit_pick(x, P.field[t]) - P.target[t]) / P.sigma[t];
    const double q = d * d;
    c = t == 0 ? q : c + q;
  }
  return c;
}

// The cells of one thread's rows.  A thread visits flat indices flat0, flat0 + step, ...: the 64-bit
// divisions of the decode i_a = (flat / stride_a) % len_a are done once, for flat0 and for the
// step, and every later row costs an add, a compare and a conditional subtract per axis (the
// divisions were most of the update's time when every row paid for them).  A 1-D map walks a
// second axis of stride 1 and length 1, whose index stays 0.
struct CellWalk {
  int64_t r[LZQ_FIT_MAX_MAPS][2];     // flat % stride
  int64_t sr[LZQ_FIT_MAX_MAPS][2];    // step % stride
  int32_t i[LZQ_FIT_MAX_MAPS][2];     // (flat / stride) % len
  int32_t si[LZQ_FIT_MAX_MAPS][2];    // (step / stride) % len

  __device__ __forceinline__ void init(const FitParams& P, int64_t flat0, int64_t step) {
#pragma unroll
    for (int m = 0; m < LZQ_FIT_MAX_MAPS; ++m) {
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        r[m][a] = sr[m][a] = 0, i[m][a] = si[m][a] = 0;
        if (m < P.n_maps) {
          const int64_t stride = a ? P.map[m].stride1 : P.map[m].stride0, len = a ? P.map[m].len1 : P.map[m].len0;
          const int64_t q = flat0 / stride, sq = step / stride;
          r[m][a] = flat0 - q * stride, i[m][a] = (int32_t)(q % len);
          sr[m][a] = step - sq * stride, si[m][a] = (int32_t)(sq % len);
        }
      }
    }
  }
  __device__ __forceinline__ int32_t cell(const FitParams& P, int m) const {
    return i[m][0] * (int32_t)P.map[m].len1 + i[m][1];
  }
  __device__ __forceinline__ void next(const FitParams& P) {
#pragma unroll
    for (int m = 0; m < LZQ_FIT_MAX_MAPS; ++m) {
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        if (m < P.n_maps) {
          const int64_t stride = a ? P.map[m].stride1 : P.map[m].stride0;
          const int32_t len = (int32_t)(a ? P.map[m].len1 : P.map[m].len0);
          r[m][a] += sr[m][a];
          const bool carry = r[m][a] >= stride;
          r[m][a] -= carry ? stride : 0;
          i[m][a] += si[m][a] + (int32_t)carry;
          i[m][a] -= i[m][a] >= len ? len : 0;
        }
      }
    }
  }
};

__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)v, s);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)v, s);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor((unsigned long long)v, s);
  return v;
}

enum { OP_MIN = 0, OP_MAX = 1, OP_SUM = 2 };
// one value per thread -> one per block, in thread 0 (red: kFitWaves words of LDS)
template <int OP>
__device__ __forceinline__ uint64_t block_reduce(uint64_t v, uint64_t* red) {
  v = OP == OP_MIN ? wave_min(v) : OP == OP_MAX ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t r = red[0];
  for (int w = 1; w < kFitWaves; ++w) {
    const uint64_t o = red[w];
    r = OP == OP_MIN ? (o < r ? o : r) : OP == OP_MAX ? (o > r ? o : r) : r + o;
  }
  return r;
}

__device__ __forceinline__ void gadd(uint64_t* p, uint64_t v) {
  if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace lzq

// Host-side validation of a fit's terms, levels and maps into the kernels' parameter block
// (lzq_fit.hip): LZQ_EINVAL with a message naming `who`.  The maps' offsets and LDS placement are
// the fit state's; *words its length.
int lzq_fit_params(const char* who, const lzq_fit_term* terms, int32_t n_terms, const double* levels,
                   int32_t n_levels, const lzq_fit_map* maps, int32_t n_maps, lzq::FitParams* P, int64_t* words);
// hipGetLastError after a launch -> LZQ_OK or LZQ_EHIP with "<who>: <error>"
int lzq_fit_launched(const char* who);
