// lzq_post.hip -- likelihood-weighted sums of a sweep's lzq_yield records: evidence, mass within
// chi2 levels, a histogram of weight by chi2 and marginal maps (no reference counterpart).
//
// A row's weight is lzq_post.h's q = exp(-(chi2 - offset)/2) in units of 2^-62, an integer.  Every
// accumulator is a PAIR of 64-bit words (sum of q >> 31, sum of q & 0x7fffffff), value
// hi * 2^31 + lo: a row adds at most 2^31 to either word, so 2^32 rows cannot overflow one, and
// integer addition is associative -- the state is the same bit for bit however the rows are split
// into chunks, blocks, shards or ranks.  No floating-point sum is taken anywhere.
//
// The state (include/lzq.h, "posterior state"):
//   [0] n_used  [1] n_zero  [2] n_above  [3] n_invalid  [4,5] Z  [6..13] weight within level l
//   [14..31] reserved  [32 .. 32 + 2 * 2048) histogram pairs  then per map `cells` pairs.
//
// Contention: near the best fit a whole wave lands in one histogram bin, and on a map over slow
// axes in one cell.  The lanes of a wave that share a destination are summed before anything
// leaves the wave (64 lanes x 2^31 stays far below 2^64); the histogram and small maps are
// block-private in LDS and only their non-zero words are flushed; zero adds are skipped.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/lzq.h"
#include "lzq_fit_common.h"
#include "lzq_internal.h"
#include "lzq_post.h"

namespace lzq {

constexpr int kPostBins = LZQ_POST_BINS;
// LDS of one block: the histogram, 2048 pairs = 32 KB, and up to 1024 map cells as pairs = 16 KB,
// plus the reduction scratch: 48 KB + 32 B, three blocks on a CU's 160 KB (the 512-block grid
// puts two on each of the 256 CUs).
constexpr int kPostLdsCells = 1024;

enum { PW_NUSED = 0, PW_NZERO = 1, PW_NABOVE = 2, PW_NINVALID = 3, PW_Z = 4, PW_LEVEL = 6,
       PW_HIST = LZQ_POST_HEADER_WORDS, PW_MAPS = LZQ_POST_HEADER_WORDS + 2 * LZQ_POST_BINS };

__device__ __forceinline__ void ladd(uint64_t* p, uint64_t v) {
  if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The lanes `has` of a wave add their (hi, lo) to pair `idx` of `base` (LDS: a block-private image;
// else the state in global memory).  Called by the whole wave; `first` is its first lane with `has`.
template <bool LDS>
__device__ __forceinline__ void wave_add_pair(uint64_t* base, bool has, int32_t idx, int first, uint64_t hi,
                                              uint64_t lo) {
  const int32_t i0 = __shfl(idx, first);
  const bool uniform = __ballot(has && idx != i0) == 0;   // one destination for the whole wave
  bool send = has;
  if (uniform) {
    hi = wave_sum(hi), lo = wave_sum(lo);   // lanes without `has` hold 0
    send = (int)(threadIdx.x & 63) == first;
  }
  if (send) {
    uint64_t* p = base + 2 * (int64_t)idx;
    if (LDS) ladd(p, hi), ladd(p + 1, lo);
    else gadd(p, hi), gadd(p + 1, lo);
  }
}

template <bool A16>
__global__ void __launch_bounds__(kFitBlock) post_update_kernel(const lzq_yield* __restrict__ rows, int64_t start,
                                                                 int64_t count, uint64_t* __restrict__ st, FitParams P,
                                                                 double offset) {
  __shared__ uint64_t shist[2 * kPostBins];
  __shared__ uint64_t smap[2 * kPostLdsCells];
  __shared__ uint64_t red[kFitWaves];
  for (int i = threadIdx.x; i < 2 * kPostBins; i += kFitBlock) shist[i] = 0;
  for (int i = threadIdx.x; i < 2 * P.lds_cells; i += kFitBlock) smap[i] = 0;
  __syncthreads();
  uint64_t n_used = 0, n_zero = 0, n_above = 0, n_invalid = 0, zhi = 0, zlo = 0;
  uint64_t lhi[LZQ_FIT_MAX_LEVELS] = {0, 0, 0, 0}, llo[LZQ_FIT_MAX_LEVELS] = {0, 0, 0, 0};
  const int64_t step = (int64_t)gridDim.x * kFitBlock;
  CellWalk walk;
  walk.init(P, start + (int64_t)blockIdx.x * kFitBlock + threadIdx.x, step);
  for (int64_t base = (int64_t)blockIdx.x * kFitBlock; base < count; base += step, walk.next(P)) {
    const int64_t r = base + threadIdx.x;
    const bool active = r < count;
    double x[6] = {0, 0, 0, 0, 0, 0};
    if (active) fit_load_row<A16>(rows, r, x);
    const double c = fit_chi2(P, x);
    const uint64_t q = post_weight(c, offset);
    const bool has = active && post_weighted(q);
    if (active) {
      n_used += has;
      n_zero += q == 0;
      n_above += q == kPostAbove;
      n_invalid += q == kPostInvalid;
    }
    // a thread sees at most 2^32 / 2^17 rows: its own sums of hi and lo parts stay below 2^47
    const uint64_t hi = has ? q >> 31 : 0, lo = has ? q & 0x7fffffffull : 0;
    zhi += hi, zlo += lo;
#pragma unroll
    for (int l = 0; l < LZQ_FIT_MAX_LEVELS; ++l) {
      const bool in = has && l < P.n_levels && c <= P.level[l];
      lhi[l] += in ? hi : 0, llo[l] += in ? lo : 0;
    }
    const uint64_t hasmask = __ballot(has);
    if (hasmask == 0) continue;   // wave-uniform
    const int first = __ffsll((unsigned long long)hasmask) - 1;
    // q > 0 means a < 86: the product (exact: a power of two) is far inside int's range
    int32_t bin = -1;
    if (has) {
      bin = (int32_t)((c - offset) * 16.0);
      bin = bin < kPostBins - 1 ? bin : kPostBins - 1;
    }
    wave_add_pair<true>(shist, has, bin, first, hi, lo);
#pragma unroll
    for (int m = 0; m < LZQ_FIT_MAX_MAPS; ++m) {
      if (m >= P.n_maps) break;
      const FitMapDev& M = P.map[m];
      const int32_t cell = has ? walk.cell(P, m) : -1;
      if (M.lds_off >= 0) wave_add_pair<true>(smap + 2 * M.lds_off, has, cell, first, hi, lo);
      else wave_add_pair<false>(st + M.off, has, cell, first, hi, lo);
    }
  }
  __syncthreads();
  // flush the block-private words that received weight
  for (int i = threadIdx.x; i < 2 * kPostBins; i += kFitBlock) gadd(st + PW_HIST + i, shist[i]);
  for (int m = 0; m < P.n_maps; ++m) {
    const FitMapDev& M = P.map[m];
    if (M.lds_off < 0) continue;
    for (int i = threadIdx.x; i < 2 * M.cells; i += kFitBlock) gadd(st + M.off + i, smap[2 * M.lds_off + i]);
  }
  uint64_t t;
  t = block_reduce<OP_SUM>(n_used, red);
  if (threadIdx.x == 0) gadd(st + PW_NUSED, t);
  t = block_reduce<OP_SUM>(n_zero, red);
  if (threadIdx.x == 0) gadd(st + PW_NZERO, t);
  t = block_reduce<OP_SUM>(n_above, red);
  if (threadIdx.x == 0) gadd(st + PW_NABOVE, t);
  t = block_reduce<OP_SUM>(n_invalid, red);
  if (threadIdx.x == 0) gadd(st + PW_NINVALID, t);
  t = block_reduce<OP_SUM>(zhi, red);
  if (threadIdx.x == 0) gadd(st + PW_Z, t);
  t = block_reduce<OP_SUM>(zlo, red);
  if (threadIdx.x == 0) gadd(st + PW_Z + 1, t);
#pragma unroll
  for (int l = 0; l < LZQ_FIT_MAX_LEVELS; ++l) {
    if (l < P.n_levels) {
      t = block_reduce<OP_SUM>(lhi[l], red);
      if (threadIdx.x == 0) gadd(st + PW_LEVEL + 2 * l, t);
      t = block_reduce<OP_SUM>(llo[l], red);
      if (threadIdx.x == 0) gadd(st + PW_LEVEL + 2 * l + 1, t);
    }
  }
}

__global__ void post_merge_kernel(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, int64_t words) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < words) dst[i] += src[i];
}

}  // namespace lzq

using lzq::FitParams;

// the fit's parameter block with the posterior state's map offsets and LDS placement
static int post_params(const char* who, const lzq_fit_term* terms, int32_t n_terms, const double* levels,
                       int32_t n_levels, const lzq_fit_map* maps, int32_t n_maps, FitParams* P, int64_t* words) {
  int64_t fit_words = 0;
  const int rc = lzq_fit_params(who, terms, n_terms, levels, n_levels, maps, n_maps, P, &fit_words);
  if (rc != LZQ_OK) return rc;
  int64_t off = lzq::PW_MAPS;
  int32_t lds = 0;
  for (int m = 0; m < n_maps; ++m) {
    lzq::FitMapDev& D = P->map[m];
    D.off = off;
    D.lds_off = lds + D.cells <= lzq::kPostLdsCells ? lds : -1;
    if (D.lds_off >= 0) lds += D.cells;
    off += 2 * (int64_t)D.cells;
  }
  P->lds_cells = lds;
  *words = off;
  return LZQ_OK;
}

static int post_offset_ok(const char* who, double offset) {
  if (isfinite(offset) && offset >= 0.0) return LZQ_OK;
  char msg[128];
  snprintf(msg, sizeof msg, "%s: offset must be finite and >= 0", who);
  return lzq_set_error(LZQ_EINVAL, msg);
}

extern "C" {

int lzq_post_weights_host(const lzq_fit_term* terms, int32_t n_terms, double offset, const lzq_yield* rows, int64_t n,
                          uint64_t* q_out) {
  FitParams P;
  int64_t words = 0;
  if (!terms) return lzq_set_error(LZQ_EINVAL, "lzq_post_weights_host: bad arguments (null terms)");
  int rc = post_params("lzq_post_weights_host", terms, n_terms, nullptr, 0, nullptr, 0, &P, &words);
  if (rc != LZQ_OK) return rc;
  if ((rc = post_offset_ok("lzq_post_weights_host", offset)) != LZQ_OK) return rc;
  if (n < 0 || (n > 0 && (!rows || !q_out)))
    return lzq_set_error(LZQ_EINVAL, "lzq_post_weights_host: bad arguments (n >= 0, non-null buffers)");
  for (int64_t i = 0; i < n; ++i) {
    const double* x = reinterpret_cast<const double*>(rows + i);
    q_out[i] = lzq::post_weight(lzq::fit_chi2(P, x), offset);
  }
  return LZQ_OK;
}

int64_t lzq_post_state_bytes(const lzq_fit_map* maps, int32_t n_maps) {
  FitParams P;
  int64_t words = 0;
  const int rc = post_params("lzq_post_state_bytes", nullptr, 0, nullptr, 0, maps, n_maps, &P, &words);
  return rc != LZQ_OK ? rc : words * 8;
}

int lzq_post_reset(const lzq_fit_map* maps, int32_t n_maps, void* d_state, void* stream) {
  FitParams P;
  int64_t words = 0;
  const int rc = post_params("lzq_post_reset", nullptr, 0, nullptr, 0, maps, n_maps, &P, &words);
  if (rc != LZQ_OK) return rc;
  if (!d_state) return lzq_set_error(LZQ_EINVAL, "lzq_post_reset: bad arguments (null state)");
  const hipError_t e = hipMemsetAsync(d_state, 0, (size_t)words * 8, (hipStream_t)stream);
  if (e != hipSuccess) return lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
  return LZQ_OK;
}

int lzq_post_update(const lzq_fit_term* terms, int32_t n_terms, const double* levels, int32_t n_levels,
                    const lzq_fit_map* maps, int32_t n_maps, double offset, const lzq_yield* d_yields, int64_t start,
                    int64_t count, void* d_state, void* stream) {
  FitParams P;
  int64_t words = 0;
  if (!terms) return lzq_set_error(LZQ_EINVAL, "lzq_post_update: bad arguments (null terms)");
  int rc = post_params("lzq_post_update", terms, n_terms, levels, n_levels, maps, n_maps, &P, &words);
  if (rc != LZQ_OK) return rc;
  if ((rc = post_offset_ok("lzq_post_update", offset)) != LZQ_OK) return rc;
  if (start < 0 || count < 0 || start > LZQ_FIT_MAX_INDEX - count || !d_state || (count > 0 && !d_yields))
    return lzq_set_error(LZQ_EINVAL, "lzq_post_update: bad arguments (start, count >= 0, start + count <= 2^62, "
                                     "non-null buffers)");
  if (count > LZQ_POST_MAX_ROWS)
    return lzq_set_error(LZQ_EINVAL, "lzq_post_update: more than 2^32 rows (the exact sums' limit per state)");
  if (count == 0) return LZQ_OK;
  const int64_t nb = (count + lzq::kFitBlock - 1) / lzq::kFitBlock;
  const dim3 grid((unsigned)(nb < lzq::kFitGrid ? nb : lzq::kFitGrid)), block(lzq::kFitBlock);
  if (((uintptr_t)d_yields & 15) == 0)
    hipLaunchKernelGGL(lzq::post_update_kernel<true>, grid, block, 0, (hipStream_t)stream, d_yields, start, count,
                       (uint64_t*)d_state, P, offset);
  else
    hipLaunchKernelGGL(lzq::post_update_kernel<false>, grid, block, 0, (hipStream_t)stream, d_yields, start, count,
                       (uint64_t*)d_state, P, offset);
  return lzq_fit_launched("lzq_post_update");
}

int lzq_post_merge(const lzq_fit_map* maps, int32_t n_maps, void* d_dst, const void* d_src, void* stream) {
  FitParams P;
  int64_t words = 0;
  const int rc = post_params("lzq_post_merge", nullptr, 0, nullptr, 0, maps, n_maps, &P, &words);
  if (rc != LZQ_OK) return rc;
  if (!d_dst || !d_src || d_dst == d_src)
    return lzq_set_error(LZQ_EINVAL, "lzq_post_merge: bad arguments (two distinct non-null states)");
  hipLaunchKernelGGL(lzq::post_merge_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint64_t*)d_dst, (const uint64_t*)d_src, words);
  return lzq_fit_launched("lzq_post_merge");
}

}  // extern "C"
