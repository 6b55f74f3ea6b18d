// lzq_obs.hip -- histograms of a fit over yield fields ("observables"): per cell the number of
// valid rows, their smallest chi2 and their posterior weight (no reference counterpart).
//
// The fit's and the posterior's states are indexed by the sweep's input axes; this one by the
// outputs.  A row's cell is lzq_obs.h's obs_cell, its chi2 lzq_fit_common.h's fit_chi2 and its
// weight lzq_post.h's q, each one definition for host and device.  Counts and weight pairs are
// integer sums and the chi2 minimum is an integer minimum (chi2 >= 0 orders like its bits), so
// the state is the same bit for bit however the rows are split into chunks, blocks, shards or
// ranks, and whichever of the paths below a cell takes.
//
// The state (include/lzq.h, "sweep observables"), per observable:
//   [0] n_in  [1] n_out  [2] n_nonfinite  [3] 0   then cells weight pairs, cells counts, cells chi2.
//
// Contention: near the best fit a whole wave lands in one cell.  When every lane of a wave that
// has a cell has the same one, the wave combines first (count = the lanes, weight by sums, chi2
// by a minimum) and one lane issues the atomics; a wave with several destinations falls back to
// per-lane atomics.  Observables of up to LZQ_OBS_LDS_CELLS cells in all are block-private in
// LDS and flushed once per block, only the words that changed; zero adds are skipped, and a chi2
// that a first read of the cell shows cannot lower it is not sent.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/lzq.h"
#include "lzq_fit_common.h"
#include "lzq_internal.h"
#include "lzq_obs.h"
#include "lzq_post.h"

namespace lzq {

// LDS of one block: 32 B a cell (a weight pair, a count, a chi2) x 1536 cells = 48 KB, plus the
// reduction scratch: three blocks on a CU's 160 KB (the 512-block grid puts two on each of the
// 256 CUs), inside HIP's 64 KB of static LDS a block.
constexpr int kObsLdsCells = LZQ_OBS_LDS_CELLS;
constexpr uint64_t kObsEmpty = 0x7ff0000000000000ull;   // +inf: no row in the cell yet

enum { OW_NIN = 0, OW_NOUT = 1, OW_NNONFINITE = 2 };

__device__ __forceinline__ uint64_t obs_gload(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the word only ever falls while updates run, so a value read first (stale or not) that v cannot
// beat means the atomic would change nothing
__device__ __forceinline__ void obs_gmin(uint64_t* p, uint64_t v) {
  if (v < obs_gload(p)) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void obs_ladd(uint64_t* p, uint64_t v) {
  if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool A16, bool WEIGHTED>
__global__ void __launch_bounds__(kFitBlock) obs_update_kernel(const lzq_yield* __restrict__ rows, int64_t count,
                                                                uint64_t* __restrict__ st, FitParams P, ObsParams O,
                                                                double offset) {
  __shared__ uint64_t swt[2 * kObsLdsCells];
  __shared__ uint64_t scnt[kObsLdsCells];
  __shared__ uint64_t schi[kObsLdsCells];
  __shared__ uint64_t red[kFitWaves];
  for (int i = threadIdx.x; i < O.lds_cells; i += kFitBlock) {
    swt[2 * i] = swt[2 * i + 1] = 0;
    scnt[i] = 0;
    schi[i] = kObsEmpty;
  }
  __syncthreads();
  uint64_t n_in[LZQ_OBS_MAX] = {0, 0, 0, 0}, n_out[LZQ_OBS_MAX] = {0, 0, 0, 0}, n_nf[LZQ_OBS_MAX] = {0, 0, 0, 0};
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * kFitBlock;
  for (int64_t base = (int64_t)blockIdx.x * kFitBlock; base < count; base += step) {
    const int64_t r = base + threadIdx.x;
    const bool active = r < count;
    double x[6] = {0, 0, 0, 0, 0, 0};
    if (active) fit_load_row<A16>(rows, r, x);
    const double c = fit_chi2(P, x);
    const bool valid = active && __builtin_isfinite(c);
    if (__ballot(valid) == 0) continue;   // wave-uniform
    const uint64_t cbits = (uint64_t)__double_as_longlong(c);   // c >= 0
    uint64_t hi = 0, lo = 0;
    if (WEIGHTED) {
      const uint64_t q = post_weight(c, offset);
      const bool has = valid && post_weighted(q);
      hi = has ? q >> 31 : 0, lo = has ? q & 0x7fffffffull : 0;
    }
#pragma unroll
    for (int k = 0; k < LZQ_OBS_MAX; ++k) {
      if (k >= O.n_obs) break;
      const ObsDev& D = O.obs[k];
      const int32_t cell = valid ? obs_cell(D, x) : -3;
      const bool in = cell >= 0;
      n_in[k] += in;
      n_out[k] += cell == kObsOut;
      n_nf[k] += cell == kObsNonfinite;
      const uint64_t inmask = __ballot(in);
      if (inmask == 0) continue;   // wave-uniform
      const int first = __ffsll((unsigned long long)inmask) - 1;
      const int32_t c0 = __shfl(cell, first);
      const bool uniform = __ballot(in && cell != c0) == 0;   // one destination for the whole wave
      uint64_t n = 1, m = cbits, whi = in ? hi : 0, wlo = in ? lo : 0;
      bool send = in;
      if (uniform) {
        n = (uint64_t)__popcll((unsigned long long)inmask);
        m = wave_min(in ? cbits : ~0ull);
        if (WEIGHTED) whi = wave_sum(whi), wlo = wave_sum(wlo);   // 64 lanes x 2^31 stays far below 2^64
        send = lane == first;
      }
      if (send) {
        if (D.lds_off >= 0) {
          const int32_t i = D.lds_off + cell;
          obs_ladd(scnt + i, n);
          __hip_atomic_fetch_min(schi + i, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (WEIGHTED) obs_ladd(swt + 2 * i, whi), obs_ladd(swt + 2 * i + 1, wlo);
        } else {
          uint64_t* w = st + D.off + LZQ_OBS_HEADER_WORDS;
          gadd(w + 2 * (int64_t)D.cells + cell, n);
          obs_gmin(w + 3 * (int64_t)D.cells + cell, m);
          if (WEIGHTED) gadd(w + 2 * (int64_t)cell, whi), gadd(w + 2 * (int64_t)cell + 1, wlo);
        }
      }
    }
  }
  __syncthreads();
  // flush the block-private cells that saw a row
  for (int k = 0; k < O.n_obs; ++k) {
    const ObsDev& D = O.obs[k];
    if (D.lds_off < 0) continue;
    uint64_t* w = st + D.off + LZQ_OBS_HEADER_WORDS;
    for (int i = threadIdx.x; i < D.cells; i += kFitBlock) {
      const uint64_t n = scnt[D.lds_off + i];
      if (n == 0) continue;
      gadd(w + 2 * (int64_t)D.cells + i, n);
      obs_gmin(w + 3 * (int64_t)D.cells + i, schi[D.lds_off + i]);
      if (WEIGHTED) gadd(w + 2 * i, swt[2 * (D.lds_off + i)]), gadd(w + 2 * i + 1, swt[2 * (D.lds_off + i) + 1]);
    }
  }
#pragma unroll
  for (int k = 0; k < LZQ_OBS_MAX; ++k) {
    if (k < O.n_obs) {
      uint64_t t;
      t = block_reduce<OP_SUM>(n_in[k], red);
      if (threadIdx.x == 0) gadd(st + O.obs[k].off + OW_NIN, t);
      t = block_reduce<OP_SUM>(n_out[k], red);
      if (threadIdx.x == 0) gadd(st + O.obs[k].off + OW_NOUT, t);
      t = block_reduce<OP_SUM>(n_nf[k], red);
      if (threadIdx.x == 0) gadd(st + O.obs[k].off + OW_NNONFINITE, t);
    }
  }
}

// true when word i of the state is a chi2 word
__device__ __forceinline__ bool obs_is_chi2(const ObsParams& O, int64_t i) {
  bool is = false;
  for (int k = 0; k < O.n_obs; ++k) {
    const int64_t a = O.obs[k].off + LZQ_OBS_HEADER_WORDS + 3 * (int64_t)O.obs[k].cells;
    is = is || (i >= a && i < a + O.obs[k].cells);
  }
  return is;
}

__global__ void obs_reset_kernel(uint64_t* __restrict__ st, int64_t words, ObsParams O) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < words) st[i] = obs_is_chi2(O, i) ? kObsEmpty : 0;
}

__global__ void obs_merge_kernel(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, int64_t words,
                                 ObsParams O) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= words) return;
  const uint64_t a = dst[i], b = src[i];
  dst[i] = obs_is_chi2(O, i) ? (b < a ? b : a) : a + b;
}

}  // namespace lzq

using lzq::ObsParams;

static int obs_fail(const char* who, int k, int a, const char* what) {
  char msg[192];
  if (a >= 0) snprintf(msg, sizeof msg, "%s: observable %d axis %d: %s", who, k, a, what);
  else snprintf(msg, sizeof msg, "%s: observable %d: %s", who, k, what);
  return lzq_set_error(LZQ_EINVAL, msg);
}

// Validate the observables into the kernels' parameter block; *words is the state's length.
static int obs_params(const char* who, const lzq_obs* obs, int32_t n_obs, ObsParams* P, int64_t* words) {
  char msg[160];
  memset(P, 0, sizeof *P);
  if (n_obs < 0 || n_obs > LZQ_OBS_MAX) {
    snprintf(msg, sizeof msg, "%s: %d observables (0..%d)", who, n_obs, LZQ_OBS_MAX);
    return lzq_set_error(LZQ_EINVAL, msg);
  }
  if (n_obs > 0 && !obs) {
    snprintf(msg, sizeof msg, "%s: bad arguments (null observables)", who);
    return lzq_set_error(LZQ_EINVAL, msg);
  }
  int64_t off = 0;
  int32_t lds = 0;
  for (int k = 0; k < n_obs; ++k) {
    const lzq_obs& S = obs[k];
    lzq::ObsDev& D = P->obs[k];
    if (S.n_axes < 1 || S.n_axes > 2) return obs_fail(who, k, -1, "1 or 2 axes");
    if (S.n_axes == 2 && S.axes[0].field == S.axes[1].field) return obs_fail(who, k, -1, "two axes over one field");
    int64_t cells = 1;
    for (int a = 0; a < S.n_axes; ++a) {
      const lzq_obs_axis& X = S.axes[a];
      lzq::ObsAxisDev& A = D.ax[a];
      if (X.field < 0 || X.field > 5) return obs_fail(who, k, a, "unknown field (0..5)");
      if (!isfinite(X.lo) || !isfinite(X.hi) || !(X.lo < X.hi)) return obs_fail(who, k, a, "lo < hi, both finite");
      A.field = X.field, A.kind = X.kind, A.lo = X.lo, A.hi = X.hi;
      if (X.kind == LZQ_OBS_LINEAR) {
        if (X.bins < 1 || X.bins > LZQ_OBS_MAX_CELLS) return obs_fail(who, k, a, "1 <= bins <= 2^20 cells");
        A.bins = X.bins;
        A.inv = (double)X.bins / (X.hi - X.lo);
        if (!isfinite(A.inv) || !(A.inv > 0.0)) return obs_fail(who, k, a, "bins / (hi - lo) must be finite and > 0");
      } else if (X.kind == LZQ_OBS_LOG2) {
        if (!(X.lo > 0.0)) return obs_fail(who, k, a, "a log axis needs lo > 0");
        if (X.log2_sub < 0 || X.log2_sub > 8) return obs_fail(who, k, a, "log2_sub in 0..8");
        A.shift = 52 - X.log2_sub;
        A.key_lo = lzq::obs_key(X.lo, A.shift);
        const int64_t nb = lzq::obs_key(X.hi, A.shift) - A.key_lo;   // below 2^19: 2047 octaves x 256
        if (nb < 1) return obs_fail(who, k, a, "a log axis needs at least one sub-bin between lo and hi");
        A.bins = (int32_t)nb;
      } else {
        return obs_fail(who, k, a, "unknown kind (LZQ_OBS_LINEAR or LZQ_OBS_LOG2)");
      }
      cells *= A.bins;
    }
    if (cells > LZQ_OBS_MAX_CELLS) return obs_fail(who, k, -1, "more than 2^20 cells");
    D.n_axes = S.n_axes, D.cells = (int32_t)cells, D.off = off;
    D.lds_off = lds + D.cells <= lzq::kObsLdsCells ? lds : -1;
    if (D.lds_off >= 0) lds += D.cells;
    off += LZQ_OBS_HEADER_WORDS + 4 * cells;
  }
  P->n_obs = n_obs, P->lds_cells = lds;
  *words = off;
  return LZQ_OK;
}

extern "C" {

int64_t lzq_obs_state_bytes(const lzq_obs* obs, int32_t n_obs) {
  ObsParams O;
  int64_t words = 0;
  const int rc = obs_params("lzq_obs_state_bytes", obs, n_obs, &O, &words);
  return rc != LZQ_OK ? rc : words * 8;
}

int lzq_obs_cells_host(const lzq_obs* obs, int32_t n_obs, int32_t k, const lzq_yield* rows, int64_t n,
                       int32_t* cell_out) {
  ObsParams O;
  int64_t words = 0;
  const int rc = obs_params("lzq_obs_cells_host", obs, n_obs, &O, &words);
  if (rc != LZQ_OK) return rc;
  if (k < 0 || k >= n_obs || n < 0 || (n > 0 && (!rows || !cell_out)))
    return lzq_set_error(LZQ_EINVAL, "lzq_obs_cells_host: bad arguments (0 <= k < n_obs, n >= 0, non-null buffers)");
  for (int64_t i = 0; i < n; ++i) cell_out[i] = lzq::obs_cell(O.obs[k], reinterpret_cast<const double*>(rows + i));
  return LZQ_OK;
}

int lzq_obs_reset(const lzq_obs* obs, int32_t n_obs, void* d_state, void* stream) {
  ObsParams O;
  int64_t words = 0;
  const int rc = obs_params("lzq_obs_reset", obs, n_obs, &O, &words);
  if (rc != LZQ_OK) return rc;
  if (!d_state) return lzq_set_error(LZQ_EINVAL, "lzq_obs_reset: bad arguments (null state)");
  if (words == 0) return LZQ_OK;
  hipLaunchKernelGGL(lzq::obs_reset_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint64_t*)d_state, words, O);
  return lzq_fit_launched("lzq_obs_reset");
}

int lzq_obs_update(const lzq_fit_term* terms, int32_t n_terms, const lzq_obs* obs, int32_t n_obs, int32_t weighted,
                   double offset, const lzq_yield* d_yields, int64_t count, void* d_state, void* stream) {
  lzq::FitParams P;
  ObsParams O;
  int64_t words = 0, fit_words = 0;
  if (!terms) return lzq_set_error(LZQ_EINVAL, "lzq_obs_update: bad arguments (null terms)");
  int rc = lzq_fit_params("lzq_obs_update", terms, n_terms, nullptr, 0, nullptr, 0, &P, &fit_words);
  if (rc != LZQ_OK) return rc;
  if ((rc = obs_params("lzq_obs_update", obs, n_obs, &O, &words)) != LZQ_OK) return rc;
  if (weighted && !(isfinite(offset) && offset >= 0.0))
    return lzq_set_error(LZQ_EINVAL, "lzq_obs_update: offset must be finite and >= 0");
  if (count < 0 || !d_state || (count > 0 && !d_yields))
    return lzq_set_error(LZQ_EINVAL, "lzq_obs_update: bad arguments (count >= 0, non-null buffers)");
  if (count > LZQ_POST_MAX_ROWS)
    return lzq_set_error(LZQ_EINVAL, "lzq_obs_update: more than 2^32 rows (the exact sums' limit per state)");
  if (count == 0 || n_obs == 0) return LZQ_OK;
  if (!weighted) offset = 0.0;
  const int64_t nb = (count + lzq::kFitBlock - 1) / lzq::kFitBlock;
  const dim3 grid((unsigned)(nb < lzq::kFitGrid ? nb : lzq::kFitGrid)), block(lzq::kFitBlock);
  const bool a16 = ((uintptr_t)d_yields & 15) == 0;
  uint64_t* st = (uint64_t*)d_state;
  hipStream_t s = (hipStream_t)stream;
  if (a16 && weighted)
    hipLaunchKernelGGL((lzq::obs_update_kernel<true, true>), grid, block, 0, s, d_yields, count, st, P, O, offset);
  else if (a16)
    hipLaunchKernelGGL((lzq::obs_update_kernel<true, false>), grid, block, 0, s, d_yields, count, st, P, O, offset);
  else if (weighted)
    hipLaunchKernelGGL((lzq::obs_update_kernel<false, true>), grid, block, 0, s, d_yields, count, st, P, O, offset);
  else
    hipLaunchKernelGGL((lzq::obs_update_kernel<false, false>), grid, block, 0, s, d_yields, count, st, P, O, offset);
  return lzq_fit_launched("lzq_obs_update");
}

int lzq_obs_merge(const lzq_obs* obs, int32_t n_obs, void* d_dst, const void* d_src, void* stream) {
  ObsParams O;
  int64_t words = 0;
  const int rc = obs_params("lzq_obs_merge", obs, n_obs, &O, &words);
  if (rc != LZQ_OK) return rc;
  if (!d_dst || !d_src || d_dst == d_src)
    return lzq_set_error(LZQ_EINVAL, "lzq_obs_merge: bad arguments (two distinct non-null states)");
  if (words == 0) return LZQ_OK;
  hipLaunchKernelGGL(lzq::obs_merge_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint64_t*)d_dst, (const uint64_t*)d_src, words, O);
  return lzq_fit_launched("lzq_obs_merge");
}

}  // extern "C"
