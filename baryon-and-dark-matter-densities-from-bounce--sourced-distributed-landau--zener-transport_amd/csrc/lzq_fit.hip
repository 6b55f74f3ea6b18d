// lzq_fit.hip -- streaming fit of lzq_yield records to targets (no reference counterpart: the
// reference evaluates one point; this reduces a sweep's table where it already is).
//
// chi2 of a row: for each term in order d = (x - target) / sigma, q = d * d, summed left to right,
// every operation rounded on its own (-ffp-contract=off), so numpy's float64 expression gives the
// same bits.  A row is valid iff its chi2 is finite.  Everything accumulated is independent of the
// order rows are seen in: integer counts, minima through integer atomics (a non-negative double
// orders like its bit pattern as an unsigned 64-bit integer; signed column values through the
// order-preserving key of fit_key), and "the lowest flat index attaining the minimum".
//
// The state is an array of 64-bit words (include/lzq.h, "fit state"):
//   [0] n_valid  [1] n_invalid  [2..5] n_within  [6] best chi2 bits  [7] best index
//   [8..13] column min keys  [14..19] column max keys  [20..25] column non-finite counts
//   [26] rows selected so far (lzq_fit_select's running offset)  [27..31] reserved
//   then per map: chi2 bits [cells], index [cells].
// An index word holds ~0 (= -1) while its cell is empty.
//
// Minimum + lowest index without a 128-bit atomic, and without a scratch map:
//   pass 1 (fit_min_kernel) takes atomic minima of the chi2 bits; whoever STRICTLY lowers a cell
//     resets its index word to ~0 (the index kept there belonged to a larger chi2);
//   pass 2 (fit_idx_kernel, after the kernel boundary) takes the unsigned atomic minimum of the
//     flat index over the rows whose chi2 equals their cell's minimum.
// A cell whose minimum a chunk only ties keeps its index, which then competes with the chunk's.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/lzq.h"
#include "lzq_fit_common.h"
#include "lzq_internal.h"

namespace lzq {

constexpr int kFitLdsCells = 4096;     // block-private map cells in LDS (32 KB: four blocks a CU)
constexpr int kFitSelIter = 8;         // rows per thread of one selection tile
constexpr uint64_t kInfBits = 0x7FF0000000000000ull;
constexpr uint64_t kNone = ~0ull;

enum { W_NVALID = 0, W_NINVALID = 1, W_WITHIN = 2, W_BEST_CHI2 = 6, W_BEST_IDX = 7, W_COLMIN = 8, W_COLMAX = 14,
       W_COLBAD = 20, W_SEL_TOTAL = 26, W_HEADER = LZQ_FIT_HEADER_WORDS };

// order-preserving key of a double that is not NaN: a < b  <=>  key(a) < key(b) (unsigned)
__device__ __forceinline__ uint64_t fit_key(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ uint64_t gmin(uint64_t* p, uint64_t v) {
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t gload(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// lower a cell's chi2; a strict improvement orphans the index kept for the old minimum.  The word
// only ever falls during the pass, so a value read first (stale or not) that bits cannot beat
// means the atomic would change nothing: once a sweep's early chunks have set the minima, almost
// every flush ends at this read instead of queueing on the cell's cache line.
__device__ __forceinline__ void cell_lower(uint64_t* chi2, uint64_t* idx, uint64_t bits) {
  if (bits >= gload(chi2)) return;
  const uint64_t old = gmin(chi2, bits);
  if (bits < old) __hip_atomic_store(idx, kNone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void fit_reset_kernel(uint64_t* st, int64_t words, FitParams P) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= words) return;
  uint64_t v = 0;
  if (i < W_HEADER) {
    if (i == W_BEST_CHI2) v = kInfBits;
    else if (i == W_BEST_IDX) v = kNone;
    else if (i >= W_COLMIN && i < W_COLMIN + 6) v = kNone;   // no finite value yet
  } else {
    for (int m = 0; m < P.n_maps; ++m) {
      const int64_t o = i - P.map[m].off;
      if (o >= 0 && o < 2 * (int64_t)P.map[m].cells) v = o < P.map[m].cells ? kInfBits : kNone;
    }
  }
  st[i] = v;
}

// pass 1: counts, column extrema, minima of chi2 (best and every map cell)
template <bool A16>
__global__ void __launch_bounds__(kFitBlock) fit_min_kernel(const lzq_yield* __restrict__ rows, int64_t start,
                                                             int64_t count, uint64_t* __restrict__ st, FitParams P) {
  __shared__ uint64_t smap[kFitLdsCells];
  __shared__ uint64_t red[kFitWaves];
  for (int i = threadIdx.x; i < P.lds_cells; i += kFitBlock) smap[i] = kNone;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  uint64_t n_valid = 0, n_invalid = 0, within[LZQ_FIT_MAX_LEVELS] = {0, 0, 0, 0}, best = kNone;
  uint64_t cmin[6], cmax[6], cbad[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) cmin[j] = kNone, cmax[j] = 0, cbad[j] = 0;
  const int64_t step = (int64_t)gridDim.x * kFitBlock;
  CellWalk walk;
  walk.init(P, start + (int64_t)blockIdx.x * kFitBlock + threadIdx.x, step);
  for (int64_t base = (int64_t)blockIdx.x * kFitBlock; base < count; base += step, walk.next(P)) {
    const int64_t r = base + threadIdx.x;
    const bool active = r < count;
    double x[6] = {0, 0, 0, 0, 0, 0};
    if (active) fit_load_row<A16>(rows, r, x);
    const double c = fit_chi2(P, x);
    const bool has = active && isfinite(c);
    const uint64_t bits = has ? (uint64_t)__double_as_longlong(c) : kNone;
    if (active) {
      n_valid += has;
      n_invalid += !has;
#pragma unroll
      for (int l = 0; l < LZQ_FIT_MAX_LEVELS; ++l) within[l] += (has && l < P.n_levels && c <= P.level[l]);
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        if (isfinite(x[j])) {
          const uint64_t k = fit_key(x[j]);
          cmin[j] = k < cmin[j] ? k : cmin[j];
          cmax[j] = k > cmax[j] ? k : cmax[j];
        } else {
          ++cbad[j];
        }
      }
    }
    best = bits < best ? bits : best;
    const uint64_t hasmask = __ballot(has);
    if (hasmask == 0) continue;   // wave-uniform
    const int first = __ffsll((unsigned long long)hasmask) - 1;
#pragma unroll
    for (int m = 0; m < LZQ_FIT_MAX_MAPS; ++m) {
      if (m >= P.n_maps) break;
      const FitMapDev& M = P.map[m];
      const int32_t cell = has ? walk.cell(P, m) : -1;
      const int32_t c0 = __shfl(cell, first);
      // the lanes of a wave that share a destination are reduced before anything leaves the wave: a
      // map over slow axes puts the whole wave in one cell
      const bool uniform = __ballot(has && cell != c0) == 0;
      uint64_t v = bits;
      bool send = has;
      if (uniform) {
        v = wave_min(bits);
        send = lane == first;
      }
      if (send) {
        if (M.lds_off >= 0)
          __hip_atomic_fetch_min(&smap[M.lds_off + cell], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
          cell_lower(st + M.off + cell, st + M.off + M.cells + cell, v);
      }
    }
  }
  __syncthreads();
  for (int m = 0; m < P.n_maps; ++m) {   // flush the block-private cells that saw a row
    const FitMapDev& M = P.map[m];
    if (M.lds_off < 0) continue;
    for (int i = threadIdx.x; i < M.cells; i += kFitBlock) {
      const uint64_t v = smap[M.lds_off + i];
      if (v != kNone) cell_lower(st + M.off + i, st + M.off + M.cells + i, v);
    }
  }
  uint64_t t;
  t = block_reduce<OP_SUM>(n_valid, red);
  if (threadIdx.x == 0) gadd(st + W_NVALID, t);
  t = block_reduce<OP_SUM>(n_invalid, red);
  if (threadIdx.x == 0) gadd(st + W_NINVALID, t);
#pragma unroll
  for (int l = 0; l < LZQ_FIT_MAX_LEVELS; ++l) {
    if (l < P.n_levels) {
      t = block_reduce<OP_SUM>(within[l], red);
      if (threadIdx.x == 0) gadd(st + W_WITHIN + l, t);
    }
  }
  t = block_reduce<OP_MIN>(best, red);
  if (threadIdx.x == 0 && t != kNone) cell_lower(st + W_BEST_CHI2, st + W_BEST_IDX, t);
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    t = block_reduce<OP_MIN>(cmin[j], red);
    if (threadIdx.x == 0 && t < gload(st + W_COLMIN + j)) gmin(st + W_COLMIN + j, t);
    t = block_reduce<OP_MAX>(cmax[j], red);
    if (threadIdx.x == 0 && t > gload(st + W_COLMAX + j))
      __hip_atomic_fetch_max(st + W_COLMAX + j, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = block_reduce<OP_SUM>(cbad[j], red);
    if (threadIdx.x == 0) gadd(st + W_COLBAD + j, t);
  }
}

// pass 2: the lowest flat index among the rows that equal their cell's minimum
template <bool A16>
__global__ void __launch_bounds__(kFitBlock) fit_idx_kernel(const lzq_yield* __restrict__ rows, int64_t start,
                                                             int64_t count, uint64_t* __restrict__ st, FitParams P) {
  __shared__ uint64_t red[kFitWaves];
  const int lane = threadIdx.x & 63;
  const uint64_t best_bits = st[W_BEST_CHI2];
  uint64_t best_idx = kNone;
  const int64_t step = (int64_t)gridDim.x * kFitBlock;
  CellWalk walk;
  walk.init(P, start + (int64_t)blockIdx.x * kFitBlock + threadIdx.x, step);
  for (int64_t base = (int64_t)blockIdx.x * kFitBlock; base < count; base += step, walk.next(P)) {
    const int64_t r = base + threadIdx.x;
    const bool active = r < count;
    double x[6] = {0, 0, 0, 0, 0, 0};
    if (active) fit_load_row<A16>(rows, r, x);
    const double c = fit_chi2(P, x);
    const bool has = active && isfinite(c);
    const uint64_t bits = has ? (uint64_t)__double_as_longlong(c) : kNone;
    const uint64_t flat = (uint64_t)(start + r);
    if (has && bits == best_bits) best_idx = flat < best_idx ? flat : best_idx;
    const uint64_t hasmask = __ballot(has);
    if (hasmask == 0) continue;
    const int first = __ffsll((unsigned long long)hasmask) - 1;
#pragma unroll
    for (int m = 0; m < LZQ_FIT_MAX_MAPS; ++m) {
      if (m >= P.n_maps) break;
      const FitMapDev& M = P.map[m];
      const int32_t cell = has ? walk.cell(P, m) : -1;
      const int32_t c0 = __shfl(cell, first);
      const bool uniform = __ballot(has && cell != c0) == 0;
      const bool eq = has && bits == st[M.off + cell];
      const uint64_t eqmask = __ballot(eq);
      if (eqmask == 0) continue;
      // one cell for the whole wave: its lowest index is the first lane that ties (lanes ascend)
      const bool send = uniform ? lane == __ffsll((unsigned long long)eqmask) - 1 : eq;
      if (send) {
        uint64_t* p = st + M.off + M.cells + cell;
        if (gload(p) > flat) gmin(p, flat);   // the word only ever falls during this pass: a stale read is larger
      }
    }
  }
  const uint64_t t = block_reduce<OP_MIN>(best_idx, red);
  if (threadIdx.x == 0 && t != kNone) gmin(st + W_BEST_IDX, t);
}

// dst <- dst merged with src (same layout): counts add, extrema by value, a cell takes the smaller
// chi2 and on a tie the lower index (~0 = empty loses every tie)
__global__ void fit_merge_kernel(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, int64_t items,
                                 FitParams P) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= items) return;
  int64_t wc, wi;
  if (i < W_HEADER) {
    if (i < W_BEST_CHI2 || (i >= W_COLBAD && i <= W_SEL_TOTAL)) { dst[i] += src[i]; return; }
    if (i >= W_COLMIN && i < W_COLMAX) { dst[i] = src[i] < dst[i] ? src[i] : dst[i]; return; }
    if (i >= W_COLMAX && i < W_COLBAD) { dst[i] = src[i] > dst[i] ? src[i] : dst[i]; return; }
    if (i != W_BEST_CHI2) return;
    wc = W_BEST_CHI2, wi = W_BEST_IDX;
  } else {
    int64_t o = i - W_HEADER;
    int m = 0;
    while (m < P.n_maps - 1 && o >= P.map[m].cells) o -= P.map[m].cells, ++m;
    wc = P.map[m].off + o, wi = wc + P.map[m].cells;
  }
  const uint64_t cs = src[wc], is = src[wi], cd = dst[wc], id = dst[wi];
  if (cs < cd || (cs == cd && is < id)) dst[wc] = cs, dst[wi] = is;
}

// ---- selection: count, scan, scatter (ascending flat indices appended at a device-side offset) ----
template <bool A16>
__device__ __forceinline__ bool sel_pred(const lzq_yield* rows, int64_t r, int64_t count, const FitParams& P,
                                         double level) {
  if (r >= count) return false;
  double x[6];
  fit_load_row<A16>(rows, r, x);
  const double c = fit_chi2(P, x);
  return isfinite(c) && c <= level;
}

template <bool A16>
__global__ void __launch_bounds__(kFitBlock) fit_sel_count_kernel(const lzq_yield* __restrict__ rows, int64_t count,
                                                                   double level, int64_t* __restrict__ counts,
                                                                   FitParams P) {
  __shared__ uint64_t red[kFitWaves];
  const int64_t tile = (int64_t)blockIdx.x * (kFitBlock * kFitSelIter);
  uint64_t n = 0;
  for (int it = 0; it < kFitSelIter; ++it) n += sel_pred<A16>(rows, tile + it * kFitBlock + threadIdx.x, count, P, level);
  const uint64_t t = block_reduce<OP_SUM>(n, red);
  if (threadIdx.x == 0) counts[blockIdx.x] = (int64_t)t;
}

// exclusive scan of counts[nb] in place (one block); counts[nb] <- the running offset before this
// chunk, which advances by the chunk's total
__global__ void __launch_bounds__(kFitBlock) fit_sel_scan_kernel(int64_t* __restrict__ counts, int64_t nb,
                                                                  uint64_t* __restrict__ st) {
  __shared__ int64_t wsum[kFitWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t carry = 0;
  for (int64_t base = 0; base < nb; base += kFitBlock) {
    const int64_t i = base + threadIdx.x;
    const int64_t v = i < nb ? counts[i] : 0;
    int64_t inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int64_t o = __shfl_up((long long)inc, s);
      if (lane >= s) inc += o;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int64_t woff = 0, total = 0;
    for (int w = 0; w < kFitWaves; ++w) {
      if (w < wave) woff += wsum[w];
      total += wsum[w];
    }
    if (i < nb) counts[i] = carry + woff + inc - v;
    carry += total;
  }
  if (threadIdx.x == 0) {
    counts[nb] = (int64_t)st[W_SEL_TOTAL];
    st[W_SEL_TOTAL] += (uint64_t)carry;
  }
}

template <bool A16>
__global__ void __launch_bounds__(kFitBlock) fit_sel_scatter_kernel(const lzq_yield* __restrict__ rows, int64_t start,
                                                                     int64_t count, double level,
                                                                     const int64_t* __restrict__ counts, int64_t nb,
                                                                     int64_t* __restrict__ sel, int64_t cap,
                                                                     FitParams P) {
  __shared__ int32_t wsum[kFitWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = (int64_t)blockIdx.x * (kFitBlock * kFitSelIter);
  int64_t off = counts[nb] + counts[blockIdx.x];
  if (off >= cap) return;   // block-uniform: nothing of this tile is kept
  for (int it = 0; it < kFitSelIter; ++it) {
    const int64_t r = tile + it * kFitBlock + threadIdx.x;
    const bool p = sel_pred<A16>(rows, r, count, P, level);
    const uint64_t mask = __ballot(p);
    const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
    __syncthreads();
    if (lane == 0) wsum[wave] = __popcll((unsigned long long)mask);
    __syncthreads();
    int woff = 0, total = 0;
    for (int w = 0; w < kFitWaves; ++w) {
      if (w < wave) woff += wsum[w];
      total += wsum[w];
    }
    const int64_t pos = off + woff + before;
    if (p && pos < cap) sel[pos] = start + r;
    off += total;
  }
}

}  // namespace lzq

using lzq::FitParams;

// host-side validation of a fit's terms, levels and maps into the kernels' parameter block
int lzq_fit_params(const char* who, const lzq_fit_term* terms, int32_t n_terms, const double* levels,
                      int32_t n_levels, const lzq_fit_map* maps, int32_t n_maps, FitParams* P, int64_t* words) {
  char msg[256];
#define FIT_FAIL(...) (snprintf(msg, sizeof msg, __VA_ARGS__), lzq_set_error(LZQ_EINVAL, msg))
  memset(P, 0, sizeof *P);
  if (n_terms < 0 || n_terms > LZQ_FIT_MAX_TERMS || (terms && n_terms < 1))
    return FIT_FAIL("%s: %d terms (1..%d)", who, n_terms, LZQ_FIT_MAX_TERMS);
  if (n_levels < 0 || n_levels > LZQ_FIT_MAX_LEVELS)
    return FIT_FAIL("%s: %d levels (0..%d)", who, n_levels, LZQ_FIT_MAX_LEVELS);
  if (n_maps < 0 || n_maps > LZQ_FIT_MAX_MAPS) return FIT_FAIL("%s: %d maps (0..%d)", who, n_maps, LZQ_FIT_MAX_MAPS);
  if ((n_terms > 0 && !terms) || (n_levels > 0 && !levels) || (n_maps > 0 && !maps))
    return FIT_FAIL("%s: bad arguments (null terms / levels / maps)", who);
  P->n_terms = n_terms, P->n_levels = n_levels, P->n_maps = n_maps;
  for (int t = 0; t < n_terms; ++t) {
    if (terms[t].field < 0 || terms[t].field > 5)
      return FIT_FAIL("%s: term %d: unknown field %d (0..5, the doubles of lzq_yield)", who, t, terms[t].field);
    if (!(terms[t].sigma > 0.0) || !isfinite(terms[t].sigma))
      return FIT_FAIL("%s: term %d: sigma must be finite and > 0", who, t);
    if (!isfinite(terms[t].target)) return FIT_FAIL("%s: term %d: target must be finite", who, t);
    P->field[t] = terms[t].field, P->target[t] = terms[t].target, P->sigma[t] = terms[t].sigma;
  }
  for (int l = 0; l < n_levels; ++l) {
    if (isnan(levels[l]) || (l > 0 && !(levels[l] > levels[l - 1])))
      return FIT_FAIL("%s: levels must be ascending", who);
    P->level[l] = levels[l];
  }
  int64_t off = LZQ_FIT_HEADER_WORDS;
  int32_t lds = 0;
  for (int m = 0; m < n_maps; ++m) {
    const lzq_fit_map& M = maps[m];
    if (M.n_axes < 1 || M.n_axes > 2) return FIT_FAIL("%s: map %d: %d axes (1 or 2)", who, m, M.n_axes);
    int64_t cells = 1;
    for (int a = 0; a < M.n_axes; ++a) {
      if (M.len[a] < 1 || M.stride[a] < 1 || M.stride[a] > LZQ_FIT_MAX_INDEX)
        return FIT_FAIL("%s: map %d: axis lengths and strides must be >= 1 (strides <= 2^62)", who, m);
      if (M.len[a] > LZQ_FIT_MAX_CELLS || (cells *= M.len[a]) > LZQ_FIT_MAX_CELLS)
        return FIT_FAIL("%s: map %d has more than 2^24 cells", who, m);
    }
    lzq::FitMapDev& D = P->map[m];
    D.stride0 = M.stride[0], D.len0 = M.len[0];
    D.stride1 = M.n_axes == 2 ? M.stride[1] : 1, D.len1 = M.n_axes == 2 ? M.len[1] : 1;
    D.off = off, D.cells = (int32_t)cells;
    D.lds_off = lds + cells <= lzq::kFitLdsCells ? lds : -1;
    if (D.lds_off >= 0) lds += (int32_t)cells;
    off += 2 * cells;
  }
  P->lds_cells = lds;
  *words = off;
  return LZQ_OK;
#undef FIT_FAIL
}

int lzq_fit_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return LZQ_OK;
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", who, hipGetErrorString(e));
  return lzq_set_error(LZQ_EHIP, msg);
}

static unsigned fit_grid(int64_t count) {
  const int64_t nb = (count + lzq::kFitBlock - 1) / lzq::kFitBlock;
  return (unsigned)(nb < lzq::kFitGrid ? nb : lzq::kFitGrid);
}

extern "C" {

int64_t lzq_fit_state_bytes(const lzq_fit_map* maps, int32_t n_maps) {
  FitParams P;
  int64_t words = 0;
  const int rc = lzq_fit_params("lzq_fit_state_bytes", nullptr, 0, nullptr, 0, maps, n_maps, &P, &words);
  return rc != LZQ_OK ? rc : words * 8;
}

int lzq_fit_reset(const lzq_fit_map* maps, int32_t n_maps, void* d_state, void* stream) {
  FitParams P;
  int64_t words = 0;
  const int rc = lzq_fit_params("lzq_fit_reset", nullptr, 0, nullptr, 0, maps, n_maps, &P, &words);
  if (rc != LZQ_OK) return rc;
  if (!d_state) return lzq_set_error(LZQ_EINVAL, "lzq_fit_reset: bad arguments (null state)");
  hipLaunchKernelGGL(lzq::fit_reset_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint64_t*)d_state, words, P);
  return lzq_fit_launched("lzq_fit_reset");
}

int lzq_fit_update(const lzq_fit_term* terms, int32_t n_terms, const double* levels, int32_t n_levels,
                   const lzq_fit_map* maps, int32_t n_maps, const lzq_yield* d_yields, int64_t start, int64_t count,
                   void* d_state, void* stream) {
  FitParams P;
  int64_t words = 0;
  if (!terms) return lzq_set_error(LZQ_EINVAL, "lzq_fit_update: bad arguments (null terms)");
  const int rc = lzq_fit_params("lzq_fit_update", terms, n_terms, levels, n_levels, maps, n_maps, &P, &words);
  if (rc != LZQ_OK) return rc;
  if (start < 0 || count < 0 || start > LZQ_FIT_MAX_INDEX - count || !d_state || (count > 0 && !d_yields))
    return lzq_set_error(LZQ_EINVAL, "lzq_fit_update: bad arguments (start, count >= 0, start + count <= 2^62, "
                                     "non-null buffers)");
  if (count == 0) return LZQ_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(fit_grid(count)), block(lzq::kFitBlock);
  uint64_t* S = (uint64_t*)d_state;
  if (((uintptr_t)d_yields & 15) == 0) {
    hipLaunchKernelGGL(lzq::fit_min_kernel<true>, grid, block, 0, st, d_yields, start, count, S, P);
    hipLaunchKernelGGL(lzq::fit_idx_kernel<true>, grid, block, 0, st, d_yields, start, count, S, P);
  } else {
    hipLaunchKernelGGL(lzq::fit_min_kernel<false>, grid, block, 0, st, d_yields, start, count, S, P);
    hipLaunchKernelGGL(lzq::fit_idx_kernel<false>, grid, block, 0, st, d_yields, start, count, S, P);
  }
  return lzq_fit_launched("lzq_fit_update");
}

int lzq_fit_select(const lzq_fit_term* terms, int32_t n_terms, double level, const lzq_yield* d_yields, int64_t start,
                   int64_t count, void* d_state, int64_t* d_selected, int64_t cap, void* stream) {
  FitParams P;
  int64_t words = 0;
  if (!terms) return lzq_set_error(LZQ_EINVAL, "lzq_fit_select: bad arguments (null terms)");
  const int rc = lzq_fit_params("lzq_fit_select", terms, n_terms, nullptr, 0, nullptr, 0, &P, &words);
  if (rc != LZQ_OK) return rc;
  if (isnan(level)) return lzq_set_error(LZQ_EINVAL, "lzq_fit_select: level is NaN");
  if (start < 0 || count < 0 || start > LZQ_FIT_MAX_INDEX - count || cap < 0 || !d_state || (count > 0 && !d_yields) ||
      (cap > 0 && !d_selected))
    return lzq_set_error(LZQ_EINVAL, "lzq_fit_select: bad arguments (start, count, cap >= 0, non-null buffers)");
  if (count == 0) return LZQ_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t tile = (int64_t)lzq::kFitBlock * lzq::kFitSelIter;
  const int64_t nb = (count + tile - 1) / tile;
  if (nb > 0x7fffffff) return lzq_set_error(LZQ_EINVAL, "lzq_fit_select: count too large for one call");
  int64_t* counts = nullptr;
  hipError_t e = hipMallocAsync((void**)&counts, (size_t)(nb + 1) * sizeof(int64_t), st);
  if (e != hipSuccess) return lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
  const dim3 grid((unsigned)nb), block(lzq::kFitBlock);
  uint64_t* S = (uint64_t*)d_state;
  const bool a16 = ((uintptr_t)d_yields & 15) == 0;
  if (a16)
    hipLaunchKernelGGL(lzq::fit_sel_count_kernel<true>, grid, block, 0, st, d_yields, count, level, counts, P);
  else
    hipLaunchKernelGGL(lzq::fit_sel_count_kernel<false>, grid, block, 0, st, d_yields, count, level, counts, P);
  hipLaunchKernelGGL(lzq::fit_sel_scan_kernel, dim3(1), block, 0, st, counts, nb, S);
  if (cap > 0) {
    if (a16)
      hipLaunchKernelGGL(lzq::fit_sel_scatter_kernel<true>, grid, block, 0, st, d_yields, start, count, level, counts,
                         nb, d_selected, cap, P);
    else
      hipLaunchKernelGGL(lzq::fit_sel_scatter_kernel<false>, grid, block, 0, st, d_yields, start, count, level, counts,
                         nb, d_selected, cap, P);
  }
  const int rl = lzq_fit_launched("lzq_fit_select");
  e = hipFreeAsync(counts, st);
  if (rl != LZQ_OK) return rl;
  if (e != hipSuccess) return lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
  return LZQ_OK;
}

int lzq_fit_merge(const lzq_fit_map* maps, int32_t n_maps, void* d_dst, const void* d_src, void* stream) {
  FitParams P;
  int64_t words = 0;
  const int rc = lzq_fit_params("lzq_fit_merge", nullptr, 0, nullptr, 0, maps, n_maps, &P, &words);
  if (rc != LZQ_OK) return rc;
  if (!d_dst || !d_src || d_dst == d_src)
    return lzq_set_error(LZQ_EINVAL, "lzq_fit_merge: bad arguments (two distinct non-null states)");
  const int64_t items = LZQ_FIT_HEADER_WORDS + (words - LZQ_FIT_HEADER_WORDS) / 2;
  hipLaunchKernelGGL(lzq::fit_merge_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint64_t*)d_dst, (const uint64_t*)d_src, items, P);
  return lzq_fit_launched("lzq_fit_merge");
}

}  // extern "C"
