// lzq_rank.hip -- the n rows of smallest chi2 of a sweep, ranked, with their records (no reference
// counterpart).
//
// The key of a row is (bits of chi2, flat index), compared as a 128-bit unsigned number: chi2 is the
// fit's expression (fit_chi2), never negative, so it orders like its bits, and flat indices are
// distinct, so the keys of a sweep's rows are a strict total order and "the n first" is one list.
//
// The state (include/lzq.h, "ranked points"):
//   [0] n  [1] filled  [2] n_valid  [3] n_invalid  [4] candidates of the running call  [5..7] 0
//   then n entries of 8 words in rank order: chi2 bits, index, the record's six doubles.
//
// lzq_rank_update is two launches:
//   rank_scan_kernel   the fit's row walk.  A block reads the list's last key tau once (all ones
//                      while the list is not full); a valid row whose key ranks before tau is a
//                      candidate, and a wave appends its candidates' keys to scratch behind ONE
//                      atomic add (ballot, popcount, lane offsets).  Once a sweep's early chunks have
//                      filled the list almost no row is one: the pass then writes two counters.
//   rank_reduce_kernel one block.  No candidate: return.  Candidates and list together within
//                      kRankCap keys: sort them in LDS (bitonic on the 128-bit key), keep n.  More:
//                      a radix select from the key's most significant byte down -- through the index
//                      word too, or a chunk of tied chi2 would not keep its lowest indices -- finds
//                      the n-th key, the keys up to it are gathered and sorted.  The new entries take
//                      their records from the old list (copied to scratch first) or from the chunk.
// lzq_rank_merge is the reduce with the other state's entries as the candidates.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <mutex>

#include "../../include/lzq.h"
#include "lzq_fit_common.h"
#include "lzq_internal.h"

namespace lzq {

constexpr int kRankBlock = 1024;              // threads of the reduce block
constexpr int kRankCap = LZQ_RANK_MAX_N;      // keys the reduce block sorts: 2 x 32 KB of LDS
constexpr int kRankCtl = 8;                   // words of the reduce block's scalars in scratch
constexpr uint64_t kRankInf = 0x7FF0000000000000ull;
constexpr uint64_t kRankNone = ~0ull;

enum { R_N = 0, R_FILLED = 1, R_NVALID = 2, R_NINVALID = 3, R_CAND = 4, R_HEADER = LZQ_RANK_HEADER_WORDS };
enum { C_TB = 0, C_TI = 1, C_NEED = 2, C_DONE = 3, C_COUNT = 4 };   // the reduce block's scalars

__device__ __forceinline__ bool key_lt(uint64_t ab, uint64_t ai, uint64_t bb, uint64_t bi) {
  return ab < bb || (ab == bb && ai < bi);
}

__global__ void rank_reset_kernel(uint64_t* st, int64_t words, int32_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= words) return;
  uint64_t v = 0;
  if (i == R_N) v = (uint64_t)n;
  else if (i >= R_HEADER) v = ((i - R_HEADER) & 7) == 0 ? kRankInf : ((i - R_HEADER) & 7) == 1 ? kRankNone : 0;
  st[i] = v;
}

// the keys of the chunk's rows that rank before the list's last entry -> cand[count] (16 B each)
template <bool A16>
__global__ void __launch_bounds__(kFitBlock) rank_scan_kernel(const lzq_yield* __restrict__ rows, int64_t start,
                                                               int64_t count, uint64_t* __restrict__ st, int32_t n,
                                                               ulonglong2* __restrict__ cand, FitParams P) {
  __shared__ uint64_t red[kFitWaves];
  const int lane = threadIdx.x & 63;
  // tau: nothing in this launch writes the entries or word [1] (the reduce block does, afterwards)
  const bool full = st[R_FILLED] >= (uint64_t)n;
  const uint64_t tb = full ? st[R_HEADER + 8 * (int64_t)(n - 1)] : kRankNone;
  const uint64_t ti = full ? st[R_HEADER + 8 * (int64_t)(n - 1) + 1] : kRankNone;
  uint64_t n_valid = 0, n_invalid = 0;
  const int64_t step = (int64_t)gridDim.x * kFitBlock;
  for (int64_t base = (int64_t)blockIdx.x * kFitBlock; base < count; base += step) {   // block-uniform trips
    const int64_t r = base + threadIdx.x;
    const bool active = r < count;
    double x[6] = {0, 0, 0, 0, 0, 0};
    if (active) fit_load_row<A16>(rows, r, x);
    const double c = fit_chi2(P, x);
    const bool has = active && isfinite(c);
    n_valid += has;
    n_invalid += active && !has;
    const uint64_t bits = (uint64_t)__double_as_longlong(c), flat = (uint64_t)(start + r);
    const bool is_cand = has && key_lt(bits, flat, tb, ti);
    const uint64_t mask = __ballot(is_cand);
    if (mask == 0) continue;   // wave-uniform: the steady state of a sweep
    const int leader = __ffsll((unsigned long long)mask) - 1;
    unsigned long long at = 0;
    if (lane == leader)
      at = __hip_atomic_fetch_add(st + R_CAND, (uint64_t)__popcll((unsigned long long)mask), __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
    at = __shfl(at, leader);
    const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
    const uint64_t pos = at + (uint64_t)before;
    if (is_cand && pos < (uint64_t)count) cand[pos] = make_ulonglong2(bits, flat);   // (a row appends at most once)
  }
  uint64_t t;
  t = block_reduce<OP_SUM>(n_valid, red);
  if (threadIdx.x == 0) gadd(st + R_NVALID, t);
  t = block_reduce<OP_SUM>(n_invalid, red);
  if (threadIdx.x == 0) gadd(st + R_NINVALID, t);
}

// the reduce block's scalars live in global scratch (its LDS is all keys): written by thread 0, read
// by every thread behind a barrier, past the vector cache
__device__ __forceinline__ void ctl_store(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ctl_load(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// byte `p` (0 = most significant of chi2, 15 = least significant of the index) of a key
__device__ __forceinline__ uint32_t key_digit(int p, uint64_t b, uint64_t i) {
  return (uint32_t)((p < 8 ? b >> (56 - 8 * p) : i >> (56 - 8 * (p - 8))) & 255u);
}
// whether a key shares the bytes above `p` with (tb, ti)
__device__ __forceinline__ bool key_prefix(int p, uint64_t b, uint64_t i, uint64_t tb, uint64_t ti) {
  if (p == 0) return true;
  if (p < 8) return (b >> (64 - 8 * p)) == (tb >> (64 - 8 * p));
  return b == tb && (p == 8 || (i >> (128 - 8 * p)) == (ti >> (128 - 8 * p)));
}

// the record words (6) of key (b, i) in a ranked list of `cnt` entries (8 words each), or null
__device__ __forceinline__ const uint64_t* rank_find(const uint64_t* list, uint32_t cnt, uint64_t b, uint64_t i) {
  uint32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (key_lt(list[8 * (int64_t)mid], list[8 * (int64_t)mid + 1], b, i)) lo = mid + 1;
    else hi = mid;
  }
  return lo < cnt && list[8 * (int64_t)lo] == b && list[8 * (int64_t)lo + 1] == i ? list + 8 * (int64_t)lo + 2 : nullptr;
}

// st <- the n first of st's entries and the m = min(*m_word, mcap) candidate keys cand[j * cstride],
// cand[j * cstride + 1].  update: the candidates are scratch keys (cstride 2, *m_word = st[R_CAND])
// of rows[index - start]; merge (src != null): they are src's entries.  One block of kRankBlock.
__global__ void __launch_bounds__(kRankBlock) rank_reduce_kernel(uint64_t* st, int32_t n,
                                                                  const uint64_t* cand, int32_t cstride,
                                                                  const uint64_t* m_word, int64_t mcap,
                                                                  uint64_t* ctl, uint64_t* old,
                                                                  const lzq_yield* __restrict__ rows, int64_t start,
                                                                  int64_t count, const uint64_t* src) {
  __shared__ uint64_t sk[kRankCap], si[kRankCap];      // the keys being sorted: chi2 bits, index
  uint32_t* hist = reinterpret_cast<uint32_t*>(si);    // the select's byte histogram, before si is filled
  const int tid = threadIdx.x;
  uint64_t m = *m_word;
  m = m > (uint64_t)mcap ? (uint64_t)mcap : m;
  const uint64_t f0 = st[R_FILLED];
  const uint32_t filled = (uint32_t)(f0 > (uint64_t)n ? (uint64_t)n : f0);
  const uint32_t src_filled = src ? (uint32_t)(src[R_FILLED] > (uint64_t)n ? (uint64_t)n : src[R_FILLED]) : 0;
  if (src && tid == 0) st[R_NVALID] += src[R_NVALID], st[R_NINVALID] += src[R_NINVALID];
  if (m == 0) return;                                  // block-uniform
  __syncthreads();                                     // every thread has read m
  if (!src && tid == 0) st[R_CAND] = 0;
  for (uint32_t i = tid; i < 8 * filled; i += kRankBlock) old[i] = st[R_HEADER + i];
  const uint64_t total = filled + m;
  auto key_at = [&](uint64_t i, uint64_t& b, uint64_t& x) {
    const uint64_t* p = i < filled ? st + R_HEADER + 8 * i : cand + (i - filled) * (uint64_t)cstride;
    b = p[0], x = p[1];
  };
  uint32_t got;
  if (total <= (uint64_t)kRankCap) {
    for (uint64_t i = tid; i < total; i += kRankBlock) key_at(i, sk[i], si[i]);
    got = (uint32_t)total;
  } else {
    // the n-th key (total > kRankCap >= n) by bytes: after byte p the keys that share T's bytes so
    // far hold the `need` smallest still to be taken.  When a byte's bucket is taken whole, or it
    // and the n - need keys below it fit the sort, the threshold is that prefix with ones below it.
    uint64_t tb = 0, ti = 0;
    uint32_t need = (uint32_t)n;
    for (int p = 0; p < 16; ++p) {
      for (int i = tid; i < 256; i += kRankBlock) hist[i] = 0;
      __syncthreads();
      uint32_t run_d = 0, run_c = 0;   // a thread's run of equal bytes is one LDS atomic (tied chi2: one bucket)
      for (uint64_t i = tid; i < total; i += kRankBlock) {
        uint64_t b, x;
        key_at(i, b, x);
        if (!key_prefix(p, b, x, tb, ti)) continue;
        const uint32_t d = key_digit(p, b, x);
        if (d != run_d && run_c) atomicAdd(&hist[run_d], run_c), run_c = 0;
        run_d = d, ++run_c;
      }
      if (run_c) atomicAdd(&hist[run_d], run_c);
      __syncthreads();
      if (tid == 0) {
        uint32_t d = 0, cum = 0;
        while (d < 255 && cum + hist[d] < need) cum += hist[d], ++d;
        need -= cum;
        const int sh = 56 - 8 * (p & 7);
        const bool whole = hist[d] <= need || ((uint32_t)n - need) + hist[d] <= (uint32_t)kRankCap;
        const uint64_t ones = whole && sh ? (1ull << sh) - 1 : 0;
        if (p < 8) tb |= ((uint64_t)d << sh) | ones, ti = whole ? kRankNone : 0;
        else ti |= ((uint64_t)d << sh) | ones;
        ctl_store(ctl + C_TB, tb), ctl_store(ctl + C_TI, ti), ctl_store(ctl + C_NEED, need);
        ctl_store(ctl + C_DONE, whole), ctl_store(ctl + C_COUNT, 0);
      }
      __syncthreads();
      tb = ctl_load(ctl + C_TB), ti = ctl_load(ctl + C_TI), need = (uint32_t)ctl_load(ctl + C_NEED);
      if (ctl_load(ctl + C_DONE)) break;               // block-uniform
    }
    __syncthreads();                                   // hist is read no more: si may be filled
    for (uint64_t i = tid; i < total; i += kRankBlock) {
      uint64_t b, x;
      key_at(i, b, x);
      if (key_lt(tb, ti, b, x)) continue;
      const uint64_t pos = __hip_atomic_fetch_add(ctl + C_COUNT, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (pos < (uint64_t)kRankCap) sk[pos] = b, si[pos] = x;
    }
    __syncthreads();
    const uint64_t c = ctl_load(ctl + C_COUNT);
    got = (uint32_t)(c > (uint64_t)kRankCap ? (uint64_t)kRankCap : c);
  }
  uint32_t pow2 = 1;
  while (pow2 < got) pow2 <<= 1;
  for (uint32_t i = got + tid; i < pow2; i += kRankBlock) sk[i] = kRankNone, si[i] = kRankNone;
  __syncthreads();
  for (uint32_t k = 2; k <= pow2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < (pow2 >> 1); t += kRankBlock) {
        const uint32_t a = 2 * t - (t & (j - 1)), b = a + j;     // the pair (a, a ^ j), a < b
        const uint64_t ab = sk[a], ai = si[a], bb = sk[b], bi = si[b];
        const bool up = (a & k) == 0;
        if (key_lt(bb, bi, ab, ai) == up) sk[a] = bb, si[a] = bi, sk[b] = ab, si[b] = ai;
      }
      __syncthreads();
    }
  }
  const uint32_t keep = got < (uint32_t)n ? got : (uint32_t)n;
  for (uint32_t j = tid; j < (uint32_t)n; j += kRankBlock) {
    uint64_t* e = st + R_HEADER + 8 * (int64_t)j;
    uint64_t w[8] = {kRankInf, kRankNone, 0, 0, 0, 0, 0, 0};
    if (j < keep) {
      w[0] = sk[j], w[1] = si[j];
      const uint64_t* rec = rank_find(old, filled, w[0], w[1]);
      if (!rec && src) rec = rank_find(src + R_HEADER, src_filled, w[0], w[1]);
      const int64_t r = (int64_t)w[1] - start;
      if (rec) {
#pragma unroll
        for (int c = 0; c < 6; ++c) w[2 + c] = rec[c];
      } else if (!src && r >= 0 && r < count) {
        const double* q = reinterpret_cast<const double*>(rows + r);
#pragma unroll
        for (int c = 0; c < 6; ++c) w[2 + c] = (uint64_t)__double_as_longlong(q[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) e[c] = w[c];
  }
  if (tid == 0) st[R_FILLED] = keep;
}

}  // namespace lzq

static int rank_n(const char* who, int32_t n) {
  if (n >= 1 && n <= LZQ_RANK_MAX_N) return LZQ_OK;
  char msg[256];
  snprintf(msg, sizeof msg, "%s: n = %d (1..%d)", who, n, LZQ_RANK_MAX_N);
  return lzq_set_error(LZQ_EINVAL, msg);
}

static int64_t rank_words(int32_t n) { return LZQ_RANK_HEADER_WORDS + 8 * (int64_t)n; }

// A call's scratch, allocated in stream order (freed with hipFreeAsync) from a pool of the library's
// own, one a device, that keeps what is freed: the device's default pool hands its memory back at
// the next synchronisation, and an update would then wait for 16 B a row of fresh memory, several
// times its own kernels.  Without such a pool (more devices than slots, or no pool support) the
// default pool serves.
static hipError_t rank_scratch(size_t bytes, hipStream_t s, uint64_t** out) {
  constexpr int kSlots = 64;
  static std::mutex mu;
  static hipMemPool_t pools[kSlots] = {};
  static bool tried[kSlots] = {};
  int dev = -1;
  hipMemPool_t pool = nullptr;
  if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kSlots) {
    std::lock_guard<std::mutex> lock(mu);
    if (!tried[dev]) {
      tried[dev] = true;
      hipMemPoolProps props = {};
      props.allocType = hipMemAllocationTypePinned;
      props.handleTypes = hipMemHandleTypeNone;
      props.location.type = hipMemLocationTypeDevice;
      props.location.id = dev;
      uint64_t keep = ~0ull;
      if (hipMemPoolCreate(&pools[dev], &props) != hipSuccess ||
          hipMemPoolSetAttribute(pools[dev], hipMemPoolAttrReleaseThreshold, &keep) != hipSuccess)
        pools[dev] = nullptr;
      (void)hipGetLastError();
    }
    pool = pools[dev];
  }
  return pool ? hipMallocFromPoolAsync((void**)out, bytes, pool, s) : hipMallocAsync((void**)out, bytes, s);
}

extern "C" {

int64_t lzq_rank_state_bytes(int32_t n) {
  const int rc = rank_n("lzq_rank_state_bytes", n);
  return rc != LZQ_OK ? rc : rank_words(n) * 8;
}

int lzq_rank_reset(int32_t n, void* d_state, void* stream) {
  const int rc = rank_n("lzq_rank_reset", n);
  if (rc != LZQ_OK) return rc;
  if (!d_state) return lzq_set_error(LZQ_EINVAL, "lzq_rank_reset: bad arguments (null state)");
  const int64_t words = rank_words(n);
  hipLaunchKernelGGL(lzq::rank_reset_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint64_t*)d_state, words, n);
  return lzq_fit_launched("lzq_rank_reset");
}

int lzq_rank_update(const lzq_fit_term* terms, int32_t n_terms, int32_t n, const lzq_yield* d_yields, int64_t start,
                    int64_t count, void* d_state, void* stream) {
  lzq::FitParams P;
  int64_t fit_words = 0;
  if (!terms) return lzq_set_error(LZQ_EINVAL, "lzq_rank_update: bad arguments (null terms)");
  int rc = lzq_fit_params("lzq_rank_update", terms, n_terms, nullptr, 0, nullptr, 0, &P, &fit_words);
  if (rc != LZQ_OK) return rc;
  if ((rc = rank_n("lzq_rank_update", n)) != LZQ_OK) return rc;
  if (start < 0 || count < 0 || start > LZQ_FIT_MAX_INDEX - count || !d_state || (count > 0 && !d_yields))
    return lzq_set_error(LZQ_EINVAL, "lzq_rank_update: bad arguments (start, count >= 0, start + count <= 2^62, "
                                     "non-null buffers)");
  if (count == 0) return LZQ_OK;
  hipStream_t s = (hipStream_t)stream;
  // scratch: the reduce block's scalars, the old list's entries, the candidates' keys
  const int64_t head = lzq::kRankCtl + 8 * (int64_t)n;
  uint64_t* scratch = nullptr;
  hipError_t e = rank_scratch((size_t)(head + 2 * count) * sizeof(uint64_t), s, &scratch);
  if (e != hipSuccess) return lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
  uint64_t* S = (uint64_t*)d_state;
  ulonglong2* cand = reinterpret_cast<ulonglong2*>(scratch + head);
  const int64_t nb = (count + lzq::kFitBlock - 1) / lzq::kFitBlock;
  const dim3 grid((unsigned)(nb < lzq::kFitGrid ? nb : lzq::kFitGrid)), block(lzq::kFitBlock);
  if (((uintptr_t)d_yields & 15) == 0)
    hipLaunchKernelGGL(lzq::rank_scan_kernel<true>, grid, block, 0, s, d_yields, start, count, S, n, cand, P);
  else
    hipLaunchKernelGGL(lzq::rank_scan_kernel<false>, grid, block, 0, s, d_yields, start, count, S, n, cand, P);
  hipLaunchKernelGGL(lzq::rank_reduce_kernel, dim3(1), dim3(lzq::kRankBlock), 0, s, S, n, (const uint64_t*)cand, 2,
                     (const uint64_t*)(S + lzq::R_CAND), count, scratch, scratch + lzq::kRankCtl, d_yields, start, count,
                     (const uint64_t*)nullptr);
  const int rl = lzq_fit_launched("lzq_rank_update");
  e = hipFreeAsync(scratch, s);
  if (rl != LZQ_OK) return rl;
  if (e != hipSuccess) return lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
  return LZQ_OK;
}

int lzq_rank_merge(int32_t n, void* d_dst, const void* d_src, void* stream) {
  const int rc = rank_n("lzq_rank_merge", n);
  if (rc != LZQ_OK) return rc;
  if (!d_dst || !d_src || d_dst == d_src)
    return lzq_set_error(LZQ_EINVAL, "lzq_rank_merge: bad arguments (two distinct non-null states)");
  hipStream_t s = (hipStream_t)stream;
  uint64_t* scratch = nullptr;
  hipError_t e = rank_scratch((size_t)(lzq::kRankCtl + 8 * (int64_t)n) * sizeof(uint64_t), s, &scratch);
  if (e != hipSuccess) return lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
  const uint64_t* src = (const uint64_t*)d_src;
  hipLaunchKernelGGL(lzq::rank_reduce_kernel, dim3(1), dim3(lzq::kRankBlock), 0, s, (uint64_t*)d_dst, n,
                     src + lzq::R_HEADER, 8, src + lzq::R_FILLED, (int64_t)n, scratch, scratch + lzq::kRankCtl,
                     (const lzq_yield*)nullptr, (int64_t)0, (int64_t)0, src);
  const int rl = lzq_fit_launched("lzq_rank_merge");
  e = hipFreeAsync(scratch, s);
  if (rl != LZQ_OK) return rl;
  if (e != hipSuccess) return lzq_set_error(LZQ_EHIP, hipGetErrorString(e));
  return LZQ_OK;
}

}  // extern "C"
