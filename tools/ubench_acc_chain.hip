// ubench_acc_chain.hip -- the accumulate-only z-loop of the dense quadrature (csrc/lzq_quad.h zsum_dead /
// zsum_held: F = fma(omega'_k, v, F) per node, omega' the fma's scalar operand, 8-node batches) at the
// headline kernel's own shape, with G = 1, 2, 4, 8 independent F chains per lane (what LZQ_GROUP_SEG
// gives a lane by sweeping G passes through z together) and three feeds of omega':
//
//   znode   the shipped interleaved ZNode table {g4, omega'} (19.2 KB), scalar loads
//   packed  an omega'-only array (9.6 KB), scalar loads
//   args    no loads at all: the batch's 8 omega' are kernel arguments (the chain alone)
//
// Geometry: 1024-thread blocks, __launch_bounds__(1024, 8), 77,824 B of dynamic LDS so that exactly two
// blocks fit a CU (8 waves per SIMD), two blocks per CU on every CU.  Every wave runs kChainPasses
// chain-passes of 1200 nodes whatever G is (kChainPasses / G sweeps of G chains), so the fma count is
// the same in every variant.  Printed, one JSON line per variant, three runs each: SIMD-cycles per
// wave-fma from s_memtime (one wave's own clock, divided by the 8 waves sharing its SIMD) and from HIP
// events (wall time x measured clock x SIMDs / wave-fmas), and their spread over the runs.
//
//   hipcc -O3 --offload-arch=gfx950 -o ubench_acc_chain tools/ubench_acc_chain.hip && ./ubench_acc_chain
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

constexpr int kNZ = 1200, kUnroll = 8, kChainPasses = 64, kThreads = 1024, kWavesPerSimd = 8;
constexpr int kLdsBytes = 77824;  // the headline kernel's LDS block size: two blocks per CU, not three
constexpr int kRuns = 3;

struct ZNode {
  double g4, omega;
};
struct Om8 {
  double om[kUnroll];
};
enum Feed { kZNode = 0, kPacked = 1, kArgs = 2 };

template <int G, int FEED>
__global__ __launch_bounds__(kThreads, kWavesPerSimd) void acc_chain(const ZNode* __restrict__ zt,
                                                                     const double* __restrict__ omp, Om8 args,
                                                                     double* out, long long* clk) {
  extern __shared__ double lds[];
  if (threadIdx.x == 0 && out == nullptr) lds[0] = 0.0;  // (the allocation is what matters)
  double v[G], F[G];
#pragma unroll
  for (int b = 0; b < G; ++b) {
    v[b] = 1.0 + 1e-3 * (double)((threadIdx.x & 63) + 64 * b);
    F[b] = 0.0;
    asm volatile("" : "+v"(F[b]));
  }
  const long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int p = 0; p < kChainPasses / G; ++p) {
    int off = 0;
    asm volatile("" : "+s"(off));  // a new sweep reads the table again (an opaque offset: the
    const ZNode* z = zt + off;     // pointers stay kernel arguments, so the loads stay scalar)
    const double* o = omp + off;
    for (int k = 0; k < kNZ; k += kUnroll) {
      double om[kUnroll];
#pragma unroll
      for (int kk = 0; kk < kUnroll; ++kk)
        om[kk] = FEED == kZNode ? z[k + kk].omega : FEED == kPacked ? o[k + kk] : args.om[kk];
#pragma unroll
      for (int kk = 0; kk < kUnroll; ++kk)
#pragma unroll
        for (int b = 0; b < G; ++b) F[b] = __builtin_fma(om[kk], v[b], F[b]);
    }
  }
  const long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    clk[0] = t1 - t0;
    clk[1] = r1 - r0;
  }
  double s = 0.0;
#pragma unroll
  for (int b = 0; b < G; ++b) s += F[b];
  if (s == 12345.678 && out != nullptr) out[threadIdx.x] = s;
}

typedef void (*kfn)(const ZNode*, const double*, Om8, double*, long long*);

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                     \
      exit(1);                                                                    \
    }                                                                             \
  } while (0)

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount, blocks = 2 * cus;
  ZNode hz[kNZ];
  double ho[kNZ];
  Om8 args;
  for (int k = 0; k < kNZ; ++k) {
    ho[k] = 1e-3 * (double)(k % 7 + 1);
    hz[k].g4 = (double)k / kNZ;
    hz[k].omega = ho[k];
  }
  for (int kk = 0; kk < kUnroll; ++kk) args.om[kk] = ho[kk];
  ZNode* dz;
  double *dom, *out;
  long long* clk;
  CHECK(hipMalloc(&dz, sizeof hz));
  CHECK(hipMalloc(&dom, sizeof ho));
  CHECK(hipMalloc(&out, kThreads * sizeof(double)));
  CHECK(hipMalloc(&clk, 16));
  CHECK(hipMemcpy(dz, hz, sizeof hz, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dom, ho, sizeof ho, hipMemcpyHostToDevice));
  struct {
    const char* feed;
    int G;
    kfn fn;
  } ks[] = {
      {"znode", 1, acc_chain<1, kZNode>},   {"znode", 2, acc_chain<2, kZNode>},   {"znode", 4, acc_chain<4, kZNode>},
      {"znode", 8, acc_chain<8, kZNode>},   {"packed", 1, acc_chain<1, kPacked>}, {"packed", 2, acc_chain<2, kPacked>},
      {"packed", 4, acc_chain<4, kPacked>}, {"packed", 8, acc_chain<8, kPacked>}, {"args", 1, acc_chain<1, kArgs>},
      {"args", 2, acc_chain<2, kArgs>},     {"args", 4, acc_chain<4, kArgs>},     {"args", 8, acc_chain<8, kArgs>},
  };
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const double fma_per_wave = (double)kChainPasses * kNZ;
  for (auto& k : ks) {
    CHECK(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    int per_cu = 0;
    CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k.fn, kThreads, kLdsBytes));
    hipLaunchKernelGGL(k.fn, dim3(blocks), dim3(kThreads), kLdsBytes, 0, dz, dom, args, out, clk);  // warm-up
    CHECK(hipDeviceSynchronize());
    double in_k[kRuns], wall[kRuns], ghz_last = 0.0;
    for (int r = 0; r < kRuns; ++r) {
      CHECK(hipEventRecord(e0, 0));
      hipLaunchKernelGGL(k.fn, dim3(blocks), dim3(kThreads), kLdsBytes, 0, dz, dom, args, out, clk);
      CHECK(hipEventRecord(e1, 0));
      CHECK(hipEventSynchronize(e1));
      float ms = 0;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      long long c[2];
      CHECK(hipMemcpy(c, clk, 16, hipMemcpyDeviceToHost));
      const double ghz = (double)c[0] / ((double)c[1] * 10.0);  // s_memrealtime counts at 100 MHz
      in_k[r] = (double)c[0] / (fma_per_wave * kWavesPerSimd);
      // wall cycles x SIMDs / wave-fmas: blocks * 16 waves over cus * 4 SIMDs = 8 waves per SIMD
      wall[r] = (double)ms * 1e6 * ghz * (4.0 * cus) / (fma_per_wave * blocks * (kThreads / 64));
      ghz_last = ghz;
    }
    auto lo = [](const double* a) { double m = a[0]; for (int i = 1; i < kRuns; ++i) m = a[i] < m ? a[i] : m; return m; };
    auto hi = [](const double* a) { double m = a[0]; for (int i = 1; i < kRuns; ++i) m = a[i] > m ? a[i] : m; return m; };
    printf("{\"feed\": \"%s\", \"chains\": %d, \"blocks_per_cu\": %d, \"waves_per_simd\": %d, "
           "\"cyc_per_wave_fma_memtime\": [%.3f, %.3f, %.3f], \"cyc_per_wave_fma_events\": [%.3f, %.3f, %.3f], "
           "\"best_memtime\": %.3f, \"spread_memtime\": %.3f, \"best_events\": %.3f, \"spread_events\": %.3f, "
           "\"ghz\": %.3f, \"cus\": %d}\n",
           k.feed, k.G, per_cu, per_cu * (kThreads / 64) / 4, in_k[0], in_k[1], in_k[2], wall[0], wall[1], wall[2],
           lo(in_k), hi(in_k) - lo(in_k), lo(wall), hi(wall) - lo(wall), ghz_last, cus);
    fflush(stdout);
  }
  CHECK(hipDeviceSynchronize());
  return 0;
}
