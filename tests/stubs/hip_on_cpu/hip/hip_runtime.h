// <hip/hip_runtime.h> for a CPU build of a kernel header (tests/stubs/interp_kernels_on_cpu.cpp): one workgroup at a time, one
// std::thread per lane, a barrier for __syncthreads and two for __shfl (every lane of the workgroup must reach it).  Test only.
#pragma once
#include <barrier>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>
#include <algorithm>
#include <functional>
#define __global__
#define __device__
#define __host__
#define __shared__ static
#define __launch_bounds__(...)
struct u3 { unsigned x = 0, y = 0, z = 0; };
inline thread_local u3 threadIdx;
inline u3 blockIdx, blockDim;
inline std::barrier<>* g_bar = nullptr;
inline double g_shf[1024];
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline double __shfl(double v, int src) {
  g_shf[threadIdx.x] = v;
  g_bar->arrive_and_wait();
  const double r = g_shf[(threadIdx.x & ~63u) + ((unsigned)src & 63u)];
  g_bar->arrive_and_wait();
  return r;
}
inline void sincos(double x, double* s, double* c) { *s = std::sin(x); *c = std::cos(x); }
using std::min;
template <class K, class A>
void launch(K kern, unsigned gx, unsigned gy, unsigned threads, A args) {
  blockDim.x = threads;
  for (unsigned by = 0; by < gy; ++by)
    for (unsigned bx = 0; bx < gx; ++bx) {
      blockIdx.x = bx; blockIdx.y = by;
      std::barrier<> bar(threads);
      g_bar = &bar;
      std::vector<std::thread> th;
      for (unsigned t = 0; t < threads; ++t) th.emplace_back([&, t] { threadIdx.x = t; kern(args); });
      for (auto& x : th) x.join();
    }
}
