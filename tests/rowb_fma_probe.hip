// Test-only probe of the row-broadcast multiply-add of the Cholesky products (csrc/dpp_rowb.hpp, rowb_fma; kernels_prep.hpp,
// prep_chol_body), compiled and loaded by tests/test_rowb_fma_semantics_gpu.py:
//     v_fmac_f64_dpp acc, src, -mul row_newbcast:n        acc += (src of lane n of the own 16-lane row) * (-mul)
// with the destination a register of its own (not the broadcast operand, unlike the form tests/rowbcast_probe.hip pins) and
// the negated plain multiplier, for n = 0..15.  Every lane runs it, as in the library.  out[n * 64 + lane].
#include <hip/hip_runtime.h>

namespace {

// s_nop 1: the two wait states between the vector write of src (its load's result is moved / converted by compiler-written
// instructions) and the DPP read of it
template <int n>
__device__ __forceinline__ double fma_bcast(double acc, const double src, const double mul) {
  asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(mul), "n"(n));
  return acc;
}

template <int n>
__device__ __forceinline__ void probe_n(const double acc, const double src, const double mul, double* out, const int lane) {
  out[n * 64 + lane] = fma_bcast<n>(acc, src, mul);
  if constexpr (n + 1 < 16) probe_n<n + 1>(acc, src, mul, out, lane);
}

__global__ __launch_bounds__(64) void rowb_fma_probe_kernel(const double* acc, const double* src, const double* mul, double* out) {
  const int lane = threadIdx.x;
  probe_n<0>(acc[lane], src[lane], mul[lane], out, lane);
}

}  // namespace

// acc, src, mul: 64 doubles each; out: 16 * 64 doubles (host memory).  Returns the HIP error code (0 = success).
extern "C" int rowb_fma_probe(const double* acc, const double* src, const double* mul, double* out) {
  constexpr size_t NOUT = 16 * 64;
  double *din = nullptr, *dout = nullptr;
  hipError_t e;
  if ((e = hipMalloc(&din, 3 * 64 * sizeof(double))) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&dout, NOUT * sizeof(double))) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(din, acc, 64 * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(din + 64, src, 64 * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(din + 128, mul, 64 * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(rowb_fma_probe_kernel, dim3(1), dim3(64), 0, 0, din, din + 64, din + 128, dout);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(out, dout, NOUT * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
  (void)hipFree(din); (void)hipFree(dout);
  return 0;
}
