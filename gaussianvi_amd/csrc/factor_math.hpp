// Scalar and wave arithmetic shared by the factor-stage kernels (prep, closed forms, orbit walks, read-out rule).
#pragma once
#include <hip/hip_runtime.h>

namespace gvi {

// reciprocal / reciprocal square root: hardware seed + one Newton-Raphson step (~1e-16 relative)
__device__ __forceinline__ double rcp_nr(double x) {
  double r = __builtin_amdgcn_rcp(x);
  return fma(fma(-x, r, 1.0), r, r);
}
__device__ __forceinline__ double rsq_nr(double x) {
  const double r = __builtin_amdgcn_rsq(x);
  return r * fma(-0.5 * x * r, r, 1.5);
}

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

}  // namespace gvi
