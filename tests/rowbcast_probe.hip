// Test-only probe of the 64-bit DPP row broadcast of gfx950 (row_newbcast:n -- every lane reads the operand from lane n of its
// own 16-lane row), compiled and loaded by tests/test_rowbcast_semantics_gpu.py.  Three forms, each for n = 0..15:
//   form 0   the 32-bit builtin on the two halves of a double (two v_mov_b32_dpp)
//   form 1   v_mov_b64_dpp
//   form 2   v_fmac_f64_dpp with destination == broadcast operand:  c += bcast_n(c) * b    (the Gauss-Jordan update of
//            kernels_chain.hpp, chain::eliminate)
// Lanes outside `mask` skip the operation (EXEC off) and keep the sentinel, so the result also shows what a lane reads whose
// source lane is switched off.  out[(form * 16 + n) * 64 + lane].
#include <hip/hip_runtime.h>

namespace {

template <int n>
__device__ __forceinline__ double bcast_builtin(const double v, const double old) {
  union { double d; int i[2]; } s, o;
  s.d = v;
  o.d = old;
  o.i[0] = __builtin_amdgcn_update_dpp(o.i[0], s.i[0], 0x150 + n, 0xf, 0xf, false);
  o.i[1] = __builtin_amdgcn_update_dpp(o.i[1], s.i[1], 0x150 + n, 0xf, 0xf, false);
  return o.d;
}

// inline asm gets no hazard handling: s_nop 4 = the five wait states between a scalar write of EXEC (the mask branch) and a DPP
// operation, which also cover the two between a vector write of the operand and its DPP read
template <int n>
__device__ __forceinline__ double bcast_mov(const double v, const double old) {
  double o = old;
  asm volatile("s_nop 4\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(o) : "v"(v), "n"(n));
  return o;
}

template <int n>
__device__ __forceinline__ double fmac_bcast(double c, const double b) {
  asm volatile("s_nop 4\n\tv_fmac_f64_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(c) : "v"(b), "n"(n));
  return c;
}

template <int n>
__device__ __forceinline__ void probe_n(const double v, const double b, const bool on, const double sentinel, double* out, const int lane) {
  double r0 = sentinel, r1 = sentinel, r2 = sentinel;
  if (on) {
    r0 = bcast_builtin<n>(v, sentinel);
    r1 = bcast_mov<n>(v, sentinel);
    r2 = fmac_bcast<n>(v, b);
  }
  out[(0 * 16 + n) * 64 + lane] = r0;
  out[(1 * 16 + n) * 64 + lane] = r1;
  out[(2 * 16 + n) * 64 + lane] = r2;
  if constexpr (n + 1 < 16) probe_n<n + 1>(v, b, on, sentinel, out, lane);
}

__global__ __launch_bounds__(64) void rowbcast_probe_kernel(const double* in, const double* b, double* out, unsigned long long mask,
                                                            double sentinel) {
  const int lane = threadIdx.x;
  probe_n<0>(in[lane], b[lane], ((mask >> lane) & 1ull) != 0, sentinel, out, lane);
}

}  // namespace

// in, b: 64 doubles; out: 3 * 16 * 64 doubles (host memory).  Returns the HIP error code (0 = success).
extern "C" int rowbcast_probe(const double* in, const double* b, double* out, unsigned long long mask, double sentinel) {
  constexpr size_t NOUT = 3 * 16 * 64;
  double *din = nullptr, *db = nullptr, *dout = nullptr;
  hipError_t e;
  if ((e = hipMalloc(&din, 64 * sizeof(double))) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&db, 64 * sizeof(double))) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&dout, NOUT * sizeof(double))) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(din, in, 64 * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(db, b, 64 * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(rowbcast_probe_kernel, dim3(1), dim3(64), 0, 0, din, db, dout, mask, sentinel);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(out, dout, NOUT * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
  (void)hipFree(din); (void)hipFree(db); (void)hipFree(dout);
  return 0;
}
