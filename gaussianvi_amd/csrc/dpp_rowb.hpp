// 64-bit DPP row broadcast (gfx950: row_newbcast:n is the one DPP control of the 64-bit ALU), shared by the chain's
// Gauss-Jordan (kernels_chain.hpp, gj_rowb) and the Cholesky products of the factor pass (kernels_prep.hpp, prep_chol_body).
#pragma once
#include <hip/hip_runtime.h>

namespace gvi {

// Every lane reads the operand from lane P of its OWN 16-lane row (tests/test_rowbcast_semantics_gpu.py pins this on the device,
// also for lanes switched off).  Inline asm gets no hazard handling from the compiler: a vector write of a register needs two
// wait states before a DPP read of it.  rowb_mov opens with the s_nop that covers them (WS = 4: also the five after a vector
// write of EXEC, for callers with divergent code in front); rowb_fmac and rowb_fma carry none -- their caller keeps every
// writer of the broadcast operand in front of a rowb_mov or a rowb_settle (rowb_pin fixes compiler-written values there).
template <int P, int WS>
__device__ __forceinline__ double rowb_mov(const double v) {
  double o;
  if constexpr (WS > 1) asm volatile("s_nop 4\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(o) : "v"(v), "n"(P));
  else asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(o) : "v"(v), "n"(P));
  return o;
}
// c += (c of lane P of the row) * b
template <int P>
__device__ __forceinline__ void rowb_fmac(double& c, const double b) {
  asm volatile("v_fmac_f64_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(c) : "v"(b), "n"(P));
}
// acc += (src of lane P of the row) * (-mul): the destination is not the broadcast operand (tests/test_rowb_fma_semantics_gpu.py
// pins this form on the device).  The same bits as fma(-mul, bcast_P(src), acc).
template <int P>
__device__ __forceinline__ void rowb_fma(double& acc, const double src, const double mul) {
  asm volatile("v_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(mul), "n"(P));
}
// the value is in its register HERE (volatile asm statements keep their order)
__device__ __forceinline__ void rowb_pin(double& v) { asm volatile("" : "+v"(v)); }
// rowb_pin + the two wait states a DPP read of the value needs, for a value the instruction in front has just written
__device__ __forceinline__ void rowb_settle(double& v) { asm volatile("s_nop 1" : "+v"(v)); }
template <int P>
__device__ __forceinline__ int rowb_int(const int v) { return __builtin_amdgcn_update_dpp(0, v, 0x150 + P, 0xf, 0xf, false); }

}  // namespace gvi
