// Sum-of-squares moments with the psi operands in SGPRs and the accumulators in registers (the dominant lane-per-point family):
//   sreg_body, sreg_pipe_body / sreg_pipe_dispatch (hand-pipelined, tile-major table)   full pass and cost pass, one factor per wave
//   moments_sreg_kernel, moments_sreg_pair_kernel (two sets), moments_planar3_kernel (the planning graph's three sets: it runs
//   reg_body with a hinge policy beside the sreg bodies, hence kernels_reg.hpp)
//   scost_mirror_body / scost_body, moments_scost_kernel, moments_scost_pair_kernel     cost pass (m0 only), F factors per wave
// psi itself is split_psi_rows of kernels_split.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "kernels_reg.hpp"
#include "kernels_split.hpp"
#include "mom_args.hpp"

namespace gvi {

// ---------------------------------------------------------------------------------------------
// moments_sreg_kernel<D, M, FULL>: moments_reg_kernel for the sum-of-squares kinds with the psi operands
// taken from SGPRs (scalar cache, see split_psi_rows) instead of LDS broadcast reads.  f.H is [D][M]: a
// column's M entries contiguous, which is the group layout split_psi_rows walks.  Block = 4 waves = 4
// consecutive factors over the same range of points.
// ---------------------------------------------------------------------------------------------
template <int D, int M, bool FULL>
__device__ __forceinline__ void sreg_body(const MomArgs& a, const int bx, const int by_, double* usb, double* redb, const int kfix = -1,
                                          const int byfix = 0) {
  constexpr int NP = FULL ? (D + 1) * (D + 2) / 2 : 1;
  constexpr int NB = (NP + 15) / 16;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  double* us_w = usb + wave * 2 * M;               // [2 M] u0 | sgn of this wave's factor
  double (*red_w)[65] = (double (*)[65])(redb + wave * 16 * 65);
  const int kq = kfix >= 0 ? kfix : bx * 4 + wave;            // (kfix: see reg_body)
  const int by = kfix >= 0 ? byfix : by_;
  const bool active = kq < a.f.K && by < a.nchunk;
  const int k = __builtin_amdgcn_readfirstlane(active ? kq : a.f.K - 1);   // inactive waves redo the last factor
  if (lane < M) {
    us_w[lane] = a.f.u0[(size_t)k * M + lane];
    us_w[M + lane] = a.f.sgn[(size_t)k * M + lane];
  }
  __syncthreads();
  const uint64_t hbase = (uint64_t)(a.f.H + (size_t)k * M * D);
  cdouble_t* hq = (cdouble_t*)(((uint64_t)__builtin_amdgcn_readfirstlane((int)(hbase >> 32)) << 32) |
                               (uint32_t)__builtin_amdgcn_readfirstlane((int)hbase));
  double acc[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) acc[j] = 0.0;
  const int64_t Np = a.f.Np;
  const int64_t i0 = (int64_t)by * a.chunk;
  const int64_t i1 = (i0 + a.chunk < Np) ? i0 + a.chunk : Np;
  const double* __restrict__ Zt = a.f.Zt;
  const double* __restrict__ w = a.f.w;
  for (int64_t base = i0; base < i1; base += 64) {             // wave-uniform loop (chunks are whole 64-point tiles)
    const int64_t i = base + lane;
    double z[D];
#pragma unroll
    for (int c = 0; c < D; ++c) z[c] = Zt[(size_t)c * Np + i];
    const double wi = w[i];
    const double psi = split_psi_rows<D, M>(hq, us_w, us_w + M, z);
    const double cw = i < a.f.N ? wi * psi : 0.0;
    acc[0] += cw;
    if (FULL) {
      int q = 1 + D;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const double t = cw * z[c];
        acc[1 + c] += t;
#pragma unroll
        for (int e = c; e < D; ++e) { acc[q] = fma(t, z[e], acc[q]); ++q; }
      }
    }
  }
  double* out = a.partial + ((size_t)k * a.nchunk + by) * NP;
#pragma unroll
  for (int bb = 0; bb < NB; ++bb) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (bb * 16 + j < NP) red_w[j][lane] = acc[bb * 16 + j];
    wave_lds_sync();
    const int j = lane & 15, part = lane >> 4;
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < 16; ++t) s += red_w[j][part * 16 + t];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (active && lane < 16 && bb * 16 + lane < NP) out[bb * 16 + lane] = s;
    wave_lds_sync();
  }
}

// ---------------------------------------------------------------------------------------------
// sreg_pipe_body<D, M, SIGNED>: the full-moments body of sreg_body, scheduled by hand.
//
// What limits sreg_body (profiles/r01_i_pmc_*: VALU pipe 68 % busy, 23 % of wave-cycles waiting): (i) the 13
// global_load_dwordx2 of a 64-point step are issued at the loop head and waited on -- the 91 accumulators leave no room for
// a second copy of z and the compiler will not reuse z's registers in place; (ii) a wave issues at most one instruction
// per 4-cycle slot, so every non-VALU instruction (64-bit VGPR address arithmetic, SALU address arithmetic of the operand
// loads, LDS reads of u0 / sgn) takes a slot in which the SIMD's only other wave must have a VALU instruction ready;
// (iii) the scalar operand loads of the next group are issued right before the wait of the current one (SMEM returns out
// of order, the wait is lgkmcnt(0)), so two scalar-cache latencies per step are exposed.  Here:
//   * the table is read from its TILE-MAJOR copy Zq[tile][row][64] (row D = weights): ONE wave-uniform base, ONE 32-bit
//     per-lane offset that advances by a tile per step, rows addressed by the instruction's immediate offset -- no address
//     arithmetic at all, every load still one coalesced 512-byte line;
//   * the loads are inline asm (the compiler's waitcnt pass does not track them), so the schedule is explicit: row c of
//     the packed M2 update is the LAST reader of z[c]; right behind it the NEXT step's z[c] is loaded into the same
//     register pair (w goes out as soon as c = w psi is formed).  Loads return in order, so "z[c] has landed" is
//     s_waitcnt vmcnt(D - 1 - c), placed in front of column c of the psi phase: every column has the rest of the
//     accumulation plus part of the psi phase to cover the L2 latency;
//   * psi operands: H is addressed through one opaque base per step (immediate offsets, no SALU arithmetic); the first two
//     operand groups of the NEXT step are requested during the accumulation phase, and inside the psi phase the request of
//     group g+1 sits behind the first column of group g, i.e. behind the wait, so it has a full group of FMAs to land;
//   * u0 stays in registers and rides in as src2 of the first column's v_fma; the sign multiply disappears when every
//     residual row has positive weight (SIGNED = false: the usual positive-definite Q^-1 / K^-1).
// The asm waits carry the registers they guard as in/out operands, so the compiler can neither hoist a use above its wait
// nor reuse a register while a load is in flight; sched_barriers pin the issue points.  Same operations in the same order
// on the same values as sreg_body: results are bit-identical (tests/test_gpu_parity.py).
// ---------------------------------------------------------------------------------------------
#define GVI_ZLOAD(dst, voff, base, imm) \
  asm volatile("global_load_dwordx2 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(base), "n"(imm) : "memory")

// compile-time recursion instead of unrolled loops: the asm statements need their immediates as constant expressions
template <int D, int BIAS, int C = 0>
__device__ __forceinline__ void pipe_zload_all(double (&z)[D], const unsigned voff, const char* const Zq) {
  if constexpr (C < D) {
    GVI_ZLOAD(z[C], voff, Zq, C * 512 - BIAS);
    pipe_zload_all<D, BIAS, C + 1>(z, voff, Zq);
  }
}

// psi phase, column C: u += H[:, C] z[C].  Operand group g = C / GC lives in hA (g even) or hB (g odd); the request of
// group g + 1 goes out behind the first column of group g (g >= 1), i.e. behind that group's wait, into the buffer
// group g - 1 has left.
// FROM_ZERO: u starts at 0 (v = H z alone, the mirror-pair form) instead of u0
template <int D, int M, int GC, bool FROM_ZERO, int C = 0>
__device__ __forceinline__ void pipe_psi_cols(double (&u)[M], double (&z)[D], double (&hA)[GC * M], double (&hB)[GC * M],
                                              const double (&u0v)[M], cdouble_t* const hp) {
  if constexpr (C < D) {
    constexpr int g = C / GC, cc = C % GC, NG = D / GC, GS = GC * M;
    double (&h)[GS] = (g % 2 == 0) ? hA : hB;
    // z[C] has landed once at most the D - 1 - C younger loads are outstanding (loads return in order).  From column 1
    // on u[0] rides along as an in/out operand: the wait then sits between column C-1's and column C's update of u[0]
    // and cannot be hoisted above earlier FMAs (a hoisted wait would wait for the youngest load far too early).
    if constexpr (C == 0) {
      asm volatile("s_waitcnt vmcnt(%1)" : "+v"(z[0]) : "n"(D - 1));
#pragma unroll
      for (int rr = 0; rr < M; ++rr) u[rr] = FROM_ZERO ? h[rr] * z[0] : fma(h[rr], z[0], u0v[rr]);
    } else {
      asm volatile("s_waitcnt vmcnt(%2)" : "+v"(z[C]), "+v"(u[0]) : "n"(D - 1 - C));
#pragma unroll
      for (int rr = 0; rr < M; ++rr) u[rr] = fma(h[cc * M + rr], z[C], u[rr]);
    }
    if constexpr (cc == 0 && g >= 1 && g + 1 < NG) {
      double (&hnext)[GS] = (g % 2 == 0) ? hB : hA;
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < GS; ++j) hnext[j] = hp[(g + 1) * GS + j];
      __builtin_amdgcn_sched_barrier(0);
    }
    pipe_psi_cols<D, M, GC, FROM_ZERO, C + 1>(u, z, hA, hB, u0v, hp);
  }
}

// accumulation phase, row C of the packed second moment; behind it the NEXT step's z[C] is loaded into the same register
// MIRROR: cw = c(z) + c(-z) feeds the (even) second moment, cm = c(z) - c(-z) the (odd) first moment
template <int D, int BIAS, bool MIRROR, int C = 0>
__device__ __forceinline__ void pipe_acc_rows(double (&acc)[(D + 1) * (D + 2) / 2], double (&z)[D], const double cw, const double cm,
                                              const unsigned voff, const char* const Zq) {
  if constexpr (C < D) {
    constexpr int q0 = 1 + D + C * D - C * (C - 1) / 2;         // packed index of (C, C)
    const double tc = cw * z[C];
    if constexpr (MIRROR) acc[1 + C] = fma(cm, z[C], acc[1 + C]);
    else acc[1 + C] += tc;
#pragma unroll
    for (int e = C; e < D; ++e) acc[q0 + e - C] = fma(tc, z[e], acc[q0 + e - C]);
    __builtin_amdgcn_sched_barrier(0);
    GVI_ZLOAD(z[C], voff, Zq, C * 512 - BIAS);                  // row C was the last reader of z[C]
    __builtin_amdgcn_sched_barrier(0);
    pipe_acc_rows<D, BIAS, MIRROR, C + 1>(acc, z, cw, cm, voff, Zq);
  }
}

template <int D, int M, bool SIGNED, bool MIRROR>
__device__ __forceinline__ void sreg_pipe_body(const MomArgs& a, const int bx, const int by_, double* usb, double* redb, const int kfix = -1,
                                               const int byfix = 0) {
  constexpr int NP = (D + 1) * (D + 2) / 2;
  constexpr int NB = (NP + 15) / 16;
  // columns per SGPR operand group: the grouping of split_psi_rows (same operand traffic, same SGPR budget)
  constexpr int GC = (D % 4 == 0 && M <= 3) ? 4 : (D % 3 == 0 && M == 6 ? 3 : (D % 2 == 0 && M <= 6 ? 2 : 1));
  constexpr int NG = D / GC, GS = GC * M;
  constexpr int TB = (D + 1) * 512;                  // bytes of one 64-point tile of Zq
  constexpr int BIAS = (TB / 2) & ~7;                // centres the row offsets in the signed 13-bit immediate
  static_assert(D * 512 - BIAS <= 4095 && -BIAS >= -4096, "row offsets must fit the immediate field");
  static_assert(D <= 16, "vmcnt immediates");
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  double* us_w = usb + wave * 2 * M;               // [2 M] u0 | sgn of this wave's factor
  double (*red_w)[65] = (double (*)[65])(redb + wave * 16 * 65);
  const int kq = kfix >= 0 ? kfix : bx * 4 + wave;            // (kfix: see reg_body)
  const int by = kfix >= 0 ? byfix : by_;
  const bool active = kq < a.f.K && by < a.nchunk;
  const int k = __builtin_amdgcn_readfirstlane(active ? kq : a.f.K - 1);   // inactive waves redo the last factor
  if (lane < M) {
    us_w[lane] = a.f.u0[(size_t)k * M + lane];
    us_w[M + lane] = a.f.sgn[(size_t)k * M + lane];
  }
  __syncthreads();
  const uint64_t hbase = (uint64_t)(a.f.H + (size_t)k * M * D);
  cdouble_t* const hq = (cdouble_t*)(((uint64_t)__builtin_amdgcn_readfirstlane((int)(hbase >> 32)) << 32) |
                                     (uint32_t)__builtin_amdgcn_readfirstlane((int)hbase));
  double acc[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) acc[j] = 0.0;
  // unpaired: u0.  Mirror pairs: s_r u0_r (the odd moment's weights) and k0 = sum_r s_r u0_r^2 (see below)
  double u0v[M], k0 = 0.0;
#pragma unroll
  for (int r = 0; r < M; ++r) {
    u0v[r] = MIRROR ? us_w[M + r] * us_w[r] : us_w[r];
    if (MIRROR) k0 = fma(u0v[r], us_w[r], k0);
  }
  const int64_t Np = MIRROR ? a.f.Nmp : a.f.Np;
  const int64_t ck = MIRROR ? a.mchunk : a.chunk;
  const int64_t i0 = (int64_t)by * ck;
  const int64_t i1 = (i0 + ck < Np) ? i0 + ck : Np;
  const int ntiles = i1 > i0 ? (int)((i1 - i0) >> 6) : 0;   // chunks are whole 64-point tiles
  // (through readfirstlane, as hq: the loads below take the base as an SGPR operand of their asm, and inside a larger kernel
  // -- factor_block3_kernel with the symmetric-root products inlined beside it -- the compiler no longer proved it uniform)
  const uint64_t zbase = (uint64_t)(MIRROR ? a.f.Zm : a.f.Zq);
  const char* const Zq = (const char*)(((uint64_t)__builtin_amdgcn_readfirstlane((int)(zbase >> 32)) << 32) |
                                       (uint32_t)__builtin_amdgcn_readfirstlane((int)zbase));
  unsigned voff = (unsigned)(i0 >> 6) * (unsigned)TB + (unsigned)lane * 8u + (unsigned)BIAS;
  unsigned idx = (unsigned)(i0 + lane);
  const unsigned nvalid = (unsigned)(MIRROR ? a.f.Nm : a.f.N);
  double z[D], wi;
  double hA[GS], hB[GS];                             // operand groups of even / odd index (SGPRs)
  if (ntiles > 0) {
    // prologue: the first step's loads in the order the psi phase waits for them (w first), and its first two groups
    GVI_ZLOAD(wi, voff, Zq, D * 512 - BIAS);
    pipe_zload_all<D, BIAS>(z, voff, Zq);
    cdouble_t* hp = hq;
    asm volatile("" : "+s"(hp));
#pragma unroll
    for (int j = 0; j < GS; ++j) hA[j] = hp[j];
    if (NG > 1) {
#pragma unroll
      for (int j = 0; j < GS; ++j) hB[j] = hp[GS + j];
    }
  }
  for (int t = 0; t < ntiles; ++t) {
    cdouble_t* hp = hq;
    asm volatile("" : "+s"(hp));                      // opaque per step: the operand loads stay inside the loop
    double u[M];
    pipe_psi_cols<D, M, GC, MIRROR>(u, z, hA, hB, u0v, hp);
    double psi = 0.0;
    if constexpr (SIGNED) {
#pragma unroll
      for (int rr = 0; rr < M; ++rr) psi = fma(us_w[M + rr] * u[rr], u[rr], psi);
    } else {
#pragma unroll
      for (int rr = 0; rr < M; ++rr) psi = fma(u[rr], u[rr], psi);
    }
    asm volatile("" : "+v"(wi));                       // w was issued before z[0]: it has landed with z[0]'s wait
    double cw, cm = 0.0;
    if constexpr (MIRROR) {
      // +-pair from ONE v = H z (u holds v, psi holds q = sum_r s_r v_r^2):  psi(+-z) = sum_r s_r (u0_r +- v_r)^2, so
      //   c+ = w (psi(z) + psi(-z)) = 2 w (q + k0),          k0 = sum_r s_r u0_r^2  (per factor)
      //   c- = w (psi(z) - psi(-z)) = 4 w sum_r (s_r u0_r) v_r                       (no cancellation)
      double l = 0.0;
#pragma unroll
      for (int rr = 0; rr < M; ++rr) l = fma(u0v[rr], u[rr], l);
      const bool ok = idx < nvalid;                    // pad rows carry w = 0, z = 0 (finite values: the select is for safety)
      const double w2 = wi + wi;
      cw = ok ? w2 * (psi + k0) : 0.0;
      cm = ok ? (w2 + w2) * l : 0.0;
    } else {
      cw = idx < nvalid ? wi * psi : 0.0;              // pad rows carry w = 0, z = 0; the select keeps a NaN psi out
    }
    // next step (the last step re-reads its own tile: no out-of-range address, the values are never used)
    const bool more = t + 1 < ntiles;
    voff += more ? (unsigned)TB : 0u;
    idx += more ? 64u : 0u;
    __builtin_amdgcn_sched_barrier(0);
    GVI_ZLOAD(wi, voff, Zq, D * 512 - BIAS);
    // the next step's first two operand groups: the whole accumulation phase to land
#pragma unroll
    for (int j = 0; j < GS; ++j) hA[j] = hp[j];
    if (NG > 1) {
#pragma unroll
      for (int j = 0; j < GS; ++j) hB[j] = hp[GS + j];
    }
    __builtin_amdgcn_sched_barrier(0);
    acc[0] += cw;
    pipe_acc_rows<D, BIAS, MIRROR>(acc, z, cw, cm, voff, Zq);
  }
  // drain: nothing below may reuse z / w registers while the (unused) loads of the last step are in flight
  if (ntiles > 0) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(wi));
#pragma unroll
    for (int c = 0; c < D; ++c) asm volatile("" : "+v"(z[c]));
  }
  double* out = a.partial + ((size_t)k * a.nchunk + by) * NP;
#pragma unroll
  for (int bb = 0; bb < NB; ++bb) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (bb * 16 + j < NP) red_w[j][lane] = acc[bb * 16 + j];
    wave_lds_sync();
    const int j = lane & 15, part = lane >> 4;
    double s = 0.0;
#pragma unroll
    for (int t2 = 0; t2 < 16; ++t2) s += red_w[j][part * 16 + t2];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (active && lane < 16 && bb * 16 + lane < NP) out[bb * 16 + lane] = s;
    wave_lds_sync();
  }
}

// every residual row of the set has positive weight (sgn = +1): the sign multiply of psi is dropped
template <int D, int M>
__device__ __forceinline__ void sreg_pipe_dispatch(const MomArgs& a, const int bx, const int by, double* usb, double* redb, const int kfix = -1,
                                                   const int byfix = 0) {
  if (a.f.Zm) {
    if (a.f.all_pos) sreg_pipe_body<D, M, false, true>(a, bx, by, usb, redb, kfix, byfix);
    else sreg_pipe_body<D, M, true, true>(a, bx, by, usb, redb, kfix, byfix);
  } else {
    if (a.f.all_pos) sreg_pipe_body<D, M, false, false>(a, bx, by, usb, redb, kfix, byfix);
    else sreg_pipe_body<D, M, true, false>(a, bx, by, usb, redb, kfix, byfix);
  }
}

// PIPE selects the hand-pipelined body for the full pass (the cost pass has its own kernels)
// (256, 2): two blocks per CU = two waves per SIMD = at most 256 registers per lane INCLUDING AGPRs; without the second
// argument the compiler may take 256 + spill AGPRs and silently halve the occupancy
template <int D, int M, bool FULL, bool PIPE = false>
__global__ __launch_bounds__(256, 2) void moments_sreg_kernel(MomArgs a) {
  if (pred_skip(a.pred, a.pred_val)) return;
  __shared__ double us[4 * 2 * M];
  __shared__ double red[4 * 16 * 65];
  if constexpr (FULL && PIPE) sreg_pipe_dispatch<D, M>(a, blockIdx.x, blockIdx.y, us, red);
  else sreg_body<D, M, FULL>(a, blockIdx.x, blockIdx.y, us, red);
}

// Two sets in one launch (the chain pattern: binary priors d = 2n and unary factors d = n).  The launches are
// independent, so fusing them removes one dependent-launch boundary (~6 us on this part) and lets the small set's
// blocks fill the tail of the large one.  Blocks [0, nb0) belong to set 0 (x fastest), the rest to set 1.
template <int D0, int M0, int D1, int M1, bool FULL, bool PIPE = false>
__global__ __launch_bounds__(256, 2) void moments_sreg_pair_kernel(MomArgs a0, MomArgs a1, int nbx0, int nb0, int nbx1) {
  if (pred_skip(a0.pred, a0.pred_val)) return;
  constexpr int MM = M0 > M1 ? M0 : M1;
  __shared__ double us[4 * 2 * MM];
  __shared__ double red[4 * 16 * 65];
  const int b = blockIdx.x;
  if constexpr (FULL && PIPE) {
    // every block takes a prior item and then (strided) unary items, so the short unary blocks do not form a serial tail
    // behind the single resident round of prior blocks; the grid is max(nb0, nb1)
    if (b < nb0) sreg_pipe_dispatch<D0, M0>(a0, b % nbx0, b / nbx0, us, red);
    const int nb1 = nbx1 * a1.nchunk;
    for (int it = b; it < nb1; it += gridDim.x) {
      __syncthreads();
      sreg_pipe_dispatch<D1, M1>(a1, it % nbx1, it / nbx1, us, red);
    }
  } else {
    if (b < nb0) sreg_body<D0, M0, FULL>(a0, b % nbx0, b / nbx0, us, red);
    else sreg_body<D1, M1, FULL>(a1, (b - nb0) % nbx1, (b - nb0) / nbx1, us, red);
  }
}

// The planning graph of the reference's own GPU workload (helpers/CudaOperation.cu:74-119: minimum-acceleration priors d = 8,
// hinge-on-SDF obstacle factors d = 4, two fixed-prior anchors d = 4) as ONE moments launch: the three sets are independent,
// three launches were three dependent kernel boundaries (5.3 + 18.8 + 4.5 us, profiles/r03_f_kernel_stats_planar1k.csv)
// around one 18.8 us kernel.  Blocks [0, nb1) = the obstacle set (the heavy one first), [nb1, nb1 + nb0) = the priors, the rest
// the anchors; every block runs its set's body unchanged (bit-identical to the three launches).
template <bool FULL>
__global__ __launch_bounds__(256, 2) void moments_planar3_kernel(MomArgs a0, MomArgs a1, MomArgs a2, int nbx0, int nb0, int nbx1, int nb1, int nbx2,
                                                                  int pipe) {
  if (pred_skip(a0.pred, a0.pred_val)) return;
  using PsiH = PsiHingeSdf<4, KIND_HINGE_SDF_2D>;
  using PsiA = PsiQuad<4, 4>;
  constexpr int HS = PsiH::LDS > PsiA::LDS ? (PsiH::LDS > 2 * 4 ? PsiH::LDS : 2 * 4) : (PsiA::LDS > 2 * 4 ? PsiA::LDS : 2 * 4);
  __shared__ double hs[4 * HS];
  __shared__ double red[4 * 16 * 65];
  const int b = (int)blockIdx.x;
  if (b < nb1) reg_body<4, PsiH, FULL>(a1, b % nbx1, b / nbx1, hs, red);
  else if (b < nb1 + nb0) {
    // (the body the set's own launch would run: the hand-pipelined one for the full pass when the tile-major table is there)
    if constexpr (FULL) {
      if (pipe) sreg_pipe_dispatch<8, 4>(a0, (b - nb1) % nbx0, (b - nb1) / nbx0, hs, red);
      else sreg_body<8, 4, true>(a0, (b - nb1) % nbx0, (b - nb1) / nbx0, hs, red);
    } else sreg_body<8, 4, false>(a0, (b - nb1) % nbx0, (b - nb1) / nbx0, hs, red);
  }
  else reg_body<4, PsiA, FULL>(a2, (b - nb1 - nb0) % nbx2, (b - nb1 - nb0) / nbx2, hs, red);
}

// ---------------------------------------------------------------------------------------------
// moments_scost_kernel<D, M, F>: cost pass (m0 only) of the sum-of-squares kinds with SGPR operands and F
// factors per wave -- one load of the 64 sigma points feeds F psi evaluations, so the L1/L2 traffic per
// evaluation drops by F (the cost pass executes only M D + M FMAs per point and is otherwise bound by the
// 8-byte-per-lane table loads).  Block = 4 waves = 4 F consecutive factors over the same range of points.
// ---------------------------------------------------------------------------------------------
// Cost pass on the mirror-half table.  For a +-pair the cross terms of the two evaluations cancel:
//   psi(z) + psi(-z) = sum_r s_r [(u0_r + v_r)^2 + (u0_r - v_r)^2] = 2 (sum_r s_r v_r^2 + sum_r s_r u0_r^2),   v = H z,
// so a pair costs ONE H z (started from zero) and one sum of squares; k0 = sum_r s_r u0_r^2 is a per-factor constant.
// (The origin is stored with half its weight: v = 0 there and the pair formula returns w psi(0).)
template <int D, int M, int F>
__device__ __forceinline__ void scost_mirror_body(const MomArgs& a, const int bx, const int by, double* usb) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  double (*us_w)[3 * M] = (double (*)[3 * M])(usb + wave * F * 3 * M);     // [F][zeros | sgn | unused]
  const int k0i = (bx * 4 + wave) * F;
  cdouble_t* hq[F];
  double kc[F];
#pragma unroll
  for (int f = 0; f < F; ++f) {
    const int k = __builtin_amdgcn_readfirstlane(k0i + f < a.f.K ? k0i + f : a.f.K - 1);
    double kk = 0.0;
#pragma unroll
    for (int r = 0; r < M; ++r) { const double u = a.f.u0[(size_t)k * M + r]; kk = fma(a.f.sgn[(size_t)k * M + r] * u, u, kk); }
    kc[f] = kk;
    if (lane < M) {
      us_w[f][lane] = 0.0;
      us_w[f][M + lane] = a.f.sgn[(size_t)k * M + lane];
    }
    const uint64_t hbase = (uint64_t)(a.f.H + (size_t)k * M * D);
    hq[f] = (cdouble_t*)(((uint64_t)__builtin_amdgcn_readfirstlane((int)(hbase >> 32)) << 32) |
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)hbase));
  }
  __syncthreads();
  double acc[F];
#pragma unroll
  for (int f = 0; f < F; ++f) acc[f] = 0.0;
  const int64_t Np = a.f.Nmp;
  const int64_t i0 = (int64_t)by * a.mchunk;
  const int64_t i1 = (i0 + a.mchunk < Np) ? i0 + a.mchunk : Np;
  const double* __restrict__ Zm = a.f.Zm;
  for (int64_t base = i0; base < i1; base += 64) {             // wave-uniform loop over whole 64-pair tiles
    const double* tile = Zm + (size_t)(base >> 6) * (D + 1) * 64 + lane;
    double z[D];
#pragma unroll
    for (int c = 0; c < D; ++c) z[c] = tile[c * 64];
    const double w2 = 2.0 * tile[D * 64];                      // pad lanes: w = 0, z = 0
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const double q = split_psi_rows<D, M>(hq[f], us_w[f], us_w[f] + M, z);   // sum_r s_r (H z)_r^2
      acc[f] = fma(w2, q + kc[f], acc[f]);
    }
  }
#pragma unroll
  for (int f = 0; f < F; ++f) {
    double s = acc[f];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0 && k0i + f < a.f.K) a.partial[(size_t)(k0i + f) * a.nchunk + by] = s;
  }
}

template <int D, int M, int F>
__device__ __forceinline__ void scost_body(const MomArgs& a, const int bx, const int by, double* usb) {
  if (a.f.Zm) { scost_mirror_body<D, M, F>(a, bx, by, usb); return; }
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  double (*us_w)[2 * M] = (double (*)[2 * M])(usb + wave * F * 2 * M);     // [F][2 M]
  const int k0 = (bx * 4 + wave) * F;
  cdouble_t* hq[F];
#pragma unroll
  for (int f = 0; f < F; ++f) {
    const int k = __builtin_amdgcn_readfirstlane(k0 + f < a.f.K ? k0 + f : a.f.K - 1);
    if (lane < M) {
      us_w[f][lane] = a.f.u0[(size_t)k * M + lane];
      us_w[f][M + lane] = a.f.sgn[(size_t)k * M + lane];
    }
    const uint64_t hbase = (uint64_t)(a.f.H + (size_t)k * M * D);
    hq[f] = (cdouble_t*)(((uint64_t)__builtin_amdgcn_readfirstlane((int)(hbase >> 32)) << 32) |
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)hbase));
  }
  __syncthreads();
  double acc[F];
#pragma unroll
  for (int f = 0; f < F; ++f) acc[f] = 0.0;
  const int64_t Np = a.f.Np;
  const int64_t i0 = (int64_t)by * a.chunk;
  const int64_t i1 = (i0 + a.chunk < Np) ? i0 + a.chunk : Np;
  const double* __restrict__ Zt = a.f.Zt;
  const double* __restrict__ w = a.f.w;
  for (int64_t base = i0; base < i1; base += 64) {             // wave-uniform loop (chunks are whole 64-point tiles)
    const int64_t i = base + lane;
    double z[D];
#pragma unroll
    for (int c = 0; c < D; ++c) z[c] = Zt[(size_t)c * Np + i];
    const double wi = i < a.f.N ? w[i] : 0.0;
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const double psi = split_psi_rows<D, M>(hq[f], us_w[f], us_w[f] + M, z);
      acc[f] += i < a.f.N ? wi * psi : 0.0;
    }
  }
#pragma unroll
  for (int f = 0; f < F; ++f) {
    double s = acc[f];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0 && k0 + f < a.f.K) a.partial[(size_t)(k0 + f) * a.nchunk + by] = s;
  }
}

template <int D, int M, int F>
__global__ __launch_bounds__(256) void moments_scost_kernel(MomArgs a) {
  if (pred_skip(a.pred, a.pred_val)) return;
  __shared__ double us[4 * F * 3 * M];
  scost_body<D, M, F>(a, blockIdx.x, blockIdx.y, us);
}

template <int D0, int M0, int D1, int M1, int F>
__global__ __launch_bounds__(256) void moments_scost_pair_kernel(MomArgs a0, MomArgs a1, int nbx0, int nb0, int nbx1) {
  if (pred_skip(a0.pred, a0.pred_val)) return;
  constexpr int MM = M0 > M1 ? M0 : M1;
  __shared__ double us[4 * F * 3 * MM];
  const int b = blockIdx.x;
  if (b < nb0) scost_body<D0, M0, F>(a0, b % nbx0, b / nbx0, us);
  else scost_body<D1, M1, F>(a1, (b - nb0) % nbx1, (b - nb0) / nbx1, us);
}

}  // namespace gvi
