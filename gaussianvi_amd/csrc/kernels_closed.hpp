// Quadrature-free moments: closed forms of E[psi], E[z psi], E[z z^T psi] for a quadratic psi, the separable squared hinge of
// HINGE_BOX and the row hinges of HINGE_HALFSPACE.  They write the packed one-chunk layout of the sigma-point kernels, so the
// epilogue (kernels_epilogue.hpp) is shared.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "box_moments.hpp"
#include "device_common.hpp"
#include "factor_lds.hpp"
#include "factor_math.hpp"
#include "halfspace_moments.hpp"
#include "mom_args.hpp"

namespace gvi {

// ---------------------------------------------------------------------------------------------
// moments_closed_kernel: quadrature-free moments of a sum-of-squares psi = sum_r s_r (u0 + H z)_r^2,
// z ~ N(0, I)  [NGDFactorizedLinear::calculate_partial_V, ngd/NGDFactorizedLinear.h:93-129].  Isserlis in
// the whitened space:  E[psi] = sum_r s_r (u0_r^2 + |h_r|^2),  E[z psi] = 2 sum_r s_r u0_r h_r,
// E[z z^T psi] = E[psi] I + 2 sum_r s_r h_r h_r^T.  Writes the same packed layout as one chunk of the
// sigma-point kernels, so the epilogue (back-transform, Lambda, temperature) is shared.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void moments_closed_kernel(MomArgs a) {
  if (pred_skip(a.pred, a.pred_val)) return;
  const FactorDev& f = a.f;
  const int d = f.d, m = f.m, k = blockIdx.x;
  const double* H = f.H + (size_t)k * d * m;      // [d][m]
  const double* u0 = f.u0 + (size_t)k * m;
  const double* sg = f.sgn + (size_t)k * m;
  double m0 = 0.0;
  for (int r = 0; r < m; ++r) {
    double q = u0[r] * u0[r];
    for (int c = 0; c < d; ++c) q = fma(H[c * m + r], H[c * m + r], q);
    m0 = fma(sg[r], q, m0);
  }
  const int npo = a.full ? npairs(d) : 1;
  double* out = a.partial + (size_t)k * a.nchunk * npo;
  if (threadIdx.x == 0) out[0] = m0;
  if (!a.full) return;
  for (int j = 1 + threadIdx.x; j < npo; j += 64) {
    double v = 0.0;
    if (j <= d) {
      const int c = j - 1;
      for (int r = 0; r < m; ++r) v = fma(sg[r] * u0[r], H[c * m + r], v);
      v *= 2.0;
    } else {
      int rem = j - 1 - d, row = 0;
      while (rem >= d - row) { rem -= d - row; ++row; }
      const int col = row + rem;
      for (int r = 0; r < m; ++r) v = fma(sg[r] * H[row * m + r], H[col * m + r], v);
      v = 2.0 * v + (row == col ? m0 : 0.0);
    }
    out[j] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// moments_box_closed_kernel: quadrature-free moments of the HINGE_BOX psi (box_moments.hpp).  psi is a
// sum over coordinates of functions of ONE coordinate x_i = mu_i + s_i z (s_i = row i of S, sd_i = |s_i|), so with the 1-D
// expectations (e0, e1, e2)_i of box_coordinate and Stein's lemma
//   E[psi] = sum_i e0_i,   E[z psi] = sum_i s_i e1_i,   E[z z^T psi] = E[psi] I + sum_i s_i s_i^T e2_i
// for any root S S^T = Sigma, S row-major as prep writes it (x = mu + S z: Ss[i * d + c] is entry c of ROW i).  Only the
// symmetric root ever reaches this kernel (FactorSet::dev sets chol for the sum-of-squares kinds alone), for which rows and
// columns coincide: the row convention is NOT exercised by any test, and a later switch of this kind to the Cholesky prep
// (S = L, lower triangular) must test it before relying on it.  One wave per factor like moments_closed_kernel and the same packed one-chunk layout, so the
// epilogue is shared.  Lane i takes coordinate i (erfc and exp once per finite side), S and (e1, e2) go through LDS
// (d d + 2 d doubles of dynamic LDS), then lane j forms output j as a d-long sum in ascending i: deterministic.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void moments_box_closed_kernel(MomArgs a) {
  if (pred_skip(a.pred, a.pred_val)) return;
  extern __shared__ double bsm[];
  const FactorDev& f = a.f;
  const int d = f.d, k = blockIdx.x, lane = threadIdx.x;
  double* Ss = bsm;                   // [d][d]
  double* e1s = Ss + d * d;           // [d]
  double* e2s = e1s + d;              // [d]
  const double* S = f.S + (size_t)k * d * d;
  const double* p = f.raw + (size_t)k * f.raw_stride;
  const double* mu = a.mu + (size_t)k * d;
  for (int e = lane; e < d * d; e += 64) Ss[e] = S[e];
  wave_lds_sync();
  double e0 = 0.0;
  for (int i = lane; i < d; i += 64) {
    double q = 0.0;
    for (int c = 0; c < d; ++c) q = fma(Ss[i * d + c], Ss[i * d + c], q);
    const BoxSide s = box_coordinate(p, d, i, mu[i], sqrt(q));
    e0 += s.e0;
    e1s[i] = s.e1;
    e2s[i] = s.e2;
  }
  const double m0 = wave_sum(e0);
  wave_lds_sync();
  const int npo = a.full ? npairs(d) : 1;
  double* out = a.partial + (size_t)k * a.nchunk * npo;
  if (lane == 0) out[0] = m0;
  if (!a.full) return;
  for (int j = 1 + lane; j < npo; j += 64) {
    double v = 0.0;
    if (j <= d) {
      const int c = j - 1;
      for (int i = 0; i < d; ++i) v = fma(Ss[i * d + c], e1s[i], v);
    } else {
      int rem = j - 1 - d, row = 0;
      while (rem >= d - row) { rem -= d - row; ++row; }
      const int col = row + rem;
      for (int i = 0; i < d; ++i) v = fma(Ss[i * d + row] * Ss[i * d + col], e2s[i], v);
      if (row == col) v += m0;
    }
    out[j] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// moments_halfspace_closed_kernel: quadrature-free moments of the HINGE_HALFSPACE psi (halfspace_moments.hpp; DESIGN.md section
// 16).  psi is a sum over rows of a squared hinge of the scalar a_j^T x, so with v_j = S^T a_j and (e0, e1, e2)_j of halfspace_row
//   E[psi] = sum_j e0_j,   E[z psi] = sum_j v_j e1_j,   E[z z^T psi] = E[psi] I + sum_j v_j v_j^T e2_j
// for any root S S^T = Sigma, S row-major as prep writes it.  The same packed one-chunk layout as moments_closed_kernel, so the
// epilogue is shared.
// Lanes are (factor, row) pairs: with Jp = J rounded up to a power of two a wave holds G = 64 / Jp factors, lane = g Jp + j;
// wave w of the launch takes factors w G .. w G + G - 1.  A block is 1 or 4 such waves (blockDim.x / 64), each on its own slice
// of the dynamic LDS and without a workgroup barrier: no wave reads what another wrote.
//   phase 1: lane (g, j) forms v_j entry by entry into the wave's slice (Vs[c * 64 + lane]: consecutive lanes, consecutive
//            banks; no d-long register array) and takes its box_side; (e1, e2) go to LDS, e0 stays in a register.  A lane of an
//            off row, of a padding row j >= J or of a factor >= K writes nothing and carries zeros.
//   phase 2: the Jp lanes of a group stride over the npairs(d) outputs of their factor; each output is a sum over the ACTIVE rows
//            in ascending j (the ballot of phase 1 says which: an off row's slice was never written), m0 is the ascending-j sum
//            of the e0 registers through shuffles.  No atomics, no tree whose shape depends on the launch: the same bits from
//            run to run.
// LDS: 64 d + 128 doubles per wave.
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline int halfspace_group(int J) { int P = 1; while (P < J) P <<= 1; return P; }

__global__ __launch_bounds__(256) void moments_halfspace_closed_kernel(MomArgs a) {
  if (pred_skip(a.pred, a.pred_val)) return;
  extern __shared__ double hsm[];
  const FactorDev& f = a.f;
  const int d = f.d, J = f.seg_J, Jp = halfspace_group(J), G = 64 / Jp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / Jp, j = lane % Jp, gbase = g * Jp;
  const int64_t kw = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * G + g;
  const bool live = kw < f.K;
  const int k = live ? (int)kw : 0;
  double* Vs = hsm + (size_t)wave * halfspace_closed_lds_doubles(d);      // [d][64]
  double* e1s = Vs + 64 * d;                                             // [64]
  double* e2s = e1s + 64;                                                // [64]
  const double* p = f.raw + (size_t)k * f.raw_stride;
  const bool act = live && j < J && p[j] > 0.0;
  BoxSide r = {0.0, 0.0, 0.0};
  if (act) r = halfspace_row(p, d, J, j, a.mu + (size_t)k * d, f.S + (size_t)k * d * d, Vs + lane, 64);
  e1s[lane] = r.e1;
  e2s[lane] = r.e2;
  const unsigned long long on = __ballot(act);
  double m0 = 0.0;
  for (int jj = 0; jj < J; ++jj) m0 += __shfl(r.e0, gbase + jj);          // ascending j; an off row carries 0
  wave_lds_sync();
  if (!live) return;
  const int npo = a.full ? npairs(d) : 1;
  double* out = a.partial + (size_t)k * a.nchunk * npo;
  if (j == 0) out[0] = m0;
  if (!a.full) return;
  for (int o = 1 + j; o < npo; o += Jp) {
    double v = 0.0;
    if (o <= d) {
      const double* vc = Vs + (o - 1) * 64 + gbase;
      for (int jj = 0; jj < J; ++jj)
        if ((on >> (gbase + jj)) & 1ull) v = fma(vc[jj], e1s[gbase + jj], v);
    } else {
      int rem = o - 1 - d, row = 0;
      while (rem >= d - row) { rem -= d - row; ++row; }
      const double* vr = Vs + row * 64 + gbase;
      const double* vc = Vs + (row + rem) * 64 + gbase;
      for (int jj = 0; jj < J; ++jj)
        if ((on >> (gbase + jj)) & 1ull) v = fma(vr[jj] * vc[jj], e2s[gbase + jj], v);
      if (rem == 0) v += m0;
    }
    out[o] = v;
  }
}

}  // namespace gvi
