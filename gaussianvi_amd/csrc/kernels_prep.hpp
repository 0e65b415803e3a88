// The per-pass products of a factor, one wave each: Sigma_k -> S_k, S_k^-1, Lam_k, H_k = A_k S_k, u0_k by Jacobi (prep_body), register
// Cholesky (prep_chol_body, prep_chol_hu0) or LDS Cholesky (prep_chol_lds_body); prep_body_d chooses, prep_kernel and prep_all_kernel
// (PrepList) launch it, the one-launch passes call it.  jko_*: the proximal map around the Jacobi.  LDS carve-ups: factor_lds.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "dpp_rowb.hpp"
#include "factor_dev.hpp"
#include "factor_lds.hpp"
#include "factor_math.hpp"

namespace gvi {

// ---------------------------------------------------------------------------------------------
// prep_kernel: one wave (block of 64) per factor.  Parallel-ordered (round-robin) cyclic Jacobi on
// the symmetric d x d block held in LDS; every round applies d/2 disjoint plane rotations at once:
//   A'_ij = al_i al_j A_ij + al_i be_j A_i,pj + be_i al_j A_pi,j + be_i be_j A_pi,pj ,
//   V'_ij = al_j V_ij + be_j V_i,pj           (p. = rotation partner, (al, be) = (c, -/+s)).
// ---------------------------------------------------------------------------------------------
// DT: d at compile time (the d-long inner products unroll and their loads -- LDS, and the GLOBAL rows of A_k in the H = A S
// product -- are issued together instead of one dependent round trip per term) or 0 for any d
template <int EPLP, int DT>   // EPLP: elements of the d x d block per lane: 1 (d <= 8), 4 (d <= 16), 16 (d <= 32)
// kin: index of the factor inside the (mu, Sigma) INPUT arrays (== k, or 0 when the caller staged this factor's
// marginal in LDS); outputs always go to slot k
__device__ __forceinline__ void prep_body(const FactorDev& f, const double* mu, const double* Sigma, int k, double* sm, int kin) {
  const int d = DT ? DT : f.d, dd = d * d, lane = threadIdx.x & 63;      // one wave per factor (the fused kernel runs several per block)
  const ProductsLds L{d};        // the Jacobi view of the products area, region by region (factor_lds.hpp)
  const int dp = L.dp();
  double* A0 = sm + L.A0();
  double* A1 = A0 + (L.A1() - L.A0());
  double* V0 = A1 + (L.V0() - L.A1());
  double* V1 = V0 + (L.V1() - L.V0());
  double* al = V1 + (L.al() - L.V1());          // [dp]
  double* be = al + (L.be() - L.al());          // [dp]
  double* lam = be + (L.lam() - L.be());        // [d] (3 functions of lambda: sqrt, 1/sqrt, 1/x)
  int* pa = (int*)(lam + (L.pa() - L.lam()));   // [dp]
  int ei[EPLP], ej[EPLP];        // (row, col) of this lane's elements, computed once (-1: none)
#pragma unroll
  for (int q = 0; q < EPLP; ++q) {
    const int e = lane + q * 64;
    ei[q] = e < dd ? e / d : -1;
    ej[q] = e < dd ? e % d : 0;
  }
  const double* Sg = Sigma + (size_t)kin * dd;
  // Warm start (device-resident NGD iteration): consecutive proposals differ little, so the previous
  // eigenvectors W almost diagonalise the new block; sweeping A0 = W^T Sigma W from V0 = W needs 2-4
  // sweeps instead of 7-8.  Any orthogonal start gives the same decomposition up to rounding; a NaN
  // in W (left by a rejected non-PSD trial) falls back to the cold start.
  bool warm = f.warm != 0 && f.Vws != nullptr;
  if (warm) {
    int bad = 0;
#pragma unroll
    for (int q = 0; q < EPLP; ++q) {
      if (ei[q] >= 0) {
        const int i = ei[q], j = ej[q], e = lane + q * 64;
        const double v = f.Vws[(size_t)k * dd + e];
        bad |= !(fabs(v) <= 2.0);
        V0[e] = v;
        A1[e] = i >= j ? Sg[i * d + j] : Sg[j * d + i];
      }
    }
    warm = __ballot(bad) == 0;
    wave_lds_sync();
    if (warm) {
#pragma unroll
      for (int q = 0; q < EPLP; ++q) {              // T = Sigma W  -> V1
        if (ei[q] >= 0) {
          const int i = ei[q], j = ej[q];
          double t = 0.0;
#pragma unroll
          for (int c = 0; c < d; ++c) t += A1[i * d + c] * V0[c * d + j];
          V1[lane + q * 64] = t;
        }
      }
      wave_lds_sync();
#pragma unroll
      for (int q = 0; q < EPLP; ++q) {              // A0 = W^T T, upper triangle mirrored (exactly symmetric)
        if (ei[q] >= 0) {
          const int i = ei[q] <= ej[q] ? ei[q] : ej[q], j = ei[q] <= ej[q] ? ej[q] : ei[q];
          double t = 0.0;
#pragma unroll
          for (int c = 0; c < d; ++c) t += V0[c * d + i] * V1[c * d + j];
          A0[lane + q * 64] = t;
        }
      }
    }
  }
  if (!warm) {
#pragma unroll
    for (int q = 0; q < EPLP; ++q) {
      if (ei[q] >= 0) {
        const int i = ei[q], j = ej[q], e = lane + q * 64;
        A0[e] = i >= j ? Sg[i * d + j] : Sg[j * d + i];   // lower triangle, like SelfAdjointEigenSolver
        V0[e] = i == j ? 1.0 : 0.0;
      }
    }
  }
  wave_lds_sync();
  double* A = A0; double* An = A1; double* V = V0; double* Vn = V1;
  for (int sweep = 0; sweep < 40; ++sweep) {
    double off = 0.0, dg = 0.0;
#pragma unroll
    for (int q = 0; q < EPLP; ++q) {
      if (ei[q] >= 0) {
        const double v = A[lane + q * 64];
        if (ei[q] == ej[q]) dg += v * v; else if (ei[q] < ej[q]) off += v * v;
      }
    }
    off = wave_sum(off);
    dg = wave_sum(dg);
    if (off <= f.jtol * dg) break;     // false for NaN input: runs the (bounded) 40 sweeps
    for (int r = 0; r < dp - 1; ++r) {
      if (lane < dp / 2) {
        int p, q;
        if (lane == 0) { p = dp - 1; q = r; }
        else {
          p = r + lane; if (p >= dp - 1) p -= dp - 1;
          q = r - lane; if (q < 0) q += dp - 1;
        }
        if (p > q) { const int t = p; p = q; q = t; }
        double c = 1.0, s = 0.0;
        const bool valid = q < d;
        if (valid) {
          const double apq = A[p * d + q];
          if (apq != 0.0) {
            // fp64 div / sqrt sequences cost ~1 400 cycles per rotation on the critical path; hardware
            // rcp / rsq + Newton steps give the same rotation.  Only (c, s) must be orthonormal to
            // working precision (c gets two Newton steps); errors in theta / t merely perturb the
            // convergence rate.
            const double theta = (A[q * d + q] - A[p * d + p]) * rcp_nr(2.0 * apq);
            if (fabs(theta) < 1e150) {               // else the rotation is the identity to fp64
              const double w1 = fma(theta, theta, 1.0);
              const double sq = w1 * rsq_nr(w1);
              const double t = copysign(rcp_nr(fabs(theta) + sq), theta);
              const double w2 = fma(t, t, 1.0);
              double rc = rsq_nr(w2);
              rc = rc * fma(fma(-0.5 * w2, rc, 0.0), rc, 1.5);   // second Newton step
              c = rc;
              s = t * c;
            }
          }
        }
        al[p] = c; be[p] = -s; pa[p] = valid ? q : p;
        al[q] = c; be[q] = s;  pa[q] = valid ? p : q;
      }
      wave_lds_sync();
#pragma unroll
      for (int q = 0; q < EPLP; ++q) {
        if (ei[q] >= 0) {
          const int i = ei[q], j = ej[q], e = lane + q * 64;
          const int pi = pa[i], pj = pa[j];
          const double ai = al[i], bi = be[i], aj = al[j], bj = be[j];
          An[e] = ai * (aj * A[i * d + j] + bj * A[i * d + pj]) + bi * (aj * A[pi * d + j] + bj * A[pi * d + pj]);
          Vn[e] = aj * V[i * d + j] + bj * V[i * d + pj];
        }
      }
      wave_lds_sync();
      double* t = A; A = An; An = t;
      t = V; V = Vn; Vn = t;
    }
  }
  if (lane < d) {
    const double l = A[lane * d + lane];
    lam[lane] = sqrt(l);               // negative eigenvalue -> NaN, as the reference's operatorSqrt
    lam[d + lane] = 1.0 / sqrt(l);
    lam[2 * d + lane] = f.jko_h > 0.0 ? 1.0 / (0.5 * l + f.jko_h + 0.5 * sqrt(l * (l + 4.0 * f.jko_h))) : 1.0 / l;
  }
  wave_lds_sync();
  // S, S^-1, Lam = V f(lambda) V^T; S is also kept in LDS (An) for H = A_k S
#pragma unroll
  for (int q = 0; q < EPLP; ++q) {
    if (ei[q] >= 0) {
      const int i = ei[q], j = ej[q], e = lane + q * 64;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int c = 0; c < d; ++c) {
        const double vv = V[i * d + c] * V[j * d + c];
        s0 += vv * lam[c]; s1 += vv * lam[d + c]; s2 += vv * lam[2 * d + c];
      }
      An[e] = s0;
      if (f.Vws) f.Vws[(size_t)k * dd + e] = V[e];
      f.S[(size_t)k * dd + e] = s0;
      f.Sinv[(size_t)k * dd + e] = s1;
      f.Lam[(size_t)k * dd + e] = s2;
    }
  }
  wave_lds_sync();
  if (f.m > 0) {
    const int m = f.m;
    const double* Ak = f.A + (size_t)k * m * d;
    for (int e = lane; e < m * d; e += 64) {
      const int r = e / d, a = e % d;
      double h = 0.0;
#pragma unroll
      for (int c = 0; c < d; ++c) h += Ak[r * d + c] * An[c * d + a];
      f.H[(size_t)k * m * d + a * m + r] = h;            // column-major [d][m]: a column's m entries contiguous
      if (f.Hq) {
        const int R = (m + 3) / 4;
        f.Hq[(((size_t)k * 4 + r / R) * d + a) * R + r % R] = h;
      }
    }
    if (lane < m) {
      double u = f.b[(size_t)k * m + lane];
#pragma unroll
      for (int c = 0; c < d; ++c) u += Ak[lane * d + c] * mu[(size_t)kin * d + c];
      f.u0[(size_t)k * m + lane] = u;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// prep_chol_body: the per-pass products from a CHOLESKY factor, one wave per factor, rows in registers.
//
// The reference maps the sigma points with the symmetric square root of Sigma (gvibase/GVIFactorizedBaseGH.h:
// updateGH -> SparseGaussHermite::update_sigmapoints, an Eigen self-adjoint eigen-decomposition) -- here a cyclic
// Jacobi solve of ~15 us per pass at d = 12.  For psi = sum_r s_r (A x + b)_r^2 the integrands psi, z psi, z z^T psi are
// polynomials of degree <= 4 in z, which a sparse Gauss-Hermite rule of degree >= 3 integrates EXACTLY: the moments
// E[psi], E[(x - mu) psi], E[(x - mu)(x - mu)^T psi] are then the same for every S with S S^T = Sigma (they are
// functions of (mu, Sigma) alone), and the back-transform only needs S^-T and Sigma^-1:
//     Vdmu = S^-T m1 / T,   Vddmu = (S^-T M2 S^-1 - Sigma^-1 m0) / T.
// So for these sets S = L (Sigma = L L^T): 66 multiply-adds per triangle at d = 12 instead of Jacobi sweeps, and the
// results agree with the symmetric-root route to rounding (tests/test_gpu_parity.py A/Bs the two; option "chol_sqrt").
// Every psi kind that is NOT a polynomial of degree <= 2 (hinge / range factors, host-evaluated psi, gvi_expand) keeps
// the symmetric root: there the node positions matter.  A non-positive pivot gives NaN exactly where a negative
// eigenvalue did (the line search rejects such a trial either way).
// lane i < d owns row i of the lower triangle.  ROWB: every 16-lane row of the wave is a replica (row = lane & 15,
// only lanes < d store) and pivots / multipliers are broadcast inside a row by DPP (dpp_rowb.hpp): a trailing update is ONE
// v_fmac_f64_dpp instead of two v_readlane, an FMA and a 64-bit select -- 66 of them in the factorisation and 66 in L^-1 at
// d = 12.  The same products with the same signs: bit-identical to the v_readlane form, NaN positions included (the entries
// above the diagonal hold scratch values until their column's step zeroes them; nothing reads them before).
// !ROWB: pivots / multipliers travel as wave-uniform scalars (v_readlane) -- what the launches of one wave per factor
// (prep_kernel, prep_all_kernel) keep; option "chol_rowb" 1 puts prep_all_kernel on the row-broadcast instance, the bitwise
// A/B inside one library.  The one-launch passes (factor_fused_kernel, factor_block3_kernel) take ROWB.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double chol_readlane(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// -DGVI_FUSED_TIMING: 100 MHz stamps of wave 0 of block 0 inside the Cholesky prep (slots 8.. of the fused kernel's stamp
// buffer; the kernel parks the pointer here)
#ifdef GVI_FUSED_TIMING
__device__ unsigned long long* gvi_prep_stamps;
#define PREP_STAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); if (blockIdx.x == 0 && (threadIdx.x & 63) == 0 && gvi_prep_stamps) gvi_prep_stamps[(i) + 16 * (threadIdx.x >> 6)] = t_; } while (0)
#else
#define PREP_STAMP(i) do { } while (0)
#endif

// ---- the row-broadcast steps (compile-time recursion: the broadcast lane of a DPP control is an immediate) ----
template <int DT, int J, int C>
__device__ __forceinline__ void chol_rowb_trail(double (&row)[DT]) {
  if constexpr (C < DT) {
    rowb_fma<C>(row[C], row[J], row[J]);                       // row[c] -= L[c][j] * own L[.][j]
    chol_rowb_trail<DT, J, C + 1>(row);
  }
}
template <int DT, int I, int J>
__device__ __forceinline__ void chol_rowb_xcol(double (&xcol)[DT], const double (&row)[DT]) {
  if constexpr (J < DT) {
    rowb_fma<J>(xcol[J], row[I], xcol[I]);                     // x_j -= L[j][i] * x_i
    chol_rowb_xcol<DT, I, J + 1>(xcol, row);
  }
}
// Wait states (dpp_rowb.hpp): the DPP-read operand of step j's updates is row[j], written by the scaling just in front --
// rowb_settle; the pivot's rowb_mov carries its own s_nop behind the updates of step j - 1; L^-1 reads the finished rows,
// settled in front of it.  Every lane executes every step.
template <int DT, int J>
__device__ __forceinline__ void chol_rowb_steps(double (&row)[DT], double (&inv)[DT], const int li) {
  if constexpr (J < DT) {
    const double pj = rowb_mov<J, 1>(row[J]);
    double r = __builtin_amdgcn_rsq(pj);                      // 1 / sqrt(pj): NaN for a negative pivot
    r = r * fma(-0.5 * pj * r, r, 1.5);
    r = r * fma(-0.5 * pj * r, r, 1.5);
    inv[J] = r;
    row[J] = li == J ? pj * r : (li > J ? row[J] * r : 0.0);
    rowb_settle(row[J]);
    chol_rowb_trail<DT, J, J + 1>(row);
    chol_rowb_steps<DT, J + 1>(row, inv, li);
  }
}
template <int DT, int I>
__device__ __forceinline__ void chol_rowb_inverse(double (&xcol)[DT], const double (&row)[DT], const double (&inv)[DT], const int li) {
  if constexpr (I < DT) {
    xcol[I] = li <= I ? xcol[I] * inv[I] : 0.0;
    chol_rowb_xcol<DT, I, I + 1>(xcol, row);
    chol_rowb_inverse<DT, I + 1>(xcol, row, inv, li);
  }
}

// the form of the one-launch passes (-DGVI_CHOL_READLANE: measurement build, the fused route's A/B leg)
#ifdef GVI_CHOL_READLANE
constexpr bool CHOL_ROWB_DEFAULT = false;
#else
constexpr bool CHOL_ROWB_DEFAULT = true;
#endif

// Zs (LDS, optional): a copy of S^-T for an epilogue in the same launch (factor_fused_kernel)
// Hs / u0s (LDS, optional; factor_fused_kernel's lean form): the psi operands H (column c at Hs + c hstride) and u0 stay in LDS
// for the walk of the same launch and NOTHING of the per-pass products goes to memory (no S / S^-T / Sigma^-1 / H / u0
// stores, Sigma^-1 is not formed: the caller's epilogue re-forms what it needs from Zs)
// l_ready (LDS, optional; lean form only): ANOTHER wave of the block forms H = A L and u0 = b + A mu for this item
// (prep_chol_hu0) -- this wave then skips the rows of A altogether and raises *l_ready once L is in its LDS area
template <int DT, bool ROWB = CHOL_ROWB_DEFAULT>
__device__ inline void prep_chol_body(const FactorDev& f, const double* mu, const double* Sigma, int k, double* sm, int kin, double* Zs = nullptr,
                                      double* Hs = nullptr, double* u0s = nullptr, const int hstride = 0, int* l_ready = nullptr) {
  const bool lean = Hs != nullptr;
  constexpr int d = DT, dd = DT * DT;
  const int lane = threadIdx.x & 63;      // one wave per factor (the fused kernel runs several per block)
  constexpr ProductsLds L{DT};           // the Cholesky view of the products area (factor_lds.hpp)
  double* Ll = sm + L.Ll();   // [d][d] L, zeros above the diagonal
  double* Xl = sm + L.Xl();   // [d][d] X = L^-1
  const double* Sg = Sigma + (size_t)kin * dd;
  static_assert(!ROWB || DT <= 16, "row-broadcast form: a row of L per lane of a 16-lane row");
  const int lr = ROWB ? (lane & 15) : lane;                  // ROWB: the four 16-lane rows of the wave are replicas
  const int li = lr < d ? lr : d - 1;                         // lanes >= d shadow the last row (results unused)
  // The rows of A (and b) the psi operands H = A L, u0 = b + A mu need do not depend on the factorisation: request them
  // NOW, so that their global-memory latency runs under the Cholesky instead of behind it (the prep is a chain of dependent
  // latencies: ~10 us per factor before this, profiles/r03 fused-pass stamps).  Element e = lane (+ 64) of H reads row e / d.
  constexpr int HPL = 2;                                       // H elements per lane: m d <= 128 for the Cholesky shapes (m <= d / 2 ... d)
  const int mm = f.m;
  const bool pre = mm > 0 && mm * d <= 64 * HPL && !l_ready;
  double arow[HPL][DT], brow = 0.0;
  if (pre) {
    const double* Ak = f.A + (size_t)k * mm * d;
#pragma unroll
    for (int q = 0; q < HPL; ++q) {
      const int e = lane + 64 * q;
      const int r = e < mm * d ? e / d : 0;
#pragma unroll
      for (int c = 0; c < d; ++c) arow[q][c] = Ak[r * d + c];
    }
    if (lane < mm) brow = f.b[(size_t)k * mm + lane];
  }
  PREP_STAMP(0);
  double row[DT];
#pragma unroll
  for (int c = 0; c < d; ++c) row[c] = c <= li ? Sg[li * d + c] : 0.0;      // lower triangle, like SelfAdjointEigenSolver
  PREP_STAMP(1);
  double inv[DT];
  if constexpr (ROWB) {
#pragma unroll
    for (int c = 0; c < d; ++c) rowb_pin(row[c]);
    chol_rowb_steps<DT, 0>(row, inv, li);
  } else {
#pragma unroll
    for (int j = 0; j < d; ++j) {
      const double pj = chol_readlane(row[j], j);
      double r = __builtin_amdgcn_rsq(pj);                    // 1 / sqrt(pj): NaN for a negative pivot
      r = r * fma(-0.5 * pj * r, r, 1.5);
      r = r * fma(-0.5 * pj * r, r, 1.5);
      inv[j] = r;
      row[j] = li == j ? pj * r : (li > j ? row[j] * r : 0.0);
#pragma unroll
      for (int c = j + 1; c < d; ++c) {
        const double lcj = chol_readlane(row[j], c);
        row[c] = li >= c ? fma(-row[j], lcj, row[c]) : 0.0;
      }
    }
  }
  PREP_STAMP(2);
  // X = L^-1 by forward substitution: lane c owns column c.  Column-oriented: x_i updates the right-hand sides of every
  // later row at once, so the dependent chain is d (multiply + one FMA) instead of the d (d - 1) / 2 FMAs of the row-wise
  // dot products -- the same FMAs in the same order per entry (bit-identical), 66 -> 24 instructions deep at d = 12
  // (in place: entry i holds the right-hand side until x_i is formed -- no second array: the 24 registers of one pushed the
  // fused pass from 20 to 56 bytes of scratch per lane, 14 MB of spill traffic per launch)
  double xcol[DT];
#pragma unroll
  for (int i = 0; i < d; ++i) xcol[i] = li == i ? 1.0 : 0.0;
  if constexpr (ROWB) {
#pragma unroll
    for (int c = 0; c < d; ++c) rowb_settle(row[c]);
    chol_rowb_inverse<DT, 0>(xcol, row, inv, li);
  } else {
#pragma unroll
    for (int i = 0; i < d; ++i) {
      xcol[i] = li <= i ? xcol[i] * inv[i] : 0.0;
#pragma unroll
      for (int j = i + 1; j < d; ++j) xcol[j] = fma(-chol_readlane(row[i], j), xcol[i], xcol[j]);
    }
  }
  PREP_STAMP(3);
  if (lane < d) {
#pragma unroll
    for (int c = 0; c < d; ++c) { Ll[lane * d + c] = row[c]; Xl[c * d + lane] = xcol[c]; }
  }
  // the prefetched rows of A also go to LDS (one copy per row: lanes e = r d hold row r), for u0 = b + A mu below
  double* Al = sm + L.Al();    // [m][d]
  if (pre) {
#pragma unroll
    for (int q = 0; q < HPL; ++q) {
      const int e = lane + 64 * q;
      if (e < mm * d && e % d == 0) {
#pragma unroll
        for (int c = 0; c < d; ++c) Al[e + c] = arow[q][c];
      }
    }
  }
  wave_lds_sync();
  if (l_ready && lane == 0) __hip_atomic_store(l_ready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (LDS operations of a wave execute in order: L is there)
  if (lean) {
    for (int e = lane; e < dd; e += 64) Zs[e] = Xl[(e % d) * d + e / d];            // S^-T = X^T
  } else {
    for (int e = lane; e < dd; e += 64) {
      const int i = e / d, j = e % d;
      double lam = 0.0;
#pragma unroll
      for (int c = 0; c < d; ++c) lam = fma(Xl[c * d + i], Xl[c * d + j], lam);      // Sigma^-1 = X^T X
      f.S[(size_t)k * dd + e] = Ll[e];
      f.Sinv[(size_t)k * dd + e] = Xl[j * d + i];                                      // S^-T = X^T
      f.Lam[(size_t)k * dd + e] = lam;
      if (Zs) Zs[e] = Xl[j * d + i];
    }
  }
  PREP_STAMP(4);
  if (f.m > 0 && !l_ready) {
    const int m = f.m;
    const double* Ak = f.A + (size_t)k * m * d;
    if (pre) {                                           // operands already in registers (same products, same order)
#pragma unroll
      for (int q = 0; q < HPL; ++q) {
        const int e = lane + 64 * q;
        if (e < m * d) {
          const int r = e / d, a = e % d;
          double h = 0.0;
#pragma unroll
          for (int c = 0; c < d; ++c) h += arow[q][c] * Ll[c * d + a];
          if (lean) Hs[a * hstride + r] = h;             // the walk's LDS layout: column a at stride hstride
          else {
            f.H[(size_t)k * m * d + a * m + r] = h;      // column-major [d][m]: a column's m entries contiguous
            if (f.Hq) {
              const int R = (m + 3) / 4;
              f.Hq[(((size_t)k * 4 + r / R) * d + a) * R + r % R] = h;
            }
          }
        }
      }
    } else {
      for (int e = lane; e < m * d; e += 64) {
        const int r = e / d, a = e % d;
        double h = 0.0;
#pragma unroll
        for (int c = 0; c < d; ++c) h += Ak[r * d + c] * Ll[c * d + a];
        f.H[(size_t)k * m * d + a * m + r] = h;
        if (f.Hq) {
          const int R = (m + 3) / 4;
          f.Hq[(((size_t)k * 4 + r / R) * d + a) * R + r % R] = h;
        }
      }
    }
    if (lane < m) {
      double u = pre ? brow : f.b[(size_t)k * m + lane];
#pragma unroll
      for (int c = 0; c < d; ++c) u += (pre ? Al[lane * d + c] : Ak[lane * d + c]) * mu[(size_t)kin * d + c];
      if (lean) u0s[lane] = u;
      else f.u0[(size_t)k * m + lane] = u;
    }
  }
  PREP_STAMP(5);
}

// The psi operands H = A L and u0 = b + A mu of an item whose Cholesky factor ANOTHER wave of the block is forming
// (factor_fused_kernel: two of a block's four waves are idle in the products phase).  u0 does not depend on the factorisation
// and is formed at once; the rows of A are requested at once too; H waits for *l_ready (raised by prep_chol_body once L is in
// that wave's LDS area Ll).  Same products in the same order as prep_chol_body's own H / u0: bit-identical.
// mul: the item's mean (LDS or global, [d] at index 0); own: this wave's LDS area (>= m d + d doubles); 0 < m d <= 128 (caller).
template <int DT>
__device__ inline void prep_chol_hu0(const FactorDev& f, const double* mul, const int k, double* own, const double* Ll, int* l_ready,
                                     double* Hs, double* u0s, const int hstride) {
  constexpr int d = DT, HPL = 2;
  const int lane = threadIdx.x & 63, m = f.m;
  const double* Ak = f.A + (size_t)k * m * d;
  double arow[HPL][DT], brow = 0.0;
#pragma unroll
  for (int q = 0; q < HPL; ++q) {
    const int e = lane + 64 * q;
    const int r = e < m * d ? e / d : 0;
#pragma unroll
    for (int c = 0; c < d; ++c) arow[q][c] = Ak[r * d + c];
  }
  if (lane < m) brow = f.b[(size_t)k * m + lane];
  double* Al = own;            // [m][d]
#pragma unroll
  for (int q = 0; q < HPL; ++q) {
    const int e = lane + 64 * q;
    if (e < m * d && e % d == 0) {
#pragma unroll
      for (int c = 0; c < d; ++c) Al[e + c] = arow[q][c];
    }
  }
  wave_lds_sync();
  if (lane < m) {
    double u = brow;
#pragma unroll
    for (int c = 0; c < d; ++c) u += Al[lane * d + c] * mul[c];
    u0s[lane] = u;
  }
  while (__hip_atomic_load(l_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) __builtin_amdgcn_s_sleep(1);
  asm volatile("" ::: "memory");
#pragma unroll
  for (int q = 0; q < HPL; ++q) {
    const int e = lane + 64 * q;
    if (e < m * d) {
      const int r = e / d, a = e % d;
      double h = 0.0;
#pragma unroll
      for (int c = 0; c < d; ++c) h += arow[q][c] * Ll[c * d + a];
      Hs[a * hstride + r] = h;
    }
  }
}

// The Cholesky route for every other dimension (d <= 32): L, X = L^-1 in LDS, any d at run time.  The register form above
// exists for the chain shapes; a d = 28 prior set (the arm graph, gp/minimum_acc_prior.h with 14-dimensional states) fell to
// the symmetric-root Jacobi solve -- 0.6 ms per prep launch, 74 % of that graph's iteration.  One wave per factor:
// right-looking factorisation with the trailing update spread over the lanes (EPLP elements each), forward substitution with
// lane = column, then the same outputs as prep_chol_body's non-lean form (S = L, S^-T, Sigma^-1 = X^T X, H = A L, u0).
template <int EPLP>
__device__ inline void prep_chol_lds_body(const FactorDev& f, const double* mu, const double* Sigma, int k, double* sm, int kin, double* Zs) {
  const int d = f.d, dd = d * d, lane = threadIdx.x & 63;
  const ProductsLds L{d};      // the Cholesky view of the products area (factor_lds.hpp); Al stays unused
  double* Ll = sm + L.Ll();    // [d][d] row-major, zeros above the diagonal
  double* Xl = Ll + (L.Xl() - L.Ll());        // [d][d] X = L^-1 (row-major, lower triangular)
  const double* Sg = Sigma + (size_t)kin * dd;
  for (int e = lane; e < dd; e += 64) {
    const int i = e / d, j = e % d;
    Ll[e] = j <= i ? Sg[i * d + j] : 0.0;        // lower triangle, like SelfAdjointEigenSolver
    Xl[e] = 0.0;
  }
  wave_lds_sync();
  for (int j = 0; j < d; ++j) {
    const double pj = Ll[j * d + j];
    double r = __builtin_amdgcn_rsq(pj);          // NaN for a negative pivot, as the register form
    r = r * fma(-0.5 * pj * r, r, 1.5);
    r = r * fma(-0.5 * pj * r, r, 1.5);
    wave_lds_sync();                              // (every lane has read the pivot before column j is rescaled)
    if (lane >= j && lane < d) Ll[lane * d + j] = lane == j ? pj * r : Ll[lane * d + j] * r;
    if (lane == j) Xl[j * d + j] = r;             // 1 / L_jj parked on X's diagonal
    wave_lds_sync();
    for (int e = lane; e < dd; e += 64) {         // trailing update of the lower triangle: L_ic -= L_ij L_cj, j < c <= i
      const int i = e / d, c = e % d;
      if (c > j && c <= i) Ll[e] = fma(-Ll[i * d + j], Ll[c * d + j], Ll[e]);
    }
    wave_lds_sync();
  }
  // X = L^-1 by forward substitution, lane c = column c: x_i = (delta_ic - sum_{c <= q < i} L_iq x_q) / L_ii
  if (lane < d) {
    const int c = lane;
    for (int i = c; i < d; ++i) {
      double acc = i == c ? 1.0 : 0.0;
      for (int q = c; q < i; ++q) acc = fma(-Ll[i * d + q], Xl[q * d + c], acc);
      const double inv = i == c ? Xl[c * d + c] : Xl[i * d + i];       // (the diagonal still holds 1 / L_ii until row i is written)
      Xl[i * d + c] = acc * inv;
    }
  }
  wave_lds_sync();
  for (int e = lane; e < dd; e += 64) {
    const int i = e / d, j = e % d;
    double lam = 0.0;
    const int lo = i > j ? i : j;
    for (int c = lo; c < d; ++c) lam = fma(Xl[c * d + i], Xl[c * d + j], lam);      // Sigma^-1 = X^T X (X lower triangular)
    f.S[(size_t)k * dd + e] = Ll[e];
    f.Sinv[(size_t)k * dd + e] = Xl[j * d + i];                                      // S^-T = X^T
    f.Lam[(size_t)k * dd + e] = lam;
    if (Zs) Zs[e] = Xl[j * d + i];
  }
  if (f.m > 0) {
    const int m = f.m;
    const double* Ak = f.A + (size_t)k * m * d;
    for (int e = lane; e < m * d; e += 64) {
      const int r = e / d, a = e % d;
      double h = 0.0;
      for (int c = a; c < d; ++c) h = fma(Ak[r * d + c], Ll[c * d + a], h);           // (L lower triangular: rows c >= a)
      f.H[(size_t)k * m * d + a * m + r] = h;
      if (f.Hq) {
        const int R = (m + 3) / 4;
        f.Hq[(((size_t)k * 4 + r / R) * d + a) * R + r % R] = h;
      }
    }
    if (lane < m) {
      double u = f.b[(size_t)k * m + lane];
      for (int c = 0; c < d; ++c) u = fma(Ak[lane * d + c], mu[(size_t)kin * d + c], u);
      f.u0[(size_t)k * m + lane] = u;
    }
  }
}

// the chain shapes of BASELINE.json get unrolled instances
// true when prep_body_d takes the Cholesky route for this set (and can leave [S^-T | Sigma^-1] in LDS)
__device__ __forceinline__ bool prep_is_chol(const FactorDev& f) {
  return f.chol && (f.d == 2 || f.d == 4 || f.d == 6 || f.d == 8 || f.d == 12);
}

// ROWB: the form of the register Cholesky (prep_chol_body).  The launches of one wave per factor keep v_readlane unless asked:
// measured on the d = 24 + 12 chain's prep launch the row-broadcast form is 1.3 us SLOWER there (profiles/r06_unit_top.txt §4)
template <int EPLP, bool ROWB = false>
__device__ inline void prep_body_d(const FactorDev& f, const double* mu, const double* Sigma, int k, double* sm, int kin, double* Zs = nullptr) {
  if (f.chol) {
    switch (f.d) {
      case 2: prep_chol_body<2, ROWB>(f, mu, Sigma, k, sm, kin, Zs); return;
      case 4: prep_chol_body<4, ROWB>(f, mu, Sigma, k, sm, kin, Zs); return;
      case 6: prep_chol_body<6, ROWB>(f, mu, Sigma, k, sm, kin, Zs); return;
      case 8: prep_chol_body<8, ROWB>(f, mu, Sigma, k, sm, kin, Zs); return;
      case 12: prep_chol_body<12, ROWB>(f, mu, Sigma, k, sm, kin, Zs); return;
      default: prep_chol_lds_body<EPLP>(f, mu, Sigma, k, sm, kin, Zs); return;
    }
  }
  if (EPLP == 1 && f.d == 2) prep_body<EPLP, 2>(f, mu, Sigma, k, sm, kin);
  else if (EPLP == 1 && f.d == 4) prep_body<EPLP, 4>(f, mu, Sigma, k, sm, kin);
  else if (EPLP == 1 && f.d == 6) prep_body<EPLP, 6>(f, mu, Sigma, k, sm, kin);
  else if (EPLP == 4 && f.d == 6) prep_body<EPLP, 6>(f, mu, Sigma, k, sm, kin);
  else if (EPLP == 4 && f.d == 12) prep_body<EPLP, 12>(f, mu, Sigma, k, sm, kin);
  else prep_body<EPLP, 0>(f, mu, Sigma, k, sm, kin);
}

template <int EPLP>
__global__ __launch_bounds__(64) void prep_kernel(FactorDev f, const double* __restrict__ mu,
                                                  const double* __restrict__ Sigma) {
  extern __shared__ double sm[];
  prep_body_d<EPLP>(f, mu, Sigma, blockIdx.x, sm, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// Proximal (JKO) update, factor level: ProxGVIFactorizedBaseGH::compute_BW_grads + BW_JKO
// (proxgd/ProxGVIFactorizedBaseGH.h:64-113, 152-160).  The quadrature moments are the NGD ones
// (b = Vdmu, S = Vddmu at unit temperature), so the map is three small launches around the prep kernel:
//   jko_half:   Sig_half = (I - h S) Sigma (I - h S)^T,  Vdmu <- -b
//   prep (jko_h = h) on Sig_half:  Lam_new = W diag(1 / (l/2 + h + sqrt(l (l + 4h))/2)) W^T
//   jko_finish: Vddmu <- (Lam_new - Lam) / h
// ---------------------------------------------------------------------------------------------
struct JkoArgs {
  int K, d;
  double h;
  double* Vdmu;          // [K][d]     in: b, out: -b
  double* Vddmu;         // [K][d][d]  in: S, out: (Lam_new - Lam) / h
  const double* Sigma;   // [K][d][d]
  const double* Lam;     // [K][d][d]
  double* Shalf;         // [K][d][d]
  const double* LamNew;  // [K][d][d]
};

__global__ __launch_bounds__(64) void jko_half_kernel(JkoArgs a) {
  extern __shared__ double sm[];
  const int d = a.d, dd = d * d, k = blockIdx.x, lane = threadIdx.x;
  const JkoLds L{d};         // region by region (factor_lds.hpp)
  double* M = sm + L.M();                  // I - h S
  double* Sg = M + (L.Sg() - L.M());
  double* Tm = Sg + (L.Tm() - L.Sg());     // M Sigma
  for (int e = lane; e < dd; e += 64) {
    const int i = e / d, j = e % d;
    M[e] = (i == j ? 1.0 : 0.0) - a.h * a.Vddmu[(size_t)k * dd + e];
    Sg[e] = a.Sigma[(size_t)k * dd + e];
  }
  for (int e = lane; e < d; e += 64) a.Vdmu[(size_t)k * d + e] = -a.Vdmu[(size_t)k * d + e];
  wave_lds_sync();
  for (int e = lane; e < dd; e += 64) {
    const int i = e / d, j = e % d;
    double s = 0.0;
    for (int c = 0; c < d; ++c) s += M[i * d + c] * Sg[c * d + j];
    Tm[e] = s;
  }
  wave_lds_sync();
  for (int e = lane; e < dd; e += 64) {
    const int i = e / d, j = e % d;
    if (i <= j) {                                           // upper triangle, mirrored: exactly symmetric
      double s = 0.0;
      for (int c = 0; c < d; ++c) s += Tm[i * d + c] * M[j * d + c];
      a.Shalf[(size_t)k * dd + i * d + j] = s;
      a.Shalf[(size_t)k * dd + j * d + i] = s;
    }
  }
}

__global__ __launch_bounds__(256) void jko_finish_kernel(JkoArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (int64_t)a.K * a.d * a.d) a.Vddmu[i] = (a.LamNew[i] - a.Lam[i]) / a.h;
}

// every factor set of the problem in ONE launch: block -> (set, factor) through the offsets
struct PrepList {
  int nsets;
  int koff[MAX_SETS + 1];
  FactorDev f[MAX_SETS];
  const double* mu[MAX_SETS];
  const double* Sigma[MAX_SETS];
  // optional fused gather (update_mu_from_joint / update_precision_from_joint, gvibase/GVIFactorizedBase.h:104-114):
  // every block first pulls its factor's (mu_k, Sigma_k) out of the chain arrays -- forming the trial mean
  // gmu + gstep * gdmu on the fly when gdmu != null -- parks them in LDS for the decomposition and writes them to
  // mu_k / Sigma_k for the later kernels; blocks past koff[nsets] write the chain-level trial mean mu_out.
  int gather, n;
  const double* gmu;
  const double* gdmu;
  double gstep;
  const double* SigD;
  const double* SigU;
  double* mu_out;
  int64_t nmu;
  const int32_t* start[MAX_SETS];
  double* mu_k[MAX_SETS];
  double* Sigma_k[MAX_SETS];
  const double* pred;    // predicated launch (device_common.hpp, pred_skip) or null
  double pred_val;
};

// ROWB: the form of the register Cholesky (option "chol_rowb"; default 0, v_readlane), an instance of its own each
template <int EPLP, bool ROWB = false>
__global__ __launch_bounds__(64) void prep_all_kernel(PrepList L) {
  extern __shared__ double sm[];
  const int lane = threadIdx.x;
  if (pred_skip(L.pred, L.pred_val)) return;
  if ((int)blockIdx.x >= L.koff[L.nsets]) {                      // chain-level trial mean (gather mode only)
    const int64_t j = (int64_t)((int)blockIdx.x - L.koff[L.nsets]) * 64 + lane;
    if (j < L.nmu) L.mu_out[j] = L.gmu[j] + L.gstep * L.gdmu[j];
    return;
  }
  int si = 0;
  while (si + 1 < L.nsets && (int)blockIdx.x >= L.koff[si + 1]) ++si;
  const int k = (int)blockIdx.x - L.koff[si];
  if (!L.gather) { prep_body_d<EPLP, ROWB>(L.f[si], L.mu[si], L.Sigma[si], k, sm, k); return; }
  const FactorDev& f = L.f[si];
  const int d = f.d, dd = d * d, n = L.n, nn = n * n;
  const ProductsLds P{d};                  // the gather staging behind the products area (factor_lds.hpp)
  double* Sl = sm + P.Sl();
  double* ml = Sl + (P.ml() - P.Sl());
  const int s = L.start[si][k];
  for (int e = lane; e < dd; e += 64) {
    const int r = e / d, c = e % d;
    double v;
    if (r < n && c < n) v = L.SigD[(size_t)s * nn + r * n + c];
    else if (r >= n && c >= n) v = L.SigD[(size_t)(s + 1) * nn + (r - n) * n + (c - n)];
    else if (r < n) v = L.SigU[(size_t)s * nn + r * n + (c - n)];
    else v = L.SigU[(size_t)s * nn + c * n + (r - n)];
    Sl[e] = v;
    L.Sigma_k[si][(size_t)k * dd + e] = v;
  }
  for (int e = lane; e < d; e += 64) {
    const size_t j = (size_t)s * n + e;
    const double v = L.gdmu ? L.gmu[j] + L.gstep * L.gdmu[j] : L.gmu[j];
    ml[e] = v;
    L.mu_k[si][(size_t)k * d + e] = v;
  }
  wave_lds_sync();
  prep_body_d<EPLP, ROWB>(f, ml, Sl, k, sm, 0);
}

}  // namespace gvi
