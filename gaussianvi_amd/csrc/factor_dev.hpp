// FactorDev: what every factor kernel knows of a set, passed BY VALUE in its kernel argument, and the packed layout of the z-space
// moments.  Plain C++ that also compiles for the host (tests/stubs/psi_point_on_cpu.cpp fills one with host pointers).
#pragma once
#include <stdint.h>

#include "hd.hpp"

namespace gvi {

GVI_HD constexpr int npairs(int d) { return (d + 1) * (d + 2) / 2; }

// packed z-space moment layout: [0] m0 | [1..d] m1 | then upper triangle of M2 row by row
GVI_HD inline int pair_index(int d, int a, int b) {  // a <= b < d
  return 1 + d + a * d - a * (a - 1) / 2 + (b - a);
}

struct FactorDev {
  int K, d, m, kind;
  int64_t N, Np;            // points, padded to a multiple of 64 (pad: z = 0, w = 0)
  const double* Zt;         // [d][Np] dimension-major: lane-over-points loads are coalesced
  const double* w;          // [Np]
  const double* Zq;         // [Np / 64][d + 1][64] tile-major copy (row d = w): one contiguous block per 64-point step
  // Mirror-half table: a sparse Gauss-Hermite grid is symmetric -- with every point z it holds -z with the same weight --
  // so only one representative per +-pair is stored (first non-zero coordinate positive; the origin with HALF its weight)
  // and the kernels evaluate psi at z and -z from one load:  Zm [Nmp / 64][d + 1][64], Nm representatives, null if the
  // table is not symmetric.
  const double* Zm;
  int64_t Nm, Nmp;
  int all_pos;              // 1: every sgn entry is +1 (sum-of-squares kinds with a positive-definite weight)
  const uint32_t* codes;    // [d/4][Np] four 8-bit node codes per word (tables with <= 256 distinct values) or null
  const double* lut;        // [256] code -> node value
  const double* A;          // [K][m][d]   sum-of-squares kinds
  const double* b;          // [K][m]
  const double* sgn;        // [K][m]
  const double* raw;        // [K][raw_stride] raw parameter block (RANGE_1D, HINGE_SDF_*, HINGE_BOX, HINGE_HALFSPACE)
  int raw_stride;
  const double* temperature;  // [K]
  // per-pass products of prep_kernel
  double* S;                // [K][d][d]
  double* Sinv;             // [K][d][d]
  double* Lam;              // [K][d][d]
  double* H;                // [K][d][m]  H = A S, stored column by column
  double* Hq;               // [K][4][d][R], R = ceil(m/4): rows v R .. v R + R of H per wave v (split kernel) or null
  double* u0;               // [K][m]
  const double* sdf;        // HINGE_SDF_2D: column-major rows x cols signed-distance grid
  int sdf_rows, sdf_cols, sdf_nz;
  double sdf_ox, sdf_oy, sdf_oz, sdf_cell;
  double sdf_inv_cell;                // 1 / sdf_cell: the look-ups multiply (an fp64 division is ~12 VALU instructions; two per 2-D look-up were 25 of the hinge kernel's 79)
  const double* arm;        // HINGE_SDF_3D_ARM: [ndof, ns, a[ndof], alpha[ndof], d[ndof], bias[ndof], frame[ns], centre[ns][3], radius[ns]]
  double jko_h;             // > 0: the third spectral output is the JKO map 1 / (l/2 + h + sqrt(l (l + 4h))/2) instead of 1/l
  double jtol;              // Jacobi stops when off^2 <= jtol * diag^2 (sums of squares)
  // 1: S is the Cholesky factor L of Sigma instead of its symmetric square root (prep_chol_body), the Sinv slot holds
  // L^-T.  Only for sum-of-squares psi on a degree >= 3 table, where the quadrature of psi {1, z, z z^T} is exact and
  // the moments do not depend on WHICH factor S S^T = Sigma maps the nodes (host: FactorSet::dev).
  int chol;
  double* Vws;              // [K][d][d] eigenvectors of the previous prep (warm start) or null
  int warm;                 // 1: start the Jacobi sweeps from Vws (resident NGD iteration only)
  int seg_J;                // HINGE_SDF_*_SEG: check points per factor (1 .. SEG_MAX_J); HINGE_HALFSPACE: rows per factor (1 .. HALFSPACE_MAX_J); else 0
};

}  // namespace gvi
