// Half-space and corridor limit factors (GVI_PSI_HINGE_HALFSPACE): psi, margin and the closed-form Gaussian
// moments of one row.  Plain C++ that also compiles for the host (tests/stubs/halfspace_on_cpu.cpp runs it under AddressSanitizer /
// UBSan); the kernels that call it are in kernels_closed.hpp.
//
// Parameter block of one factor, J rows on a slice of dimension d:  p = [sigma (J) | eps (J) | b (J) | A (J x d, row-major)]
//   psi(x)    = sum_j sigma_j max(0, a_j^T x - (b_j - eps_j))^2
//   margin(x) = min over rows with sigma_j > 0 of (b_j - a_j^T x) / |a_j|
// A row with sigma_j = 0 is off: it adds nothing, is skipped in the margin, and its a_j is not read.
//
// For x = mu + S z, z ~ N(0, I), S ANY root of Sigma stored row-major (S[i * d + c] is entry c of row i), the scalar
// s_j = a_j^T x = a_j^T mu + v_j^T z with v_j = S^T a_j is a 1-D Gaussian of standard deviation sd_j = |v_j|.  Row j is then the
// upper side of a box hinge on s_j, and box_side (box_moments.hpp) gives (e0, e1, e2)_j = (E[h], E[h'], E[h'']).  Stein's lemma
// along v_j:
//   E[psi] = sum_j e0_j      E[z psi] = sum_j v_j e1_j      E[z z^T psi] = E[psi] I + sum_j v_j v_j^T e2_j
#pragma once
#include <math.h>

#include "box_moments.hpp"

namespace gvi {

// psi at the slice x [d]
GVI_HD inline double psi_hinge_halfspace(const double* p, const double* x, int d, int J) {
  const double* A = p + 3 * J;
  double cost = 0.0;
  for (int j = 0; j < J; ++j) {
    const double sigma = p[j];
    if (!(sigma > 0.0)) continue;
    double s = 0.0;
    for (int i = 0; i < d; ++i) s = fma(A[j * d + i], x[i], s);
    const double e = s - (p[2 * J + j] - p[J + j]);
    if (e > 0.0) cost += sigma * e * e;
  }
  return cost;
}

// signed Euclidean distance to the nearest active face (negative: past it); eps plays no part; +inf when every row is off
GVI_HD inline double halfspace_margin(const double* p, const double* x, int d, int J) {
  const double* A = p + 3 * J;
  double mg = INFINITY;
  for (int j = 0; j < J; ++j) {
    if (!(p[j] > 0.0)) continue;
    double s = 0.0, q = 0.0;
    for (int i = 0; i < d; ++i) {
      s = fma(A[j * d + i], x[i], s);
      q = fma(A[j * d + i], A[j * d + i], q);
    }
    mg = fmin(mg, (p[2 * J + j] - s) / sqrt(q));
  }
  return mg;
}

// One row's work: v_out[c * vstride] = v_j[c] = sum_i a_j[i] S[i * d + c] (c = 0 .. d - 1; vstride lets a kernel interleave the
// rows of a wave), sd_j = |v_j|, gap = a_j^T mu - (b_j - eps_j); returns box_side of the upper side.  An off row (sigma_j = 0)
// returns zeros and writes nothing.
GVI_HD inline BoxSide halfspace_row(const double* p, int d, int J, int j, const double* mu, const double* S, double* v_out,
                                        int vstride = 1) {
  const double sigma = p[j];
  if (!(sigma > 0.0)) return BoxSide{0.0, 0.0, 0.0};
  const double* a = p + 3 * J + j * d;
  double q = 0.0, s = 0.0;
  for (int c = 0; c < d; ++c) {
    double v = 0.0;
    for (int i = 0; i < d; ++i) v = fma(a[i], S[i * d + c], v);
    v_out[c * vstride] = v;
    q = fma(v, v, q);
    s = fma(a[c], mu[c], s);
  }
  return box_side(sigma, sqrt(q), s - (p[2 * J + j] - p[J + j]), 1.0);
}

}  // namespace gvi
