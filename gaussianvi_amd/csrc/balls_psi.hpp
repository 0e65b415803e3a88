// psi and clearance of GVI_PSI_HINGE_BALLS_2D / _3D (include/gvi_hip.h): a hinge on the exact signed
// distance to a union of balls that move with constant velocities.  Plain C++17 that also compiles for the host
// (tests/stubs/balls_check.cpp runs it under AddressSanitizer / UBSan); psi_point and hinge_psi_clearance of
// psi_point.hpp call it, and PsiHingeBalls of kernels_reg.hpp is the register form of the same walk.
//
// One factor's block p, P = 2 / 3, x its slice [d], J check points, BALLS_SLOTS = GVI_BALLS_MAX_M ball slots:
//   p = [sigma, eps, r | J x ( W_j (P x d, row-major) | c_j (P) | tau_j ) | BALLS_SLOTS x ( o_m (P) | v_m (P) | R_m )]
//   q_j = W_j x + c_j,   sd_j = min over the slots with R_m != -inf of |q_j - (o_m + tau_j v_m)| - R_m   (+inf when every slot is empty),
//   psi = sigma sum_j max(0, eps + r - sd_j)^2,   clearance = min_j sd_j - r.
#pragma once
#include <math.h>

#include "readout_view.hpp"

namespace gvi {

constexpr int BALLS_SLOTS = GVI_BALLS_MAX_M;
constexpr int balls_point_stride(int P, int d) { return readout_stride(READOUT_BALLS, P, d); }   // W_j | c_j | tau_j
constexpr int balls_slot_stride(int P) { return 2 * P + 1; }                 // o_m | v_m | R_m
GVI_HD_INLINE bool balls_slot_empty(double R) { return R == -INFINITY; }

// Signed distance from the read-out point q [P] to the union of the slots that are not empty, the balls taken at time tau
// (+inf when every slot is empty).  balls: the BALLS_SLOTS slots of the factor's block.  The one distance code of the kind: psi
// and the clearance at a sample (hinge_balls_points) and f_j at a quadrature point of the read-out rule (readout_moments.hpp).
template <int P>
GVI_HD_INLINE double balls_signed_distance(const double* balls, double tau, const double* q) {
  double sd = INFINITY;
  const double* b = balls;
  for (int m = 0; m < BALLS_SLOTS; ++m, b += balls_slot_stride(P)) {
    const double R = b[2 * P];
    if (balls_slot_empty(R)) continue;
    double d2 = 0.0;
    for (int r = 0; r < P; ++r) {
      const double e = q[r] - fma(tau, b[P + r], b[r]);
      d2 = fma(e, e, d2);
    }
    sd = fmin(sd, sqrt(d2) - R);
  }
  return sd;
}

// Walks the J check points of one factor at the slice x and calls visit(sd_j, r), as the *_points functions of
// psi_point.hpp do: psi and the clearance are two visitors of this walk.
template <int P, typename V>
GVI_HD_INLINE void hinge_balls_points(const double* p, const double* x, int d, int J, V&& visit) {
  const int stride = balls_point_stride(P, d);   // a plain pointer walk, as hinge_sdf_seg_points (psi_point.hpp)
  const double* balls = p + 3 + J * stride;
  const double* wc = p + 3;
  for (int j = 0; j < J; ++j, wc += stride) {
    double q[P];
    for (int r = 0; r < P; ++r) {
      double v = wc[P * d + r];
      for (int c = 0; c < d; ++c) v = fma(wc[r * d + c], x[c], v);
      q[r] = v;
    }
    visit(balls_signed_distance<P>(balls, wc[P * (d + 1)], q), p[2]);
  }
}

template <int P>
GVI_HD_INLINE double psi_hinge_balls(const double* p, const double* x, int d, int J) {
  double cost = 0.0;
  hinge_balls_points<P>(p, x, d, J, [&](double sd, double r) { cost += hinge_sq(sd, p[1] + r, 1.0, p[0]); });
  return cost;
}

template <int P>
GVI_HD_INLINE double balls_clearance(const double* p, const double* x, int d, int J) {
  double c = INFINITY;
  hinge_balls_points<P>(p, x, d, J, [&](double sd, double r) { c = fmin(c, sd - r); });
  return c;
}

}  // namespace gvi
