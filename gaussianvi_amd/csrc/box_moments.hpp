// Closed-form Gaussian moments of one side of the squared hinge of GVI_PSI_HINGE_BOX.  Plain C++ that
// also compiles for the host (tests/stubs/box_side_on_cpu.cpp runs it under AddressSanitizer / UBSan); the kernels that call
// it are in kernels_closed.hpp (PsiBoxHinge of kernels_reg.hpp is the quadrature form).
//
// One coordinate x = m + sd z, z ~ N(0, 1), one side with threshold a:  h(x) = sigma max(0, sgn (x - a))^2, sgn = +1 for the
// upper side (a = hi - eps), -1 for the lower one (a = lo + eps).  With t = sgn (m - a) / sd -- the distance of the mean INTO the
// hinge in standard deviations -- Phi the normal distribution function and phi its density:
//   e0 = E[h]      = sigma sd^2 [(1 + t^2) Phi(t) + t phi(t)]
//   e1 = E[h'(x)]  = sgn 2 sigma sd [t Phi(t) + phi(t)]
//   e2 = E[h''(x)] = 2 sigma Phi(t)
// By Stein's lemma E[z h] = sd e1 and E[(z^2 - 1) h] = sd^2 e2, which is what the z-space moments of the factor need.
// Phi goes through erfc, so the lower tail keeps its digits: Phi(-6) = 9.9e-10 to full precision, where 1 - Phi(6) holds 7
// digits.  The brackets themselves cancel for t < 0 -- (1 + t^2) Phi(t) and t phi(t) agree to t^4 / 2 of their size, 3 digits at
// t = -6 -- so for t <= -3 the three brackets come from the repeated integrals of erfc at x = -t / sqrt 2 instead:
//   Phi(t) = i0erfc(x) / 2,   t Phi + phi = i1erfc(x) / sqrt 2,   (1 + t^2) Phi + t phi = 2 i2erfc(x),
// with i(-1)erfc = 2 / sqrt(pi) exp(-x^2) and the ratios r_n = i(n)erfc / i(n-1)erfc = 1 / (2 x + 2 (n + 1) r_(n+1)), a continued
// fraction of positive terms evaluated backwards from r_65 = 0 (converged to the last bit for x >= 2.1): products only, no
// difference of nearly equal numbers.  sd = 0 (a deterministic coordinate) takes the limit: the hinge at the mean itself.
#pragma once
#include <math.h>

#include "hd.hpp"

namespace gvi {

struct BoxSide { double e0, e1, e2; };

#define BOX_TAIL_T (-3.0)            /* at and below: the continued fraction */
#define BOX_TAIL_TERMS 64

// gap = sgn (m - a): how far the mean is inside the hinge (negative: outside).  The caller skips an infinite side: t phi(t) at
// t = +-inf is 0 * inf.
GVI_HD inline BoxSide box_side(double sigma, double sd, double gap, double sgn) {
  BoxSide r;
  if (!(sd > 0.0)) {
    const double g = gap > 0.0 ? gap : 0.0;
    r.e0 = sigma * g * g;
    r.e1 = sgn * 2.0 * sigma * g;
    r.e2 = gap > 0.0 ? 2.0 * sigma : 0.0;
    return r;
  }
  const double t = gap / sd;
  double b0, b1, b2;                  // Phi(t),  t Phi + phi,  (1 + t^2) Phi + t phi
  if (t <= BOX_TAIL_T) {
    const double x = -t * 0.70710678118654752440;
    double rn = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
    for (int n = BOX_TAIL_TERMS; n >= 0; --n) {
      rn = 1.0 / (2.0 * x + 2.0 * (n + 1) * rn);
      if (n == 2) r2 = rn;
      if (n == 1) r1 = rn;
      if (n == 0) r0 = rn;
    }
    const double i0 = r0 * (1.12837916709551257390 * exp(-x * x)), i1 = r1 * i0, i2 = r2 * i1;
    b0 = 0.5 * i0;
    b1 = 0.70710678118654752440 * i1;
    b2 = 2.0 * i2;
  } else {
    const double phi = 0.39894228040143267794 * exp(-0.5 * t * t);
    b0 = 0.5 * erfc(-t * 0.70710678118654752440);
    b1 = t * b0 + phi;
    b2 = (1.0 + t * t) * b0 + t * phi;
  }
  r.e0 = sigma * sd * sd * b2;
  r.e1 = sgn * 2.0 * sigma * sd * b1;
  r.e2 = 2.0 * sigma * b0;
  return r;
}

// The two sides of coordinate i of a factor: p = [sigma (d) | eps (d) | lo (d) | hi (d)], mean m, standard deviation sd.
// An infinite limit switches its side off.
GVI_HD inline BoxSide box_coordinate(const double* p, int d, int i, double m, double sd) {
  const double sigma = p[i], eps = p[d + i], lo = p[2 * d + i], hi = p[3 * d + i];
  BoxSide s = {0.0, 0.0, 0.0};
  if (hi < INFINITY) {
    const BoxSide u = box_side(sigma, sd, m - (hi - eps), 1.0);
    s.e0 += u.e0; s.e1 += u.e1; s.e2 += u.e2;
  }
  if (lo > -INFINITY) {
    const BoxSide l = box_side(sigma, sd, (lo + eps) - m, -1.0);
    s.e0 += l.e0; s.e1 += l.e1; s.e2 += l.e2;
  }
  return s;
}

// psi(x) = sum_i sigma_i [max(0, x_i - (hi_i - eps_i))^2 + max(0, (lo_i + eps_i) - x_i)^2]; an infinite side adds nothing and
// a coordinate without a finite side is not read
GVI_HD inline double psi_hinge_box(const double* p, const double* x, int d) {
  double cost = 0.0;
  for (int i = 0; i < d; ++i) {
    const double sigma = p[i], eps = p[d + i], lo = p[2 * d + i], hi = p[3 * d + i];
    if (hi < INFINITY) {
      const double e = x[i] - (hi - eps);
      if (e > 0.0) cost += sigma * e * e;
    }
    if (lo > -INFINITY) {
      const double e = (lo + eps) - x[i];
      if (e > 0.0) cost += sigma * e * e;
    }
  }
  return cost;
}

// margin(x) = min_i min(hi_i - x_i, x_i - lo_i): negative where a limit itself (not its eps band) is passed; +inf without limits
GVI_HD inline double box_margin(const double* p, const double* x, int d) {
  double mg = INFINITY;
  for (int i = 0; i < d; ++i) {
    const double lo = p[2 * d + i], hi = p[3 * d + i];
    mg = fmin(mg, fmin(hi - x[i], x[i] - lo));
  }
  return mg;
}

}  // namespace gvi
