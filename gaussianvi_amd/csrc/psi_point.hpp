// psi and clearance of the kinds that keep their raw parameter block (PSI_RAW, psi_kinds.hpp) at ONE state slice x: the grid
// look-ups, the check-point walks of the hinge-on-SDF kinds, and psi_point / hinge_psi_clearance, THE chain from a kind to its
// psi_* function, for the generic moments kernel, the sample-cost kernel and (the psi_* functions) the register and sign-orbit
// kernels.  Plain C++17 that also compiles for the host: tests/stubs/psi_point_on_cpu.cpp fills a FactorDev with host pointers and
// runs every kind under AddressSanitizer / UBSan.  The look-ups keep their products unfused as written.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "balls_psi.hpp"
#include "box_moments.hpp"
#include "factor_dev.hpp"
#include "halfspace_moments.hpp"

namespace gvi {

GVI_HD inline double psi_range_1d(const double* p, double x) {
  // p = [y, mu_p, f*b, sig_r_sq, sig_p_sq]            (src/1d_example.cpp:25-35)
  const double e = x - p[1], r = p[0] - p[2] / x;
  return e * e / p[4] / 2 + r * r / p[3] / 2;
}

// PlanarSDF::getSignedDistance (helpers/CudaOperation.h:61-103): query clamped to the grid, bilinear
// interpolation of the column-major field (data[r + c rows], :130).
GVI_HD inline double sdf2d_lookup(const FactorDev& f, double px, double py) {
  const double xmax = f.sdf_ox + (f.sdf_cols - 1.0) * f.sdf_cell, ymax = f.sdf_oy + (f.sdf_rows - 1.0) * f.sdf_cell;
  const double xin = px < f.sdf_ox ? f.sdf_ox : (px > xmax ? xmax : px);
  const double yin = py < f.sdf_oy ? f.sdf_oy : (py > ymax ? ymax : py);
  const double col = (xin - f.sdf_ox) * f.sdf_inv_cell, row = (yin - f.sdf_oy) * f.sdf_inv_cell;
  const double lr = floor(row), lc = floor(col), hr = lr + 1.0, hc = lc + 1.0;
  const int lri = (int)lr, lci = (int)lc;
  const int hri = lri + 1 < f.sdf_rows ? lri + 1 : f.sdf_rows - 1;    // weight is 0 there; keeps the read in bounds
  const int hci = lci + 1 < f.sdf_cols ? lci + 1 : f.sdf_cols - 1;
  const int R = f.sdf_rows;
  return (hr - row) * (hc - col) * f.sdf[lri + lci * R] + (row - lr) * (hc - col) * f.sdf[hri + lci * R] +
         (hr - row) * (col - lc) * f.sdf[lri + hci * R] + (row - lr) * (col - lc) * f.sdf[hri + hci * R];
}

// SignedDistanceField::getSignedDistance (helpers/CudaOperation.h:165-226): clamped trilinear interpolation of
// data[r + c rows + z rows cols] (:304-306); x -> column, y -> row, z -> slice.
GVI_HD inline double sdf3d_lookup(const FactorDev& f, double px, double py, double pz) {
  const double xmax = f.sdf_ox + (f.sdf_cols - 1.0) * f.sdf_cell, ymax = f.sdf_oy + (f.sdf_rows - 1.0) * f.sdf_cell,
               zmax = f.sdf_oz + (f.sdf_nz - 1.0) * f.sdf_cell;
  const double xin = px < f.sdf_ox ? f.sdf_ox : (px > xmax ? xmax : px);
  const double yin = py < f.sdf_oy ? f.sdf_oy : (py > ymax ? ymax : py);
  const double zin = pz < f.sdf_oz ? f.sdf_oz : (pz > zmax ? zmax : pz);
  const double col = (xin - f.sdf_ox) * f.sdf_inv_cell, row = (yin - f.sdf_oy) * f.sdf_inv_cell, zz = (zin - f.sdf_oz) * f.sdf_inv_cell;
  const double lr = floor(row), lc = floor(col), lz = floor(zz), hr = lr + 1.0, hc = lc + 1.0, hz = lz + 1.0;
  const int lri = (int)lr, lci = (int)lc, lzi = (int)lz;
  const int hri = lri + 1 < f.sdf_rows ? lri + 1 : f.sdf_rows - 1;
  const int hci = lci + 1 < f.sdf_cols ? lci + 1 : f.sdf_cols - 1;
  const int hzi = lzi + 1 < f.sdf_nz ? lzi + 1 : f.sdf_nz - 1;
  const size_t R = f.sdf_rows, RC = R * f.sdf_cols;
  const double* g = f.sdf;
  return (hr - row) * (hc - col) * (hz - zz) * g[lri + lci * R + lzi * RC] + (row - lr) * (hc - col) * (hz - zz) * g[hri + lci * R + lzi * RC] +
         (hr - row) * (col - lc) * (hz - zz) * g[lri + hci * R + lzi * RC] + (row - lr) * (col - lc) * (hz - zz) * g[hri + hci * R + lzi * RC] +
         (hr - row) * (hc - col) * (zz - lz) * g[lri + lci * R + hzi * RC] + (row - lr) * (hc - col) * (zz - lz) * g[hri + lci * R + hzi * RC] +
         (hr - row) * (col - lc) * (zz - lz) * g[lri + hci * R + hzi * RC] + (row - lr) * (col - lc) * (zz - lz) * g[hri + hci * R + hzi * RC];
}

// Check points of the hinge-on-SDF kinds.  Each *_points function walks the check points b of one factor at one state and
// calls visit(sd_b, r_b) with the signed distance at the point and the radius of its ball; psi (the sum of the hinges, hinge_sq
// of readout_view.hpp) and the clearance (min_b sd_b - r_b, costs of sampled trajectories: kernels_sample_cost.hpp) are two
// visitors of the SAME points in the same arithmetic.

// planar point robot (CudaOperation_PlanarPR::cost_obstacle_planar, helpers/CudaOperation.h:491-523): one ball at
// (x0, x1), slope 1.  p = [sigma, eps, r].
template <typename V>
GVI_HD_INLINE void hinge_sdf2d_points(const FactorDev& f, const double* p, double px, double py, V&& visit) {
  visit(sdf2d_lookup(f, px, py), p[2]);
}
GVI_HD inline double psi_hinge_sdf2d(const FactorDev& f, const double* p, double px, double py) {
  double cost = 0.0;
  hinge_sdf2d_points(f, p, px, py, [&](double sd, double r) { cost = hinge_sq(sd, p[1] + r, 1.0, p[0]); });
  return cost;
}

// planar quadrotor body (CudaOperation_Quad::cost_obstacle_planar / vec_balls, helpers/CudaOperation.h:565-606):
// pose (x, z, phi) = x[0:3]; n_balls check points along the body axis starting at
// pos - (L - 1.5 r)/2 (cos phi, sin phi), spaced L/n_balls.  p = [sigma, eps, r, slope, n_balls, L].
template <typename V>
GVI_HD_INLINE void hinge_sdf2d_body_points(const FactorDev& f, const double* p, double px, double pz, double phi, V&& visit) {
  double sn, cs;
  sincos(phi, &sn, &cs);
  const double r = p[2], L = p[5];
  const int nb = (int)p[4];
  const double lx = px - (L - r * 1.5) * cs / 2.0, lz = pz - (L - r * 1.5) * sn / 2.0;
  for (int i = 0; i < nb; ++i) visit(sdf2d_lookup(f, lx + L * cs / nb * i, lz + L * sn / nb * i), r);
}
GVI_HD inline double psi_hinge_sdf2d_body(const FactorDev& f, const double* p, double px, double pz, double phi) {
  const double thr = p[1] + p[2];
  double cost = 0.0;
  hinge_sdf2d_body_points(f, p, px, pz, phi, [&](double sd, double) { cost += hinge_sq(sd, thr, p[3], p[0]); });
  return cost;
}

// 3-D point robot (CudaOperation_3dpR::cost_obstacle_planar, helpers/CudaOperation.h:650-683).  p = [sigma, eps, r].
template <typename V>
GVI_HD_INLINE void hinge_sdf3d_points(const FactorDev& f, const double* p, double px, double py, double pz, V&& visit) {
  visit(sdf3d_lookup(f, px, py, pz), p[2]);
}
GVI_HD inline double psi_hinge_sdf3d(const FactorDev& f, const double* p, double px, double py, double pz) {
  double cost = 0.0;
  hinge_sdf3d_points(f, p, px, py, pz, [&](double sd, double r) { cost = hinge_sq(sd, p[1] + r, 1.0, p[0]); });
  return cost;
}

// 7-DOF-style arm (CudaOperation_3dArm::cost_obstacle + ForwardKinematics, helpers/CudaOperation.h:325-399, 752-771):
// sphere s sits on frame[s] of the DH chain T = prod_{i <= frame} DH(i, x_i + bias_i); n_balls = the factor dimension
// (theta.size(), :753), cost = sigma sum_s hinge(eps + radius_s - sdf(p_s))^2.  The reference builds every DH matrix
// from cosf / sinf (single precision, :388-395; products of two trig terms are float products) -- restated as such.
// Frames are non-decreasing (checked on the host), so the chain is advanced once.  p = [sigma, eps].
template <typename V>
GVI_HD_INLINE void hinge_sdf3d_arm_points(const FactorDev& f, const double* x, int d, V&& visit) {
  const double* A = f.arm;
  const int nd = (int)A[0], ns = (int)A[1];
  const double *a = A + 2, *al = a + nd, *dl = al + nd, *tb = dl + nd, *fr = tb + nd, *ce = fr + ns, *ra = ce + 3 * ns;
  double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};           // rows 0..2 of the homogeneous transform
  const int nb = d < ns ? d : ns;
  int done = -1;                                                  // last joint folded into T
  for (int s = 0; s < nb; ++s) {
    const int frame = (int)fr[s];
    while (done < frame) {
      const int i = ++done;
      const float th = (float)(x[i] + tb[i]), alf = (float)al[i];
      // cosf / sinf of the reference: float in, float out.  Libm's differ in the last float bit; the correctly rounded
      // value (double trig of the float argument, rounded to float) is the representative, as in the oracle
      const float c = (float)cos((double)th), sn = (float)sin((double)th), cA = (float)cos((double)alf), sA = (float)sin((double)alf);
      const double m00 = c, m01 = -sn * cA, m02 = sn * sA, m03 = a[i] * c;
      const double m10 = sn, m11 = c * cA, m12 = -c * sA, m13 = a[i] * sn;
      const double m21 = sA, m22 = cA, m23 = dl[i];
      GVI_UNROLL
      for (int r = 0; r < 3; ++r) {
        const double t0 = T[r * 4], t1 = T[r * 4 + 1], t2 = T[r * 4 + 2], t3 = T[r * 4 + 3];
        T[r * 4] = t0 * m00 + t1 * m10;
        T[r * 4 + 1] = t0 * m01 + t1 * m11 + t2 * m21;
        T[r * 4 + 2] = t0 * m02 + t1 * m12 + t2 * m22;
        T[r * 4 + 3] = t0 * m03 + t1 * m13 + t2 * m23 + t3;
      }
    }
    const double cx = ce[3 * s], cy = ce[3 * s + 1], cz = ce[3 * s + 2];
    const double px = T[3] + (T[0] * cx + T[1] * cy + T[2] * cz);
    const double py = T[7] + (T[4] * cx + T[5] * cy + T[6] * cz);
    const double pz = T[11] + (T[8] * cx + T[9] * cy + T[10] * cz);
    visit(sdf3d_lookup(f, px, py, pz), ra[s]);
  }
}
GVI_HD inline double psi_hinge_sdf3d_arm(const FactorDev& f, const double* p, const double* x, int d) {
  double cost = 0.0;
  hinge_sdf3d_arm_points(f, x, d, [&](double sd, double r) { cost += hinge_sq(sd, p[1] + r, 1.0, p[0]); });
  return cost;
}

// Obstacle factor on a segment (no reference counterpart): J = f.seg_J check points, each a linear
// read-out q_j = W_j x + c_j of the factor's slice x [d] (for d = 2n the pair of support states: W_j = the position rows of the
// Gauss-Markov interpolation [A(tau_j) | B(tau_j)]), one ball of radius r at each, slope 1.
// p = [sigma, eps, r | W_0 (P x d, row-major) | c_0 (P) | ... | W_{J-1} | c_{J-1}].  P = 2: the planar grid, P = 3: the 3-D field.
template <int P, typename V>
GVI_HD_INLINE void hinge_sdf_seg_points(const FactorDev& f, const double* p, const double* x, int d, V&& visit) {
  const double* wc = p + 3;
  for (int j = 0; j < f.seg_J; ++j, wc += P * (d + 1)) {
    double q[P];
    GVI_UNROLL
    for (int r = 0; r < P; ++r) {
      double v = wc[P * d + r];
      for (int c = 0; c < d; ++c) v = fma(wc[r * d + c], x[c], v);
      q[r] = v;
    }
    if constexpr (P == 2) visit(sdf2d_lookup(f, q[0], q[1]), p[2]);
    else visit(sdf3d_lookup(f, q[0], q[1], q[P - 1]), p[2]);
  }
}
template <int P>
GVI_HD inline double psi_hinge_sdf_seg(const FactorDev& f, const double* p, const double* x, int d) {
  double cost = 0.0;
  hinge_sdf_seg_points<P>(f, p, x, d, [&](double sd, double r) { cost += hinge_sq(sd, p[1] + r, 1.0, p[0]); });
  return cost;
}

// psi of factor k of a set that keeps its raw parameter block (PSI_RAW, psi_kinds.hpp) at the state slice x [d]: THE chain
// from a kind to its psi_* function.  NaN for a kind without raw psi (sum of squares: the caller's (A, b, sgn) form; host psi).
GVI_HD_INLINE double psi_point(const FactorDev& f, int k, const double* x) {
  const double* p = f.raw + (size_t)k * f.raw_stride;
  if (f.kind == KIND_RANGE_1D) return psi_range_1d(p, x[0]);
  if (f.kind == KIND_HINGE_SDF_2D) return psi_hinge_sdf2d(f, p, x[0], x[1]);
  if (f.kind == KIND_HINGE_SDF_2D_BODY) return psi_hinge_sdf2d_body(f, p, x[0], x[1], x[2]);
  if (f.kind == KIND_HINGE_SDF_3D) return psi_hinge_sdf3d(f, p, x[0], x[1], x[2]);
  if (f.kind == KIND_HINGE_SDF_3D_ARM) return psi_hinge_sdf3d_arm(f, p, x, f.d);
  if (f.kind == KIND_HINGE_SDF_2D_SEG) return psi_hinge_sdf_seg<2>(f, p, x, f.d);
  if (f.kind == KIND_HINGE_SDF_3D_SEG) return psi_hinge_sdf_seg<3>(f, p, x, f.d);
  if (f.kind == KIND_HINGE_BOX) return psi_hinge_box(p, x, f.d);
  if (f.kind == KIND_HINGE_HALFSPACE) return psi_hinge_halfspace(p, x, f.d, f.seg_J);
  if (f.kind == KIND_HINGE_BALLS_2D) return psi_hinge_balls<2>(p, x, f.d, f.seg_J);
  if (f.kind == KIND_HINGE_BALLS_3D) return psi_hinge_balls<3>(p, x, f.d, f.seg_J);
  return __builtin_nan("");
}

// psi and / or clearance of factor k of a raw-block set at the state slice x [d].  psi is psi_point; the clearance (PSI_CLEARANCE
// kinds) walks the same *_points as the kind's psi with a min-visitor.  eps and slope play no part in the clearance.
GVI_HD_INLINE void hinge_psi_clearance(const FactorDev& f, int k, const double* x, bool want_psi, bool want_clr, double& psi, double& clr) {
  if (want_psi) psi = psi_point(f, k, x);
  if (!want_clr) return;
  const double* p = f.raw + (size_t)k * f.raw_stride;
  double c = __builtin_inf();
  auto keep = [&](double sd, double r) { c = fmin(c, sd - r); };
  if (f.kind == KIND_HINGE_SDF_2D) hinge_sdf2d_points(f, p, x[0], x[1], keep);
  else if (f.kind == KIND_HINGE_SDF_2D_BODY) hinge_sdf2d_body_points(f, p, x[0], x[1], x[2], keep);
  else if (f.kind == KIND_HINGE_SDF_3D) hinge_sdf3d_points(f, p, x[0], x[1], x[2], keep);
  else if (f.kind == KIND_HINGE_SDF_3D_ARM) hinge_sdf3d_arm_points(f, x, f.d, keep);
  else if (f.kind == KIND_HINGE_SDF_2D_SEG) hinge_sdf_seg_points<2>(f, p, x, f.d, keep);
  else if (f.kind == KIND_HINGE_SDF_3D_SEG) hinge_sdf_seg_points<3>(f, p, x, f.d, keep);
  else if (f.kind == KIND_HINGE_BOX) c = box_margin(p, x, f.d);                        // limits on the slice itself (box_moments.hpp): the margin
  else if (f.kind == KIND_HINGE_HALFSPACE) c = halfspace_margin(p, x, f.d, f.seg_J);   // rows a_j^T x <= b_j (halfspace_moments.hpp): distance to the nearest active face
  else if (f.kind == KIND_HINGE_BALLS_2D) hinge_balls_points<2>(p, x, f.d, f.seg_J, keep);   // analytic balls (balls_psi.hpp): no grid
  else if (f.kind == KIND_HINGE_BALLS_3D) hinge_balls_points<3>(p, x, f.d, f.seg_J, keep);
  else c = __builtin_nan("");   // no clearance for this kind: the host refuses such a set before any launch
  clr = c;
}

}  // namespace gvi
