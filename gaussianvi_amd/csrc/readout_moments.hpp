// Read-out-space quadrature of the obstacle kinds on linear read-outs (PSI_READOUT, psi_kinds.hpp): the
// arithmetic without lane structure.  Plain C++17 that also compiles for the host (tests/stubs/readout_on_cpu.cpp runs it under
// AddressSanitizer / UBSan); the kernel that calls it is in kernels_readout.hpp.
//
// psi(x) = sum_j f_j(q_j), q_j = W_j x + c_j of dimension P = 2 / 3.  For x = mu + S z, z ~ N(0, I), S ANY root of Sigma stored
// row-major (S[i * d + c] is entry c of row i):
//   G_j = W_j S (P x d),  g_j = W_j mu + c_j,  C_j = G_j G_j^T = W_j Sigma W_j^T,
//   L_j   the lower Cholesky factor of C_j in the row order of W_j, under the semidefinite rule of readout_chol,
//   Gam_j = "L_j^-1 G_j" by forward substitution over the kept coordinates (rows of dropped coordinates are zero).
// xi = Gam_j z is a standard Gaussian on the kept coordinates and q_j = g_j + L_j xi, so with the order-q tensor Gauss-Hermite
// rule (xi_a, om_a) over the kept coordinates
//   e0_j = sum om f,   h_j = sum om xi f,   H_j = sum om (xi xi^T - I) f,      f = f_j(g_j + L_j xi),
//   E[psi] = sum_j e0_j     E[z psi] = sum_j Gam_j^T h_j     E[z z^T psi] = E[psi] I + sum_j Gam_j^T H_j Gam_j.
// The tensor rule depends on the root of C_j, so L_j is exactly the Cholesky factor; it does not depend on the root S of Sigma.
// Every product that is added goes through fma explicitly, so the host build and the device build round alike.
// Where W_j, c_j and tau_j sit in a block, and the entries of G_j and g_j (readout_G_entry / readout_g_entry): readout_view.hpp.
#pragma once
#include <math.h>
#include <stdint.h>

#include "balls_psi.hpp"

namespace gvi {

constexpr int READOUT_MAX_ORDER = 16;       // nodes of the 1-D rule
constexpr int READOUT_MAX_POINTS = 1024;    // order^P nodes of the tensor rule of one check point

// order^P
constexpr int64_t readout_points(int order, int P) {
  int64_t n = 1;
  for (int k = 0; k < P; ++k) n *= order;
  return n;
}
// a rule gvi_factors_set_readout_rule accepts for a kind of read-out dimension P (0 switches the rule off and is not asked here)
constexpr bool readout_order_ok(int order, int P) {
  return order >= 2 && order <= READOUT_MAX_ORDER && readout_points(order, P) <= READOUT_MAX_POINTS;
}

// The lower Cholesky factor of the P x P matrix C (only its lower triangle is read) under the semidefinite rule, per column k:
//   pivot p = C_kk - sum_{i<k} L_ki^2, thr = 64 2^-52 C_kk;
//   |p| <= thr: coordinate k is DROPPED -- its column of L is zero and its rule is the single node 0 with weight 1;
//   p NaN, p < -thr or C_kk < 0: ok = false, every output of the factor is NaN.
template <int P>
struct ReadoutChol {
  double L[P * P];      // row-major, zero above the diagonal
  bool keep[P];
  bool ok;
  int nkept;
};
template <int P>
GVI_HD_INLINE ReadoutChol<P> readout_chol(const double* C) {
  ReadoutChol<P> o;
  o.ok = true;
  o.nkept = 0;
  GVI_UNROLL
  for (int e = 0; e < P * P; ++e) o.L[e] = 0.0;
  GVI_UNROLL
  for (int k = 0; k < P; ++k) {
    const double ckk = C[k * P + k];
    double p = ckk;
  GVI_UNROLL
    for (int i = 0; i < k; ++i) p = fma(-o.L[k * P + i], o.L[k * P + i], p);
    const double thr = 64.0 * 0x1p-52 * ckk;
    if (isnan(p) || p < -thr || ckk < 0.0) o.ok = false;
    o.keep[k] = o.ok && !(fabs(p) <= thr);
    if (o.keep[k]) {
      ++o.nkept;
      const double piv = sqrt(p);
      o.L[k * P + k] = piv;
  GVI_UNROLL
      for (int r = k + 1; r < P; ++r) {
        double v = C[r * P + k];
  GVI_UNROLL
        for (int i = 0; i < k; ++i) v = fma(-o.L[r * P + i], o.L[k * P + i], v);
        o.L[r * P + k] = v / piv;
      }
    }
  }
  return o;
}

// Column c of Gam by forward substitution, in place: col[k * stride] holds G_kc on entry and Gam_kc on return.
template <int P>
GVI_HD_INLINE void readout_gamma_col(const ReadoutChol<P>& ch, double* col, int stride) {
  double gm[P];
  GVI_UNROLL
  for (int k = 0; k < P; ++k) {
    double v = col[k * stride];
  GVI_UNROLL
    for (int i = 0; i < k; ++i) v = fma(-ch.L[k * P + i], gm[i], v);
    gm[k] = ch.keep[k] ? v / ch.L[k * P + k] : 0.0;
    col[k * stride] = gm[k];
  }
}

// nodes of the tensor rule of one check point: order^nkept
template <int P>
GVI_HD_INLINE int readout_node_count(const ReadoutChol<P>& ch, int order) {
  int n = 1;
  GVI_UNROLL
  for (int k = 0; k < P; ++k)
    if (ch.keep[k]) n *= order;
  return n;
}

// Node idx of the tensor rule: the kept coordinates are the digits of idx in base `order`, the first kept coordinate the lowest
// digit.  xi [P] (0 on a dropped coordinate), the weight is returned.  nodes / weights: the 1-D rule [order] each.
template <int P>
GVI_HD_INLINE double readout_node(const ReadoutChol<P>& ch, int order, const double* nodes, const double* weights, int idx, double* xi) {
  double om = 1.0;
  GVI_UNROLL
  for (int k = 0; k < P; ++k) {
    if (ch.keep[k]) {
      const int a = idx % order;
      idx /= order;
      xi[k] = nodes[a];
      om *= weights[a];
    } else {
      xi[k] = 0.0;
    }
  }
  return om;
}

// q = g + L xi
template <int P>
GVI_HD_INLINE void readout_point(const ReadoutChol<P>& ch, const double* g, const double* xi, double* q) {
  GVI_UNROLL
  for (int r = 0; r < P; ++r) {
    double v = g[r];
  GVI_UNROLL
    for (int k = 0; k <= r; ++k) v = fma(ch.L[r * P + k], xi[k], v);
    q[r] = v;
  }
}

// the sums of one check point: e0, h [P], H [P x P] (the upper triangle k <= l is accumulated; readout_store_sums mirrors it)
template <int P>
struct ReadoutSums {
  double e0;
  double h[P];
  double H[P * (P + 1) / 2];
};
template <int P>
GVI_HD_INLINE void readout_zero(ReadoutSums<P>& s) {
  s.e0 = 0.0;
  GVI_UNROLL
  for (int k = 0; k < P; ++k) s.h[k] = 0.0;
  GVI_UNROLL
  for (int e = 0; e < P * (P + 1) / 2; ++e) s.H[e] = 0.0;
}
template <int P>
GVI_HD_INLINE void readout_accumulate(ReadoutSums<P>& s, double om, const double* xi, double f) {
  const double wf = om * f;
  s.e0 += wf;
  int e = 0;
  GVI_UNROLL
  for (int k = 0; k < P; ++k) {
    s.h[k] = fma(wf, xi[k], s.h[k]);
  GVI_UNROLL
    for (int l = k; l < P; ++l, ++e) s.H[e] = fma(wf, fma(xi[k], xi[l], k == l ? -1.0 : 0.0), s.H[e]);
  }
}
// h -> hs [P], H -> Hs [P x P] symmetric; zero on the dropped coordinates (H is defined on the kept ones)
template <int P>
GVI_HD_INLINE void readout_store_sums(const ReadoutChol<P>& ch, const ReadoutSums<P>& s, double* hs, double* Hs) {
  int e = 0;
  GVI_UNROLL
  for (int k = 0; k < P; ++k) {
    hs[k] = ch.keep[k] ? s.h[k] : 0.0;
  GVI_UNROLL
    for (int l = k; l < P; ++l, ++e) {
      const double v = ch.keep[k] && ch.keep[l] ? s.H[e] : 0.0;
      Hs[k * P + l] = v;
      Hs[l * P + k] = v;
    }
  }
}

// f at a read-out point for the analytic balls: the hinge of psi_hinge_balls on the distance of hinge_balls_points.
// p: the factor's block, balls its slots and tau the time of the check point (ReadoutView::balls, tau).
template <int P>
GVI_HD_INLINE double readout_f_balls(const double* p, const double* balls, double tau, const double* q) {
  return hinge_sq(balls_signed_distance<P>(balls, tau, q), p[1] + p[2], 1.0, p[0]);
}

// One check point, the nodes one after the other (a wave of the kernel strides its lanes over them and adds the lanes' sums up):
// Gam [P x d] row-major, the sums in *s.  f(q) is the check point's function of the read-out point.  false: the factor is NaN.
template <int P, typename F>
inline bool readout_check_point(int d, const double* W, const double* cvec, const double* mu, const double* S, int order,
                                const double* nodes, const double* weights, F&& f, double* Gam, ReadoutSums<P>* s) {
  double C[P * P], g[P];
  for (int r = 0; r < P; ++r) {
    for (int c = 0; c < d; ++c) Gam[r * d + c] = readout_G_entry(W, S, d, r, c);
    g[r] = readout_g_entry(W, cvec, mu, d, r);
  }
  for (int r = 0; r < P; ++r)
    for (int t = 0; t <= r; ++t) {
      double v = 0.0;
      for (int c = 0; c < d; ++c) v = fma(Gam[r * d + c], Gam[t * d + c], v);
      C[r * P + t] = v;
      C[t * P + r] = v;
    }
  const ReadoutChol<P> ch = readout_chol<P>(C);
  readout_zero(*s);
  if (!ch.ok) return false;
  for (int c = 0; c < d; ++c) readout_gamma_col<P>(ch, Gam + c, d);
  const int nn = readout_node_count<P>(ch, order);
  ReadoutSums<P> acc;
  readout_zero(acc);
  for (int idx = 0; idx < nn; ++idx) {
    double xi[P], q[P];
    const double om = readout_node<P>(ch, order, nodes, weights, idx, xi);
    readout_point<P>(ch, g, xi, q);
    readout_accumulate<P>(acc, om, xi, f(q));
  }
  double hs[P], Hs[P * P];
  readout_store_sums<P>(ch, acc, hs, Hs);
  s->e0 = acc.e0;
  int e = 0;
  for (int k = 0; k < P; ++k) {
    s->h[k] = hs[k];
    for (int l = k; l < P; ++l, ++e) s->H[e] = Hs[k * P + l];
  }
  return true;
}

}  // namespace gvi
