// What the obstacle kinds on linear read-outs (PSI_READOUT, psi_kinds.hpp) share -- the register policies of kernels_reg.hpp,
// the read-out-space rule of readout_moments.hpp, balls_psi.hpp: where check point j's W_j | c_j | tau_j sit in a factor's block,
// the sums G = W S, g = W mu + c in ONE association, and the hinge.  Plain C++17 for host and device.  Every product that is
// added goes through fma explicitly, so the host build and the device build round alike whatever the contraction setting.
#pragma once
#include <math.h>

#include "psi_kinds.hpp"

namespace gvi {

// the squared hinge of every obstacle kind: sigma (slope max(0, thr - sd))^2
GVI_HD_INLINE double hinge_sq(double sd, double thr, double slope, double sigma) {
  const double err = sd > thr ? 0.0 : (thr - sd) * slope;
  return err * err * sigma;
}

// One factor's read-outs in its parameter block p = [sigma, eps, r | J check points | (BALLS: the ball slots)]: check point j has
// W(j) [P x d] row-major, c(j) [P] and, for the balls, the time tau(j).  LEAD: W and c are null, which readout_G_entry /
// readout_g_entry take for W = [I | 0], c = 0.
struct ReadoutView {
  const double* p;
  int P, d, J, cls;
  GVI_HD_INLINE int stride() const { return readout_stride(cls, P, d); }
  GVI_HD_INLINE const double* W(int j) const { return cls == READOUT_LEAD ? nullptr : p + 3 + j * stride(); }
  GVI_HD_INLINE const double* c(int j) const { return cls == READOUT_LEAD ? nullptr : W(j) + P * d; }
  GVI_HD_INLINE double tau(int j) const { return W(j)[P * (d + 1)]; }          // BALLS only
  GVI_HD_INLINE const double* balls() const { return p + 3 + J * stride(); }   // BALLS only
};

// entry (r, c) of G = W S (S row-major: S[i * d + c] is entry c of row i), and g_r = (W mu + c)_r: start from c_r, ascending i
GVI_HD_INLINE double readout_G_entry(const double* W, const double* S, int d, int r, int c) {
  if (!W) return S[r * d + c];
  double v = 0.0;
  for (int i = 0; i < d; ++i) v = fma(W[r * d + i], S[i * d + c], v);
  return v;
}
GVI_HD_INLINE double readout_g_entry(const double* W, const double* cvec, const double* mu, int d, int r) {
  if (!W) return mu[r];
  double v = cvec[r];
  for (int i = 0; i < d; ++i) v = fma(W[r * d + i], mu[i], v);
  return v;
}

// The register policies' fold of one factor, once per (factor, chunk): out [J][P (D + 1)] = (G_j [P][D] | g_j [P]), one entry per
// lane and pass (lane of 64).  At a sigma point x = mu + S z the read-out is then readout_q: P D FMAs, and x is never formed.
template <int D, int P>
GVI_HD_INLINE void readout_fold(const ReadoutView& v, const double* S, const double* mu, double* out, int lane) {
  constexpr int STRIDE = P * (D + 1);
  for (int e = lane; e < v.J * STRIDE; e += 64) {
    const int j = e / STRIDE, rem = e - j * STRIDE;
    out[e] = rem < P * D ? readout_G_entry(v.W(j), S, D, rem / D, rem - rem / D * D) : readout_g_entry(v.W(j), v.c(j), mu, D, rem - P * D);
  }
}
// q = g + G z from one (G [P][D] | g [P]) block
template <int D, int P>
GVI_HD_INLINE void readout_q(const double* Gg, const double (&z)[D], double (&q)[P]) {
  GVI_UNROLL
  for (int r = 0; r < P; ++r) {
    double v = Gg[P * D + r];
    GVI_UNROLL
    for (int c = 0; c < D; ++c) v = fma(Gg[r * D + c], z[c], v);
    q[r] = v;
  }
}

}  // namespace gvi
