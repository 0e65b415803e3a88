// The planning problem of planar_example.cpp with SPEED LIMITS: one limit factor per state (DevicePsi::hinge_box,
// GVI_PSI_HINGE_BOX) that bounds |vx| and |vy| and leaves the position free.  The factor is a squared hinge per coordinate, so
// the device takes its Gaussian moments in closed form -- no sigma points.  The problem is solved twice, without and with the
// limits, and trajectories sampled from each posterior are scored by the margin min_t min(v_max - |vx_t|, w_max - |vy_t|) of
// sample_clearance: negative where a sampled trajectory exceeds a limit at some state.
//   Usage: planar_limits_example [iterations]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "gvi/gvi_host.hpp"

using namespace gvi;

static const int T = 17, n = 4, nd = 2, K = T - 1, p = 3;
static const double V_MAX = 1.9, W_MAX = 0.6;

// share of the S sampled trajectories whose speeds stay inside the limits at every state, and the largest mean speeds
static void solve(bool limits, int iters, std::shared_ptr<const PlanarSDF> sdf, double* share, double* vx_max, double* vy_max) {
  const double dt = 0.25, qc = 0.8, inf = std::numeric_limits<double>::infinity();
  MatrixXd Phi = MatrixXd::Identity(n, n), Qinv(n, n);
  for (int i = 0; i < nd; ++i) {
    Phi(i, nd + i) = dt;
    Qinv(i, i) = 12.0 / (dt * dt * dt) / qc;
    Qinv(i, nd + i) = Qinv(nd + i, i) = -6.0 / (dt * dt) / qc;
    Qinv(nd + i, nd + i) = 4.0 / dt / qc;
  }
  const double sx = -3.0, sy = -0.4, gx = 3.0, gy = 0.4, horizon = (T - 1) * dt;
  const double vx = (gx - sx) / horizon, vy = (gy - sy) / horizon;
  VectorXd init_mu(T * n);
  for (int t = 0; t < T; ++t) {
    init_mu(t * n + 0) = sx + vx * t * dt; init_mu(t * n + 1) = sy + vy * t * dt;
    init_mu(t * n + 2) = vx; init_mu(t * n + 3) = vy;
  }
  MatrixXd Kinv = MatrixXd::Identity(n, n);
  for (int i = 0; i < n; ++i) Kinv(i, i) = 100.0;
  SpMat init_prec(T * n, T * n);
  {
    MatrixXd Lam(n, 2 * n), M(2 * n, 2 * n);
    for (int i = 0; i < n; ++i) { for (int j = 0; j < n; ++j) Lam(i, j) = -Phi(i, j); Lam(i, n + i) = 1.0; }
    for (int a = 0; a < 2 * n; ++a)
      for (int b = 0; b < 2 * n; ++b) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) s += Lam(i, a) * Qinv(i, j) * Lam(j, b);
        M(a, b) = s;
      }
    for (int k = 0; k < K; ++k)
      for (int a = 0; a < 2 * n; ++a)
        for (int b = 0; b < 2 * n; ++b) init_prec.coeffRef(k * n + a, k * n + b) += M(a, b);
    for (int i = 0; i < n; ++i) { init_prec.coeffRef(i, i) += 200.0; init_prec.coeffRef((T - 1) * n + i, (T - 1) * n + i) += 200.0; }
    for (int i = 0; i < T * n; ++i) init_prec.coeffRef(i, i) += 0.5;
  }
  // the limits: positions free (both sides infinite), |vx| <= V_MAX, |vy| <= W_MAX; the hinge starts eps = 0.05 inside.
  // The run without them has no such set: its samples are scored against the same limits by hand below.
  VectorXd sigma(n), eps(n), lo(n), hi(n);
  for (int i = 0; i < n; ++i) { sigma(i) = 500.0; eps(i) = 0.05; lo(i) = -inf; hi(i) = inf; }
  lo(2) = -V_MAX; hi(2) = V_MAX; lo(3) = -W_MAX; hi(3) = W_MAX;
  using Factor = NGDFactorizedBaseGH<NoneType>;
  auto none = [](const VectorXd&, const NoneType&) { return 0.0; };
  std::vector<std::shared_ptr<Factor>> factors;
  for (int k = 0; k < K; ++k)
    factors.emplace_back(new Factor(2 * n, n, p, none, NoneType{}, T, k, 1.0, 10.0, DevicePsi::QuadPrior(Phi, Qinv)));
  for (int t = 0; t < T; ++t)
    factors.emplace_back(new Factor(n, n, p + 1, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::HingeSdf2D(15.5, 0.5, 0.3, sdf)));
  for (int e = 0; e < 2; ++e) {
    const int t = e ? T - 1 : 0;
    VectorXd m0(n);
    for (int i = 0; i < n; ++i) m0(i) = init_mu(t * n + i);
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::FixedPrior(m0, Kinv)));
  }
  if (limits)
    for (int t = 0; t < T; ++t)
      factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::hinge_box(sigma, eps, lo, hi)));
  NGDGH<Factor> opt{factors, n, T, iters};
  opt.set_niter_low_temperature(iters);
  opt.set_initial_values(init_mu, init_prec);
  opt.optimize(false);
  const VectorXd mu = opt.mean();
  *vx_max = *vy_max = 0.0;
  for (int t = 0; t < T; ++t) { *vx_max = std::fmax(*vx_max, std::fabs(mu(t * n + 2))); *vy_max = std::fmax(*vy_max, std::fabs(mu(t * n + 3))); }
  const int S = 512;
  int inside = 0;
  if (limits) {
    // set 3: the sets are formed in the order the factors were given (priors, obstacles, anchors, limits)
    const VectorXd margin = opt.sample_clearance(S, 7, 3);
    for (int j = 0; j < S; ++j) inside += margin(j) >= 0.0;
  } else {
    const MatrixXd X = opt.sample(S, 7);                               // T n x S, the same stream
    for (int j = 0; j < S; ++j) {
      double m = inf;
      for (int t = 0; t < T; ++t) m = std::fmin(m, std::fmin(V_MAX - std::fabs(X(t * n + 2, j)), W_MAX - std::fabs(X(t * n + 3, j))));
      inside += m >= 0.0;
    }
  }
  *share = (double)inside / S;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 12;
  auto sdf = std::make_shared<PlanarSDF>();
  sdf->origin_x = -5.0; sdf->origin_y = -4.0; sdf->cell_size = 0.1;
  sdf->field = MatrixXd(81, 101);
  const double cx[2] = {0.0, -1.0}, cy[2] = {1.6, -2.2}, cr[2] = {1.2, 0.9};
  for (int r = 0; r < 81; ++r)
    for (int c = 0; c < 101; ++c) {
      const double x = -5.0 + c * 0.1, y = -4.0 + r * 0.1;
      double best = 1e300;
      for (int o = 0; o < 2; ++o) best = std::fmin(best, std::hypot(x - cx[o], y - cy[o]) - cr[o]);
      sdf->field(r, c) = best;
    }
  for (int limits = 0; limits < 2; ++limits) {
    double share, vx, vy;
    solve(limits != 0, iters, sdf, &share, &vx, &vy);
    std::printf("%s limits: largest mean |vx| %.4f |vy| %.4f; sampled trajectories inside |vx| <= %.1f, |vy| <= %.1f at every state: %.3f\n",
                limits ? "with" : "without", vx, vy, V_MAX, W_MAX, share);
  }
  return 0;
}
