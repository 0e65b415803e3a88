// The planning problem of planar_example.cpp inside a SAFE CORRIDOR: one half-space factor per state (DevicePsi::hinge_halfspace,
// GVI_PSI_HINGE_HALFSPACE) whose four rows n_j^T pos <= b_j are the faces of a strip of half-width HALF_WIDTH around the
// straight line from start to goal, closed at both ends; the velocity columns of the rows are zero.  A row is a squared hinge of
// the scalar n_j^T pos, a 1-D Gaussian, so the device takes the factor's Gaussian moments in closed form -- no sigma points.
// The problem is solved twice, without and with the corridor, and trajectories sampled from each posterior are scored by the
// distance to the nearest face, min_t min_j (b_j - n_j^T pos_t): negative where a sampled trajectory leaves the corridor.
//   Usage: planar_corridor_example [iterations]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "gvi/gvi_host.hpp"

using namespace gvi;

static const int T = 17, n = 4, nd = 2, K = T - 1, p = 3;
static const double HALF_WIDTH = 0.35, MARGIN_X = 0.3;      // the strip, and how far it reaches past start and goal

// share of the S sampled trajectories that stay inside the corridor at every state, and the smallest distance of the mean path to a face
static void solve(bool corridor, int iters, std::shared_ptr<const PlanarSDF> sdf, double* share, double* mean_margin) {
  const double dt = 0.25, qc = 0.8, inf = std::numeric_limits<double>::infinity();
  const int J = 4;
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
  // the corridor: unit normal u across the line start -> goal, unit tangent w along it; faces +-u (the strip) and +-w (its ends);
  // the hinge starts eps = 0.05 inside.  The run without it has no such set: its samples are scored against the same faces by
  // hand below.
  const double len = std::hypot(gx - sx, gy - sy), wx = (gx - sx) / len, wy = (gy - sy) / len, ux = -wy, uy = wx;
  MatrixXd A(J, n);
  VectorXd b(J), sigma(J), eps(J);
  A(0, 0) = ux; A(0, 1) = uy; b(0) = ux * sx + uy * sy + HALF_WIDTH;
  A(1, 0) = -ux; A(1, 1) = -uy; b(1) = -(ux * sx + uy * sy) + HALF_WIDTH;
  A(2, 0) = wx; A(2, 1) = wy; b(2) = wx * gx + wy * gy + MARGIN_X;
  A(3, 0) = -wx; A(3, 1) = -wy; b(3) = -(wx * sx + wy * sy) + MARGIN_X;
  for (int j = 0; j < J; ++j) { sigma(j) = 500.0; eps(j) = 0.05; }
  auto margin_of = [&](double x, double y) {
    double m = inf;
    for (int j = 0; j < J; ++j) m = std::fmin(m, b(j) - A(j, 0) * x - A(j, 1) * y);
    return m;
  };
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
  if (corridor)
    for (int t = 0; t < T; ++t)
      factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::hinge_halfspace(A, b, sigma, eps)));
  NGDGH<Factor> opt{factors, n, T, iters};
  opt.set_niter_low_temperature(iters);
  opt.set_initial_values(init_mu, init_prec);
  opt.optimize(false);
  const VectorXd mu = opt.mean();
  *mean_margin = inf;
  for (int t = 0; t < T; ++t) *mean_margin = std::fmin(*mean_margin, margin_of(mu(t * n), mu(t * n + 1)));
  const int S = 512;
  int inside = 0;
  if (corridor) {
    // set 3: the sets are formed in the order the factors were given (priors, obstacles, anchors, corridor); the normals are unit
    // vectors, so the distance sample_clearance returns is b_j - n_j^T pos
    const VectorXd margin = opt.sample_clearance(S, 7, 3);
    for (int j = 0; j < S; ++j) inside += margin(j) >= 0.0;
  } else {
    const MatrixXd X = opt.sample(S, 7);                               // T n x S, the same stream
    for (int j = 0; j < S; ++j) {
      double m = inf;
      for (int t = 0; t < T; ++t) m = std::fmin(m, margin_of(X(t * n, j), X(t * n + 1, j)));
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
  for (int corridor = 0; corridor < 2; ++corridor) {
    double share, margin;
    solve(corridor != 0, iters, sdf, &share, &margin);
    std::printf("%s corridor: smallest distance of the mean path to a face %.4f; sampled trajectories inside the strip of half-width %.2f at every state: %.3f\n",
                corridor ? "with" : "without", margin, HALF_WIDTH, share);
  }
  return 0;
}
