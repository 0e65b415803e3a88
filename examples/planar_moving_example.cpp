// A planar point robot whose straight path from start to goal is crossed by a MOVING obstacle at mid-horizon: one ball with a
// constant velocity, stated as a ball factor per state (DevicePsi::hinge_balls2d, GVI_PSI_HINGE_BALLS_2D).  Factor t carries
// the ball where it is at the time of state t, so no grid is rasterised and no state sees the scene of another time: the ball
// stands on the path only at t = T / 2, and a static obstacle at its first or at its last position would leave the straight
// path free.  The clearance of the mean path -- the smallest distance of a state to the ball at that state's time, less the
// robot's radius -- is printed before and after the optimisation.
//   Usage: planar_moving_example [iterations]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "gvi/gvi_host.hpp"

using namespace gvi;

static const int T = 17, n = 4, nd = 2, K = T - 1, p = 3;
static const double BALL_RADIUS = 0.5, ROBOT_RADIUS = 0.1, EPS = 0.2, SIGMA = 15.0;

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 12;
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
  // the ball comes down the line x = 0.3 with speed 1.6 and is on the path, at (0.3, 0), at mid-horizon
  const double bvx = 0.0, bvy = -1.6, bx0 = 0.3, by0 = -bvy * horizon / 2;
  auto ball_at = [&](int t, double* x, double* y) { *x = bx0 + bvx * t * dt; *y = by0 + bvy * t * dt; };
  auto clearance_of = [&](const VectorXd& mu) {
    double c = inf;
    for (int t = 0; t < T; ++t) {
      double x, y;
      ball_at(t, &x, &y);
      c = std::fmin(c, std::hypot(mu(t * n) - x, mu(t * n + 1) - y) - BALL_RADIUS - ROBOT_RADIUS);
    }
    return c;
  };
  std::vector<MatrixXd> W{MatrixXd::Zero(nd, n)};
  std::vector<VectorXd> c{VectorXd::Zero(nd)};
  for (int r = 0; r < nd; ++r) W[0](r, r) = 1.0;
  MatrixXd vel(1, 2);
  vel(0, 0) = bvx; vel(0, 1) = bvy;
  VectorXd radii(1);
  radii(0) = BALL_RADIUS;
  using Factor = NGDFactorizedBaseGH<NoneType>;
  auto none = [](const VectorXd&, const NoneType&) { return 0.0; };
  std::vector<std::shared_ptr<Factor>> factors;
  for (int k = 0; k < K; ++k)
    factors.emplace_back(new Factor(2 * n, n, p, none, NoneType{}, T, k, 1.0, 10.0, DevicePsi::QuadPrior(Phi, Qinv)));
  for (int t = 0; t < T; ++t) {
    MatrixXd centre(1, 2);
    ball_at(t, &centre(0, 0), &centre(0, 1));
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 5.0, 10.0,
                                    DevicePsi::hinge_balls2d(SIGMA, EPS, ROBOT_RADIUS, W, c, {0.0}, centre, vel, radii)));
  }
  for (int e = 0; e < 2; ++e) {
    const int t = e ? T - 1 : 0;
    VectorXd m0(n);
    for (int i = 0; i < n; ++i) m0(i) = init_mu(t * n + i);
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::FixedPrior(m0, Kinv)));
  }
  NGDGH<Factor> opt{factors, n, T, iters};
  opt.set_niter_low_temperature(iters);
  opt.set_initial_values(init_mu, init_prec);
  const double before = clearance_of(init_mu);
  opt.optimize(false);
  const double after = clearance_of(opt.mean());
  // set 1: the sets are formed in the order the factors were given (priors, balls, anchors)
  const VectorXd sampled = opt.sample_clearance(512, 7, 1);
  int clear = 0;
  for (int j = 0; j < sampled.size(); ++j) clear += sampled(j) >= 0.0;
  std::printf("clearance of the mean path to the moving ball: %.4f before, %.4f after %d iterations; sampled trajectories that stay clear of it: %.3f\n",
              before, after, iters, (double)clear / (double)sampled.size());
  return 0;
}
