// Moving obstacles as analytic balls on the shim: DevicePsi::hinge_balls2d / hinge_balls3d with NGDFactorizedBaseGH, unary on
// a state's position and binary on the read-outs of MinimumAccGP::segment_readout, and the replacement of a set's parameters
// (set_device_psi + update_device_psi_params) when the predicted scene changes.
//   balls_callsite host   no device call: the parameter block, the padding with empty slots, the grouping rule, the refusals
//   balls_callsite gpu    a small planar planning graph whose straight-line start is crossed by one ball at the time of state 2:
//                         the ball factors there have a positive cost; a step runs; with the scene replaced by one whose ball
//                         stays away every ball factor costs exactly 0
// Prints "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "gvi/gvi_host.hpp"

using namespace gvi;

static int fails = 0;
static void expect(bool ok, const char* what) {
  if (!ok) { std::fprintf(stderr, "FAILED: %s\n", what); ++fails; }
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s host | gpu\n", argv[0]); return 2; }
  const int T = 5, nd = 2, n = 4, K = T - 1, p = 3;
  const double dt = 0.5, qc = 0.8;
  MinimumAccGP gp(MatrixXd::Identity(nd, nd) * qc, 0, dt, VectorXd::Zero(n));
  const double sigma = 15.5, eps = 0.1, radius = 0.05;
  // the start trajectory runs along y = 0 from x = -0.5 with speed 1; the ball comes down the line x = 0.5 and is at
  // (0.5, 0.02) at t = 1, the time of state 2
  MatrixXd centre0(1, 2), vel(1, 2), centre_far(1, 2);
  centre0(0, 0) = 0.5; centre0(0, 1) = 1.52; vel(0, 0) = 0.0; vel(0, 1) = -1.5;
  centre_far(0, 0) = 0.5; centre_far(0, 1) = 40.0;
  VectorXd radii(1);
  radii(0) = 0.2;
  std::vector<MatrixXd> W1{MatrixXd::Zero(nd, n)}, W, W3{MatrixXd::Zero(3, n)};
  std::vector<VectorXd> c1{VectorXd::Zero(nd)}, c, c3{VectorXd::Zero(3)};
  for (int r = 0; r < nd; ++r) W1[0](r, r) = W3[0](r, r) = 1.0;
  const std::vector<double> taus{dt / 4, dt / 2, 3 * dt / 4};
  gp.segment_readout(taus, nd, W, c);
  // ball m of factor i: where it is at the factor's time stamp t_i = i dt
  auto scene = [&](const MatrixXd& at0, int i) {
    MatrixXd o = at0;
    for (int r = 0; r < 2; ++r) o(0, r) += i * dt * vel(0, r);
    return o;
  };
  auto scene3 = [&](const MatrixXd& at0, int i, MatrixXd& v3) {
    MatrixXd o3 = MatrixXd::Zero(1, 3);
    v3 = MatrixXd::Zero(1, 3);
    const MatrixXd o = scene(at0, i);
    for (int r = 0; r < 2; ++r) { o3(0, r) = o(0, r); v3(0, r) = vel(0, r); }
    return o3;
  };

  if (std::strcmp(argv[1], "gpu") != 0) {
    const DevicePsi u = DevicePsi::hinge_balls2d(sigma, eps, radius, W1, c1, {0.0}, centre0, vel, radii);
    const DevicePsi b = DevicePsi::hinge_balls2d(sigma, eps, radius, W, c, taus, centre0, vel, radii);
    expect(u.kind == GVI_PSI_HINGE_BALLS_2D && GVI_PSI_HINGE_BALLS_2D == 13 && GVI_PSI_HINGE_BALLS_3D == 14 && GVI_BALLS_MAX_M == 8, "kind numbers");
    expect((int)u.params.size() == 3 + 1 * (nd * (n + 1) + 1) + 8 * (2 * nd + 1), "parameter block, unary, J = 1");
    expect((int)b.params.size() == 3 + 3 * (nd * (2 * n + 1) + 1) + 8 * (2 * nd + 1), "parameter block, binary, J = 3");
    const int ball = 3 + 1 * (nd * (n + 1) + 1);
    expect(u.params[0] == sigma && u.params[1] == eps && u.params[2] == radius && u.params[3] == 1.0 && u.params[ball - 1] == 0.0, "head, W and tau");
    expect(u.params[ball] == 0.5 && u.params[ball + 1] == 1.52 && u.params[ball + 3] == -1.5 && u.params[ball + 4] == 0.2, "the ball's slot");
    bool empty = true;
    for (int m = 1; m < 8; ++m) empty = empty && u.params[ball + m * 5 + 4] == -std::numeric_limits<double>::infinity();
    expect(empty, "seven empty slots: radius -inf");
    expect(b.params[3 + nd * 2 * n + nd] == taus[0], "tau of the first check point");
    expect(u.same_group(u) && !u.same_group(b), "sets with different block sizes stay apart");
    MatrixXd v3;
    const MatrixXd o3 = scene3(centre0, 0, v3);
    const DevicePsi t = DevicePsi::hinge_balls3d(sigma, eps, radius, W3, c3, {0.0}, o3, v3, radii);
    expect(t.kind == GVI_PSI_HINGE_BALLS_3D && (int)t.params.size() == 3 + (3 * (n + 1) + 1) + 8 * 7, "3-D descriptor");
    int threw = 0;
    try { (void)DevicePsi::hinge_balls2d(sigma, eps, radius, W3, c3, {0.0}, centre0, vel, radii); } catch (const std::invalid_argument&) { ++threw; }
    try { (void)DevicePsi::hinge_balls2d(sigma, eps, radius, W1, c1, {0.0, 1.0}, centre0, vel, radii); } catch (const std::invalid_argument&) { ++threw; }
    try { (void)DevicePsi::hinge_balls2d(sigma, eps, radius, W1, c1, {0.0}, MatrixXd::Zero(9, 2), MatrixXd::Zero(9, 2), VectorXd::Zero(9)); }
    catch (const std::invalid_argument&) { ++threw; }
    try { (void)DevicePsi::hinge_balls3d(sigma, eps, radius, W3, c3, {0.0}, centre0, vel, radii); } catch (const std::invalid_argument&) { ++threw; }
    expect(threw == 4, "a 3-row read-out, a missing tau, nine balls and 2-D centres for the 3-D kind are refused");
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
  }

  MatrixXd Kinv = MatrixXd::Identity(n, n) * 100.0;
  using Factor = NGDFactorizedBaseGH<NoneType>;
  auto none = [](const VectorXd&, const NoneType&) { return 0.0; };
  VectorXd init_mu(T * n);
  for (int t = 0; t < T; ++t) {
    init_mu(t * n) = -0.5 + 0.5 * t; init_mu(t * n + 1) = 0.0; init_mu(t * n + 2) = 1.0; init_mu(t * n + 3) = 0.0;
  }
  SpMat init_prec(T * n, T * n);
  for (int i = 0; i < T * n; ++i) init_prec.coeffRef(i, i) = 30000.0;
  for (int i = 0; i + n < T * n; ++i) init_prec.coeffRef(i, i + n) = init_prec.coeffRef(i + n, i) = -6000.0;
  std::vector<std::shared_ptr<Factor>> factors;
  for (int k = 0; k < K; ++k)
    factors.emplace_back(new Factor(2 * n, n, p, none, NoneType{}, T, k, 1.0, 10.0, gp.device_psi()));
  for (int t = 0; t < T; ++t)
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0,
                                    DevicePsi::hinge_balls2d(sigma, eps, radius, W1, c1, {0.0}, scene(centre0, t), vel, radii)));
  for (int k = 0; k < K; ++k)
    factors.emplace_back(new Factor(2 * n, n, p, none, NoneType{}, T, k, 1.0, 10.0,
                                    DevicePsi::hinge_balls2d(sigma, eps, radius, W, c, taus, scene(centre0, k), vel, radii)));
  for (int t = 0; t < T; ++t) {
    MatrixXd v3;
    const MatrixXd o3 = scene3(centre0, t, v3);
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::hinge_balls3d(sigma, eps, radius, W3, c3, {0.0}, o3, v3, radii)));
  }
  VectorXd m0[2] = {VectorXd(n), VectorXd(n)};
  for (int e = 0; e < 2; ++e) {
    const int t = e ? T - 1 : 0;
    for (int i = 0; i < n; ++i) m0[e](i) = init_mu(t * n + i);
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::FixedPrior(m0[e], Kinv)));
  }
  NGDGH<Factor> opt{factors, n, T, 2};
  opt.set_initial_values(init_mu, init_prec);
  const int U0 = K, B0 = K + T, S0 = K + T + K;              // first unary 2-D, binary 2-D, unary 3-D ball factor
  VectorXd fc = opt.factor_cost_vector();
  expect(fc.size() == (int)factors.size(), "one cost per factor");
  expect(fc(U0 + 2) > 0.0 && fc(U0) == 0.0 && fc(U0 + 4) == 0.0, "the ball meets the path at state 2 and at no end state");
  expect(fc(S0 + 2) > 0.0 && std::fabs(fc(S0 + 2) - fc(U0 + 2)) <= 1e-12 * fc(U0 + 2), "the 3-D kind on the plane z = 0 sees the same ball");
  double seg = 0.0;
  for (int k = 0; k < K; ++k) seg += fc(B0 + k);
  expect(seg > 0.0, "the binary factors see it between the states");
  opt.optimize(false);
  const VectorXd mean = opt.mean();
  bool fin = true;
  for (int i = 0; i < mean.size(); ++i) fin = fin && std::isfinite(mean(i));
  expect(fin, "finite iterate");
  const VectorXd clr = opt.sample_clearance(5, 3, 1);          // needs no grid
  for (int j = 0; j < clr.size(); ++j) expect(std::isfinite(clr(j)), "finite clearance");
  // the prediction changes: the ball is far away at all times
  for (int t = 0; t < T; ++t)
    factors[U0 + t]->set_device_psi(DevicePsi::hinge_balls2d(sigma, eps, radius, W1, c1, {0.0}, scene(centre_far, t), vel, radii));
  for (int k = 0; k < K; ++k)
    factors[B0 + k]->set_device_psi(DevicePsi::hinge_balls2d(sigma, eps, radius, W, c, taus, scene(centre_far, k), vel, radii));
  for (int t = 0; t < T; ++t) {
    MatrixXd v3;
    const MatrixXd o3 = scene3(centre_far, t, v3);
    factors[S0 + t]->set_device_psi(DevicePsi::hinge_balls3d(sigma, eps, radius, W3, c3, {0.0}, o3, v3, radii));
  }
  opt.update_device_psi_params();
  fc = opt.factor_cost_vector();
  double left = 0.0;
  for (int i = U0; i < S0 + T; ++i) left += std::fabs(fc(i));
  expect(left == 0.0, "with the ball away every ball factor costs exactly 0");
  bool threw = false;
  try { factors[U0]->set_device_psi(DevicePsi::hinge_balls2d(sigma, eps, radius, W, c, taus, centre0, vel, radii)); } catch (const std::invalid_argument&) { threw = true; }
  expect(threw, "another block size is refused by the factor");
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
