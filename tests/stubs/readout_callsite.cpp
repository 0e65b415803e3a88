// The read-out-space rule on the shim: DevicePsi::set_readout_rule on a descriptor, NGDFactorizedBaseGH::set_readout_rule on a
// factor before it joins an optimizer, and the optimizer's set_readout_rule for the set that holds a factor.
//   readout_callsite host     no device call: the descriptor keeps the order, the grouping rule, the refusals
//   readout_callsite device   the planning graph of balls_callsite.cpp with its unary ball set on the rule at order 8: the ball
//                             factor at state 2 has a positive cost that differs from the sparse rule's; a step runs; with the rule
//                             switched off on the optimizer the sparse rule's cost returns, bit for bit
// Prints "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "gvi/gvi_host.hpp"

using namespace gvi;

static int fails = 0;
static void expect(bool ok, const char* what) {
  if (!ok) { std::fprintf(stderr, "FAILED: %s\n", what); ++fails; }
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s host | device\n", argv[0]); return 2; }
  const int T = 5, nd = 2, n = 4, K = T - 1, p = 3;
  const double dt = 0.5, qc = 0.8;
  MinimumAccGP gp(MatrixXd::Identity(nd, nd) * qc, 0, dt, VectorXd::Zero(n));
  const double sigma = 15.5, eps = 0.1, radius = 0.05;
  MatrixXd centre0(1, 2), vel(1, 2);
  centre0(0, 0) = 0.5; centre0(0, 1) = 1.52; vel(0, 0) = 0.0; vel(0, 1) = -1.5;
  VectorXd radii(1);
  radii(0) = 0.2;
  std::vector<MatrixXd> W1{MatrixXd::Zero(nd, n)}, W3{MatrixXd::Zero(3, n)};
  std::vector<VectorXd> c1{VectorXd::Zero(nd)}, c3{VectorXd::Zero(3)};
  for (int r = 0; r < nd; ++r) W1[0](r, r) = W3[0](r, r) = 1.0;
  auto scene = [&](int i) {
    MatrixXd o = centre0;
    for (int r = 0; r < 2; ++r) o(0, r) += i * dt * vel(0, r);
    return o;
  };

  if (std::strcmp(argv[1], "host") == 0) {
    DevicePsi u = DevicePsi::hinge_balls2d(sigma, eps, radius, W1, c1, {0.0}, centre0, vel, radii);
    expect(u.readout_order == 0, "off by default");
    const DevicePsi plain = u;
    expect(u.set_readout_rule(8).readout_order == 8 && u.kind == GVI_PSI_HINGE_BALLS_2D, "the descriptor keeps the order");
    expect(u.same_group(u) && !u.same_group(plain), "factors with and without the rule land in different sets");
    u.set_readout_rule(16);
    u.set_readout_rule(0);
    expect(u.same_group(plain), "order 0 is the sparse rule");
    DevicePsi t = DevicePsi::hinge_balls3d(sigma, eps, radius, W3, c3, {0.0}, MatrixXd::Zero(1, 3), MatrixXd::Zero(1, 3), radii);
    t.set_readout_rule(10);
    int threw = 0;
    try { t.set_readout_rule(11); } catch (const std::invalid_argument&) { ++threw; }
    try { u.set_readout_rule(17); } catch (const std::invalid_argument&) { ++threw; }
    try { u.set_readout_rule(1); } catch (const std::invalid_argument&) { ++threw; }
    try { DevicePsi::Range1D(1.0, 2.0, 3.0, 4.0, 5.0).set_readout_rule(4); } catch (const std::invalid_argument&) { ++threw; }
    try { DevicePsi::FixedPrior(VectorXd::Zero(n), MatrixXd::Identity(n, n)).set_readout_rule(4); } catch (const std::invalid_argument&) { ++threw; }
    expect(threw == 5 && t.readout_order == 10, "order 11 at P = 3, orders 17 and 1, and kinds without a linear read-out are refused");
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
  auto build = [&](int order) {
    std::vector<std::shared_ptr<Factor>> factors;
    for (int k = 0; k < K; ++k) factors.emplace_back(new Factor(2 * n, n, p, none, NoneType{}, T, k, 1.0, 10.0, gp.device_psi()));
    for (int t = 0; t < T; ++t) {
      factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::hinge_balls2d(sigma, eps, radius, W1, c1, {0.0}, scene(t), vel, radii)));
      if (order) factors.back()->set_readout_rule(order);          // before the factor joins the optimizer
    }
    for (int e = 0; e < 2; ++e) {
      const int t = e ? T - 1 : 0;
      VectorXd m0(n);
      for (int i = 0; i < n; ++i) m0(i) = init_mu(t * n + i);
      factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::FixedPrior(m0, Kinv)));
    }
    return factors;
  };
  const int U0 = K;
  auto sparse_factors = build(0);
  NGDGH<Factor> sparse{sparse_factors, n, T, 2};
  sparse.set_initial_values(init_mu, init_prec);
  const VectorXd fs = sparse.factor_cost_vector();
  auto factors = build(8);
  NGDGH<Factor> opt{factors, n, T, 2};
  opt.set_initial_values(init_mu, init_prec);
  const VectorXd fr = opt.factor_cost_vector();
  expect(fr(U0 + 2) > 0.0 && fs(U0 + 2) > 0.0 && fr(U0 + 2) != fs(U0 + 2), "the rule and the sparse rule both see the ball and give different numbers");
  for (int k = 0; k < K; ++k) expect(fr(k) == fs(k), "the prior set is untouched");
  opt.set_readout_rule(U0, 0);                                     // the whole set returns to its sparse rule
  const VectorXd fb = opt.factor_cost_vector();
  bool same = true;
  for (int i = 0; i < fb.size(); ++i) same = same && fb(i) == fs(i);
  expect(same, "order 0 on the optimizer gives the sparse rule's costs bit for bit");
  opt.set_readout_rule(U0 + 1, 8);
  bool threw = false;
  try { opt.set_readout_rule(0, 8); } catch (const std::exception&) { threw = true; }
  expect(threw, "a prior set refuses the rule");
  opt.optimize(false);
  const VectorXd mean = opt.mean();
  bool fin = true;
  for (int i = 0; i < mean.size(); ++i) fin = fin && std::isfinite(mean(i));
  expect(fin, "finite iterate");
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
