// Limit factors (GVI_PSI_HINGE_BOX) on the shim: DevicePsi::hinge_box used with NGDFactorizedBaseGH exactly as the other
// device descriptors are.
//   box_callsite host   no device call: the parameter block, the grouping rule, every refused argument
//   box_callsite gpu    a small planar graph (priors, anchors, speed limits below the speed of the start trajectory): the
//                       limit factors cost something at the start, two iterations run on the device and bring the mean
//                       speed down, and sample_clearance returns the margin to the limits
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
static bool refused(const VectorXd& sigma, const VectorXd& eps, const VectorXd& lo, const VectorXd& hi) {
  try { (void)DevicePsi::hinge_box(sigma, eps, lo, hi); } catch (const std::invalid_argument&) { return true; }
  return false;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s host | gpu\n", argv[0]); return 2; }
  const int T = 5, nd = 2, n = 4, K = T - 1, p = 3;
  const double dt = 0.5, qc = 0.8, inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  VectorXd sigma(n), eps(n), lo(n), hi(n);
  for (int i = 0; i < n; ++i) { sigma(i) = 20.0; eps(i) = 0.05; lo(i) = -inf; hi(i) = inf; }
  lo(2) = -0.8; hi(2) = 0.8; lo(3) = -0.3; hi(3) = 0.3;                 // the start trajectory moves at (1, 0)

  if (std::strcmp(argv[1], "gpu") != 0) {
    const DevicePsi b = DevicePsi::hinge_box(sigma, eps, lo, hi);
    expect(b.kind == GVI_PSI_HINGE_BOX && (int)b.params.size() == 4 * n, "parameter block of 4 d");
    expect(b.params[0] == 20.0 && b.params[n] == 0.05 && b.params[2 * n] == -inf && b.params[2 * n + 2] == -0.8 &&
           b.params[3 * n] == inf && b.params[3 * n + 3] == 0.3, "block layout [sigma | eps | lo | hi]");
    expect(!b.sdf2d && !b.sdf3d && !b.arm, "needs no field and no arm");
    expect(b.same_group(DevicePsi::hinge_box(sigma, eps, lo, hi)), "limit factors of one dimension share a set");
    VectorXd v = sigma;
    VectorXd shorter(n - 1);
    for (int i = 0; i < n - 1; ++i) shorter(i) = 1.0;
    expect(refused(shorter, eps, lo, hi) && refused(sigma, shorter, lo, hi) && refused(sigma, eps, shorter, hi) &&
           refused(sigma, eps, lo, shorter) && refused(VectorXd(0), VectorXd(0), VectorXd(0), VectorXd(0)), "sizes");
    v = sigma; v(1) = -1.0; expect(refused(v, eps, lo, hi), "sigma < 0");
    v = sigma; v(1) = inf; expect(refused(v, eps, lo, hi), "sigma = inf");
    v = sigma; v(1) = nan; expect(refused(v, eps, lo, hi), "sigma = NaN");
    v = eps; v(0) = inf; expect(refused(sigma, v, lo, hi), "eps = inf");
    v = eps; v(0) = nan; expect(refused(sigma, v, lo, hi), "eps = NaN");
    v = lo; v(2) = 0.8; expect(refused(sigma, eps, v, hi), "lo = hi");
    v = lo; v(2) = 2.0; expect(refused(sigma, eps, v, hi), "lo > hi");
    v = lo; v(0) = inf; expect(refused(sigma, eps, v, hi), "lo = +inf");
    v = lo; v(0) = nan; expect(refused(sigma, eps, v, hi), "lo = NaN");
    v = hi; v(0) = -inf; expect(refused(sigma, eps, lo, v), "hi = -inf");
    v = hi; v(3) = nan; expect(refused(sigma, eps, lo, v), "hi = NaN");
    v = sigma; v(0) = 0.0; expect(!refused(v, eps, lo, hi), "sigma = 0 is legal");
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
  }

  MinimumAccGP gp(MatrixXd::Identity(nd, nd) * qc, 0, dt, VectorXd::Zero(n));
  MatrixXd Kinv = MatrixXd::Identity(n, n) * 100.0;
  using Factor = NGDFactorizedBaseGH<NoneType>;
  auto none = [](const VectorXd&, const NoneType&) { return 0.0; };
  VectorXd init_mu(T * n);
  for (int t = 0; t < T; ++t) {
    init_mu(t * n) = -1.0 + 0.5 * t; init_mu(t * n + 1) = 0.0; init_mu(t * n + 2) = 1.0; init_mu(t * n + 3) = 0.0;
  }
  SpMat init_prec(T * n, T * n);
  for (int i = 0; i < T * n; ++i) init_prec.coeffRef(i, i) = 300.0;
  for (int i = 0; i + n < T * n; ++i) init_prec.coeffRef(i, i + n) = init_prec.coeffRef(i + n, i) = -60.0;
  std::vector<std::shared_ptr<Factor>> factors;
  for (int k = 0; k < K; ++k)
    factors.emplace_back(new Factor(2 * n, n, p, none, NoneType{}, T, k, 1.0, 10.0, gp.device_psi()));
  for (int t = 0; t < T; ++t)
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::hinge_box(sigma, eps, lo, hi)));
  // anchors on the positions of the end states only in effect: a weak weight on their velocities lets the limits act
  VectorXd m0[2] = {VectorXd(n), VectorXd(n)};
  for (int e = 0; e < 2; ++e) {
    const int t = e ? T - 1 : 0;
    for (int i = 0; i < n; ++i) m0[e](i) = init_mu(t * n + i);
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::FixedPrior(m0[e], Kinv)));
  }
  NGDGH<Factor> opt{factors, n, T, 2};
  opt.set_initial_values(init_mu, init_prec);
  const VectorXd fc = opt.factor_cost_vector();
  expect(fc.size() == (int)factors.size(), "one cost per factor");
  double box0 = 0.0;
  for (int t = 0; t < T; ++t) box0 += fc(K + t);
  expect(box0 > 0.0 && std::isfinite(box0), "the start trajectory is faster than the limit: the limit factors cost something");
  opt.optimize(false);
  const VectorXd mean = opt.mean();
  bool fin = true;
  for (int i = 0; i < mean.size(); ++i) fin = fin && std::isfinite(mean(i));
  expect(fin, "finite iterate");
  expect(mean(2 * n + 2) < 1.0, "the mean speed of the middle state came down");
  const VectorXd margin = opt.sample_clearance(5, 3, 1);
  for (int j = 0; j < margin.size(); ++j) expect(std::isfinite(margin(j)) && margin(j) <= 0.8, "margin to the limits");
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
