// Half-space factors (GVI_PSI_HINGE_HALFSPACE) on the shim: DevicePsi::hinge_halfspace used with NGDFactorizedBaseGH exactly as
// the other device descriptors are.
//   halfspace_callsite host   no device call: the parameter block, the grouping rule, every refused argument
//   halfspace_callsite gpu    a small planar graph (priors, anchors, a corridor of four faces per state that the start
//                             trajectory leaves on one side): the corridor factors cost something at the start, the iterations
//                             run on the device and bring the path back towards the corridor, and sample_clearance returns the
//                             distance to the faces
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
static bool refused(const MatrixXd& A, const VectorXd& b, const VectorXd& sigma, const VectorXd& eps) {
  try { (void)DevicePsi::hinge_halfspace(A, b, sigma, eps); } catch (const std::invalid_argument&) { return true; }
  return false;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s host | gpu\n", argv[0]); return 2; }
  const int T = 5, nd = 2, n = 4, K = T - 1, p = 3, J = 4;
  const double dt = 0.5, qc = 0.8, inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  // the corridor |y| <= 0.25, |x| <= 3 on the position of a state [x, y, vx, vy]; the start trajectory runs at y = 0.4
  MatrixXd A(J, n);
  VectorXd b(J), sigma(J), eps(J);
  A(0, 1) = 1.0; A(1, 1) = -1.0; A(2, 0) = 1.0; A(3, 0) = -1.0;
  b(0) = 0.25; b(1) = 0.25; b(2) = 3.0; b(3) = 3.0;
  for (int j = 0; j < J; ++j) { sigma(j) = 20.0; eps(j) = 0.05; }

  if (std::strcmp(argv[1], "gpu") != 0) {
    const DevicePsi h = DevicePsi::hinge_halfspace(A, b, sigma, eps);
    expect(h.kind == GVI_PSI_HINGE_HALFSPACE && (int)h.params.size() == J * (n + 3), "parameter block of J (d + 3)");
    expect(h.params[0] == 20.0 && h.params[J] == 0.05 && h.params[2 * J] == 0.25 && h.params[2 * J + 2] == 3.0 &&
           h.params[3 * J + 1] == 1.0 && h.params[3 * J + n + 1] == -1.0 && h.params[3 * J + 2 * n] == 1.0, "block layout [sigma | eps | b | A]");
    expect(!h.sdf2d && !h.sdf3d && !h.arm, "needs no field and no arm");
    expect(h.same_group(DevicePsi::hinge_halfspace(A, b, sigma, eps)), "half-space factors of one J share a set");
    MatrixXd A2(2, n);
    VectorXd two(2);
    A2(0, 0) = 1.0; A2(1, 1) = 1.0; two(0) = 1.0; two(1) = 1.0;
    expect(!refused(A2, two, two, two) && !h.same_group(DevicePsi::hinge_halfspace(A2, two, two, two)), "another J: another set");
    VectorXd shorter(J - 1);
    for (int j = 0; j < J - 1; ++j) shorter(j) = 1.0;
    expect(refused(A, shorter, sigma, eps) && refused(A, b, shorter, eps) && refused(A, b, sigma, shorter), "sizes");
    expect(refused(MatrixXd(0, n), VectorXd(0), VectorXd(0), VectorXd(0)), "J = 0");
    {
      const int big = (int)GVI_HALFSPACE_MAX_J + 1;
      MatrixXd Ab(big, n);
      VectorXd vb(big);
      for (int j = 0; j < big; ++j) { Ab(j, 0) = 1.0; vb(j) = 1.0; }
      expect(refused(Ab, vb, vb, vb), "J = 17");
      MatrixXd Ac((int)GVI_HALFSPACE_MAX_J, n);
      VectorXd vc((int)GVI_HALFSPACE_MAX_J);
      for (int j = 0; j < (int)GVI_HALFSPACE_MAX_J; ++j) { Ac(j, 0) = 1.0; vc(j) = 1.0; }
      expect(!refused(Ac, vc, vc, vc), "J = 16 is legal");
    }
    VectorXd v;
    v = sigma; v(1) = -1.0; expect(refused(A, b, v, eps), "sigma < 0");
    v = sigma; v(1) = inf; expect(refused(A, b, v, eps), "sigma = inf");
    v = sigma; v(1) = nan; expect(refused(A, b, v, eps), "sigma = NaN");
    v = eps; v(0) = inf; expect(refused(A, b, sigma, v), "eps = inf");
    v = eps; v(0) = nan; expect(refused(A, b, sigma, v), "eps = NaN");
    v = b; v(2) = -inf; expect(refused(A, v, sigma, eps), "b = -inf");
    v = b; v(2) = nan; expect(refused(A, v, sigma, eps), "b = NaN");
    MatrixXd M = A;
    M(3, 2) = nan; expect(refused(M, b, sigma, eps), "NaN in A");
    M = A; M(3, 2) = inf; expect(refused(M, b, sigma, eps), "inf in A");
    M = A; M(3, 0) = 0.0; expect(refused(M, b, sigma, eps), "all-zero normal on an active row");
    v = sigma; v(3) = 0.0; expect(!refused(M, b, v, eps), "all-zero normal on a row that is off is legal");
    v = eps; v(0) = -0.1; expect(!refused(A, b, sigma, v), "eps < 0 is legal");
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
    init_mu(t * n) = -1.0 + 0.5 * t; init_mu(t * n + 1) = 0.4; init_mu(t * n + 2) = 1.0; init_mu(t * n + 3) = 0.0;
  }
  SpMat init_prec(T * n, T * n);
  for (int i = 0; i < T * n; ++i) init_prec.coeffRef(i, i) = 300.0;
  for (int i = 0; i + n < T * n; ++i) init_prec.coeffRef(i, i + n) = init_prec.coeffRef(i + n, i) = -60.0;
  std::vector<std::shared_ptr<Factor>> factors;
  for (int k = 0; k < K; ++k)
    factors.emplace_back(new Factor(2 * n, n, p, none, NoneType{}, T, k, 1.0, 10.0, gp.device_psi()));
  for (int t = 0; t < T; ++t)
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::hinge_halfspace(A, b, sigma, eps)));
  // weak anchors on the end states: the corridor can pull them
  VectorXd m0[2] = {VectorXd(n), VectorXd(n)};
  for (int e = 0; e < 2; ++e) {
    const int t = e ? T - 1 : 0;
    for (int i = 0; i < n; ++i) m0[e](i) = init_mu(t * n + i);
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::FixedPrior(m0[e], Kinv * 0.01)));
  }
  NGDGH<Factor> opt{factors, n, T, 2};
  opt.set_initial_values(init_mu, init_prec);
  const VectorXd fc = opt.factor_cost_vector();
  expect(fc.size() == (int)factors.size(), "one cost per factor");
  double c0 = 0.0;
  for (int t = 0; t < T; ++t) c0 += fc(K + t);
  expect(c0 > 0.0 && std::isfinite(c0), "the start trajectory is outside the corridor: the corridor factors cost something");
  opt.optimize(false);
  const VectorXd mean = opt.mean();
  bool fin = true;
  for (int i = 0; i < mean.size(); ++i) fin = fin && std::isfinite(mean(i));
  expect(fin, "finite iterate");
  expect(mean(2 * n + 1) < 0.4, "the middle state moved towards the corridor");
  const VectorXd margin = opt.sample_clearance(5, 3, 1);
  for (int j = 0; j < margin.size(); ++j) expect(std::isfinite(margin(j)) && margin(j) <= 0.25, "distance to the faces");
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
