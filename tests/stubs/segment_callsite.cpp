// Obstacle factors on the segment between two support states, on the shim: DevicePsi::hinge_sdf2d_segment /
// hinge_sdf3d_segment with the read-outs of MinimumAccGP::segment_readout, used with NGDFactorizedBaseGH at d = 2n exactly as
// the other device descriptors are.
//   segment_callsite host   no device call: the read-outs at the end points, the parameter block, the grouping rule
//   segment_callsite gpu    a small planar planning graph whose straight-line start passes an obstacle BETWEEN two support
//                           states: with unary obstacle factors only every support state is clear and their costs vanish, while
//                           the segment set sees the obstacle (positive cost); two iterations run on the device
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
  if (argc < 2) { std::fprintf(stderr, "usage: %s host | gpu\n", argv[0]); return 2; }
  const int T = 5, nd = 2, n = 4, K = T - 1, p = 3;
  const double dt = 0.5, qc = 0.8;
  MinimumAccGP gp(MatrixXd::Identity(nd, nd) * qc, 0, dt, VectorXd::Zero(n));
  // one disc of radius 0.1 at (0.25, 0): between the support states at x = 0 and x = 0.5 of the start trajectory
  auto sdf = std::make_shared<PlanarSDF>();
  sdf->origin_x = -2.0; sdf->origin_y = -1.0; sdf->cell_size = 0.05;
  sdf->field = MatrixXd(41, 81);
  for (int r = 0; r < 41; ++r)
    for (int c = 0; c < 81; ++c) sdf->field(r, c) = std::hypot(-2.0 + c * 0.05 - 0.25, -1.0 + r * 0.05) - 0.1;
  const double sigma = 15.5, eps = 0.05, radius = 0.05;
  std::vector<MatrixXd> W, W2;
  std::vector<VectorXd> c, c2;
  gp.segment_readout({dt / 4, dt / 2, 3 * dt / 4}, nd, W, c);
  gp.segment_readout({0.0, dt}, nd, W2, c2);

  if (std::strcmp(argv[1], "gpu") != 0) {
    expect(W.size() == 3 && c.size() == 3 && W[0].rows() == nd && W[0].cols() == 2 * n && c[0].size() == nd, "read-out shapes");
    bool ends = true;
    for (int r = 0; r < nd; ++r)
      for (int q = 0; q < 2 * n; ++q) {
        ends = ends && W2[0](r, q) == (q == r ? 1.0 : 0.0) && W2[1](r, q) == (q == n + r ? 1.0 : 0.0);
      }
    expect(ends, "read-outs at tau = 0 and tau = dt are [I 0 | 0] and [0 | I 0]");
    // the midpoint of a constant-velocity segment: (x_i + x_i+1) / 2 + dt / 8 (v_i - v_i+1)
    expect(std::fabs(W[1](0, 0) - 0.5) < 1e-14 && std::fabs(W[1](0, n) - 0.5) < 1e-14 && std::fabs(W[1](0, nd) - dt / 8) < 1e-14 &&
           std::fabs(W[1](0, n + nd) + dt / 8) < 1e-14, "midpoint read-out");
    const DevicePsi s3 = DevicePsi::hinge_sdf2d_segment(sdf, sigma, eps, radius, W, c);
    const DevicePsi s2 = DevicePsi::hinge_sdf2d_segment(sdf, sigma, eps, radius, W2, c2);
    expect(s3.kind == GVI_PSI_HINGE_SDF_2D_SEG && (int)s3.params.size() == 3 + 3 * nd * (2 * n + 1), "parameter block, J = 3");
    expect((int)s2.params.size() == 3 + 2 * nd * (2 * n + 1), "parameter block, J = 2");
    expect(s3.params[0] == sigma && s3.params[1] == eps && s3.params[2] == radius && s3.params[3] == W[0](0, 0), "block layout");
    expect(s3.same_group(s3) && !s3.same_group(s2), "sets with different J stay apart");
    auto field3 = std::make_shared<SignedDistanceField>();
    std::vector<MatrixXd> W3{MatrixXd::Zero(3, 12)};
    std::vector<VectorXd> c3{VectorXd::Zero(3)};
    expect(DevicePsi::hinge_sdf3d_segment(field3, sigma, eps, radius, W3, c3).kind == GVI_PSI_HINGE_SDF_3D_SEG, "3-D descriptor");
    bool threw = false;
    try { (void)DevicePsi::hinge_sdf2d_segment(sdf, sigma, eps, radius, W3, c3); } catch (const std::invalid_argument&) { threw = true; }
    expect(threw, "a 3-row read-out is refused by the 2-D descriptor");
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
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::HingeSdf2D(sigma, eps, radius, sdf)));
  for (int k = 0; k < K; ++k)
    factors.emplace_back(new Factor(2 * n, n, p, none, NoneType{}, T, k, 1.0, 10.0,
                                    DevicePsi::hinge_sdf2d_segment(sdf, sigma, eps, radius, W, c)));
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
  double unary = 0.0, seg = 0.0;
  for (int t = 0; t < T; ++t) unary += fc(K + t);
  for (int k = 0; k < K; ++k) seg += fc(K + T + k);
  expect(unary == 0.0, "every support state is clear of the obstacle");
  expect(seg > 0.0 && fc(K + T + 1) > 0.0, "the segment factor between states 1 and 2 sees it");
  opt.optimize(false);
  const VectorXd mean = opt.mean();
  bool fin = true;
  for (int i = 0; i < mean.size(); ++i) fin = fin && std::isfinite(mean(i));
  expect(fin, "finite iterate");
  // samples: the clearance of the segment set is the minimum over its check points
  const VectorXd clr = opt.sample_clearance(5, 3, 2);
  for (int j = 0; j < clr.size(); ++j) expect(std::isfinite(clr(j)), "finite clearance");
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
