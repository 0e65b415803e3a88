// GVIGH::sample_costs / sample_clearance on the shim: cost, log q and obstacle clearance of sampled trajectories.
//   sample_cost_callsite host   no device call: a NULL context is GVI_ERR_ARG at every entry point
//   sample_cost_callsite gpu    a small planar planning graph (priors, hinge-on-SDF obstacle factors, anchors): two iterations
//                               on the device, then the resident and the FactorWise paths must give the same J, log q and
//                               minimum clearance bit for bit; J against psi evaluated on the host at the shim's own samples
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
  if (std::strcmp(argv[1], "gpu") != 0) {
    double x = 0.0;
    expect(gvi_sample_factor_costs(nullptr, 0, 1, &x, &x) == GVI_ERR_ARG, "sample_factor_costs(NULL)");
    expect(gvi_sample_clearance(nullptr, 0, 1, &x, &x) == GVI_ERR_ARG, "sample_clearance(NULL)");
    expect(gvi_sample_clearance_dev(nullptr, 0, 1, &x, &x) == GVI_ERR_ARG, "sample_clearance_dev(NULL)");
    expect(gvi_sample_costs(nullptr, 1, &x, &x) == GVI_ERR_ARG, "sample_costs(NULL)");
    expect(gvi_sample_costs_dev(nullptr, 1, &x, &x) == GVI_ERR_ARG, "sample_costs_dev(NULL)");
    expect(gvi_ngd_sample_costs(nullptr, 1, 0, 0, -1, nullptr, &x, nullptr, nullptr) == GVI_ERR_ARG, "ngd_sample_costs(NULL)");
    expect(gvi_ngd_sample_costs_dev(nullptr, 1, 0, 0, -1, nullptr, &x, nullptr, nullptr) == GVI_ERR_ARG, "ngd_sample_costs_dev(NULL)");
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
  }

  const int T = 7, nd = 2, n = 4, K = T - 1, p = 3, S = 9;
  const double dt = 0.25, qc = 0.8;
  MinimumAccGP gp(MatrixXd::Identity(nd, nd) * qc, 0, dt, VectorXd::Zero(n));
  // one disc of radius 0.8 at (0, 0.3) on a 0.1 grid
  auto sdf = std::make_shared<PlanarSDF>();
  sdf->origin_x = -3.0; sdf->origin_y = -2.0; sdf->cell_size = 0.1;
  sdf->field = MatrixXd(41, 61);
  for (int r = 0; r < 41; ++r)
    for (int c = 0; c < 61; ++c) sdf->field(r, c) = std::hypot(-3.0 + c * 0.1, -2.0 + r * 0.1 - 0.3) - 0.8;
  const double sigma = 15.5, eps = 0.5, radius = 0.3;
  MatrixXd Kinv = MatrixXd::Identity(n, n) * 100.0;
  using Factor = NGDFactorizedBaseGH<NoneType>;
  auto none = [](const VectorXd&, const NoneType&) { return 0.0; };
  VectorXd init_mu(T * n);
  for (int t = 0; t < T; ++t) {
    init_mu(t * n) = -1.5 + 0.5 * t; init_mu(t * n + 1) = -0.4 + 0.1 * t; init_mu(t * n + 2) = 2.0; init_mu(t * n + 3) = 0.4;
  }
  SpMat init_prec(T * n, T * n);
  for (int i = 0; i < T * n; ++i) init_prec.coeffRef(i, i) = 30.0;
  for (int i = 0; i + n < T * n; ++i) init_prec.coeffRef(i, i + n) = init_prec.coeffRef(i + n, i) = -6.0;
  std::vector<std::shared_ptr<Factor>> factors;
  for (int k = 0; k < K; ++k)
    factors.emplace_back(new Factor(2 * n, n, p, none, NoneType{}, T, k, 1.0, 10.0, gp.device_psi()));
  for (int t = 0; t < T; ++t)
    factors.emplace_back(new Factor(n, n, p + 1, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::HingeSdf2D(sigma, eps, radius, sdf)));
  VectorXd m0[2] = {VectorXd(n), VectorXd(n)};
  for (int e = 0; e < 2; ++e) {
    const int t = e ? T - 1 : 0;
    for (int i = 0; i < n; ++i) m0[e](i) = init_mu(t * n + i);
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::FixedPrior(m0[e], Kinv)));
  }
  NGDGH<Factor> opt{factors, n, T, 2};
  opt.set_initial_values(init_mu, init_prec);
  opt.optimize(false);

  const MatrixXd Jq = opt.sample_costs(S, 5);
  const VectorXd clr = opt.sample_clearance(S, 5, 1);
  const MatrixXd X = opt.sample(S, 5);
  const VectorXd lq = opt.log_density(X);
  opt.set_execution(Execution::FactorWise);
  const MatrixXd Jqf = opt.sample_costs(S, 5);
  const VectorXd clrf = opt.sample_clearance(S, 5, 1);
  expect(Jq.rows() == 2 && Jq.cols() == S && clr.size() == S, "shapes");
  bool threw = false;
  try { (void)opt.sample_clearance(S, 5, 0); } catch (const GviError&) { threw = true; }
  expect(threw, "clearance of the prior set throws");
  MatrixXd Phi, Qinv;
  {
    // the prior's blocks as the device holds them: psi = 1/2 (Phi x1 - x2)^T Qinv (Phi x1 - x2)
    Phi = MatrixXd::Identity(n, n); Qinv = MatrixXd::Zero(n, n);
    for (int i = 0; i < nd; ++i) {
      Phi(i, nd + i) = dt;
      Qinv(i, i) = 12.0 / (dt * dt * dt) / qc;
      Qinv(i, nd + i) = Qinv(nd + i, i) = -6.0 / (dt * dt) / qc;
      Qinv(nd + i, nd + i) = 4.0 / dt / qc;
    }
  }
  for (int j = 0; j < S; ++j) {
    expect(Jq(0, j) == Jqf(0, j) && Jq(1, j) == Jqf(1, j), "resident and FactorWise J / log q agree bit for bit");
    expect(clr(j) == clrf(j), "resident and FactorWise clearance agree bit for bit");
    expect(Jq(1, j) == lq(j), "log q is log_density of the same samples");
    // host restatement at the shim's own samples; the obstacle term from the nearest-disc distance is only approximate
    // on the grid, so it is bounded through the clearance instead: psi_obstacle = sigma hinge(eps - clearance_t)^2
    double prior = 0.0;
    for (int k = 0; k < K; ++k) {
      VectorXd r(n);
      for (int i = 0; i < n; ++i) {
        double s = -X((k + 1) * n + i, j);
        for (int c = 0; c < n; ++c) s += Phi(i, c) * X(k * n + c, j);
        r(i) = s;
      }
      for (int i = 0; i < n; ++i) for (int c = 0; c < n; ++c) prior += 0.5 * r(i) * Qinv(i, c) * r(c);
    }
    double anchor = 0.0;
    for (int e = 0; e < 2; ++e) {
      const int t = e ? T - 1 : 0;
      for (int i = 0; i < n; ++i) { const double d = X(t * n + i, j) - m0[e](i); anchor += 100.0 * d * d; }
    }
    const double worst = std::fmax(0.0, eps - clr(j));          // eps + r - sd at the closest state
    const double lo = prior + anchor + sigma * worst * worst, hi = prior + anchor + T * sigma * worst * worst;
    expect(Jq(0, j) >= lo * (1.0 - 1e-9) - 1e-9 && Jq(0, j) <= hi * (1.0 + 1e-9) + 1e-9, "J within the bounds the clearance implies");
    expect(std::isfinite(Jq(0, j)) && std::isfinite(clr(j)), "finite results");
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
