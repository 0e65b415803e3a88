// MinimumAccGP::interpolation and GVIGH::set_interpolation / interpolate / sample_interpolated on the shim: the posterior
// between the support states.
//   interp_callsite host [file]  no device call: the interpolation operators' own identities, the error statuses that need no
//                                device, and -- with a file "nd qc dt count" followed by count records "tau A B Qt" (row-major)
//                                -- the operators against those numbers (tests/test_interp_host.py writes the Python helper's)
//   interp_callsite gpu          optimises two iterations on the device, then checks that the resident and the FactorWise
//                                paths give the same interpolated moments and samples, and that a query at a support time
//                                returns that state's mean
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

static double max_abs(const MatrixXd& M) {
  double m = 0.0;
  for (int i = 0; i < M.rows(); ++i) for (int j = 0; j < M.cols(); ++j) m = std::fmax(m, std::fabs(M(i, j)));
  return m;
}

static bool same(const MatrixXd& X, const MatrixXd& Y) {
  if (X.rows() != Y.rows() || X.cols() != Y.cols()) return false;
  for (int i = 0; i < X.rows(); ++i) for (int j = 0; j < X.cols(); ++j) if (!(X(i, j) == Y(i, j))) return false;
  return true;
}

static MatrixXd read_matrix(std::FILE* f, int n) {
  MatrixXd M(n, n);
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) if (std::fscanf(f, "%lf", &M(i, j)) != 1) ++fails;
  return M;
}

static int host_checks(const char* path) {
  // the operators' own identities: a constant-velocity motion is reproduced, the end points are exact
  const int nd = 2, n = 2 * nd;
  const double dt = 0.37, qc = 0.8;
  MinimumAccGP gp(MatrixXd::Identity(nd, nd) * qc, 0, dt, VectorXd::Zero(n));
  MatrixXd A, B, Qt;
  gp.interpolation(0.0, A, B, Qt);
  expect(same(A, MatrixXd::Identity(n, n)) && same(B, MatrixXd::Zero(n, n)) && same(Qt, MatrixXd::Zero(n, n)), "tau = 0 is (I, 0, 0)");
  gp.interpolation(dt, A, B, Qt);
  expect(same(A, MatrixXd::Zero(n, n)) && same(B, MatrixXd::Identity(n, n)) && same(Qt, MatrixXd::Zero(n, n)), "tau = dt is (0, I, 0)");
  const double tau = 0.3 * dt;
  gp.interpolation(tau, A, B, Qt);
  VectorXd x0(n), x1(n), xt(n);
  for (int i = 0; i < nd; ++i) {
    const double p = 0.5 + i, v = 1.0 - 0.7 * i;
    x0(i) = p; x0(nd + i) = v;
    x1(i) = p + dt * v; x1(nd + i) = v;
    xt(i) = p + tau * v; xt(nd + i) = v;
  }
  const VectorXd got = A * x0 + B * x1;
  for (int i = 0; i < n; ++i) expect(std::fabs(got(i) - xt(i)) <= 1e-12, "constant-velocity motion is reproduced");
  expect(max_abs(Qt - Qt.transpose()) == 0.0, "Qt symmetric");
  for (int i = 0; i < n; ++i) expect(Qt(i, i) > 0.0, "Qt has a positive diagonal inside the interval");
  bool threw = false;
  try { gp.interpolation(1.5 * dt, A, B, Qt); } catch (const std::invalid_argument&) { threw = true; }
  expect(threw, "tau outside [0, dt] throws");

  // statuses that need no device: a NULL context is GVI_ERR_ARG at every entry point
  int Q = 0, nbad = 0;
  double x = 0.0;
  const int32_t idx = 0;
  expect(gvi_interp_set(nullptr, 1, &idx, &x, &x, nullptr, nullptr) == GVI_ERR_ARG, "interp_set(NULL)");
  expect(gvi_interp_info(nullptr, &Q, &nbad) == GVI_ERR_ARG, "interp_info(NULL)");
  expect(gvi_bt_interp(nullptr, &x, &x, &x, &x, &x) == GVI_ERR_ARG, "bt_interp(NULL)");
  expect(gvi_ngd_interp(nullptr, &x, &x) == GVI_ERR_ARG, "ngd_interp(NULL)");
  expect(gvi_ngd_interp_dev(nullptr, &x, &x) == GVI_ERR_ARG, "ngd_interp_dev(NULL)");
  expect(gvi_bt_interp_samples(nullptr, 1, &x, 0, 0, nullptr, &x) == GVI_ERR_ARG, "bt_interp_samples(NULL)");
  expect(gvi_ngd_sample_interp(nullptr, 1, 0, 0, 0, nullptr, &x) == GVI_ERR_ARG, "ngd_sample_interp(NULL)");
  expect(gvi_ngd_sample_interp_dev(nullptr, 1, 0, 0, 0, nullptr, &x) == GVI_ERR_ARG, "ngd_sample_interp_dev(NULL)");

  if (path) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 1; }
    int fnd = 0, count = 0;
    double fqc = 0, fdt = 0;
    if (std::fscanf(f, "%d %lf %lf %d", &fnd, &fqc, &fdt, &count) != 4) ++fails;
    const int fn = 2 * fnd;
    MinimumAccGP g2(MatrixXd::Identity(fnd, fnd) * fqc, 0, fdt, VectorXd::Zero(fn));
    for (int r = 0; r < count && !fails; ++r) {
      double t = 0;
      if (std::fscanf(f, "%lf", &t) != 1) ++fails;
      const MatrixXd Ar = read_matrix(f, fn), Br = read_matrix(f, fn), Qr = read_matrix(f, fn);
      g2.interpolation(t, A, B, Qt);
      expect(max_abs(A - Ar) <= 1e-13 * std::fmax(1.0, max_abs(Ar)), "A matches the Python helper");
      expect(max_abs(B - Br) <= 1e-13 * std::fmax(1.0, max_abs(Br)), "B matches the Python helper");
      expect(max_abs(Qt - Qr) <= 1e-13 * max_abs(Qr), "Qt matches the Python helper");
    }
    expect(count > 0, "records in the file");
    std::fclose(f);
  }
  return fails;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s host [file] | gpu\n", argv[0]); return 2; }
  if (std::strcmp(argv[1], "gpu") != 0) {
    if (host_checks(argc > 2 ? argv[2] : nullptr)) return 1;
    std::printf("ok\n");
    return 0;
  }

  const int T = 9, nd = 1, n = 2, K = T - 1, p = 3, S = 3;
  const double dt = 0.25, qc = 0.8;
  MinimumAccGP gp(MatrixXd::Identity(nd, nd) * qc, 0, dt, VectorXd::Zero(n));
  MatrixXd Kinv = MatrixXd::Identity(n, n) * 50.0;
  using Factor = NGDFactorizedBaseGH<NoneType>;
  auto none = [](const VectorXd&, const NoneType&) { return 0.0; };
  VectorXd init_mu(T * n);
  for (int t = 0; t < T; ++t) { init_mu(t * n) = 0.2 * t; init_mu(t * n + 1) = 0.2; }
  SpMat init_prec(T * n, T * n);
  for (int i = 0; i < T * n; ++i) init_prec.coeffRef(i, i) = 20.0;
  for (int i = 0; i + n < T * n; ++i) init_prec.coeffRef(i, i + n) = init_prec.coeffRef(i + n, i) = -4.0;
  std::vector<std::shared_ptr<Factor>> factors;
  for (int k = 0; k < K; ++k)
    factors.emplace_back(new Factor(2 * n, n, p, none, NoneType{}, T, k, 1.0, 10.0, gp.device_psi()));
  for (int e = 0; e < 2; ++e) {
    const int t = e ? T - 1 : 0;
    VectorXd m0(n);
    for (int i = 0; i < n; ++i) m0(i) = init_mu(t * n + i);
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::FixedPrior(m0, Kinv)));
  }
  NGDGH<Factor> opt{factors, n, T, 2};
  opt.set_initial_values(init_mu, init_prec);
  opt.optimize(false);

  // queries: unsorted, the first at a support time
  const std::vector<int> states{3, 7, 0, 3};
  const std::vector<double> taus{0.0, 0.5 * dt, 0.25 * dt, 0.9 * dt};
  std::vector<MatrixXd> A(4), B(4), Qt(4);
  for (int q = 0; q < 4; ++q) gp.interpolation(taus[q], A[q], B[q], Qt[q]);
  opt.set_interpolation(states, A, B, {}, Qt);
  MatrixXd m, c, mf, cf;
  opt.interpolate(m, c);
  const MatrixXd Xq = opt.sample_interpolated(S, 5, 6);
  const VectorXd mu = opt.mean();
  opt.set_execution(Execution::FactorWise);
  opt.interpolate(mf, cf);
  const MatrixXd Xqf = opt.sample_interpolated(S, 5, 6);
  expect(m.rows() == n && m.cols() == 4 && c.rows() == n && c.cols() == 4 * n, "shapes of interpolate");
  expect(Xq.rows() == 4 * n && Xq.cols() == S, "shape of sample_interpolated");
  expect(same(m, mf) && same(c, cf), "resident and FactorWise moments agree bit for bit");
  expect(same(Xq, Xqf), "resident and FactorWise samples agree bit for bit");
  for (int i = 0; i < n; ++i) expect(m(i, 0) == mu(3 * n + i), "a query at a support time returns that state's mean");
  for (int i = 0; i < Xq.rows(); ++i) for (int j = 0; j < S; ++j) expect(std::isfinite(Xq(i, j)), "finite samples");
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
