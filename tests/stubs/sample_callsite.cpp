// GVIGH::sample / GVIGH::log_density on the shim: samples of q = N(mean(), precision()^-1), one per column.
//   sample_callsite host   compiles and builds the problem (CPU suite: no device call)
//   sample_callsite gpu    optimises two iterations on the device, then prints the state (mean, D, U), the samples of the
//                          resident path, the samples of the FactorWise path and log q of the resident samples (%.17g)
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "gvi/gvi_host.hpp"

using namespace gvi;

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s host|gpu\n", argv[0]); return 2; }
  const bool gpu = std::strcmp(argv[1], "gpu") == 0;
  const int T = 9, n = 2, K = T - 1, p = 3, S = 5;
  const uint64_t seed = 20261016;
  MatrixXd Phi = MatrixXd::Identity(n, n), Qinv = MatrixXd::Identity(n, n) * 4.0;
  Phi(0, 1) = 0.1;
  MatrixXd Kinv = MatrixXd::Identity(n, n) * 50.0;
  using Factor = NGDFactorizedBaseGH<NoneType>;
  auto none = [](const VectorXd&, const NoneType&) { return 0.0; };
  VectorXd init_mu(T * n);
  for (int t = 0; t < T; ++t) { init_mu(t * n) = 0.2 * t; init_mu(t * n + 1) = 0.2; }
  SpMat init_prec(T * n, T * n);
  for (int i = 0; i < T * n; ++i) init_prec.coeffRef(i, i) = 20.0;
  for (int i = 0; i + n < T * n; ++i) init_prec.coeffRef(i, i + n) = init_prec.coeffRef(i + n, i) = -4.0;
  if (!gpu) { std::printf("ok\n"); return 0; }

  std::vector<std::shared_ptr<Factor>> factors;
  for (int k = 0; k < K; ++k)
    factors.emplace_back(new Factor(2 * n, n, p, none, NoneType{}, T, k, 1.0, 10.0, DevicePsi::QuadPrior(Phi, Qinv)));
  for (int e = 0; e < 2; ++e) {
    const int t = e ? T - 1 : 0;
    VectorXd m0(n);
    for (int i = 0; i < n; ++i) m0(i) = init_mu(t * n + i);
    factors.emplace_back(new Factor(n, n, p, none, NoneType{}, T, t, 1.0, 10.0, DevicePsi::FixedPrior(m0, Kinv)));
  }
  NGDGH<Factor> opt{factors, n, T, 2};
  opt.set_initial_values(init_mu, init_prec);
  opt.optimize(false);
  const MatrixXd X = opt.sample(S, seed);
  const VectorXd logq = opt.log_density(X);
  opt.set_execution(Execution::FactorWise);
  const MatrixXd Xf = opt.sample(S, seed);
  if (X.rows() != T * n || X.cols() != S || Xf.rows() != T * n || Xf.cols() != S || logq.size() != S) return 1;

  const VectorXd mu = opt.mean();
  const SpMat P = opt.precision();
  std::printf("T %d n %d S %d seed %llu\n", T, n, S, (unsigned long long)seed);
  std::printf("mu");
  for (int i = 0; i < T * n; ++i) std::printf(" %.17g", mu(i));
  std::printf("\nD");
  for (int t = 0; t < T; ++t)
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) std::printf(" %.17g", P.coeff(t * n + r, t * n + c));
  std::printf("\nU");
  for (int t = 0; t + 1 < T; ++t)
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) std::printf(" %.17g", P.coeff(t * n + r, (t + 1) * n + c));
  for (int v = 0; v < 2; ++v) {
    const MatrixXd& M = v ? Xf : X;
    std::printf("\n%s", v ? "Xf" : "X");
    for (int j = 0; j < S; ++j)
      for (int i = 0; i < T * n; ++i) std::printf(" %.17g", M(i, j));
  }
  std::printf("\nlogq");
  for (int j = 0; j < S; ++j) std::printf(" %.17g", logq(j));
  std::printf("\n");
  return 0;
}
