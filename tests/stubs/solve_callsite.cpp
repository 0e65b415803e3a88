// GVIGH::solve / covariance_columns / cross_covariance on the shim: precision()^-1 applied to a block of right-hand sides, and
// block columns of the joint covariance beyond its tridiagonal pattern.
//   solve_callsite host   compiles and builds the problem (CPU suite: no device call)
//   solve_callsite gpu    optimises two iterations on the device, then prints the state (D, U), the right-hand sides B, the
//                         states asked for, and solve(B), covariance_columns(states), cross_covariance(i, j) of the resident
//                         path, followed by the first two of the FactorWise path (%.17g)
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "gvi/gvi_host.hpp"

using namespace gvi;

static void print_matrix(const char* name, const MatrixXd& M) {   // column by column: one right-hand side after the other
  std::printf("\n%s", name);
  for (int j = 0; j < M.cols(); ++j)
    for (int i = 0; i < M.rows(); ++i) std::printf(" %.17g", M(i, j));
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s host|gpu\n", argv[0]); return 2; }
  const bool gpu = std::strcmp(argv[1], "gpu") == 0;
  const int T = 9, n = 2, K = T - 1, p = 3, R = 3, ci = 7, cj = 1;
  const std::vector<int> states{8, 0, 4, 0};
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
  MatrixXd B(T * n, R);
  for (int j = 0; j < R; ++j)
    for (int i = 0; i < T * n; ++i) B(i, j) = 0.25 * ((i * 7 + j * 3) % 11) - 1.0;
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
  const MatrixXd X = opt.solve(B);
  const MatrixXd Cc = opt.covariance_columns(states);
  const MatrixXd Cij = opt.cross_covariance(ci, cj);
  opt.set_execution(Execution::FactorWise);
  const MatrixXd Xf = opt.solve(B);
  const MatrixXd Ccf = opt.covariance_columns(states);
  const int nc = (int)states.size();
  if (X.rows() != T * n || X.cols() != R || Xf.rows() != T * n || Xf.cols() != R) return 1;
  if (Cc.rows() != T * n || Cc.cols() != nc * n || Ccf.rows() != T * n || Ccf.cols() != nc * n) return 1;
  if (Cij.rows() != n || Cij.cols() != n) return 1;

  const SpMat P = opt.precision();
  std::printf("T %d n %d R %d i %d j %d\n", T, n, R, ci, cj);
  std::printf("states");
  for (int s : states) std::printf(" %d", s);
  std::printf("\nD");
  for (int t = 0; t < T; ++t)
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) std::printf(" %.17g", P.coeff(t * n + r, t * n + c));
  std::printf("\nU");
  for (int t = 0; t + 1 < T; ++t)
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) std::printf(" %.17g", P.coeff(t * n + r, (t + 1) * n + c));
  print_matrix("B", B);
  print_matrix("X", X);
  print_matrix("Xf", Xf);
  print_matrix("C", Cc);
  print_matrix("Cf", Ccf);
  print_matrix("Cij", Cij);
  std::printf("\n");
  return 0;
}
