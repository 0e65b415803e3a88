// The three kernels of gaussianvi_amd/csrc/kernels_interp.hpp compiled for the CPU (tests/stubs/hip_on_cpu: one std::thread per
// lane, barriers for __syncthreads / __shfl, one workgroup at a time) against a plain reference: prepare (Cholesky rule, packing,
// bad flag), moments, and the sweep with ragged tiles in both directions, a zero Qt, a bad query, caller-supplied eps and
// Qt = NULL.  Built with AddressSanitizer and UBSan by tests/test_interp_host.py, so an index outside a buffer is an error here
// and not on a device.  Prints "ALL OK".
#include <cstdio>
#include <random>
#include "kernels_interp.hpp"
using namespace gvi;
static int interp_tile(int S, int Q, int n) {
  const int64_t qblocks = ((int64_t)Q + INTERP_SWEEP_WAVES * (64 / n) - 1) / (INTERP_SWEEP_WAVES * (64 / n));
  int tile = 1;
  while (tile < INTERP_TILE_MAX && qblocks * ((S + 2 * tile - 1) / (2 * tile)) >= INTERP_TARGET_BLOCKS) tile *= 2;
  return tile;
}
int run(int T, int n, int Q, int S, bool noise, bool useeps, int force_tile) {
  std::mt19937_64 g(T * 100 + n);
  std::normal_distribution<double> N;
  const int nn = n * n;
  std::vector<double> A(Q * nn), B(Q * nn), c(Q * n), Qt(Q * nn), mu(T * n), SD(T * nn), SU((T - 1) * nn), X((size_t)S * T * n), eps((size_t)S * Q * n);
  std::vector<int32_t> idx(Q), bad(Q);
  for (auto& v : A) v = N(g); for (auto& v : B) v = N(g); for (auto& v : c) v = N(g); for (auto& v : mu) v = N(g);
  for (auto& v : SD) v = N(g); for (auto& v : SU) v = N(g); for (auto& v : X) v = N(g); for (auto& v : eps) v = N(g);
  for (int q = 0; q < Q; ++q) {
    idx[q] = (int)(g() % (T - 1));
    std::vector<double> W(nn);
    for (auto& v : W) v = N(g);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { double s = i == j ? 0.5 : 0.0; for (int k = 0; k < n; ++k) s += W[i * n + k] * W[j * n + k] / n; Qt[q * nn + i * n + j] = s; }
  }
  if (Q > 2) { for (int e = 0; e < nn; ++e) Qt[1 * nn + e] = 0.0; Qt[2 * nn + 0] = -1.0; }   // a zero Qt, a bad one
  const int st = 3 * n + 1;
  std::vector<double> ops((size_t)Q * n * st), mean(Q * n), cov(Q * nn), Xq((size_t)S * Q * n, -777.0);
  InterpPrepArgs pa{Q, n, A.data(), B.data(), c.data(), noise ? Qt.data() : nullptr, ops.data(), bad.data()};
  launch(interp_prepare_kernel, Q, 1, 64, pa);
  int fails = 0;
  // check L
  for (int q = 0; q < Q && noise; ++q) {
    if (Q > 2 && q == 2) { if (!bad[q]) { printf("bad flag missing\n"); ++fails; } continue; }
    if (bad[q]) { printf("unexpected bad %d\n", q); ++fails; }
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) {
      double s = 0; for (int k = 0; k < n; ++k) s += ops[((size_t)q * n + i) * st + 2 * n + k] * ops[((size_t)q * n + j) * st + 2 * n + k];
      if (std::fabs(s - Qt[q * nn + i * n + j]) > 1e-12) { printf("LLt q %d %d %d: %g vs %g\n", q, i, j, s, Qt[q * nn + i * n + j]); ++fails; }
      if (j > i && ops[((size_t)q * n + i) * st + 2 * n + j] != 0.0) { printf("upper nonzero\n"); ++fails; }
    }
  }
  InterpMomArgs ma{Q, n, idx.data(), ops.data(), noise ? Qt.data() : nullptr, mu.data(), SD.data(), SU.data(), mean.data(), cov.data()};
  launch(interp_moments_kernel, Q, 1, 64, ma);
  for (int q = 0; q < Q; ++q) {
    const int i = idx[q];
    const double *a = &A[q * nn], *b = &B[q * nn], *sii = &SD[i * nn], *su = &SU[i * nn], *sjj = &SD[(i + 1) * nn];
    for (int r = 0; r < n; ++r) {
      double m = c[q * n + r];
      for (int k = 0; k < n; ++k) m += a[r * n + k] * mu[i * n + k] + b[r * n + k] * mu[(i + 1) * n + k];
      if (std::fabs(m - mean[q * n + r]) > 1e-11) { printf("mean q %d r %d\n", q, r); ++fails; }
      for (int cc = 0; cc < n; ++cc) {
        double v = noise ? Qt[q * nn + r * n + cc] : 0.0;
        for (int k = 0; k < n; ++k) for (int l = 0; l < n; ++l)
          v += a[r * n + k] * sii[k * n + l] * a[cc * n + l] + a[r * n + k] * su[k * n + l] * b[cc * n + l] + b[r * n + k] * su[l * n + k] * a[cc * n + l] +
               b[r * n + k] * sjj[k * n + l] * b[cc * n + l];
        if (std::fabs(v - cov[q * nn + r * n + cc]) > 1e-10 * (1 + std::fabs(v))) { printf("cov q %d %d %d: %g vs %g\n", q, r, cc, v, cov[q * nn + r * n + cc]); ++fails; }
      }
    }
  }
  InterpSweepArgs sa{};
  sa.T = T; sa.n = n; sa.Q = Q; sa.S = S; sa.tile = force_tile ? force_tile : interp_tile(S, Q, n); sa.noise = noise; sa.noise_seed = 77; sa.first = 3;
  sa.idx = idx.data(); sa.ops = ops.data(); sa.bad = bad.data(); sa.eps = useeps ? eps.data() : nullptr; sa.X = X.data(); sa.Xq = Xq.data();
  const int qpb = INTERP_SWEEP_WAVES * (64 / n);
  const unsigned gx = (Q + qpb - 1) / qpb, gy = (S + sa.tile - 1) / sa.tile;
  if (n <= 4) launch(interp_sweep_kernel<4>, gx, gy, 256, sa);
  else if (n <= 8) launch(interp_sweep_kernel<8>, gx, gy, 256, sa);
  else launch(interp_sweep_kernel<16>, gx, gy, 256, sa);
  for (int j = 0; j < S; ++j) for (int q = 0; q < Q; ++q) for (int r = 0; r < n; ++r) {
    const int i = idx[q];
    double v = c[q * n + r];
    for (int k = 0; k < n; ++k) v += A[q * nn + r * n + k] * X[((size_t)j * T + i) * n + k] + B[q * nn + r * n + k] * X[((size_t)j * T + i + 1) * n + k];
    if (noise) for (int k = 0; k < n; ++k) {
      double z;
      if (useeps) z = eps[((size_t)j * Q + q) * n + k];
      else { const uint64_t num = (uint64_t)(3 + j) * Q * n + (uint64_t)q * n + k; double z0, z1; randn_pair(77, num >> 1, z0, z1); z = (num & 1) ? z1 : z0; }
      v += ops[((size_t)q * n + r) * st + 2 * n + k] * z;
    }
    const double got = Xq[((size_t)j * Q + q) * n + r];
    if (noise && bad[q]) { if (got == got) { printf("bad query not NaN\n"); ++fails; } continue; }
    if (!(std::fabs(got - v) <= 1e-11 * (1 + std::fabs(v)))) { if (fails < 10) printf("Xq j %d q %d r %d: %g vs %g\n", j, q, r, got, v); ++fails; }
  }
  printf("T %d n %d Q %d S %d noise %d eps %d tile %d grid %u x %u: %d failures\n", T, n, Q, S, noise, useeps, sa.tile, gx, gy, fails);
  return fails;
}
int main() {
  int f = 0;
  f += run(2, 1, 4, 3, true, false, 0);
  f += run(2, 16, 5, 2, true, false, 0);
  f += run(3, 2, 7, 3, true, true, 0);
  f += run(7, 4, 19, 5, true, false, 2);
  f += run(9, 9, 30, 3, true, false, 0);
  f += run(5, 6, 41, 5, true, false, 4);
  f += run(5, 6, 41, 3, false, false, 2);
  f += run(4, 14, 10, 3, true, false, 0);
  printf(f ? "FAILED\n" : "ALL OK\n");
  return f != 0;
}
