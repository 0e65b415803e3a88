// Stand-alone check + timing of the chain kernels (kernels_chain.hpp) against a sequential host solver, both chain
// operations of an NGD iteration side by side:
//   factorisation of Lam (1/2 log det + tridiagonal blocks of the inverse)  ||  pivoted solve V x = -g
// Build:  hipcc --offload-arch=gfx950 -O3 -std=c++20 -I gaussianvi_amd/csrc tools/ubench/chain_bench.hip -o tools/ubench/chain_bench
// Run:    tools/ubench/chain_bench [T=1025] [n=6] [reps=200]        (ASM_LEG=0: without the assemble-on-load leg; CHAIN_PAIR=0:
//         the v_readlane eliminations in every leg but the chain_pair A/B)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "chain_launch.hpp"

using namespace gvi;

#define CK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e__)); exit(2); } } while (0)

// ---- host reference: sequential block LDL^T, solve, selected inverse ----
struct Mat { int n; std::vector<double> a; Mat(int n_ = 0) : n(n_), a((size_t)n_ * n_, 0.0) {} double& operator()(int r, int c) { return a[(size_t)r * n + c]; } double operator()(int r, int c) const { return a[(size_t)r * n + c]; } };
static Mat mul(const Mat& A, const Mat& B, bool tA = false, bool tB = false) {
  const int n = A.n; Mat C(n);
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { long double s = 0; for (int k = 0; k < n; ++k) s += (long double)(tA ? A(k, i) : A(i, k)) * (tB ? B(j, k) : B(k, j)); C(i, j) = (double)s; }
  return C;
}
static Mat inv(const Mat& A, double* logdet) {
  const int n = A.n; std::vector<long double> M((size_t)n * 2 * n, 0);
  for (int i = 0; i < n; ++i) { for (int j = 0; j < n; ++j) M[(size_t)i * 2 * n + j] = A(i, j); M[(size_t)i * 2 * n + n + i] = 1; }
  long double ld = 0;
  for (int p = 0; p < n; ++p) {
    int best = p; for (int r = p + 1; r < n; ++r) if (fabsl(M[(size_t)r * 2 * n + p]) > fabsl(M[(size_t)best * 2 * n + p])) best = r;
    if (best != p) for (int j = 0; j < 2 * n; ++j) std::swap(M[(size_t)p * 2 * n + j], M[(size_t)best * 2 * n + j]);
    const long double piv = M[(size_t)p * 2 * n + p]; ld += logl(fabsl(piv));
    for (int j = 0; j < 2 * n; ++j) M[(size_t)p * 2 * n + j] /= piv;
    for (int r = 0; r < n; ++r) if (r != p) { const long double f = M[(size_t)r * 2 * n + p]; for (int j = 0; j < 2 * n; ++j) M[(size_t)r * 2 * n + j] -= f * M[(size_t)p * 2 * n + j]; }
  }
  Mat R(n); for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) R(i, j) = (double)M[(size_t)i * 2 * n + n + j];
  if (logdet) *logdet = (double)ld;
  return R;
}
static Mat blk(const std::vector<double>& v, int t, int n) { Mat M(n); for (int i = 0; i < n * n; ++i) M.a[i] = v[(size_t)t * n * n + i]; return M; }

static void host_chain(int T, int n, const std::vector<double>& D, const std::vector<double>& U, const std::vector<double>& rhs, double scale,
                       std::vector<double>& SigD, std::vector<double>& SigU, std::vector<double>& x, double& hld) {
  const int nn = n * n;
  std::vector<Mat> Sinv(T, Mat(n));
  std::vector<std::vector<double>> y(T, std::vector<double>(n));
  double ld = 0, l;
  Mat S = blk(D, 0, n);
  for (int i = 0; i < n; ++i) y[0][i] = scale * rhs[i];
  for (int t = 0; t < T; ++t) {
    Sinv[t] = inv(S, &l); ld += l;
    if (t + 1 < T) {
      const Mat Ut = blk(U, t, n);
      const Mat W = mul(Sinv[t], Ut);            // S_t^-1 U_t
      const Mat C = mul(Ut, W, true, false);     // U_t^T S_t^-1 U_t
      S = blk(D, t + 1, n);
      for (int i = 0; i < nn; ++i) S.a[i] -= C.a[i];
      for (int i = 0; i < n; ++i) { long double s = scale * rhs[(size_t)(t + 1) * n + i]; for (int k = 0; k < n; ++k) { long double w = 0; for (int q = 0; q < n; ++q) w += (long double)Sinv[t](k, q) * y[t][q]; s -= (long double)Ut(k, i) * w; } y[t + 1][i] = (double)s; }
    }
  }
  hld = 0.5 * ld;
  x.assign((size_t)T * n, 0.0); SigD.assign((size_t)T * nn, 0.0); SigU.assign((size_t)std::max(0, T - 1) * nn, 0.0);
  for (int t = T - 1; t >= 0; --t) {
    std::vector<long double> r(n);
    for (int i = 0; i < n; ++i) r[i] = y[t][i];
    if (t + 1 < T) { const Mat Ut = blk(U, t, n); for (int i = 0; i < n; ++i) for (int k = 0; k < n; ++k) r[i] -= (long double)Ut(i, k) * x[(size_t)(t + 1) * n + k]; }
    for (int i = 0; i < n; ++i) { long double s = 0; for (int k = 0; k < n; ++k) s += (long double)Sinv[t](i, k) * r[k]; x[(size_t)t * n + i] = (double)s; }
    if (t == T - 1) { for (int i = 0; i < nn; ++i) SigD[(size_t)t * nn + i] = Sinv[t].a[i]; }
    else {
      const Mat Ut = blk(U, t, n), Sn = blk(SigD, t + 1, n);
      const Mat W = mul(Sinv[t], Ut);                       // S^-1 U
      const Mat WS = mul(W, Sn);                            // S^-1 U Sig_{t+1}
      for (int i = 0; i < nn; ++i) SigU[(size_t)t * nn + i] = -WS.a[i];
      const Mat Q = mul(WS, W, false, true);                // S^-1 U Sig U^T S^-1
      for (int i = 0; i < nn; ++i) SigD[(size_t)t * nn + i] = Sinv[t].a[i] + Q.a[i];
    }
  }
}

static double relerr(const std::vector<double>& a, const std::vector<double>& b) {
  double num = 0, den = 0;
  for (size_t i = 0; i < a.size(); ++i) { num = std::max(num, fabs(a[i] - b[i])); den = std::max(den, fabs(b[i])); }
  return num / (den > 0 ? den : 1);
}

// Assemble-on-load leg: what the factor pass leaves for the chain's first pass -- per-factor Vdmu / Vddmu of a binary set
// (K = T - 1, d = 2n) and a unary set (K = T, d = n) -- rewritten by a launch of its own in front of every chain call, so the
// first pass reads lines that other XCDs wrote a moment ago, as in the iteration.  Values: SPD-dominant blocks that depend
// on `salt` (a different matrix every call; the unary set carries the diagonal weight).
__global__ void asm_fill_kernel(double* Vdmu_b, double* Vddmu_b, double* Vdmu_u, double* Vddmu_u, int T, int n, unsigned salt) {
  const int d = 2 * n;
  const size_t nb = (size_t)(T - 1) * d * d, nu = (size_t)T * n * n, gb = (size_t)(T - 1) * d, gu = (size_t)T * n;
  const size_t total = nb + nu + gb + gu;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u + salt * 40503u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    const double v = (double)(h & 0xffff) / 65536.0 - 0.5;            // [-0.5, 0.5)
    if (i < nb) { const size_t e = i % ((size_t)d * d); const int r = (int)(e / d), c = (int)(e % d); Vddmu_b[i] = r == c ? 1.0 + 0.1 * v : 0.0; if (r != c) { const int lo = r < c ? r : c, hi = r < c ? c : r; unsigned g = (unsigned)((i / ((size_t)d * d)) * d * d + lo * d + hi) * 2654435761u + salt * 40503u; g ^= g >> 15; g *= 2246822519u; g ^= g >> 13; Vddmu_b[i] = 0.3 * ((double)(g & 0xffff) / 65536.0 - 0.5) / n; } }
    else if (i < nb + nu) { const size_t e = (i - nb) % ((size_t)n * n); const int r = (int)(e / n), c = (int)(e % n); Vddmu_u[i - nb] = r == c ? 3.0 + 0.1 * v : 0.0; }
    else if (i < nb + nu + gb) Vdmu_b[i - nb - nu] = v;
    else Vdmu_u[i - nb - nu - gb] = v;
  }
}

// the switches the legs below time (chain_plan.hpp); merge holds only where next_sync hands words out
static gvi::ChainRules g_rules{true, true, true, true};

// CHAIN_MERGE=1: the top pass and the first backward pass in one launch (chain_launch.hpp::ChainSync)
static unsigned* g_sync_words = nullptr;
static unsigned g_sync_seq = 0;
static gvi::ChainSync next_sync() {
  gvi::ChainSync sy;
  const char* e = getenv("CHAIN_MERGE");
  if (!e || atoi(e) == 0) return sy;
  if (!g_sync_words) { (void)hipMalloc(&g_sync_words, 64 * 2 * sizeof(unsigned)); (void)hipMemset(g_sync_words, 0, 64 * 2 * sizeof(unsigned)); }
  if (++g_sync_seq == 0) ++g_sync_seq;
  sy.seq = g_sync_seq;
  sy.words = g_sync_words + 2 * (sy.seq % 64);
  return sy;
}

static int run(int T, int n, int reps) {
  const int nn = n * n, NP = chain_padded(n);
  std::mt19937_64 rng(1234 + T + n);
  std::normal_distribution<double> nd(0.0, 1.0);
  // two chains: Lam (SPD, factorised) and V (SPD here too, solved with pivoting), diagonally dominant blocks
  auto make = [&](std::vector<double>& D, std::vector<double>& U) {
    D.assign((size_t)T * nn, 0.0); U.assign((size_t)std::max(0, T - 1) * nn, 0.0);
    for (int t = 0; t < T; ++t) {
      std::vector<double> B(nn);
      for (auto& v : B) v = nd(rng);
      for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { double s = 0; for (int k = 0; k < n; ++k) s += B[i * n + k] * B[j * n + k]; D[(size_t)t * nn + i * n + j] = s / n + (i == j ? 3.0 : 0.0); }
      if (t + 1 < T) for (int i = 0; i < nn; ++i) U[(size_t)t * nn + i] = 0.6 * nd(rng) / std::sqrt((double)n);
    }
  };
  std::vector<double> D0, U0, D1, U1, rhs((size_t)T * n);
  make(D0, U0); make(D1, U1);
  for (auto& v : rhs) v = nd(rng);
  std::vector<double> rSigD, rSigU, rx, dummyD, dummyU, dx;
  double rhld, dh;
  host_chain(T, n, D0, U0, rhs, 1.0, rSigD, rSigU, dx, rhld);
  host_chain(T, n, D1, U1, rhs, -1.0, dummyD, dummyU, rx, dh);

  const size_t btD = (size_t)T * nn, btU = (size_t)std::max(0, T - 1) * nn;
  double *dD0, *dD1, *drhs, *dSig, *dx_, *dhld, *ws0, *ws1;
  int *wi0, *wi1;
  CK(hipMalloc(&dD0, (btD + btU + 1) * 8)); CK(hipMalloc(&dD1, (btD + btU + 1) * 8)); CK(hipMalloc(&drhs, (size_t)T * n * 8));
  CK(hipMalloc(&dSig, (btD + btU + 1) * 8)); CK(hipMalloc(&dx_, (size_t)T * n * 8)); CK(hipMalloc(&dhld, 8));
  CK(hipMalloc(&ws0, chain_ws_doubles(T, NP) * 8)); CK(hipMalloc(&ws1, chain_ws_doubles(T, NP) * 8));
  CK(hipMalloc(&wi0, chain_lp_entries(T) * 4)); CK(hipMalloc(&wi1, chain_lp_entries(T) * 4));
  CK(hipMemcpy(dD0, D0.data(), btD * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(dD0 + btD, U0.data(), btU * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(dD1, D1.data(), btD * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(dD1 + btD, U1.data(), btU * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(drhs, rhs.data(), (size_t)T * n * 8, hipMemcpyHostToDevice));
  // poison the workspaces: nothing may depend on their initial contents
  CK(hipMemset(ws0, 0xff, chain_ws_doubles(T, NP) * 8)); CK(hipMemset(ws1, 0xff, chain_ws_doubles(T, NP) * 8));
  hipStream_t st;
  CK(hipStreamCreate(&st));

  ChainArgs a0{}, a1{};
  a0.T = T; a0.need_back = 1; a0.D = dD0; a0.U = dD0 + btD; a0.rhs = nullptr; a0.rhs_scale = 1.0; a0.ws = ws0; a0.wsi = wi0;
  a0.SigD = dSig; a0.SigU = dSig + btD; a0.x = nullptr; a0.hld = dhld; a0.mixV = nullptr; a0.mixOut = nullptr; a0.mix_step = 0; a0.pred = nullptr; a0.pred_val = 0;
  a1 = a0;
  a1.need_back = 0; a1.D = dD1; a1.U = dD1 + btD; a1.rhs = drhs; a1.rhs_scale = -1.0; a1.ws = ws1; a1.wsi = wi1; a1.SigD = nullptr; a1.SigU = nullptr; a1.x = dx_; a1.hld = nullptr;
  const ChainPasses pl = chain_passes(T, n);
  printf("T = %d, n = %d (kernels at N = %d): %d forward pass(es), %d threads\n", T, n, NP, pl.npass, pl.threads);

  auto check = [&](const char* name) {
    std::vector<double> SigD(btD), SigU(btU), x((size_t)T * n);
    double hld;
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(SigD.data(), dSig, btD * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(SigU.data(), dSig + btD, btU * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(x.data(), dx_, (size_t)T * n * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(&hld, dhld, 8, hipMemcpyDeviceToHost));
    const double e1 = relerr(SigD, rSigD), e2 = btU ? relerr(SigU, rSigU) : 0.0, e3 = relerr(x, rx), e4 = fabs(hld - rhld) / fabs(rhld);
    printf("%-6s errors vs host: SigD %.2e  SigU %.2e  x %.2e  half-logdet %.2e (%.12g)\n", name, e1, e2, e3, e4, hld);
    return (e1 < 1e-10 && e2 < 1e-10 && e3 < 1e-10 && e4 < 1e-12) ? 0 : 1;
  };
  auto clear_out = [&]() { CK(hipMemsetAsync(dSig, 0xff, (btD + btU) * 8, st)); CK(hipMemsetAsync(dx_, 0xff, (size_t)T * n * 8, st)); CK(hipMemsetAsync(dhld, 0xff, 8, st)); };

  int fail = 0;
  clear_out();
  CK(chain_launch(n, g_rules, a0, a1, true, true, st, nullptr, next_sync()));
  fail |= check("both");
  // single operations through the same kernels
  clear_out();
  CK(chain_launch(n, g_rules, a0, a1, true, false, st, nullptr, next_sync()));
  CK(chain_launch(n, g_rules, a0, a1, false, true, st, nullptr, next_sync()));
  fail |= check("single");
  // run-to-run bit identity
  {
    std::vector<double> A(btD + btU), B(btD + btU);
    CK(chain_launch(n, g_rules, a0, a1, true, true, st, nullptr, next_sync())); CK(hipStreamSynchronize(st));
    CK(hipMemcpy(A.data(), dSig, (btD + btU) * 8, hipMemcpyDeviceToHost));
    int diff = 0;
    for (int it = 0; it < 5; ++it) {
      CK(chain_launch(n, g_rules, a0, a1, true, true, st, nullptr, next_sync())); CK(hipStreamSynchronize(st));
      CK(hipMemcpy(B.data(), dSig, (btD + btU) * 8, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < A.size(); ++i) diff += A[i] != B[i];
    }
    printf("run-to-run differing words: %d\n", diff);
    fail |= diff != 0;
  }
  // chain_pair 1 against 0 (N = 6: two-row eliminations with DPP row-broadcast pivots against the v_readlane form): every output word
  const bool pair_default = g_rules.pair;
  {
    const size_t nout = btD + btU + (size_t)T * n + 1;
    std::vector<double> R[2];
    for (int leg = 0; leg < 2; ++leg) {
      g_rules.pair = leg == 0;
      clear_out();
      CK(hipMemsetAsync(ws0, 0xff, chain_ws_doubles(T, NP) * 8, st)); CK(hipMemsetAsync(ws1, 0xff, chain_ws_doubles(T, NP) * 8, st));
      CK(chain_launch(n, g_rules, a0, a1, true, true, st, nullptr, next_sync()));
      CK(hipStreamSynchronize(st));
      R[leg].resize(nout);
      double* o = R[leg].data();
      CK(hipMemcpy(o, dSig, (btD + btU) * 8, hipMemcpyDeviceToHost)); o += btD + btU;
      CK(hipMemcpy(o, dx_, (size_t)T * n * 8, hipMemcpyDeviceToHost)); o += (size_t)T * n;
      CK(hipMemcpy(o, dhld, 8, hipMemcpyDeviceToHost));
    }
    g_rules.pair = pair_default;
    size_t diff = 0, nan = 0;
    for (size_t i = 0; i < nout; ++i) { diff += memcmp(&R[0][i], &R[1][i], 8) != 0; nan += R[0][i] != R[0][i]; }
    printf("chain_pair 1 vs 0 differing words: %zu of %zu (NaN: %zu)\n", diff, nout, nan);
    fail |= diff != 0 || nan != 0;
  }
#ifdef GVI_CHAIN_TIMING
  {
    // shader-clock stamps of thread 0 of the top pass (factorisation): label every delta by hand from the stamp order in
    // kernels_chain.hpp (pass start, load, barrier, then per elimination of wave 0: [col | GJ | logp | factors | products+adds],
    // barrier after each level, root, ..., backward: per node [phase 1 | sync | phase 2], barrier)
    int zero = 0;
    CK(hipMemcpyToSymbol(HIP_SYMBOL(gvi_chain_nstamp), &zero, sizeof(int)));
    CK(chain_launch(n, g_rules, a0, a1, true, false, st, nullptr, next_sync()));
    CK(hipStreamSynchronize(st));
    int ns = 0;
    std::vector<unsigned long long> stp(256);
    CK(hipMemcpyFromSymbol(&ns, HIP_SYMBOL(gvi_chain_nstamp), sizeof(int)));
    CK(hipMemcpyFromSymbol(stp.data(), HIP_SYMBOL(gvi_chain_stamps), 256 * sizeof(unsigned long long)));
    printf("stamps (%d), cycles between:", ns);
    for (int i = 1; i < ns; ++i) printf(" %llu", stp[i] - stp[i - 1]);
    printf("\n");
  }
#endif
  // ---- assemble-on-load leg (ASM_LEG=0 skips it) ----
  const char* leg_env = getenv("ASM_LEG");
  const bool asm_leg = T > 1 && !(leg_env && atoi(leg_env) == 0);
  double *dVb = nullptr, *dGb = nullptr, *dVu = nullptr, *dGu = nullptr, *dMix = nullptr, *dAsm = nullptr;
  ChainArgs b0 = a0, b1 = a1;
  AsmList AL{};
  unsigned salt = 1;
  if (asm_leg) {
    const int d = 2 * n;
    CK(hipMalloc(&dVb, (size_t)(T - 1) * d * d * 8)); CK(hipMalloc(&dGb, (size_t)(T - 1) * d * 8));
    CK(hipMalloc(&dVu, (size_t)T * nn * 8)); CK(hipMalloc(&dGu, (size_t)T * n * 8));
    CK(hipMalloc(&dMix, (btD + btU + 1) * 8)); CK(hipMalloc(&dAsm, ((size_t)T * n + btD + btU + 1) * 8));
    AL.nsets = 2;
    AL.s[0].K = T - 1; AL.s[0].d = d; AL.s[0].Vdmu = dGb; AL.s[0].Vddmu = dVb; AL.s[0].nsp = 0;
    AL.s[1].K = T; AL.s[1].d = n; AL.s[1].Vdmu = dGu; AL.s[1].Vddmu = dVu; AL.s[1].nsp = 0;
    // as in the iteration: the factorisation takes D + step (V - D) with V assembled, the solve operates on V and g
    b0.asm_on = 1; b0.mixV = nullptr; b0.mixOut = dMix; b0.mix_step = 0.55;
    b1.asm_on = 1; b1.asmG = dAsm; b1.asmD = dAsm + (size_t)T * n; b1.asmU = b1.asmD + btD; b1.D = nullptr; b1.U = nullptr; b1.rhs = drhs;
    auto fill = [&]() { hipLaunchKernelGGL(asm_fill_kernel, dim3(256), dim3(256), 0, st, dGb, dVb, dGu, dVu, T, n, salt++); };
    // dense path against the generic set loop, same inputs: every output bit for bit
    const size_t nout = btD + btU + (size_t)T * n + 1 + (btD + btU) + ((size_t)T * n + btD + btU);
    std::vector<double> R[2];
    for (int leg = 0; leg < 2; ++leg) {
      g_rules.asm_dense = leg == 0;
      clear_out();
      CK(hipMemsetAsync(dMix, 0xff, (btD + btU) * 8, st)); CK(hipMemsetAsync(dAsm, 0xff, ((size_t)T * n + btD + btU) * 8, st));
      salt = 77;
      fill();
      CK(chain_launch(n, g_rules, b0, b1, true, true, st, &AL, next_sync()));
      CK(hipStreamSynchronize(st));
      R[leg].resize(nout);
      double* o = R[leg].data();
      CK(hipMemcpy(o, dSig, (btD + btU) * 8, hipMemcpyDeviceToHost)); o += btD + btU;
      CK(hipMemcpy(o, dx_, (size_t)T * n * 8, hipMemcpyDeviceToHost)); o += (size_t)T * n;
      CK(hipMemcpy(o, dhld, 8, hipMemcpyDeviceToHost)); o += 1;
      CK(hipMemcpy(o, dMix, (btD + btU) * 8, hipMemcpyDeviceToHost)); o += btD + btU;
      CK(hipMemcpy(o, dAsm, ((size_t)T * n + btD + btU) * 8, hipMemcpyDeviceToHost));
    }
    g_rules.asm_dense = true;
    size_t diff = 0, nan = 0;
    for (size_t i = 0; i < nout; ++i) { diff += memcmp(&R[0][i], &R[1][i], 8) != 0; nan += R[0][i] != R[0][i]; }
    printf("assemble-on-load: dense vs generic differing words: %zu of %zu (NaN: %zu)\n", diff, nout, nan);
    fail |= diff != 0 || nan != 0;
  }
#ifdef GVI_CHAIN_TIMING
  if (asm_leg) {
    // the same stamps with the assemble-on-load in the first pass, its inputs freshly written; then with the generic set loop
    for (int leg = 0; leg < 2; ++leg) {
      g_rules.asm_dense = leg == 0;
      for (int rep = 0; rep < 3; ++rep) {
        int zero = 0;
        hipLaunchKernelGGL(asm_fill_kernel, dim3(256), dim3(256), 0, st, dGb, dVb, dGu, dVu, T, n, salt++);
        CK(hipStreamSynchronize(st));
        CK(hipMemcpyToSymbol(HIP_SYMBOL(gvi_chain_nstamp), &zero, sizeof(int)));
        CK(chain_launch(n, g_rules, b0, b1, true, true, st, &AL, next_sync()));
        CK(hipStreamSynchronize(st));
        int ns = 0;
        std::vector<unsigned long long> stp(256);
        CK(hipMemcpyFromSymbol(&ns, HIP_SYMBOL(gvi_chain_nstamp), sizeof(int)));
        CK(hipMemcpyFromSymbol(stp.data(), HIP_SYMBOL(gvi_chain_stamps), 256 * sizeof(unsigned long long)));
        printf("asm-on-load %s stamps (%d), cycles between:", leg == 0 ? "dense  " : "generic", ns);
        for (int i = 1; i < ns && i < 12; ++i) printf(" %llu", stp[i] - stp[i - 1]);
        printf("\n");
      }
    }
    g_rules.asm_dense = true;
  }
#endif
  // timing
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  auto time_it = [&](const char* name, auto&& fn) {
    for (int i = 0; i < 20; ++i) fn();
    CK(hipStreamSynchronize(st));
    CK(hipEventRecord(e0, st));
    for (int i = 0; i < reps; ++i) fn();
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    printf("%-28s %8.2f us per call\n", name, 1e3 * ms / reps);
  };
  for (int rep = 0; rep < 3; ++rep) {                // interleaved: chain_pair 1, 0, 1, 0, 1, 0
    g_rules.pair = true;
    time_it("factor || solve chain_pair=1", [&]() { CK(chain_launch(n, g_rules, a0, a1, true, true, st, nullptr, next_sync())); });
    g_rules.pair = false;
    time_it("factor || solve chain_pair=0", [&]() { CK(chain_launch(n, g_rules, a0, a1, true, true, st, nullptr, next_sync())); });
  }
  g_rules.pair = pair_default;
  time_it("factor || solve", [&]() { CK(chain_launch(n, g_rules, a0, a1, true, true, st, nullptr, next_sync())); });
  time_it("factor only", [&]() { CK(chain_launch(n, g_rules, a0, a1, true, false, st, nullptr, next_sync())); });
  time_it("solve only", [&]() { CK(chain_launch(n, g_rules, a0, a1, false, true, st, nullptr, next_sync())); });
  if (asm_leg) {
    auto call = [&]() {
      hipLaunchKernelGGL(asm_fill_kernel, dim3(256), dim3(256), 0, st, dGb, dVb, dGu, dVu, T, n, salt++);
      CK(chain_launch(n, g_rules, b0, b1, true, true, st, &AL, next_sync()));
    };
    time_it("fill only", [&]() { hipLaunchKernelGGL(asm_fill_kernel, dim3(256), dim3(256), 0, st, dGb, dVb, dGu, dVu, T, n, salt++); });
    for (int rep = 0; rep < 2; ++rep) {              // interleaved: dense, generic, dense, generic
      g_rules.asm_dense = true;
      time_it("fill + asm-on-load dense", call);
      g_rules.asm_dense = false;
      time_it("fill + asm-on-load generic", call);
    }
    g_rules.asm_dense = true;
  }
  {
    // the same launches with a predicate that does not hold: every block returns at its first instruction -- what the launch
    // configuration itself costs (dispatch of 2 x 33 workgroups of 16 waves with ~100 KB of LDS each, kernel arguments, drain)
    double* dpred = nullptr;
    CK(hipMalloc(&dpred, 8));
    CK(hipMemset(dpred, 0, 8));
    ChainArgs s0 = a0, s1 = a1;
    s0.pred = s1.pred = dpred; s0.pred_val = s1.pred_val = 1.0;
    time_it("skipped (predicate): both", [&]() { CK(chain_launch(n, g_rules, s0, s1, true, true, st, nullptr, next_sync())); });
    CK(hipFree(dpred));
  }
  return fail;
}

int main(int argc, char** argv) {
  const int T = argc > 1 ? atoi(argv[1]) : 1025, n = argc > 2 ? atoi(argv[2]) : 6, reps = argc > 3 ? atoi(argv[3]) : 200;
  if (const char* e = getenv("CHAIN_PAIR")) g_rules.pair = atoi(e) != 0;      // the default of every leg but the chain_pair A/B
  if (!chain_supported(n)) { fprintf(stderr, "n must be in 1..16\n"); return 2; }
  const int rc = run(T, n, reps);
  printf(rc ? "FAILED\n" : "OK\n");
  return rc;
}
