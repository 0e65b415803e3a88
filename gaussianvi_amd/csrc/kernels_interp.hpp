// Dense-time posterior: moments and samples of q at times BETWEEN the support states.  No reference
// counterpart (the reference evaluates q at its support states only).
//
// For a chain whose non-prior factors touch support states only, the state at a time tau in [t_i, t_i+1] is, under q, the
// Gauss-Markov prior's conditional on (x_i, x_i+1):  x(tau) = A x_i + B x_i+1 + c + L eps,  L L^T = Qt,  eps ~ N(0, I), so
//     mean = A mu_i + B mu_i+1 + c
//     cov  = A S_ii A^T + A S_i,i+1 B^T + (A S_i,i+1 B^T)^T + B S_i+1,i+1 B^T + Qt
// need the tridiagonal blocks of Sigma only.  A query is (i, A, B, c, Qt); the set of queries is prepared once and kept.
//
// interp_prepare_kernel (one launch per gvi_interp_set, one wave per query): the SEMIDEFINITE Cholesky factor of the lower
// triangle of Qt by a fixed rule -- column k has pivot p = Qt_kk - sum_{j<k} L_kj^2 and thr = 64 * 2^-52 * Qt_kk;
//     |p| <= thr: column k of L is zero;   p > thr: the ordinary column;   p NaN, p < -thr or Qt_kk < 0: the query is BAD
// -- and the row-wise packing ops[q][r] = [A row r | B row r | L row r | c_r] (3 n + 1 doubles): what one lane of the sweep
// keeps in registers, contiguous, so it loads its row in one pass.
//
// interp_moments_kernel (one wave per query, lane = (row, col)): P = A S_ii + B S_i,i+1^T, R = A S_i,i+1 + B S_i+1,i+1,
// cov = P A^T + R B^T + Qt (as given), mean as above.  With (A, B) = (I, 0) or (0, I) every product is exact: a query at a
// support time returns that state's mu and SigD block bit for bit.
//
// interp_sweep_kernel (the hot path): X [S][T][n] -> Xq [S][Q][n].  A lane owns one (query, row) pair, a wave 64 / n whole
// queries = a contiguous run of pairs (one sample's stores of a wave are contiguous), a workgroup four such runs and a tile of
// samples.  The 3 n + 1 operator numbers of the pair stay in registers across the tile.  The 2 n support numbers of (sample,
// query) are read through the cache (the n lanes of a query read the same 2 n numbers).  The normal of (sample j, query q,
// component k) is number (first + j) Q n + q n + k of stream noise_seed (rng.hpp): lane (q, k) generates it -- it computes the
// Philox / Box-Muller pair of its counter and keeps its half -- and the n lanes of a query exchange them by wave shuffles.
// No workgroup reads what another one wrote; plain vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rng.hpp"

namespace gvi {

constexpr int INTERP_NMAX = 16;
constexpr int INTERP_SWEEP_WAVES = 4;         // waves per workgroup of the sweep: 4 (64 / n) queries per workgroup
constexpr int INTERP_TILE_MAX = 16;           // samples per workgroup: a power of two <= this
constexpr int INTERP_TARGET_BLOCKS = 1024;    // the tile grows only while the grid keeps this many workgroups

struct InterpPrepArgs {
  int Q, n;
  const double* A;     // [Q][n][n]
  const double* B;
  const double* c;     // [Q][n] or null (zero)
  const double* Qt;    // [Q][n][n] or null (no noise)
  double* ops;         // [Q][n][3 n + 1]
  int32_t* bad;        // [Q]
};

__global__ __launch_bounds__(64) void interp_prepare_kernel(InterpPrepArgs a) {
  constexpr int NM = INTERP_NMAX;
  __shared__ double Lm[NM * NM];
  __shared__ int badf;
  const int q = blockIdx.x, n = a.n, nn = n * n, tid = threadIdx.x;
  for (int e = tid; e < nn; e += 64) Lm[e] = 0.0;
  if (tid == 0) badf = 0;
  __syncthreads();
  if (a.Qt) {
    const double* Qq = a.Qt + (size_t)q * nn;
    for (int k = 0; k < n; ++k) {
      // the pivot, evaluated by every lane (columns < k are complete: barrier at the end of the previous round)
      const double qkk = Qq[k * n + k];
      double s = 0.0;
      for (int j = 0; j < k; ++j) s += Lm[k * n + j] * Lm[k * n + j];
      const double p = qkk - s, thr = 64.0 * 0x1p-52 * qkk;
      const bool isbad = !(p == p) || p < -thr || qkk < 0.0;
      if (isbad && tid == 0) badf = 1;
      if (!isbad && p > thr) {
        const double d = sqrt(p);
        if (tid == k) Lm[k * n + k] = d;
        if (tid > k && tid < n) {
          double t = 0.0;
          for (int j = 0; j < k; ++j) t += Lm[tid * n + j] * Lm[k * n + j];
          Lm[tid * n + k] = (Qq[tid * n + k] - t) / d;
        }
      }
      __syncthreads();
    }
  }
  const int st = 3 * n + 1;
  const size_t qo = (size_t)q * nn;
  double* out = a.ops + (size_t)q * n * st;
  for (int e = tid; e < n * st; e += 64) {
    const int r = e / st, o = e - r * st;
    double v;
    if (o < n) v = a.A[qo + r * n + o];
    else if (o < 2 * n) v = a.B[qo + r * n + (o - n)];
    else if (o < 3 * n) v = Lm[r * n + (o - 2 * n)];
    else v = a.c ? a.c[(size_t)q * n + r] : 0.0;
    out[e] = v;
  }
  if (tid == 0) a.bad[q] = badf;
}

struct InterpMomArgs {
  int Q, n;
  const int32_t* idx;  // [Q] left support state, in [0, T - 2]
  const double* ops;
  const double* Qt;    // as given to gvi_interp_set, or null
  const double* mu;    // [T][n]
  const double* SigD;  // [T][n][n]
  const double* SigU;  // [T-1][n][n], block (i, i + 1)
  double* mean;        // [Q][n] or null
  double* cov;         // [Q][n][n] or null
};

__global__ __launch_bounds__(64) void interp_moments_kernel(InterpMomArgs a) {
  constexpr int NN = INTERP_NMAX * INTERP_NMAX;
  __shared__ double sA[NN], sB[NN], Sii[NN], Su[NN], Sjj[NN], P[NN], R[NN];
  const int q = blockIdx.x, n = a.n, nn = n * n, tid = threadIdx.x, st = 3 * n + 1;
  const size_t i = (size_t)a.idx[q];
  const double* op = a.ops + (size_t)q * n * st;
  for (int e = tid; e < nn; e += 64) {
    const int r = e / n, k = e - r * n;
    sA[e] = op[r * st + k];
    sB[e] = op[r * st + n + k];
    Sii[e] = a.SigD[i * nn + e];
    Su[e] = a.SigU[i * nn + e];
    Sjj[e] = a.SigD[(i + 1) * nn + e];
  }
  __syncthreads();
  if (tid < n && a.mean) {
    double sa = 0.0, sb = 0.0;
    for (int k = 0; k < n; ++k) sa += sA[tid * n + k] * a.mu[i * n + k];
    for (int k = 0; k < n; ++k) sb += sB[tid * n + k] * a.mu[(i + 1) * n + k];
    a.mean[(size_t)q * n + tid] = sa + sb + op[tid * st + 3 * n];
  }
  if (!a.cov) return;
  for (int e = tid; e < nn; e += 64) {
    const int r = e / n, c = e - r * n;
    double p1 = 0.0, p2 = 0.0, r1 = 0.0, r2 = 0.0;
    for (int k = 0; k < n; ++k) {
      p1 += sA[r * n + k] * Sii[k * n + c];
      p2 += sB[r * n + k] * Su[c * n + k];
      r1 += sA[r * n + k] * Su[k * n + c];
      r2 += sB[r * n + k] * Sjj[k * n + c];
    }
    P[e] = p1 + p2;
    R[e] = r1 + r2;
  }
  __syncthreads();
  for (int e = tid; e < nn; e += 64) {
    const int r = e / n, c = e - r * n;
    double v1 = 0.0, v2 = 0.0;
    for (int k = 0; k < n; ++k) {
      v1 += P[r * n + k] * sA[c * n + k];
      v2 += R[r * n + k] * sB[c * n + k];
    }
    double v = v1 + v2;
    if (a.Qt) v += a.Qt[(size_t)q * nn + e];
    a.cov[(size_t)q * nn + e] = v;
  }
}

struct InterpSweepArgs {
  int T, n, Q, S, tile;
  int noise;             // 0: the set has no Qt -- nothing is generated, eps is not read
  uint64_t noise_seed;
  int64_t first;
  const int32_t* idx;
  const double* ops;
  const int32_t* bad;
  const double* eps;     // [S][Q][n] or null (then generated)
  const double* X;       // [S][T][n]
  double* Xq;            // [S][Q][n]
};

// NM >= n bounds the register rows
template <int NM>
__global__ __launch_bounds__(INTERP_SWEEP_WAVES * 64) void interp_sweep_kernel(InterpSweepArgs a) {
  const int n = a.n, G = 64 / n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane / n, r = lane - grp * n, gl0 = grp * n;
  const int64_t q = ((int64_t)blockIdx.x * INTERP_SWEEP_WAVES + wave) * G + grp;
  const bool valid = grp < G && q < a.Q;      // a query's n lanes are valid or invalid together
  const size_t Tn = (size_t)a.T * n, Qn = (size_t)a.Q * n;
  const size_t p = valid ? (size_t)q * n + r : 0;
  double Ar[NM], Br[NM], Lr[NM], cr = 0.0;
  size_t xo = 0;
  bool isbad = false;
  {
    const double* op = a.ops + p * (size_t)(3 * n + 1);
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      const bool on = valid && k < n;
      Ar[k] = on ? op[k] : 0.0;
      Br[k] = on ? op[n + k] : 0.0;
      Lr[k] = on ? op[2 * n + k] : 0.0;
    }
    if (valid) {
      cr = op[3 * n];
      xo = (size_t)a.idx[q] * n;
      isbad = a.bad[q] != 0;
    }
  }
  const int j0 = (int)blockIdx.y * a.tile;
  const int tj = min(a.tile, a.S - j0);
  for (int j = 0; j < tj; ++j) {
    const size_t js = (size_t)(j0 + j);
    double nz = 0.0;
    if (a.noise) {                              // uniform over the launch: every lane reaches the shuffles
      double z = 0.0;
      if (valid) {
        if (a.eps) {
          z = a.eps[js * Qn + p];
        } else {
          const uint64_t num = ((uint64_t)a.first + js) * (uint64_t)Qn + p;
          double z0, z1;
          randn_pair(a.noise_seed, num >> 1, z0, z1);
          z = (num & 1) ? z1 : z0;
        }
      }
#pragma unroll
      for (int k = 0; k < NM; ++k) if (k < n) nz += Lr[k] * __shfl(z, gl0 + k);
    }
    if (valid) {
      const double* xa = a.X + js * Tn + xo;    // x_i followed by x_i+1: 2 n contiguous numbers
      double sa = 0.0, sb = 0.0;
#pragma unroll
      for (int k = 0; k < NM; ++k) if (k < n) sa += Ar[k] * xa[k];
#pragma unroll
      for (int k = 0; k < NM; ++k) if (k < n) sb += Br[k] * xa[n + k];
      const double v = ((sa + sb) + cr) + nz;
      a.Xq[js * Qn + p] = isbad ? __builtin_nan("") : v;
    }
  }
}

}  // namespace gvi
