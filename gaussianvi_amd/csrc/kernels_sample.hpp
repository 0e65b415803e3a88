// Exact sampling of q = N(mu, Lambda^-1) for the block-tridiagonal joint precision Lambda = (D, U), and its log-density.
// No reference counterpart (the reference has no sampler).
//
// Factorisation (sample_factor_kernel, one launch per level): the block cyclic reduction of kernels_chain.hpp, written
// as a dedicated kernel so that EVERY node's elimination blocks reach global memory (the chain kernels keep the top pass's
// blocks in LDS).  Level l keeps the nodes that are multiples of 2^l and eliminates the odd ones; eliminating e with
// a = e - 2^l, b = e + 2^l, Ua = A[a,e], Ub = A[e,b]:
//     P_e = L L^T (Cholesky),  R_e = L^-T  (R R^T = E = P_e^-1),  GA = E Ua^T,  GB = E Ub
//     D_a -= Ua GA,  D_b -= Ub^T GB,  A[a,b] = -Ua GB
// The launch of level l takes every node alive at l (one wave each): it first applies the updates of level l - 1 to its own
// blocks (the GA / GB of level l - 1 were written by the previous launch), then eliminates itself if it is odd at level l.
// Updated blocks go to a ping-pong buffer, so no workgroup reads what another one writes in the same launch.  The root
// (node 0 at level L = ceil(log2 T)) sums the log-pivots of all nodes in a fixed order: 1/2 log det, NaN when a pivot is
// not positive.
//
// Sampling sweep (sample_sweep_kernel, ONE launch): y ~ N(0, Lambda^-1) is the solver's back-substitution with the
// right-hand side replaced by standard normals,
//     y_root = R_root eps_root,   y_e = R_e eps_e - GA y_a - GB y_b   (levels top-down),   x = mu + y.
// (2 x 2 block case level by level: cov(y_o) = A^-1 + A^-1 B S^-1 B^T A^-1, cov(y_o, y_e) = -A^-1 B S^-1.)  A workgroup owns
// a tile of samples and walks all levels itself -- no hand-over between workgroups.  Lanes are (node, row) groups of n lanes
// inside ONE wave, so eps_e can be overwritten by y_e in place: a lane's store depends on every eps_e load of its group.
// The tile's y lives in LDS when T n 8 tile fits (SAMPLE_LDS_BYTES), else in the output buffer; then every level ends with an
// explicit vmcnt drain before the barrier (the write-through stores must have left the wave before another wave reads).
//
// Log-density (logpdf_quad_kernel + logpdf_reduce_kernel): (x - mu)^T Lambda (x - mu) over (sample, node), a fixed-order
// per-sample reduction, plus the half log-det of the chain kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rng.hpp"

namespace gvi {

constexpr int SAMPLE_NMAX = 16;
constexpr int SAMPLE_SWEEP_THREADS = 512;
constexpr int SAMPLE_LDS_BYTES = 80 * 1024;
constexpr int SAMPLE_TILE_MAX = 8;

struct SampleFactorArgs {
  int T, n, level, L;
  const double* D;     // level 0: the caller's blocks D[T][n][n], U[T-1][n][n]
  const double* U;
  const double* Dr;    // level >= 1: blocks of level - 1 written by the previous launch
  const double* Cr;    //   C[x] = A[x, x + 2^(level-1)]
  double* Dw;          // blocks of this level (read by the next launch)
  double* Cw;
  double* R;           // [T][n][n] per node: R = L^-T, GA, GB (row-major), lp = sum log diag L
  double* GA;
  double* GB;
  double* lp;          // [T]
  double* hld;         // [1] written by the root
};

__global__ __launch_bounds__(64) void sample_factor_kernel(SampleFactorArgs a) {
  constexpr int NM = SAMPLE_NMAX;
  __shared__ double P[NM * NM], Ua[NM * NM], Ub[NM * NM], Li[NM * NM], E[NM * NM];
  __shared__ double red[64];
  const int n = a.n, nn = n * n, tid = threadIdx.x, l = a.level, T = a.T;
  const int x = (int)blockIdx.x << l, step = 1 << l;
  const bool root = l == a.L;
  const bool elim = !root && (blockIdx.x & 1);
  const bool hasB = x + step < T;            // A[x, x + 2^l] exists at this level
  const size_t xo = (size_t)x * nn;
  if (l == 0) {
    for (int e = tid; e < nn; e += 64) {
      P[e] = a.D[xo + e];
      if (hasB) Ub[e] = a.U[xo + e];
      if (elim) Ua[e] = a.U[xo - nn + e];
    }
  } else {
    const int h = step >> 1, xR = x + h, xL = x - h;
    const double* Cx = a.Cr + xo;
    for (int e = tid; e < nn; e += 64) {
      const int r = e / n, c = e % n;
      double v = a.Dr[xo + e];
      if (xR < T) {                          // D_x -= C[x] GA[xR]      (x is the left neighbour of xR)
        const double* G = a.GA + (size_t)xR * nn;
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += Cx[r * n + k] * G[k * n + c];
        v -= s;
      }
      if (x > 0) {                           // D_x -= C[xL]^T GB[xL]   (x is the right neighbour of xL)
        const double* C = a.Cr + (size_t)xL * nn;
        const double* G = a.GB + (size_t)xL * nn;
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += C[k * n + r] * G[k * n + c];
        v -= s;
      }
      P[e] = v;
      if (hasB) {                            // A[x, x + 2h] = -C[x] GB[xR]
        const double* G = a.GB + (size_t)xR * nn;
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += Cx[r * n + k] * G[k * n + c];
        Ub[e] = -s;
      }
      if (elim) {                            // A[x - 2h, x] = -C[x - 2h] GB[x - h]
        const double* C = a.Cr + (size_t)(x - step) * nn;
        const double* G = a.GB + (size_t)xL * nn;
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += C[r * n + k] * G[k * n + c];
        Ua[e] = -s;
      }
    }
  }
  __syncthreads();
  if (!root) {
    for (int e = tid; e < nn; e += 64) {
      if (!elim) a.Dw[xo + e] = P[e];
      if (hasB) a.Cw[xo + e] = Ub[e];
    }
  }
  if (!elim && !root) return;
  // Cholesky P = L L^T in place (lower triangle)
  double lsum = 0.0;
  for (int j = 0; j < n; ++j) {
    if (tid == 0) {
      const double d = P[j * n + j];
      const double ljj = d > 0.0 ? sqrt(d) : __builtin_nan("");
      P[j * n + j] = ljj;
      lsum += log(ljj);
    }
    __syncthreads();
    const double piv = P[j * n + j];
    for (int i = j + 1 + tid; i < n; i += 64) P[i * n + j] /= piv;
    __syncthreads();
    for (int e = tid; e < nn; e += 64) {
      const int i = e / n, k = e % n;
      if (k > j && i >= k) P[i * n + k] -= P[i * n + j] * P[k * n + j];
    }
    __syncthreads();
  }
  // Li = L^-1 (lower): column c by forward substitution, one lane per column
  for (int c = tid; c < n; c += 64) {
    for (int i = 0; i < n; ++i) {
      if (i < c) { Li[i * n + c] = 0.0; continue; }
      double s = i == c ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) s -= P[i * n + k] * Li[k * n + c];
      Li[i * n + c] = s / P[i * n + i];
    }
  }
  __syncthreads();
  // E = L^-T L^-1,  R = L^-T
  for (int e = tid; e < nn; e += 64) {
    const int r = e / n, c = e % n;
    double s = 0.0;
    for (int k = (r > c ? r : c); k < n; ++k) s += Li[k * n + r] * Li[k * n + c];
    E[e] = s;
    a.R[xo + e] = Li[c * n + r];
  }
  __syncthreads();
  for (int e = tid; e < nn; e += 64) {
    const int r = e / n, c = e % n;
    double ga = 0.0, gb = 0.0;
    if (elim) for (int k = 0; k < n; ++k) ga += E[r * n + k] * Ua[c * n + k];
    if (hasB) for (int k = 0; k < n; ++k) gb += E[r * n + k] * Ub[k * n + c];
    a.GA[xo + e] = ga;
    a.GB[xo + e] = gb;
  }
  if (!root) {
    if (tid == 0) a.lp[x] = lsum;
    return;
  }
  // root: 1/2 log det = sum of every node's log-pivots (fixed order; node 0's own sum from the register)
  double s = 0.0;
  for (int t = 1 + tid; t < T; t += 64) s += a.lp[t];
  red[tid] = s;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) *a.hld = lsum + red[0];
}

struct SampleSweepArgs {
  int T, n, L, S, tile;
  uint64_t seed;
  int64_t first;       // sample j uses normals (first + j) T n ... of `seed`
  const double* eps;   // [S][T][n] or null (then generated)
  const double* R;
  const double* GA;
  const double* GB;
  const double* mu;    // [T][n]
  const double* hld;   // NaN: every entry of X is NaN
  double* X;           // [S][T][n]
};

// one wave-local group of n lanes per (node, row); NM >= n bounds the register rows
template <int NM, bool LDSY>
__global__ __launch_bounds__(SAMPLE_SWEEP_THREADS) void sample_sweep_kernel(SampleSweepArgs a) {
  extern __shared__ double ylds[];
  const int T = a.T, n = a.n, tid = threadIdx.x;
  const int64_t Tn = (int64_t)T * n;
  const int j0 = (int)blockIdx.x * a.tile;
  const int tj = min(a.tile, a.S - j0);
  double* Xt = a.X + (size_t)j0 * Tn;
  double* Y = LDSY ? ylds : Xt;
  const int64_t cnt = (int64_t)tj * Tn;
  if (!(*a.hld == *a.hld)) {                 // not positive definite (NaN convention of gvi_bt_logdet)
    for (int64_t i = tid; i < cnt; i += blockDim.x) Xt[i] = __builtin_nan("");
    return;
  }
  // eps of the tile
  if (a.eps) {
    const double* ep = a.eps + (size_t)j0 * Tn;
    for (int64_t i = tid; i < cnt; i += blockDim.x) Y[i] = ep[i];
  } else {
    const uint64_t base = (uint64_t)(a.first + j0) * (uint64_t)Tn;
    const uint64_t c0 = base >> 1, c1 = (base + cnt - 1) >> 1;
    for (uint64_t c = c0 + tid; c <= c1; c += blockDim.x) {
      double z0, z1;
      randn_pair(a.seed, c, z0, z1);
      const int64_t i = (int64_t)(2 * c - base);
      if (i >= 0) Y[i] = z0;
      if (i + 1 < cnt) Y[i + 1] = z1;
    }
  }
  if (!LDSY) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int lane = tid & 63, G = 64 / n;
  const int grp = lane / n, r = lane % n;
  const bool act = grp < G;
  const int NG = (int)(blockDim.x >> 6) * G;
  const int g = (int)(tid >> 6) * G + grp;
  for (int l = a.L; l >= 0; --l) {
    const int step = 1 << l;
    const int count = l == a.L ? 1 : (((T + step - 1) >> l) >> 1);
    for (int q = g; act && q < count; q += NG) {
      const int e = l == a.L ? 0 : step + 2 * q * step;
      const int ia = l == a.L ? -1 : e - step;
      const int ib = (l == a.L || e + step >= T) ? -1 : e + step;
      const size_t mo = ((size_t)e * n + r) * n;
      double Rr[NM], Ar[NM], Br[NM];
#pragma unroll
      for (int k = 0; k < NM; ++k) {
        Rr[k] = k < n ? a.R[mo + k] : 0.0;
        Ar[k] = (k < n && ia >= 0) ? a.GA[mo + k] : 0.0;
        Br[k] = (k < n && ib >= 0) ? a.GB[mo + k] : 0.0;
      }
      for (int j = 0; j < tj; ++j) {
        double* Yj = Y + (size_t)j * Tn;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < NM; ++k) if (k < n) acc += Rr[k] * Yj[(size_t)e * n + k];
        if (ia >= 0) {
#pragma unroll
          for (int k = 0; k < NM; ++k) if (k < n) acc -= Ar[k] * Yj[(size_t)ia * n + k];
        }
        if (ib >= 0) {
#pragma unroll
          for (int k = 0; k < NM; ++k) if (k < n) acc -= Br[k] * Yj[(size_t)ib * n + k];
        }
        Yj[(size_t)e * n + r] = acc;
      }
    }
    if (!LDSY) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  // x = mu + y
  for (int j = 0; j < tj; ++j) {
    const double* Yj = Y + (size_t)j * Tn;
    double* Xj = Xt + (size_t)j * Tn;
    for (int64_t i = tid; i < Tn; i += blockDim.x) Xj[i] = a.mu[i] + Yj[i];
  }
}

// normals first .. first + count - 1 of `seed`
__global__ void randn_kernel(uint64_t seed, int64_t first, int64_t count, double* out) {
  const uint64_t c0 = (uint64_t)first >> 1, c1 = ((uint64_t)first + (uint64_t)count - 1) >> 1;
  const uint64_t c = c0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > c1) return;
  double z0, z1;
  randn_pair(seed, c, z0, z1);
  const int64_t i = (int64_t)(2 * c - (uint64_t)first);
  if (i >= 0) out[i] = z0;
  if (i + 1 < count) out[i + 1] = z1;
}

// Q[j][t] = d_t^T (Lambda d)_t,  d = x_j - mu
__global__ __launch_bounds__(256) void logpdf_quad_kernel(int T, int n, int S, const double* D, const double* U, const double* mu, const double* X,
                                   double* Q) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)S * T) return;
  const int j = (int)(idx / T), t = (int)(idx % T);
  const int nn = n * n;
  const double* xj = X + (size_t)j * T * n;
  double d[SAMPLE_NMAX], dl[SAMPLE_NMAX], dr[SAMPLE_NMAX];
#pragma unroll
  for (int k = 0; k < SAMPLE_NMAX; ++k) {
    d[k] = k < n ? xj[(size_t)t * n + k] - mu[(size_t)t * n + k] : 0.0;
    dl[k] = (k < n && t > 0) ? xj[(size_t)(t - 1) * n + k] - mu[(size_t)(t - 1) * n + k] : 0.0;
    dr[k] = (k < n && t + 1 < T) ? xj[(size_t)(t + 1) * n + k] - mu[(size_t)(t + 1) * n + k] : 0.0;
  }
  double v = 0.0;
#pragma unroll
  for (int r = 0; r < SAMPLE_NMAX; ++r) {      // unrolled with guards: d / dl / dr stay in registers
    if (r >= n) break;
    double s = 0.0;
    const double* Dt = D + (size_t)t * nn + r * n;
#pragma unroll
    for (int c = 0; c < SAMPLE_NMAX; ++c) if (c < n) s += Dt[c] * d[c];
    if (t + 1 < T) {
      const double* Ut = U + (size_t)t * nn + r * n;
#pragma unroll
      for (int c = 0; c < SAMPLE_NMAX; ++c) if (c < n) s += Ut[c] * dr[c];
    }
    if (t > 0) {
      const double* Ul = U + (size_t)(t - 1) * nn + r;
#pragma unroll
      for (int c = 0; c < SAMPLE_NMAX; ++c) if (c < n) s += Ul[c * n] * dl[c];
    }
    v += d[r] * s;
  }
  Q[idx] = v;
}

// logq[j] = -1/2 sum_t Q[j][t] + hld - (T n / 2) log 2 pi    (one workgroup of 256 per sample, fixed order)
__global__ __launch_bounds__(256) void logpdf_reduce_kernel(int T, int n, const double* Q, const double* hld, double* logq) {
  __shared__ double red[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int t = tid; t < T; t += 256) s += Q[(size_t)j * T + t];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) logq[j] = -0.5 * red[0] + *hld - 0.5 * (double)T * n * 1.8378770664093453;   // log(2 pi)
}

}  // namespace gvi
