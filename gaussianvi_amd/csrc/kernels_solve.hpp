// X_r = Lambda^-1 B_r for a batch of right-hand sides, and block columns of Lambda^-1, for the symmetric positive definite
// block-tridiagonal Lambda = (D, U).  No reference counterpart (inverse_GBP / inv_sparse fill the tridiagonal pattern only,
// gvibase/GVI-GH-GBP-impl.h:246-305).
//
// Factorisation: sample_factor_kernel of kernels_sample.hpp, unchanged -- every node of the cyclic reduction leaves
// R_e (R R^T = E = P_e^-1), GA_e = E Ua^T, GB_e = E Ub and the half log-det in global memory.
//
// Sweep (solve_sweep_kernel, ONE launch): a workgroup owns a tile of right-hand sides and walks every level itself, up and
// then down -- no hand-over between workgroups.  With step = 2^l:
//     up,   l = 0 .. L-1, every survivor x (multiple of 2 step) GATHERS from its eliminated neighbours:
//             r_x -= GA[x+step]^T r_{x+step}   (x + step < T),     r_x -= GB[x-step]^T r_{x-step}   (x - step >= 0)
//     down, l = L .. 0:   x_root = R_0 (R_0^T r_0),    x_e = R_e (R_e^T r_e) - GA_e x_{e-step} - GB_e x_{e+step}
// The survivor gathers (the eliminated node does not scatter): no atomics, one fixed summation order, so results are
// bit-identical from run to run and a right-hand side's arithmetic does not depend on the tile it lands in.
// Lanes are (node, row) groups of n lanes inside ONE wave, as in sample_sweep_kernel; a lane holds its row / column of the
// node's blocks in registers over the tile.  w = R^T r is exchanged inside the group by wave shuffles (no barrier per node),
// and x_e overwrites r_e in place: a lane's store depends on every r_e load of its group.
// The tile's vectors live in LDS when T n 8 tile fits (SOLVE_LDS_BYTES), else in the output buffer; then every level ends
// with an explicit vmcnt drain before the barrier (the write-through stores must have left the wave before another wave reads).
//
// Covariance columns: right-hand side j = c n + k is the unit vector at (nodes[c], k), generated here from the node list;
// the result goes out transposed, C[c][t][r][k] = x_j[t][r].  On the output-buffer path the vectors are kept in that layout
// from the start.  The arithmetic is the general solve's, operation for operation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gvi {

constexpr int SOLVE_NMAX = 16;
constexpr int SOLVE_SWEEP_THREADS = 512;
constexpr int SOLVE_LDS_BYTES = 80 * 1024;     // two workgroups per CU (160 KiB of LDS)
constexpr int SOLVE_TILE_MAX = 8;

struct SolveSweepArgs {
  int T, n, L, R, tile;
  const double* B;        // [R][T][n], or null: unit columns from `nodes`
  const int32_t* nodes;   // [R / n] when B is null
  const double* Rf;       // [T][n][n] per node: R, GA, GB of sample_factor_kernel
  const double* GA;
  const double* GB;
  const double* hld;      // NaN: every entry of X is NaN
  double* X;              // [R][T][n], or C[R / n][T][n][n] for the columns
};

// one wave-local group of n lanes per (node, row); NM >= n bounds the register rows
template <int NM, bool LDSY>
__global__ __launch_bounds__(SOLVE_SWEEP_THREADS) void solve_sweep_kernel(SolveSweepArgs a) {
  extern __shared__ double ylds[];
  const int T = a.T, n = a.n, tid = threadIdx.x;
  const int64_t Tn = (int64_t)T * n;
  const int j0 = (int)blockIdx.x * a.tile;
  const int tj = min(a.tile, a.R - j0);
  const bool cols = a.B == nullptr;
  // element i of right-hand side j0 + jj in the output: X[obase(jj) + i * os]
  const int os = cols ? n : 1;
  auto obase = [&](int jj) -> size_t {
    const int j = j0 + jj;
    return cols ? (size_t)(j / n) * (size_t)Tn * n + (size_t)(j % n) : (size_t)j * (size_t)Tn;
  };
  if (!(*a.hld == *a.hld)) {                 // not positive definite (NaN convention of gvi_bt_logdet)
    for (int jj = 0; jj < tj; ++jj) {
      double* Xj = a.X + obase(jj);
      for (int64_t i = tid; i < Tn; i += blockDim.x) Xj[i * os] = __builtin_nan("");
    }
    return;
  }
  // the tile's vectors: Yv(jj)[i * ys]
  const int ys = LDSY ? 1 : os;
  auto Yv = [&](int jj) -> double* { return LDSY ? ylds + (size_t)jj * Tn : a.X + obase(jj); };
  for (int jj = 0; jj < tj; ++jj) {
    double* Yj = Yv(jj);
    if (cols) {
      const int j = j0 + jj;
      const int64_t one = (int64_t)a.nodes[j / n] * n + j % n;
      for (int64_t i = tid; i < Tn; i += blockDim.x) Yj[i * ys] = i == one ? 1.0 : 0.0;
    } else {
      const double* Bj = a.B + (size_t)(j0 + jj) * Tn;
      for (int64_t i = tid; i < Tn; i += blockDim.x) Yj[i] = Bj[i];
    }
  }
  if (!LDSY) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int lane = tid & 63, G = 64 / n;
  const int grp = lane / n, r = lane % n;
  const bool act = grp < G;
  const int NG = (int)(blockDim.x >> 6) * G;
  const int g = (int)(tid >> 6) * G + grp;
  const int gl0 = grp * n;                   // first lane of the group
  // up: survivors gather from the nodes eliminated at this level
  for (int l = 0; l < a.L; ++l) {
    const int step = 1 << l;
    const int count = (int)(((int64_t)T + 2 * step - 1) >> (l + 1));
    for (int q = g; act && q < count; q += NG) {
      const int x = q << (l + 1);
      const int ie = x + step < T ? x + step : -1;     // eliminated against x as its left neighbour: GA
      const int ib = x >= step ? x - step : -1;         // eliminated against x as its right neighbour: GB
      double Ac[NM], Bc[NM];                            // column r of GA[ie], GB[ib]
#pragma unroll
      for (int k = 0; k < NM; ++k) {
        Ac[k] = (k < n && ie >= 0) ? a.GA[((size_t)ie * n + k) * n + r] : 0.0;
        Bc[k] = (k < n && ib >= 0) ? a.GB[((size_t)ib * n + k) * n + r] : 0.0;
      }
      for (int jj = 0; jj < tj; ++jj) {
        double* Yj = Yv(jj);
        double acc = Yj[((size_t)x * n + r) * ys];
        if (ie >= 0) {
#pragma unroll
          for (int k = 0; k < NM; ++k) if (k < n) acc -= Ac[k] * Yj[((size_t)ie * n + k) * ys];
        }
        if (ib >= 0) {
#pragma unroll
          for (int k = 0; k < NM; ++k) if (k < n) acc -= Bc[k] * Yj[((size_t)ib * n + k) * ys];
        }
        Yj[((size_t)x * n + r) * ys] = acc;
      }
    }
    if (!LDSY) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  // down: the root, then the eliminated nodes level by level
  for (int l = a.L; l >= 0; --l) {
    const int step = 1 << l;
    const int count = l == a.L ? 1 : (((T + step - 1) >> l) >> 1);
    for (int q = g; act && q < count; q += NG) {
      const int e = l == a.L ? 0 : step + 2 * q * step;
      const int ia = l == a.L ? -1 : e - step;
      const int ib = (l == a.L || e + step >= T) ? -1 : e + step;
      const size_t mo = ((size_t)e * n + r) * n;
      double Rc[NM], Rr[NM], Ar[NM], Br[NM];            // column r and row r of R, row r of GA, GB
#pragma unroll
      for (int k = 0; k < NM; ++k) {
        Rc[k] = k < n ? a.Rf[((size_t)e * n + k) * n + r] : 0.0;
        Rr[k] = k < n ? a.Rf[mo + k] : 0.0;
        Ar[k] = (k < n && ia >= 0) ? a.GA[mo + k] : 0.0;
        Br[k] = (k < n && ib >= 0) ? a.GB[mo + k] : 0.0;
      }
      for (int jj = 0; jj < tj; ++jj) {
        double* Yj = Yv(jj);
        double w = 0.0;                                 // (R^T r_e)[r]
#pragma unroll
        for (int k = 0; k < NM; ++k) if (k < n) w += Rc[k] * Yj[((size_t)e * n + k) * ys];
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < NM; ++k) if (k < n) acc += Rr[k] * __shfl(w, gl0 + k);
        if (ia >= 0) {
#pragma unroll
          for (int k = 0; k < NM; ++k) if (k < n) acc -= Ar[k] * Yj[((size_t)ia * n + k) * ys];
        }
        if (ib >= 0) {
#pragma unroll
          for (int k = 0; k < NM; ++k) if (k < n) acc -= Br[k] * Yj[((size_t)ib * n + k) * ys];
        }
        Yj[((size_t)e * n + r) * ys] = acc;
      }
    }
    if (!LDSY) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (!LDSY) return;                         // the output buffer already holds the result
  if (!cols) {
    double* Xt = a.X + (size_t)j0 * Tn;
    const int64_t cnt = (int64_t)tj * Tn;
    for (int64_t i = tid; i < cnt; i += blockDim.x) Xt[i] = ylds[i];
  } else {
    // consecutive lanes take consecutive right-hand sides: the k of C[c][t][r][k] is the fastest index (cnt fits int: LDS)
    const int cnt = tj * (int)Tn;
    for (int idx = tid; idx < cnt; idx += blockDim.x) {
      const int jj = idx % tj, i = idx / tj;
      a.X[obase(jj) + (size_t)i * n] = ylds[(size_t)jj * Tn + i];
    }
  }
}

}  // namespace gvi
