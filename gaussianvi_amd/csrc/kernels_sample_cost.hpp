// Costs of sampled trajectories: the factors' psi, and the clearance of the hinge-on-SDF factors, evaluated at samples
// X [S][T][n] of q instead of at sigma points.  No reference counterpart (the reference evaluates psi at sigma points only;
// the psi functions called here cite their reference lines in psi_point.hpp).
//
//   cost[s][k] = psi_k(x_s[start_k n .. start_k n + d)) / temperature_k        clr[s][k] = min_b sdf(p_b) - r_b
//
// sample_cost_kernel, ONE launch for every set of the list (block -> set through the block offsets, like PrepList of kernels_prep.hpp):
//   sum-of-squares sets (QUAD_PRIOR / FIXED_PRIOR, closed-form sets included): psi = sum_r sgn_r (b_r + A_r x)^2.  A workgroup
//     of four waves owns a tile of 4 G consecutive factors and walks a chunk of samples.  Lanes are (factor, residual row r) groups
//     of P = 2^ceil(log2 m) lanes inside ONE wave, G = 64 / P factors per wave: a lane loads row r of A_k, b_r and sgn_r ONCE into
//     registers, then per sample reads the d entries of its factor's slice (the lanes of a group share the addresses, consecutive
//     factors of a chain set read consecutive states: a wave touches one contiguous stretch of (G + 1) n doubles of the sample),
//     forms its residual and squares it; the m squares are summed by an xor butterfly over the group (rows m .. P - 1 carry 0),
//     a fixed tree.  Lane r = 0 stores.
//   the other kinds (RANGE_1D, HINGE_SDF_*): one thread per (sample, factor), factor index fastest, through the psi_* functions
//     and the *_points walkers of psi_point.hpp (hinge_psi_clearance).
//   A slice that holds a non-finite value gives NaN without entering the psi / SDF code (no index is formed from a NaN).
// sample_cost_reduce_kernel, one workgroup of 256 per sample: J[s] = sum over the concatenated cost row [set 0 | set 1 | ...]
//   -- thread t adds entries t, t + 256, ... in ascending order, then the 256 partial sums are folded by halving (t += t + 128,
//   64, ... 1) -- and clr_min[s] = min over the clearance row (NaN if any entry is NaN).  The order depends on the sets only.
// Every operand (A, b, sgn, raw parameters, temperatures, grids, arm model) was uploaded before the launch; X comes from an
// earlier launch or copy.  Plain global loads and vector stores; no atomics, no hand-over between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "device_common.hpp"   // MAX_SETS
#include "factor_dev.hpp"
#include "psi_point.hpp"

namespace gvi {

constexpr int SCOST_WAVES = 4;
constexpr int SCOST_THREADS = SCOST_WAVES * 64;
constexpr int SCOST_DMAX = 32;            // widest sum-of-squares slice held in registers
constexpr int SCOST_TARGET_BLOCKS = 2048; // blocks a sum-of-squares set aims for before its sample chunks grow

struct SampleCostList {
  int nsets, T, n, S;
  const double* X;                 // [S][T][n]
  int boff[MAX_SETS + 1];         // first block of set i
  FactorDev f[MAX_SETS];
  const int32_t* start[MAX_SETS];
  int ftiles[MAX_SETS];           // sum-of-squares sets: factor tiles; blocks = ftiles * ceil(S / schunk)
  int schunk[MAX_SETS];           //   samples per block
  double* cost[MAX_SETS];         // [S][ld_cost] at column 0 of the set, or null
  double* clr[MAX_SETS];          // [S][ld_clr], hinge kinds only, or null
  int64_t ld_cost[MAX_SETS], ld_clr[MAX_SETS];
};
static_assert(sizeof(SampleCostList) <= 4096, "kernel arguments");

__host__ __device__ inline int scost_group(int m) { int P = 1; while (P < m) P <<= 1; return P; }

__device__ __forceinline__ bool scost_finite(double v) { return fabs(v) < __builtin_inf(); }   // false for NaN

// NM >= d: register rows.  Padding columns read entry 0 of the slice against a zero coefficient.
template <int NM>
__device__ __forceinline__ void scost_sumsq_body(const SampleCostList& L, const int si, const int blk) {
  const FactorDev& f = L.f[si];
  const int m = f.m, d = f.d, P = scost_group(m), G = 64 / P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane / P, r = lane % P;
  const int ft = blk % L.ftiles[si], sc = blk / L.ftiles[si];
  const int k = (ft * SCOST_WAVES + wave) * G + grp;
  const bool act = k < f.K && r < m;
  double Ar[NM];
#pragma unroll
  for (int c = 0; c < NM; ++c) Ar[c] = (act && c < d) ? f.A[((size_t)k * m + r) * d + c] : 0.0;
  const double br = act ? f.b[(size_t)k * m + r] : 0.0;
  const double sg = act ? f.sgn[(size_t)k * m + r] : 0.0;
  const double temp = k < f.K ? f.temperature[k] : 1.0;
  const size_t off = k < f.K ? (size_t)L.start[si][k] * L.n : 0;
  const size_t Tn = (size_t)L.T * L.n;
  const int s0 = sc * L.schunk[si], s1 = min(L.S, s0 + L.schunk[si]);
  double* out = L.cost[si];
  for (int s = s0; s < s1; ++s) {
    const double* xs = L.X + (size_t)s * Tn + off;
    double x[NM];
#pragma unroll
    for (int c = 0; c < NM; ++c) x[c] = xs[c < d ? c : 0];
    double acc = br;
    bool fin = true;
#pragma unroll
    for (int c = 0; c < NM; ++c) {
      fin = fin && scost_finite(x[c]);
      acc = fma(Ar[c], x[c], acc);
    }
    double sq = fin ? sg * acc * acc : __builtin_nan("");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
      if (o < P) sq += __shfl_xor(sq, o);
    if (r == 0 && k < f.K) out[(size_t)s * L.ld_cost[si] + k] = sq / temp;
  }
}

// one thread per (sample, factor) of a non-polynomial set
__device__ __forceinline__ void scost_point_body(const SampleCostList& L, const int si, const int blk) {
  const FactorDev& f = L.f[si];
  const int64_t item = (int64_t)blk * SCOST_THREADS + threadIdx.x;
  if (item >= (int64_t)f.K * L.S) return;
  const int k = (int)(item % f.K);
  const size_t s = (size_t)(item / f.K);
  const double* xs = L.X + s * ((size_t)L.T * L.n) + (size_t)L.start[si][k] * L.n;
  bool fin = true;
  for (int c = 0; c < f.d; ++c) fin = fin && scost_finite(xs[c]);
  double* cost = L.cost[si];
  double* clr = L.clr[si];
  double psi = __builtin_nan(""), cl = __builtin_nan("");
  if (fin) hinge_psi_clearance(f, k, xs, cost != nullptr, clr != nullptr, psi, cl);
  if (cost) cost[s * L.ld_cost[si] + k] = psi / f.temperature[k];
  if (clr) clr[s * L.ld_clr[si] + k] = cl;
}

template <int NM>
__global__ __launch_bounds__(SCOST_THREADS) void sample_cost_kernel(SampleCostList L) {
  int si = 0;
  while (si + 1 < L.nsets && (int)blockIdx.x >= L.boff[si + 1]) ++si;
  const int blk = (int)blockIdx.x - L.boff[si];
  if (!psi_kind_is<PSI_SUMSQ>(L.f[si].kind)) { scost_point_body(L, si, blk); return; }
  if constexpr (NM >= 8) {
    if (2 * L.f[si].d <= NM) { scost_sumsq_body<NM / 2>(L, si, blk); return; }   // the unary set beside a binary one
  }
  scost_sumsq_body<NM>(L, si, blk);
}

struct SampleCostReduceArgs {
  int Kt, Kc;
  const double* cost;   // [S][Kt] or null
  const double* clr;    // [S][Kc] or null
  double* J;            // [S]
  double* clr_min;      // [S]
};

__global__ __launch_bounds__(256) void sample_cost_reduce_kernel(SampleCostReduceArgs a) {
  __shared__ double red[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  if (a.cost) {
    const double* row = a.cost + (size_t)j * a.Kt;
    double s = 0.0;
    for (int i = tid; i < a.Kt; i += 256) s += row[i];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) red[tid] += red[tid + w];
      __syncthreads();
    }
    if (tid == 0) a.J[j] = red[0];
  }
  if (a.clr) {
    __syncthreads();
    const double* row = a.clr + (size_t)j * a.Kc;
    // NaN-propagating minimum: a minimum has no rounding, so any order gives the same bits
    auto nmin = [](double p, double q) { return (p != p || q != q) ? __builtin_nan("") : (q < p ? q : p); };
    double v = __builtin_inf();
    for (int i = tid; i < a.Kc; i += 256) v = nmin(v, row[i]);
    red[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) red[tid] = nmin(red[tid], red[tid + w]);
      __syncthreads();
    }
    if (tid == 0) a.clr_min[j] = red[0];
  }
}

}  // namespace gvi
