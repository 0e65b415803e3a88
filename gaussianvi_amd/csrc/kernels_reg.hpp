// Lane-per-point moments for every psi kind that is not a polynomial (and for sum-of-squares sets without an SGPR instance):
//   moments_generic_kernel   any d <= 32, any psi kind, host-evaluated psi included: the reference-shaped fallback
//   Psi* policies            what a kind loads into LDS once per factor and how it evaluates psi at one point (PsiQuad, PsiRange1D,
//                            PsiHingeSdf, PsiHingeSeg, PsiHingeBalls, PsiBoxHinge); routes.hpp names them by tag only
//   reg_body / moments_reg_kernel<D, Psi, FULL>   accumulators in registers; kernels_sreg.hpp and kernels_block.hpp call reg_body
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "factor_lds.hpp"
#include "mom_args.hpp"
#include "psi_point.hpp"

namespace gvi {

// ---------------------------------------------------------------------------------------------
// moments_generic_kernel: any d (<= 32), any psi kind.  Block = 256 threads handles one factor and a
// range of points in sub-chunks of 256: stage 1 (thread = point) expands x = mu + S z, evaluates
// psi and parks [z, 1] and c = w psi in LDS; stage 2 (thread = output pair (a,b)) accumulates
// sum_i c_i zh_i[a] zh_i[b].  LDS-bound; it is the reference-shaped fallback and the parity
// cross-check for the register kernel.
// ---------------------------------------------------------------------------------------------
constexpr int GEN_MAX_OUT = 3;   // outputs per thread: npairs(d) <= 768 -> d <= 37

__global__ __launch_bounds__(GEN_BS) void moments_generic_kernel(MomArgs a) {
  if (pred_skip(a.pred, a.pred_val)) return;
  extern __shared__ double sm[];
  const FactorDev& f = a.f;
  const int d = f.d, m = f.m, k = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
  const GenericLds L{d, m};                // region by region (factor_lds.hpp)
  const int dz = L.dz();
  double* zs = sm + L.zs();                // [256][dz]   z and the constant 1
  double* xs = zs + (L.xs() - L.zs());     // [256][dz]   x = mu + S z
  double* cs = xs + (L.cs() - L.xs());     // [256]
  double* Ssh = cs + (L.Ssh() - L.cs());   // [d][d]
  double* mush = Ssh + (L.mush() - L.Ssh());   // [d]
  double* Ash = mush + (L.Ash() - L.mush());   // [m][d]
  double* bsh = Ash + (L.bsh() - L.Ash());     // [m]
  double* gsh = bsh + (L.gsh() - L.bsh());     // [m]
  for (int e = tid; e < d * d; e += GEN_BS) Ssh[e] = f.S[(size_t)k * d * d + e];
  for (int e = tid; e < d; e += GEN_BS) mush[e] = a.mu[(size_t)k * d + e];
  for (int e = tid; e < m * d; e += GEN_BS) Ash[e] = f.A[(size_t)k * m * d + e];
  for (int e = tid; e < m; e += GEN_BS) { bsh[e] = f.b[(size_t)k * m + e]; gsh[e] = f.sgn[(size_t)k * m + e]; }
  const int npo = a.full ? npairs(d) : 1;
  int oa[GEN_MAX_OUT], ob[GEN_MAX_OUT];
  double acc[GEN_MAX_OUT];
#pragma unroll
  for (int o = 0; o < GEN_MAX_OUT; ++o) {
    acc[o] = 0.0;
    const int j = tid + o * GEN_BS;
    int pa_ = d, pb_ = d;                   // j == 0 -> (1,1)
    if (j >= 1 && j <= d) { pa_ = j - 1; pb_ = d; }
    else if (j > d) {
      int rem = j - 1 - d, row = 0;
      while (row < d && rem >= d - row) { rem -= d - row; ++row; }
      pa_ = row; pb_ = row + rem;
    }
    oa[o] = pa_; ob[o] = pb_;
  }
  double csum = 0.0;
  const int64_t i0 = (int64_t)chunk * a.chunk;
  const int64_t i1 = (i0 + a.chunk < f.Np) ? i0 + a.chunk : f.Np;
  __syncthreads();
  for (int64_t base = i0; base < i1; base += GEN_BS) {
    const int64_t i = base + tid;
    double* zr = zs + tid * dz;
    double* xr = xs + tid * dz;
    double wi = 0.0;
    if (i < i1) {
      wi = f.w[i];
      for (int c = 0; c < d; ++c) zr[c] = f.Zt[(size_t)c * f.Np + i];
    } else {
      for (int c = 0; c < d; ++c) zr[c] = 0.0;
    }
    zr[d] = 1.0;
    double psi = 0.0;
    if (i < f.N) {
      for (int r = 0; r < d; ++r) {
        double x = mush[r];
        for (int c = 0; c < d; ++c) x += Ssh[r * d + c] * zr[c];
        xr[r] = x;
      }
      if (a.psi_ext) psi = a.psi_ext[(size_t)k * f.N + i];
      else if (psi_kind_is<PSI_RAW>(f.kind)) psi = psi_point(f, k, xr);
      else {
        for (int r = 0; r < m; ++r) {
          double u = bsh[r];
          for (int c = 0; c < d; ++c) u += Ash[r * d + c] * xr[c];
          psi += gsh[r] * u * u;
        }
      }
    }
    const double c = wi * psi;
    cs[tid] = c;
    csum += c;
    __syncthreads();
    if (a.full) {
#pragma unroll
      for (int o = 0; o < GEN_MAX_OUT; ++o) {
        if (tid + o * GEN_BS < npo) {
          double s = acc[o];
          const int pa_ = oa[o], pb_ = ob[o];
          for (int t = 0; t < GEN_BS; ++t) s += cs[t] * zs[t * dz + pa_] * zs[t * dz + pb_];
          acc[o] = s;
        }
      }
    }
    __syncthreads();
  }
  double* out = a.partial + ((size_t)k * a.nchunk + chunk) * npo;
  if (a.full) {
#pragma unroll
    for (int o = 0; o < GEN_MAX_OUT; ++o)
      if (tid + o * GEN_BS < npo) out[tid + o * GEN_BS] = acc[o];
  } else {
    cs[tid] = csum;
    __syncthreads();
    for (int s = GEN_BS / 2; s > 0; s >>= 1) {
      if (tid < s) cs[tid] += cs[tid + s];
      __syncthreads();
    }
    if (tid == 0) out[0] = cs[0];
  }
}

// ---------------------------------------------------------------------------------------------
// moments_reg_kernel<D, Psi, FULL>: the hot kernel.  Block = 4 waves = 4 consecutive factors over
// the same range of points (so a Z chunk is fetched once per block into L1/L2 and reused by the
// four waves).  Lane owns points i = base + lane: d coalesced 8-byte loads from the dimension-major
// table, psi through the factor's LDS-resident H (wave-uniform broadcast reads), and all
// (d+1)(d+2)/2 z-space accumulators in registers.  Cross-lane reduction once per wave: 16 accumulators
// at a time through a padded LDS tile, then two xor-shuffles.  No atomics: partials are written per
// (factor, chunk) and summed in fixed order by epilogue_kernel.
// ---------------------------------------------------------------------------------------------
template <int D, int M>
struct PsiQuad {
  static constexpr int LDS = M * D + 2 * M;
  static constexpr bool GUARD = false;
  __device__ static void load(const MomArgs& a, int k, double* hs, int lane) {
    for (int e = lane; e < M * D; e += 64) hs[e] = a.f.H[(size_t)k * M * D + e];
    if (lane < M) {
      hs[M * D + lane] = a.f.u0[(size_t)k * M + lane];
      hs[M * D + M + lane] = a.f.sgn[(size_t)k * M + lane];
    }
  }
  __device__ static double eval(const double (&z)[D], const double* hs, const MomArgs&) {
    double u[M];                      // M independent FMA chains (column-outer order)
#pragma unroll
    for (int r = 0; r < M; ++r) u[r] = hs[M * D + r];
#pragma unroll
    for (int c = 0; c < D; ++c) {
#pragma unroll
      for (int r = 0; r < M; ++r) u[r] = fma(hs[c * M + r], z[c], u[r]);
    }
    double psi = 0.0;
#pragma unroll
    for (int r = 0; r < M; ++r) psi = fma(hs[M * D + M + r] * u[r], u[r], psi);
    return psi;
  }
};

struct PsiRange1D {
  static constexpr int LDS = 8;
  static constexpr bool GUARD = true;
  __device__ static void load(const MomArgs& a, int k, double* hs, int lane) {
    if (lane == 0) { hs[0] = a.mu[k]; hs[1] = a.f.S[k]; }
    if (lane < 5) hs[2 + lane] = a.f.raw[(size_t)k * a.f.raw_stride + lane];
  }
  __device__ static double eval(const double (&z)[1], const double* hs, const MomArgs&) {
    return psi_range_1d(hs + 2, fma(hs[1], z[0], hs[0]));
  }
};

// nonlinear obstacle costs: pose = (mu + S z)[0:NPOSE] (NPOSE rows of S in LDS), SDF look-ups straight from L2
template <int D, int KIND>
struct PsiHingeSdf {
  static constexpr int NPOSE = psi_kind_lead(KIND);
  static constexpr int NPAR = KIND == KIND_HINGE_SDF_2D_BODY ? 6 : 3;
  static constexpr int LDS = NPOSE * D + NPOSE + NPAR;
  static constexpr bool GUARD = false;
  __device__ static void load(const MomArgs& a, int k, double* hs, int lane) {
    if (lane < NPOSE * D) hs[lane] = a.f.S[(size_t)k * D * D + lane];       // rows 0 .. NPOSE-1 of S
    if (lane < NPOSE) hs[NPOSE * D + lane] = a.mu[(size_t)k * D + lane];
    if (lane < NPAR) hs[NPOSE * D + NPOSE + lane] = a.f.raw[(size_t)k * a.f.raw_stride + lane];
  }
  __device__ static double eval(const double (&z)[D], const double* hs, const MomArgs& a) {
    double pose[NPOSE];
    readout_q<D, NPOSE>(hs, z, pose);                                       // (S rows | mu) is a (G | g) block
    const double* p = hs + NPOSE * D + NPOSE;
    if (KIND == KIND_HINGE_SDF_2D) return psi_hinge_sdf2d(a.f, p, pose[0], pose[1]);
    if (KIND == KIND_HINGE_SDF_2D_BODY) return psi_hinge_sdf2d_body(a.f, p, pose[0], pose[1], pose[NPOSE - 1]);
    return psi_hinge_sdf3d(a.f, p, pose[0], pose[1], pose[NPOSE - 1]);
  }
};
template <int D> using PsiHingeSdf2D = PsiHingeSdf<D, KIND_HINGE_SDF_2D>;

// Obstacle factor on a segment (hinge_sdf_seg_points): psi needs only the J check points, and at a sigma point
// x = mu + S z they are q_j = (W_j mu + c_j) + (W_j S) z.  load forms G = W S (J P rows of D) and g = W mu + c ONCE per
// (factor, chunk) into the wave's LDS slice -- J P D dot products of length D shared by the 64 lanes, from a.f.S (row-major)
// and the raw block; eval is then P D FMAs against wave-uniform LDS reads plus one grid look-up per check point, and the full
// x is never formed.  J is a run-time field (f.seg_J): the loop over j stays a loop, the FMAs inside it are unrolled.
// hs: [J][P (D + 1)] = (G_j [P][D] | g_j [P]) in the raw block's own order, then [sigma, eps, r] at SEG_MAX_J P (D + 1).
template <int D, int P>
struct PsiHingeSeg {
  static constexpr int STRIDE = P * (D + 1);
  static constexpr int LDS = SEG_MAX_J * STRIDE + 3;
  static constexpr bool GUARD = false;
  __device__ static void load(const MomArgs& a, int k, double* hs, int lane) {
    const double* raw = a.f.raw + (size_t)k * a.f.raw_stride;
    const double* S = a.f.S + (size_t)k * D * D;
    const double* mu = a.mu + (size_t)k * D;
    const int J = a.f.seg_J < SEG_MAX_J ? a.f.seg_J : SEG_MAX_J;      // the host admits 1 .. SEG_MAX_J; keeps the LDS slice
    readout_fold<D, P>(ReadoutView{raw, P, D, J, READOUT_SEG}, S, mu, hs, lane);
    if (lane < 3) hs[SEG_MAX_J * STRIDE + lane] = raw[lane];
  }
  __device__ static double eval(const double (&z)[D], const double* hs, const MomArgs& a) {
    const double sigma = hs[SEG_MAX_J * STRIDE], thr = hs[SEG_MAX_J * STRIDE + 1] + hs[SEG_MAX_J * STRIDE + 2];
    const int J = a.f.seg_J < SEG_MAX_J ? a.f.seg_J : SEG_MAX_J;
    double cost = 0.0;
#pragma unroll 1
    for (int j = 0; j < J; ++j) {
      double q[P];
      readout_q<D, P>(hs + j * STRIDE, z, q);
      const double sd = P == 2 ? sdf2d_lookup(a.f, q[0], q[1]) : sdf3d_lookup(a.f, q[0], q[1], q[P - 1]);
      cost += hinge_sq(sd, thr, 1.0, sigma);
    }
    return cost;
  }
};

// Moving balls (hinge_balls_points, balls_psi.hpp).  As for PsiHingeSeg, load forms G_j = W_j S and
// g_j = W_j mu + c_j once per (factor, chunk), so eval pays P D FMAs per check point and never forms x.  load also COMPACTS the
// slots: the M non-empty ones come first, M is wave-uniform, and eval's loop over balls runs M times.  The centres
// o_m + tau_j v_m are formed in load per (check point, active ball) -- 64 P doubles of LDS at most instead of P FMAs per
// (sigma point, check point, ball) in eval.  Per active ball eval forms the squared distance and compares it with
// (eps + r + R_m)^2; only inside that branch is the fp64 square root taken, and the value is hinge_sq's own clamp of
// eps + r - (sqrt(dist^2) - R_m): the pretest skips work, it decides nothing.  No grid pointer is touched.
// hs: [SEG_MAX_J][P (D + 1)] = (G_j [P][D] | g_j [P]) | sigma, eps + r, M, - | [BALLS_SLOTS] (R_m, (eps + r + R_m)^2) |
//     [SEG_MAX_J][BALLS_SLOTS][P] centres.
template <int D, int P>
struct PsiHingeBalls {
  static constexpr int STRIDE = P * (D + 1);
  static constexpr int HEAD = SEG_MAX_J * STRIDE;
  static constexpr int RB = HEAD + 4;
  static constexpr int CEN = RB + 2 * BALLS_SLOTS;
  static constexpr int LDS = CEN + SEG_MAX_J * BALLS_SLOTS * P;
  static constexpr bool GUARD = false;
  static_assert(SEG_MAX_J * BALLS_SLOTS <= 64, "load places one (check point, slot) pair per lane");
  static_assert((4 * LDS + 4 * 16 * 65) * 8 < 64 * 1024, "static LDS of a block of moments_reg_kernel");
  __device__ static void load(const MomArgs& a, int k, double* hs, int lane) {
    const double* raw = a.f.raw + (size_t)k * a.f.raw_stride;
    const double* S = a.f.S + (size_t)k * D * D;
    const double* mu = a.mu + (size_t)k * D;
    const int J = a.f.seg_J < SEG_MAX_J ? a.f.seg_J : SEG_MAX_J;      // the host admits 1 .. SEG_MAX_J; keeps the LDS slice
    const ReadoutView v{raw, P, D, J, READOUT_BALLS};
    readout_fold<D, P>(v, S, mu, hs, lane);
    const double* balls = v.balls();
    const double thr = raw[1] + raw[2];
    if (lane < J * BALLS_SLOTS) {                                     // lane = (check point j, slot m)
      const int j = lane / BALLS_SLOTS, m = lane - j * BALLS_SLOTS;
      const double* b = balls + m * (2 * P + 1);
      const double R = b[2 * P];
      if (!balls_slot_empty(R)) {
        int rank = 0;                                                 // non-empty slots before m
        for (int q = 0; q < m; ++q) rank += balls_slot_empty(balls[q * (2 * P + 1) + 2 * P]) ? 0 : 1;
        const double tau = v.tau(j);
#pragma unroll
        for (int r = 0; r < P; ++r) hs[CEN + (j * BALLS_SLOTS + rank) * P + r] = fma(tau, b[P + r], b[r]);
        if (j == 0) {
          const double t = thr + R;                                   // t <= 0: no distance is below it
          hs[RB + 2 * rank] = R;
          hs[RB + 2 * rank + 1] = t > 0.0 ? t * t : -1.0;
        }
      }
    }
    if (lane == 0) {
      int M = 0;
      for (int q = 0; q < BALLS_SLOTS; ++q) M += balls_slot_empty(balls[q * (2 * P + 1) + 2 * P]) ? 0 : 1;
      hs[HEAD] = raw[0];
      hs[HEAD + 1] = thr;
      hs[HEAD + 2] = (double)M;
    }
  }
  __device__ static double eval(const double (&z)[D], const double* hs, const MomArgs& a) {
    const double sigma = hs[HEAD], thr = hs[HEAD + 1];
    const int M = __builtin_amdgcn_readfirstlane((int)hs[HEAD + 2]);
    const int J = a.f.seg_J < SEG_MAX_J ? a.f.seg_J : SEG_MAX_J;
    double cost = 0.0;
#pragma unroll 1
    for (int j = 0; j < J; ++j) {
      double q[P];
      readout_q<D, P>(hs + j * STRIDE, z, q);
      const double* cen = hs + CEN + j * BALLS_SLOTS * P;
      double sd = INFINITY;
#pragma unroll 1
      for (int m = 0; m < M; ++m) {
        double d2 = 0.0;
#pragma unroll
        for (int r = 0; r < P; ++r) {
          const double e = q[r] - cen[m * P + r];
          d2 = fma(e, e, d2);
        }
        if (d2 < hs[RB + 2 * m + 1]) sd = fmin(sd, sqrt(d2) - hs[RB + 2 * m]);
      }
      cost += hinge_sq(sd, thr, 1.0, sigma);
    }
    return cost;
  }
};
// The tag the instance lists hand out for a hinge on a signed distance is PsiHingeSdf<D, KIND> (routes.hpp); for the two
// analytic kinds it IS the policy above.
template <int D> struct PsiHingeSdf<D, KIND_HINGE_BALLS_2D> : PsiHingeBalls<D, 2> {};
template <int D> struct PsiHingeSdf<D, KIND_HINGE_BALLS_3D> : PsiHingeBalls<D, 3> {};

// Limits on the slice itself (HINGE_BOX, box_moments.hpp).  hs: S [D][D] | mu [D] | sigma [D] | upper threshold hi - eps [D] |
// lower threshold lo + eps [D], an infinite threshold for a side that is off.  eval forms x_i = mu_i + s_i z only for a
// coordinate with a finite side (a wave-uniform test on LDS values): a set that limits the velocities of a state pays for
// those rows of S only.
template <int D>
struct PsiBoxHinge {
  static constexpr int LDS = D * D + 4 * D;
  static constexpr bool GUARD = false;
  __device__ static void load(const MomArgs& a, int k, double* hs, int lane) {
    const double* p = a.f.raw + (size_t)k * a.f.raw_stride;
    for (int e = lane; e < D * D; e += 64) hs[e] = a.f.S[(size_t)k * D * D + e];
    if (lane < D) {
      hs[D * D + lane] = a.mu[(size_t)k * D + lane];
      hs[D * D + D + lane] = p[lane];
      hs[D * D + 2 * D + lane] = p[3 * D + lane] - p[D + lane];
      hs[D * D + 3 * D + lane] = p[2 * D + lane] + p[D + lane];
    }
  }
  __device__ static double eval(const double (&z)[D], const double* hs, const MomArgs&) {
    double cost = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double up = hs[D * D + 2 * D + i], dn = hs[D * D + 3 * D + i];
      if (up < INFINITY || dn > -INFINITY) {
        double x = hs[D * D + i];
#pragma unroll
        for (int c = 0; c < D; ++c) x = fma(hs[i * D + c], z[c], x);
        const double eu = x - up, ed = dn - x;           // -inf on a side that is off
        const double sg = hs[D * D + D + i];
        if (eu > 0.0) cost += sg * eu * eu;
        if (ed > 0.0) cost += sg * ed * ed;
      }
    }
    return cost;
  }
};

// (bx, by): the block's position in the (ceil(K / 4), nchunk) grid of the set -- the launch's own blockIdx, or a virtual one
// when several sets share a launch (moments_planar3_kernel).  hs_: [4][Psi::LDS], red_: [4][16][65] doubles of LDS.
// kfix >= 0 (factor_block3_kernel): the calling wave takes chunk byfix of factor kfix (idle when kfix >= K or byfix >= nchunk);
// (bx, by) are then unused.  Same points per (factor, chunk), same sums.
template <int D, typename Psi, bool FULL>
__device__ __forceinline__ void reg_body(const MomArgs& a, const int bx, const int by_, double* hs_, double* red_, const int kfix = -1,
                                         const int byfix = 0) {
  constexpr int NP = FULL ? (D + 1) * (D + 2) / 2 : 1;
  constexpr int NB = (NP + 15) / 16;
  double (*hs)[Psi::LDS] = (double (*)[Psi::LDS])hs_;
  double (*red)[16][65] = (double (*)[16][65])red_;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = kfix >= 0 ? kfix : bx * 4 + wave;
  const int by = kfix >= 0 ? byfix : by_;
  const bool active = k < a.f.K && by < a.nchunk;
  if (active) Psi::load(a, k, hs[wave], lane);
  __syncthreads();
  double acc[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) acc[j] = 0.0;
  const int64_t Np = a.f.Np;
  const int64_t i0 = (int64_t)by * a.chunk;
  const int64_t i1 = (i0 + a.chunk < Np) ? i0 + a.chunk : Np;
  const double* __restrict__ Zt = a.f.Zt;
  const double* __restrict__ w = a.f.w;
  if (active) {
    for (int64_t i = i0 + lane; i < i1; i += 64) {
      double z[D];
#pragma unroll
      for (int c = 0; c < D; ++c) z[c] = Zt[(size_t)c * Np + i];
      // padded tail (i >= N) carries w = 0, z = 0; the select keeps a non-finite psi(mu) out
      const double cw = i < a.f.N ? w[i] * Psi::eval(z, hs[wave], a) : 0.0;
      acc[0] += cw;
      if (FULL) {
        int q = 1 + D;
#pragma unroll
        for (int c = 0; c < D; ++c) {
          const double t = cw * z[c];
          acc[1 + c] += t;
#pragma unroll
          for (int e = c; e < D; ++e) { acc[q] = fma(t, z[e], acc[q]); ++q; }
        }
      }
    }
  }
  double* out = a.partial + ((size_t)(active ? k : 0) * a.nchunk + by) * NP;
#pragma unroll
  for (int bb = 0; bb < NB; ++bb) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (bb * 16 + j < NP) red[wave][j][lane] = acc[bb * 16 + j];
    __syncthreads();
    const int j = lane & 15, part = lane >> 4;
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < 16; ++t) s += red[wave][j][part * 16 + t];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (active && lane < 16 && bb * 16 + lane < NP) out[bb * 16 + lane] = s;
    __syncthreads();
  }
}

template <int D, typename Psi, bool FULL>
__global__ __launch_bounds__(256) void moments_reg_kernel(MomArgs a) {
  if (pred_skip(a.pred, a.pred_val)) return;
  __shared__ double hs[4 * Psi::LDS];
  __shared__ double red[4 * 16 * 65];
  reg_body<D, Psi, FULL>(a, (int)blockIdx.x, (int)blockIdx.y, hs, red);
}

}  // namespace gvi
