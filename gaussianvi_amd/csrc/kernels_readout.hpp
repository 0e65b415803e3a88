// moments_readout_kernel: Gaussian moments of the obstacle kinds on linear read-outs (PSI_READOUT) by a dense, positive-weight
// tensor Gauss-Hermite rule in the P-dimensional read-out space instead of the sparse rule in the d-dimensional slice
// (readout_moments.hpp has the mathematics and the arithmetic without lane structure).  Opt-in per set:
// gvi_factors_set_readout_rule.  Writes the packed one-chunk layout of the closed-form kernels, so the epilogue is shared.
//
// One wave owns one factor and loops over its J check points; a block is 1 or 4 such waves (blockDim.x / 64), each on its own
// slice of the dynamic LDS and without a workgroup barrier: no wave reads what another wrote.
//   per check point j:
//     lanes form G_j = W_j S entry by entry into the wave's slice; C_j = G_j G_j^T, g_j and the Cholesky factor with its drop
//     rule are computed by every lane alike (wave-uniform, <= 6 d-long sums from LDS); lanes c < d turn column c of G_j into
//     column c of Gam_j in place; the lanes then stride over the order^nkept nodes (node index = lane + 64 pass), each adds its
//     1 + P + P (P + 1) / 2 sums in registers, and a fixed-shape 64-bit DPP wave sum (wave_sum_f64, kernels_orbit.hpp) follows.
//     (h_j, H_j) are parked in LDS beside Gam_j; e0_j is added to m0 in ascending j.
//   then the lanes stride over the npairs(d) outputs, each a sum over j ascending (phase 2 of moments_halfspace_closed_kernel).
// No atomics and no reduction whose shape depends on K or the grid: a factor's result is the same bits whatever K it is launched
// with and from run to run.  full = 0 writes m0 only and skips Gam.  LDS per wave: 32 + J (P d + P + P P) doubles (<= 7 KB).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "kernels_orbit.hpp"
#include "mom_args.hpp"
#include "psi_point.hpp"
#include "readout_moments.hpp"

namespace gvi {

struct ReadoutArgs {
  MomArgs a;
  const double* rule;        // [nodes (order) | weights (order)] of the 1-D rule, uploaded by gvi_factors_set_readout_rule
  int order;
};

__host__ __device__ inline size_t readout_park_doubles(int P, int d) { return (size_t)P * d + P + (size_t)P * P; }
__host__ __device__ inline size_t readout_lds_doubles(int P, int d, int J) { return 2 * READOUT_MAX_ORDER + (size_t)J * readout_park_doubles(P, d); }

template <int P, int CLS>
__global__ __launch_bounds__(256) void moments_readout_kernel(ReadoutArgs ra) {
  const MomArgs& a = ra.a;
  if (pred_skip(a.pred, a.pred_val)) return;
  extern __shared__ double rosm[];
  const FactorDev& f = a.f;
  const int d = f.d, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, order = ra.order;
  const int J = readout_check_points(CLS, f.seg_J);
  const int64_t kw = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (kw >= f.K) return;                                       // the whole wave; nothing below waits for another wave
  const int k = (int)kw;
  const int per = (int)readout_park_doubles(P, d);
  double* nodes = rosm + (size_t)wave * readout_lds_doubles(P, d, J);      // [16]
  double* weights = nodes + READOUT_MAX_ORDER;                             // [16]
  double* park = weights + READOUT_MAX_ORDER;                              // [J][Gam (P d) | h (P) | H (P P)]
  if (lane < order) {
    nodes[lane] = ra.rule[lane];
    weights[lane] = ra.rule[order + lane];
  }
  const double* p = f.raw + (size_t)k * f.raw_stride;
  const double* mu = a.mu + (size_t)k * d;
  const double* S = f.S + (size_t)k * d * d;
  // Not through ReadoutView: its form of the same addresses took the <3, SEG / BALLS> instances from 127 / 125 to 129 VGPRs, one
  // occupancy step; P * (d + 1) spelled out keeps the SEG instances' code what it was (profiles/psi_point_refactor.txt).
  const int stride = CLS == READOUT_BALLS ? readout_stride(CLS, P, d) : P * (d + 1);
  const double* balls = p + 3 + J * stride;                    // READOUT_BALLS only
  const double sigma = p[0], thr = p[1] + p[2];
  const bool full = a.full != 0;
  bool bad = false;
  double m0 = 0.0;
  for (int j = 0; j < J; ++j) {
    const double* W = CLS == READOUT_LEAD ? nullptr : p + 3 + j * stride;
    const double* cvec = CLS == READOUT_LEAD ? nullptr : W + P * d;
    double* Gam = park + (size_t)j * per;
    for (int e = lane; e < P * d; e += 64) Gam[e] = readout_G_entry(W, S, d, e / d, e % d);
    wave_lds_sync();
    double C[P * P], g[P];
#pragma unroll
    for (int r = 0; r < P; ++r) {
      g[r] = readout_g_entry(W, cvec, mu, d, r);
#pragma unroll
      for (int t = 0; t <= r; ++t) {
        double v = 0.0;
        for (int c = 0; c < d; ++c) v = fma(Gam[r * d + c], Gam[t * d + c], v);
        C[r * P + t] = v;
        C[t * P + r] = v;
      }
    }
    const ReadoutChol<P> ch = readout_chol<P>(C);
    ReadoutSums<P> s;
    readout_zero(s);
    if (ch.ok) {                                               // wave-uniform
      if (full) {
        wave_lds_sync();                                       // every lane has read G_j
        for (int c = lane; c < d; c += 64) readout_gamma_col<P>(ch, Gam + c, d);
      }
      const int nn = readout_node_count<P>(ch, order);
      for (int idx = lane; idx < nn; idx += 64) {
        double xi[P], q[P];
        const double om = readout_node<P>(ch, order, nodes, weights, idx, xi);
        readout_point<P>(ch, g, xi, q);
        double fv;
        if constexpr (CLS == READOUT_BALLS) {
          fv = readout_f_balls<P>(p, balls, W[P * (d + 1)], q);
        } else if constexpr (P == 2) {
          fv = hinge_sq(sdf2d_lookup(f, q[0], q[1]), thr, 1.0, sigma);
        } else {
          fv = hinge_sq(sdf3d_lookup(f, q[0], q[1], q[2]), thr, 1.0, sigma);
        }
        readout_accumulate<P>(s, om, xi, fv);
      }
    } else {
      bad = true;
    }
    s.e0 = wave_sum_f64(s.e0);
    m0 += s.e0;
    if (full) {
#pragma unroll
      for (int e = 0; e < P; ++e) s.h[e] = wave_sum_f64(s.h[e]);
#pragma unroll
      for (int e = 0; e < P * (P + 1) / 2; ++e) s.H[e] = wave_sum_f64(s.H[e]);
      if (lane == 0) readout_store_sums<P>(ch, s, Gam + P * d, Gam + P * d + P);
    }
  }
  wave_lds_sync();
  const int npo = full ? npairs(d) : 1;
  double* out = a.partial + (size_t)k * a.nchunk * npo;
  const double nan = __builtin_nan("");
  if (lane == 0) out[0] = bad ? nan : m0;
  if (!full) return;
  for (int o = 1 + lane; o < npo; o += 64) {
    double v = 0.0;
    if (o <= d) {
      const int c = o - 1;
      for (int j = 0; j < J; ++j) {
        const double* Gam = park + (size_t)j * per;
        const double* hs = Gam + P * d;
#pragma unroll
        for (int r = 0; r < P; ++r) v = fma(Gam[r * d + c], hs[r], v);
      }
    } else {
      int rem = o - 1 - d, row = 0;
      while (rem >= d - row) { rem -= d - row; ++row; }
      const int col = row + rem;
      for (int j = 0; j < J; ++j) {
        const double* Gam = park + (size_t)j * per;
        const double* Hs = Gam + P * d + P;
#pragma unroll
        for (int r = 0; r < P; ++r) {
          double t = 0.0;
#pragma unroll
          for (int l = 0; l < P; ++l) t = fma(Hs[r * P + l], Gam[l * d + col], t);
          v = fma(Gam[r * d + row], t, v);
        }
      }
      if (rem == 0) v += m0;
    }
    out[o] = bad ? nan : v;
  }
}

}  // namespace gvi
