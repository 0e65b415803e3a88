// Behind the moments: ordered sum of the chunk partials, back-transform to x-space, Vdmu_k / Vddmu_k  [calculate_partial_V,
// ngd/NGDFactorizedBaseGH.h:53-74].
//   epilogue_body_t / _p / epilogue_body   one wave per factor; epilogue_kernel (one set), epilogue_all_kernel (EpiList: every set)
//   cost_tail_kernel                       per-factor cost + ordered sum + publish for a cost pass, one launch
//   EpiTail, CostList, epi_tail_arrive     the arrival count / last-block sum / publish protocol of the one-launch passes
//   expand_kernel                          X = mu + S z for the host-callback psi route (no epilogue: kept last, where it was)
// LDS carve-up: factor_lds.hpp (EpilogueLds).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "factor_dev.hpp"
#include "factor_lds.hpp"

namespace gvi {

// ---------------------------------------------------------------------------------------------
// epilogue_kernel: one wave per factor.
// ---------------------------------------------------------------------------------------------
struct EpiArgs {
  FactorDev f;
  const double* partial;   // [K][nchunk][npo]
  int nchunk, full;
  double* Ephi;            // [K] or null
  double* cost;            // [K] or null   (E[psi] / T_k)
  double* Vdmu;            // [K][d] or null
  double* Vddmu;           // [K][d][d] or null
  double* E_xmuphi;        // [K][d] or null       raw integrals
  double* E_xxphi;         // [K][d][d] or null
};

// returns the factor's cost E[psi] / T_k (wave-uniform).
// DT = d at compile time (inner products fully unrolled: their LDS loads pipeline) or 0 (any d).  The operands of the
// back-transform (Sinv, Lam; S for the raw integrals) are fetched into LDS in one round trip at the top -- with the
// loads inside the d-long inner loops every product paid d dependent global round trips (profiles/r02_e: 15 us for
// what is ~2 us of arithmetic).  Summation orders are unchanged (c ascending, chunk index ascending).
// phase 0: everything; 1: chunk sums, E[psi] and cost only (Ms stays in LDS); 2: the back-transform after a phase-1 call
// P: the factor's chunk partials ([nchunk][npo]): a.partial + k nchunk npo, or LDS (factor_fused_kernel)
// Zs: S^-T of this factor already in LDS (factor_fused_kernel, Cholesky route; Sigma^-1 = S^-T S^-1 is then re-formed
// here by the prep's own sequence of operations: bit-identical) or null (both fetched here)
template <int DT>
__device__ __forceinline__ double epilogue_body_t(const EpiArgs& a, int k, double* sm, int phase, const double* P, double* Zs = nullptr) {
  const FactorDev& f = a.f;
  const int d = DT ? DT : f.d, dd = d * d, lane = threadIdx.x & 63;      // one wave per factor (the fused kernel runs several per block)
  const int npo = a.full ? npairs(d) : 1;
  const EpilogueLds L{d};       // the epilogue area, region by region (factor_lds.hpp)
  double* Ms = sm + L.Ms();                     // [npo]
  double* M2 = Ms + (L.M2() - L.Ms());          // [d][d]
  double* Tm = M2 + (L.Tm() - L.M2());          // [d][d]
  double* Sv = Zs ? Zs : Tm + (L.Sv() - L.Tm());    // [d][d] Sinv
  double* Lv = Tm + (L.Lv() - L.Tm());          // [d][d] Lam (unused when Zs)
  const double Tk = f.temperature[k];                     // issued with the other loads, used after the chunk sums
  const bool want_v = a.full && (a.Vdmu || a.Vddmu);
  if (want_v && phase != 2 && !Zs) {
    const double* Sinv = f.Sinv + (size_t)k * dd;
    const double* Lam = f.Lam + (size_t)k * dd;
    for (int e = lane; e < dd; e += 64) { Sv[e] = Sinv[e]; Lv[e] = Lam[e]; }
  }
  for (int j = lane; j < npo && phase != 2; j += 64) {
    double s = 0.0;
    for (int c0 = 0; c0 < a.nchunk; c0 += 8) {                   // eight loads in flight, then the ordered sum
      double pv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) pv[q] = c0 + q < a.nchunk ? P[(size_t)(c0 + q) * npo + j] : 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) s += pv[q];                    // fixed order (x + 0.0 == x): deterministic
    }
    Ms[j] = s;
  }
  wave_lds_sync();
  const double m0 = Ms[0];
  const double costk = m0 / Tk;
  if (lane == 0 && phase != 2) {
    if (a.Ephi) a.Ephi[k] = m0;
    if (a.cost) a.cost[k] = costk;
  }
  if (!a.full || phase == 1) return costk;
  for (int e = lane; e < dd; e += 64) {
    const int i = e / d, j = e % d;
    M2[e] = i <= j ? Ms[pair_index(d, i, j)] : Ms[pair_index(d, j, i)];
  }
  wave_lds_sync();
  if (a.Vdmu) {
    for (int i = lane; i < d; i += 64) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < d; ++c) s += Sv[i * d + c] * Ms[1 + c];
      a.Vdmu[(size_t)k * d + i] = s / Tk;
    }
  }
  if (a.Vddmu) {
    for (int e = lane; e < dd; e += 64) {
      const int i = e / d, j = e % d;
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < d; ++c) s += Sv[i * d + c] * M2[c * d + j];
      Tm[e] = s;
    }
    wave_lds_sync();
    for (int e = lane; e < dd; e += 64) {
      const int i = e / d, j = e % d;
      if (i <= j) {           // upper triangle, mirrored (ngd/NGDFactorizedBaseGH.h:71-72)
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < d; ++c) s += Tm[i * d + c] * Sv[j * d + c];     // (W M2) W^T, W = S^-T (symmetric root: W = Sinv)
        double lam;
        if (Zs) {
          lam = 0.0;
#pragma unroll
          for (int c = 0; c < d; ++c) lam = fma(Sv[i * d + c], Sv[j * d + c], lam);   // prep_chol_body: Sigma^-1 = X^T X
        } else lam = Lv[i * d + j];
        const double v = (s - lam * m0) / Tk;
        a.Vddmu[(size_t)k * dd + i * d + j] = v;
        a.Vddmu[(size_t)k * dd + j * d + i] = v;
      }
    }
    wave_lds_sync();
  }
  if (a.E_xmuphi || a.E_xxphi) {
    const double* S = f.S + (size_t)k * dd;
    for (int e = lane; e < dd; e += 64) Sv[e] = S[e];            // Sinv is dead: reuse its slot
    wave_lds_sync();
  }
  if (a.E_xmuphi) {
    for (int i = lane; i < d; i += 64) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < d; ++c) s += Sv[i * d + c] * Ms[1 + c];
      a.E_xmuphi[(size_t)k * d + i] = s;
    }
  }
  if (a.E_xxphi) {
    for (int e = lane; e < dd; e += 64) {
      const int i = e / d, j = e % d;
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < d; ++c) s += Sv[i * d + c] * M2[c * d + j];
      Tm[e] = s;
    }
    wave_lds_sync();
    for (int e = lane; e < dd; e += 64) {
      const int i = e / d, j = e % d;
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < d; ++c) s += Tm[i * d + c] * Sv[j * d + c];
      a.E_xxphi[(size_t)k * dd + e] = s;
    }
  }
  return costk;
}

// the chain shapes of BASELINE.json get unrolled instances; everything else runs the runtime-d body
__device__ __forceinline__ double epilogue_body_p(const EpiArgs& a, int k, double* sm, int phase, const double* P, double* Zs = nullptr) {
  switch (a.f.d) {
    case 2: return epilogue_body_t<2>(a, k, sm, phase, P, Zs);
    case 4: return epilogue_body_t<4>(a, k, sm, phase, P, Zs);
    case 6: return epilogue_body_t<6>(a, k, sm, phase, P, Zs);
    case 8: return epilogue_body_t<8>(a, k, sm, phase, P, Zs);
    case 12: return epilogue_body_t<12>(a, k, sm, phase, P, Zs);
    default: return epilogue_body_t<0>(a, k, sm, phase, P, Zs);
  }
}
__device__ inline double epilogue_body(const EpiArgs& a, int k, double* sm, int phase = 0) {
  return epilogue_body_p(a, k, sm, phase, a.partial + (size_t)k * a.nchunk * (a.full ? npairs(a.f.d) : 1));
}

__global__ __launch_bounds__(64) void epilogue_kernel(EpiArgs a) {
  extern __shared__ double sm[];
  epilogue_body(a, blockIdx.x, sm);
}

struct EpiList {
  int nsets;
  int koff[MAX_SETS + 1];
  EpiArgs e[MAX_SETS];
};

// Tail of a cost pass in ONE launch: per-factor cost = (ordered chunk sum of m0) / T_k for every set, the ordered
// sum over all factors (same order as cost_sum_all_kernel: thread-strided partial sums, then a fixed 256-leaf tree
// per set) into acc[0], and -- single-process iteration only -- the publish into host-mapped memory
// ({cost_sum, half_logdet, sequence}).  Replaces epilogue_all_kernel(full = 0) -> cost_sum_all_kernel -> publish_kernel.
__global__ __launch_bounds__(256) void cost_tail_kernel(EpiList L, double* acc, const double* half_logdet, double* host_out,
                                                        double seq, unsigned* counter) {
  __shared__ double sh[256];
  __shared__ int last;
  // phase 1 (all blocks): per-factor costs to global, one factor per thread
  const int gtid = (int)blockIdx.x * 256 + threadIdx.x, gthreads = (int)gridDim.x * 256;
  for (int si = 0; si < L.nsets; ++si) {
    const EpiArgs& e = L.e[si];
    for (int k = gtid; k < e.f.K; k += gthreads) {
      const double* P = e.partial + (size_t)k * e.nchunk;
      double m0 = 0.0;
      for (int c0 = 0; c0 < e.nchunk; c0 += 8) {                   // eight loads in flight, then the ordered sum
        double p[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j] = c0 + j < e.nchunk ? P[c0 + j] : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) m0 += p[j];                    // fixed order (x + 0.0 == x): deterministic
      }
      e.cost[k] = m0 / e.f.temperature[k];
    }
  }
  // the block that arrives last does the (deterministic, fixed-order) reduction over all factors
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(counter, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();
  // phase 2: the summation order of cost_sum_all_kernel (thread-strided partial sums, 256-leaf tree per set)
  double total = 0.0;
  for (int si = 0; si < L.nsets; ++si) {
    const EpiArgs& e = L.e[si];
    const volatile double* cost = e.cost;
    double s = 0.0;
    for (int k = threadIdx.x; k < e.f.K; k += 256) s += cost[k];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
      __syncthreads();
    }
    total += sh[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *counter = 0u;                       // ready for the next launch (stream-ordered)
    acc[0] = total;
    if (host_out) {
      publish_to_host(host_out, total + half_logdet[0], seq);
    }
  }
}

// Optional tail of the fused-trial iteration: the block that finishes LAST sums the factor costs of every set (the
// association of cost_sum_all_kernel: 256 strided partial sums, then a fixed 256-leaf tree per set -- bit-identical) and
// publishes {cost sum, half log-det, sequence} to host-mapped memory.  Replaces two dependent launches
// (cost_sum_all_kernel, publish_kernel) behind the epilogue.
constexpr int EPI_GROUP = 64;
struct EpiTail {
  int on;
  double* acc;                 // [1] cost sum
  const double* half_logdet;   // [1]
  double* host_out;            // host-mapped {cost_sum, half_logdet, sequence} or null
  double seq;
  unsigned* counter;           // [32 (1 + ceil(blocks / EPI_GROUP))] arrival counters, 128 B apart, zero before the launch
  // pipelined iterations (gvi_ngd_run): the accept decision is ALSO taken on the device, so that the next iteration's
  // launches -- queued before the host has read this cost -- can be predicated on it.  accept[0] <- seq if
  // cost < current cost else 0; cost_dev[slot_trial] <- cost; the current cost is c0_imm or cost_dev[slot_cur].
  const double* pred;          // predicate of THIS launch (device_common.hpp, pred_skip) or null
  double pred_val;
  double* accept;              // null: no device-side decision
  double* cost_dev;            // [2] cost of the state in slot 0 / 1
  int slot_cur, slot_trial;
  int c0_use_imm;
  double c0_imm;
  // option "safe_publish": the arrival counters carry release / acquire order (agent scope) instead of the fence-free
  // protocol (write-through store + vmcnt(0) + relaxed counters) -- an L2 write-back per arriving block, the price list of
  // DESIGN 4.2 -- and the publish takes the checked four-word form (device_common.hpp)
  int safe;
};

// The factor costs of every set, as the tail sums them
struct CostList {
  int nsets;
  double* cost[MAX_SETS];
  int K[MAX_SETS];
};

// Tail protocol, executed by ONE wave of every block (lane = its lane index) after the block's factor cost `costk` is known:
// store it, count the block in; the one that arrives last sums the costs of all sets and publishes.  `last`: one LDS int
// private to the calling wave.
// Cross-block hand-over WITHOUT device-scope fences: on this multi-XCD part a release fence writes the XCD's whole L2
// back (the epilogue has just dirtied megabytes: 2049 blocks x __threadfence() cost ~45 us, measured).  Only the
// factor's cost has to be seen by the last block, so it is stored write-through at agent scope, the wave waits for
// that one store (vmcnt), and the arrival counters are relaxed agent-scope atomics.  Everything else the epilogue
// wrote is consumed by later launches (ordinary end-of-kernel release).
__device__ __forceinline__ void epi_tail_arrive(const CostList& cl, const EpiTail& tail, double* cost_slot, const double costk, const int lane,
                                                const unsigned bid, const unsigned nblocks, int* last) {
  if (lane == 0) {
    __hip_atomic_store(cost_slot, costk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // two-level arrival count: thousands of atomics on ONE address serialise in L2; groups of EPI_GROUP blocks count on
    // their own 128-byte-spaced word, the last of each group counts on the top word
    const unsigned grp = bid / EPI_GROUP, ngrp = (nblocks + EPI_GROUP - 1) / EPI_GROUP;
    const unsigned in_grp = grp + 1 < ngrp ? (unsigned)EPI_GROUP : nblocks - grp * EPI_GROUP;
    unsigned* gc = tail.counter + 32u * (1u + grp);
    int l = 0;
    const bool lastg = tail.safe ? __hip_atomic_fetch_add(gc, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == in_grp - 1
                                 : __hip_atomic_fetch_add(gc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_grp - 1;
    if (lastg) {
      __hip_atomic_store(gc, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch
      // (a single group -- <= EPI_GROUP factors, BASELINE configs[1] -- needs no second level: one atomic round trip less
      // on the chain that ends in the publish)
      l = ngrp == 1 ? 1
                    : (tail.safe ? __hip_atomic_fetch_add(tail.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == ngrp - 1
                                 : __hip_atomic_fetch_add(tail.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ngrp - 1);
    }
    *last = l;
  }
  wave_lds_sync();
  if (!*last) return;
  double total = 0.0;
  // The summation order is that of cost_sum_all_kernel (256 strided partial sums, then a fixed 256-leaf tree per set).
  // All loads of a set's first 8 x 256 factors (per lane: 4 virtual threads x 8) are issued before the first add: the
  // tail is one wave on the critical path of the iteration, and one round trip per virtual thread cost ~6 us.
  for (int s2 = 0; s2 < cl.nsets; ++s2) {
    const double* cost = cl.cost[s2];
    const int K = cl.K[s2];
    double p[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int k = lane + 64 * j + q * 256;
        p[j][q] = k < K ? __hip_atomic_load(cost + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      }
    double vs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                       // virtual thread v = lane + 64 j of the 256-thread kernel
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) s += p[j][q];         // ordered (x + 0.0 == x)
      for (int k0 = lane + 64 * j + 8 * 256; k0 < K; k0 += 8 * 256) {   // K > 2048: further batches of eight
        double pp[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int k = k0 + q * 256;
          pp[q] = k < K ? __hip_atomic_load(cost + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) s += pp[q];
      }
      vs[j] = s;
    }
    // the 256-leaf tree sh[v] += sh[v + w], w = 128 ... 1, with the leaves in registers: the first two levels pair the
    // virtual threads of one lane, the rest are lane shuffles -- the same association as the LDS tree it replaces
    double t = (vs[0] + vs[2]) + (vs[1] + vs[3]);       // w = 128: v += v + 128 ; w = 64: v += v + 64
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) t += __shfl_down(t, w);
    total += __shfl(t, 0);
  }
  if (lane == 0) {
    __hip_atomic_store(tail.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    tail.acc[0] = total;
    const double c1 = total + tail.half_logdet[0];
    if (tail.host_out) publish_to_host(tail.host_out, c1, tail.seq);
    if (tail.accept) {                                    // same comparison as the host's (NaN compares false: rejected)
      const double c0 = tail.c0_use_imm ? tail.c0_imm : tail.cost_dev[tail.slot_cur];
      tail.cost_dev[tail.slot_trial] = c1;
      tail.accept[0] = c1 < c0 ? tail.seq : 0.0;
    }
  }
  wave_lds_sync();
}

__global__ __launch_bounds__(64) void epilogue_all_kernel(EpiList L, EpiTail tail, CostList cl) {
  extern __shared__ double sm[];
  if (pred_skip(tail.pred, tail.pred_val)) return;
  int si = 0;
  while (si + 1 < L.nsets && (int)blockIdx.x >= L.koff[si + 1]) ++si;
  const int kf = (int)blockIdx.x - L.koff[si];
  if (!tail.on) { epilogue_body(L.e[si], kf, sm); return; }
  // With the tail on, the factor's cost goes out FIRST (phase 1: chunk sums only), the last block to arrive sums and
  // publishes, and only then does every block do its back-transform (phase 2): the host has the trial cost -- and
  // launches the next iteration's chain kernels -- while the epilogue's products and the assemble are still running,
  // instead of ~10 us after them.
  const double costk = epilogue_body(L.e[si], kf, sm, 1);
  __shared__ int last;
  epi_tail_arrive(cl, tail, L.e[si].cost + kf, costk, (int)threadIdx.x, blockIdx.x, gridDim.x, &last);
  epilogue_body(L.e[si], kf, sm, 2);
}

// X[k][a][i] = mu_a + sum_b S_ab z_b[i]  (reference CUDA-path layout [factor][dim][point])
__global__ __launch_bounds__(256) void expand_kernel(FactorDev f, const double* __restrict__ mu,
                                                     double* __restrict__ X) {
  const int k = blockIdx.y, d = f.d;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= f.N) return;
  const double* S = f.S + (size_t)k * d * d;
  for (int r = 0; r < d; ++r) {
    double x = mu[(size_t)k * d + r];
    for (int c = 0; c < d; ++c) x += S[r * d + c] * f.Zt[(size_t)c * f.Np + i];
    X[((size_t)k * d + r) * f.N + i] = x;
  }
}

}  // namespace gvi
