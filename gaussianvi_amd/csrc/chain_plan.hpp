// The decisions of the chain stage: how a chain of T blocks of n x n is cut into passes, which kernel family and form runs each
// pass, how many workgroups and how much LDS every launch gets, whether the top pass carries the last segmented pass's backward
// workgroups, which way an assemble-on-load goes, and when the shape is refused.  Everything here is arithmetic on a chain's
// shape and a handful of switches: chain_decide allocates nothing and calls no HIP function, so tests/test_chain_plan_host.py
// runs it on the CPU (tests/stubs/chain_plan_check.cpp, plain and sanitized builds).  chain_launch.hpp binds a plan to kernel
// arguments and launches it; the kernel headers take their sizes from here.  Plain C++17, no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "hd.hpp"

namespace gvi {

// ---- the shape of a chain ----
// compile-time block size a chain of n x n blocks runs at (blocks padded by the identity), 0 = unsupported
inline int chain_padded(int n) {
  for (int N : {1, 2, 3, 4, 6, 8, 12, 16}) if (n <= N) return n >= 1 ? N : 0;
  return 0;
}
inline bool chain_supported(int n) { return chain_padded(n) != 0; }

inline int chain_levels(int T) {
  int L = 0;
  while (((int64_t)1 << L) < T) ++L;
  return L;
}

constexpr int chain_threads(int n) { return n <= 8 ? 1024 : 512; }

constexpr int CHAIN_MATS = 10;   // E, GAt, GBt, NUt, Deff, Ls[2], Rs, SL, SR      each [T][N][N]
constexpr int CHAIN_VECS = 5;    // v, yLs[2], yRs, yeff                           each [T][N]

GVI_HD inline size_t chain_lp_entries(int T) { return (size_t)2 * T + 1024; }
GVI_HD inline size_t chain_ws_doubles(int T, int n) {
  return (size_t)CHAIN_MATS * T * n * n + (size_t)CHAIN_VECS * T * n + chain_lp_entries(T);
}

// the lane-per-node kernel (kernels_chain_wave.hpp): one wave per operation
namespace chain_wave {
constexpr int WN = 2;            // compiled block size (n = 1 is padded by the identity)
constexpr int WT_MAX = 65;
}  // namespace chain_wave

// ---- LDS footprints (doubles) of the pass bodies of kernels_chain.hpp; HAS_E: factorisation, HAS_Y: solve ----
namespace chain {

// doubles of LDS behind the arrays of a two-row pass: the table (64 lanes x 16 bytes), an identity block and a zero block of
// N x N each -- the columns of I, of a missing neighbour's coupling and of a lane outside the tile are LOADED from them like any
// other column (chain_lane_record.hpp)
GVI_HD constexpr int lane_record_doubles(int N) { return 128 + 2 * N * N; }

GVI_HD constexpr size_t fwd_lds_doubles(bool HAS_E, bool HAS_Y, bool TOP, int N, int S, bool rowb) {   // rowb: the two-row form (N = 6) runs this pass
  const int nn = N * N;
  size_t w = (size_t)2 * (S + 1) * nn + (size_t)2 * S * nn;              // Dl, Rl, Ct, NUt
  if (TOP) w += (size_t)3 * S * nn + (HAS_E ? (size_t)S * nn : 0);       // El, GAl, GBl (+ SRt of the backward recursion)
  if (HAS_Y) w += (size_t)2 * (S + 1) * N + (TOP ? (size_t)(2 * S + 1) * N : 0);   // yl, yRl (+ vl, xl)
  return w + N + (N & 1) + 128 + (rowb ? 96 + lane_record_doubles(N) : 0);   // zero block, log-det reduction; two-row form: eliminate2's log-pivot slots, lane records
}
GVI_HD constexpr size_t bwd_lds_doubles(bool HAS_E, int N, int S) {
  const int nn = N * N;
  return (HAS_E ? (size_t)5 * (S + 1) * nn + (size_t)3 * S * nn            // Sg, SL, SLt, SR, SRt ; E, GA, GB
                : (size_t)(S + 1) * N + (size_t)S * N + (size_t)2 * S * nn)   // x, v, GA, GB
         + 2;                                                              // chain_wait's word
}

}  // namespace chain

constexpr size_t CHAIN_LDS_LIMIT = 160 * 1024;   // bytes of dynamic LDS a chain kernel may be given (chain_launch.hpp::chain_allow_lds)

// ---- the pass list ----
struct ChainPass { int level0, m, S, top, first, par, lp_off, blocks; };

// A segmented pass runs at least 3 levels, so a chain of 2^31 states has at most ceil(31 / 3) of them and a top pass; every
// pass but the top one may have a backward launch of its own.
constexpr int CHAIN_MSEG_MIN = 3;
constexpr int CHAIN_MAX_PASSES = 12;
constexpr int CHAIN_MAX_LAUNCHES = 2 * CHAIN_MAX_PASSES - 1;
static_assert(CHAIN_MAX_PASSES >= (31 + CHAIN_MSEG_MIN - 1) / CHAIN_MSEG_MIN + 1, "passes of a chain of 2^31 states");
static_assert(CHAIN_MAX_LAUNCHES == 23, "a forward launch per pass, a backward launch per segmented pass");

struct ChainPasses { ChainPass pass[CHAIN_MAX_PASSES]; int npass; int threads; };

inline ChainPasses chain_passes(int T, int n_actual) {
  const int n = chain_padded(n_actual);
  const int m_seg = n <= 6 ? 5 : (n <= 8 ? 4 : 3);                 // (>= CHAIN_MSEG_MIN)
  // top-pass nodes: the forward arrays and the factors of all of them must fit LDS.  Small blocks leave room for a long top
  // pass, and a chain that fits it is done in ONE launch (the 65-state planar / configs[1] chains: launch floor, not arithmetic)
  const int cap = n <= 2 ? 128 : (n <= 4 ? 64 : (n <= 6 ? 48 : (n <= 8 ? 24 : 8)));
  ChainPasses p{};
  p.threads = chain_threads(n);
  const int nwaves = p.threads / 64, nlevels = chain_levels(T);
  auto alive = [&](int l) { return (int)(((int64_t)T + ((int64_t)1 << l) - 1) >> l); };
  int level0 = 0, lp = 0, par = 0;
  while (alive(level0) > cap) {
    const int S = 1 << m_seg;
    p.pass[p.npass++] = {level0, m_seg, S, 0, level0 == 0, par, lp, alive(level0 + m_seg)};   // blocks = ceil(T / (S << level0))
    lp += p.pass[p.npass - 1].blocks * nwaves;
    level0 += m_seg;
    par ^= 1;
  }
  p.pass[p.npass++] = {level0, nlevels - level0, alive(level0), 1, level0 == 0, par, lp, 1};
  return p;
}

// N = 6: a pass is crowded when its first level has more eliminations than two per SIMD -- the levels on which the two-row form
// puts two nodes into one wave.  Without a crowded level the two-row form is the slower one (also with its lane records, by ~260
// stamped cycles per one-node level where it was ~740; profiles/chain_index_work.txt section 2).
constexpr bool chain_crowded(int S, int threads) { return (S >> 1) > threads / 128; }

// ---- the batched assemble load (kernels_chain.hpp, AsmDense) ----
// what the shape test reads of one factor set of an assemble list: factors, dimension, sparse states, both arrays present
struct AsmSetFacts { int K, d, nsp; bool data; };
// at most ONE binary set (d = 2n) and at most ONE unary set (d = n), neither sparse, every set present with data; set order free
inline bool chain_asm_dense(const AsmSetFacts* s, int nsets, int n) {
  if (nsets < 1 || nsets > 2) return false;
  int nb = 0, nu = 0;
  for (int i = 0; i < nsets; ++i) {
    if (s[i].nsp != 0 || s[i].K < 1 || !s[i].data) return false;
    if (s[i].d == 2 * n) ++nb;
    else if (s[i].d == n) ++nu;
    else return false;
  }
  return nb <= 1 && nu <= 1;
}

// ---- facts and rules -> plan ----
struct ChainFacts {
  int T, n;                    // n: the caller's block size
  bool on0, back0, on1;        // factorisation (log-det); + its selected inverse; pivoted solve, side by side in the same launches
  bool asm_list, asm_dense_shape;    // an assemble list came with the operation; its sets have chain_asm_dense's shape
};
struct ChainRules {
  bool wave = true;            // option chain_wave: short chains of 2 x 2 blocks on the lane-per-node kernel
  bool asm_dense = true;       // option asm_dense: the batched first-pass load where the sets fit it
  bool pair = true;            // option chain_pair: N = 6, the two-row form on crowded passes
  bool merge = false;          // hand-over words are available: top pass + first backward pass in one launch
};

enum class ChainKernel { Wave, Forward, TopBack, Backward };
// Own: the only form of the kernel (every N but 6, the wave and backward kernels); N = 6: the two-row bodies of the templated
// kernels, or the v_readlane kernels
enum class ChainForm { Own, TwoRow, Readlane };
enum class ChainAsm { Off, Generic, Dense };
enum class ChainStatus { Ok, BlockSize, Lds };      // unsupported: no kernel of this block size / a launch does not fit LDS

// The grid of a launch is nb workgroups; [0, nb0) belong to the factorisation.  TopBack: [0, nbt) are the top pass's (the first
// nb0 of them the factorisation's), behind them the carried pass's backward workgroups, the first nb0c of them the factorisation's.
struct ChainLaunch {
  ChainKernel kernel;
  ChainForm form;
  int pass, carried;           // index into ChainLaunchPlan::pass; carried: TopBack only, else -1
  int nb0, nb, nbt, nb0c;
  unsigned lds;                // bytes
};

struct ChainLaunchPlan {
  ChainStatus status;
  ChainAsm assemble;
  int threads;
  int npass, nlaunch;
  ChainPass pass[CHAIN_MAX_PASSES];
  ChainLaunch launch[CHAIN_MAX_LAUNCHES];     // in launch order; none when status != Ok
};

inline ChainLaunchPlan chain_decide(const ChainFacts& f, const ChainRules& r) {
  ChainLaunchPlan p{};
  p.assemble = !f.asm_list ? ChainAsm::Off : (r.asm_dense && f.asm_dense_shape && f.T > 1) ? ChainAsm::Dense : ChainAsm::Generic;
  const int N = chain_padded(f.n);
  if (!N) { p.status = ChainStatus::BlockSize; return p; }
  const bool on0 = f.on0, on1 = f.on1, back0 = on0 && f.back0;
  if (!on0 && !on1) return p;
  if (r.wave && f.n <= chain_wave::WN && f.T >= 1 && f.T <= chain_wave::WT_MAX) {
    p.threads = 64;
    p.launch[p.nlaunch++] = {ChainKernel::Wave, ChainForm::Own, 0, -1, on0 ? 1 : 0, (on0 ? 1 : 0) + (on1 ? 1 : 0), 0, 0, 0u};
    return p;
  }
  const ChainPasses ps = chain_passes(f.T, f.n);
  p.threads = ps.threads;
  p.npass = ps.npass;
  for (int i = 0; i < ps.npass; ++i) p.pass[i] = ps.pass[i];

  auto form = [&](const ChainPass& q) {
    return N != 6 ? ChainForm::Own : (r.pair && chain_crowded(q.S, p.threads)) ? ChainForm::TwoRow : ChainForm::Readlane;
  };
  auto larger = [](size_t a, size_t b) { return a > b ? a : b; };
  // a launch gets the largest footprint of the bodies it runs
  auto fwd_lds = [&](const ChainPass& q) {
    const bool rowb = form(q) == ChainForm::TwoRow;
    return 8 * larger(on0 ? chain::fwd_lds_doubles(true, false, q.top, N, q.S, rowb) : 0, on1 ? chain::fwd_lds_doubles(false, true, q.top, N, q.S, rowb) : 0);
  };
  auto bwd_lds = [&](const ChainPass& q) {
    return 8 * larger(back0 ? chain::bwd_lds_doubles(true, N, q.S) : 0, on1 ? chain::bwd_lds_doubles(false, N, q.S) : 0);
  };
  auto push = [&](ChainKernel k, ChainForm fm, int pass, int carried, int nb0, int nb, int nbt, int nb0c, size_t lds) {
    if (lds > CHAIN_LDS_LIMIT) p.status = ChainStatus::Lds;
    p.launch[p.nlaunch++] = {k, fm, pass, carried, nb0, nb, nbt, nb0c, (unsigned)lds};
  };

  const bool back = back0 || on1;
  const int top = p.npass - 1, last_seg = top - 1;
  // the top pass carries the backward workgroups of the last segmented pass when there is one and the launch's LDS fits
  const size_t lds_merged = last_seg >= 0 ? larger(fwd_lds(p.pass[top]), bwd_lds(p.pass[last_seg])) : 0;
  const bool merged = r.merge && back && last_seg >= 0 && lds_merged <= CHAIN_LDS_LIMIT;
  for (int i = 0; i < top; ++i) {
    const ChainPass& q = p.pass[i];
    const int nb0 = on0 ? q.blocks : 0;
    push(ChainKernel::Forward, form(q), i, -1, nb0, nb0 + (on1 ? q.blocks : 0), 0, 0, fwd_lds(q));
  }
  if (merged) {
    const int blocks = p.pass[last_seg].blocks;
    const int nb0 = on0 ? 1 : 0, nbt = nb0 + (on1 ? 1 : 0), nb0c = back0 ? blocks : 0;
    push(ChainKernel::TopBack, form(p.pass[top]), top, last_seg, nb0, nbt + nb0c + (on1 ? blocks : 0), nbt, nb0c, lds_merged);
  } else {
    push(ChainKernel::Forward, form(p.pass[top]), top, -1, on0 ? 1 : 0, (on0 ? 1 : 0) + (on1 ? 1 : 0), 0, 0, fwd_lds(p.pass[top]));
  }
  for (int i = last_seg - (merged ? 1 : 0); back && i >= 0; --i) {
    const ChainPass& q = p.pass[i];
    const int nb0 = back0 ? q.blocks : 0;
    push(ChainKernel::Backward, ChainForm::Own, i, -1, nb0, nb0 + (on1 ? q.blocks : 0), 0, 0, bwd_lds(q));
  }
  if (p.status != ChainStatus::Ok) p.nlaunch = 0;
  return p;
}

}  // namespace gvi
