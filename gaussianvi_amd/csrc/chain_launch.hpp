// Host side of kernels_chain.hpp: binds a plan of chain_plan.hpp (chain_decide: which launches, in which form, with how many
// workgroups and how much LDS) to kernel arguments and launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

#include "chain_plan.hpp"
#include "kernels_chain.hpp"
#include "kernels_chain_wave.hpp"

namespace gvi {

// Raise the dynamic-LDS limit of the kernels of block size N once per device.
template <int N>
inline hipError_t chain_allow_lds() {
  static bool done[64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
  const int lim = (int)CHAIN_LDS_LIMIT;
  if ((e = hipFuncSetAttribute((const void*)chain_forward_kernel<N, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lim)) != hipSuccess) return e;
  if ((e = hipFuncSetAttribute((const void*)chain_forward_kernel<N, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lim)) != hipSuccess) return e;
  if ((e = hipFuncSetAttribute((const void*)chain_backward_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, lim)) != hipSuccess) return e;
  if ((e = hipFuncSetAttribute((const void*)chain_top_back_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, lim)) != hipSuccess) return e;
  if constexpr (N == 6) {
    if ((e = hipFuncSetAttribute((const void*)chain_forward_readlane_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lim)) != hipSuccess) return e;
    if ((e = hipFuncSetAttribute((const void*)chain_forward_readlane_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lim)) != hipSuccess) return e;
    if ((e = hipFuncSetAttribute((const void*)chain_top_back_readlane_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lim)) != hipSuccess) return e;
  }
  if (dev >= 0 && dev < 64) done[dev] = true;
  return hipSuccess;
}

// The hand-over words of a merged top + backward launch (kernels_chain.hpp::chain_top_back_kernel): two device words (one per
// operation) and a sequence number the caller advances with every chain_launch.  words == nullptr: separate launches.
struct ChainSync { unsigned* words = nullptr; unsigned seq = 0; unsigned fault = 0; };   // fault: test hook (ChainArgs::sync_fault)

// The kernels of block size N in a form: N = 6 has the v_readlane kernels beside the templated ones (two-row bodies).
template <int N>
struct ChainKernels {
  void (*forward)(ChainArgs, ChainArgs, int, AsmList);
  void (*top)(ChainArgs, ChainArgs, int, AsmList);
  void (*top_back)(ChainArgs, ChainArgs, int, AsmList, ChainPassDev, int, int);
  explicit ChainKernels(ChainForm form) : forward(chain_forward_kernel<N, false>), top(chain_forward_kernel<N, true>), top_back(chain_top_back_kernel<N>) {
    if constexpr (N == 6) {
      if (form == ChainForm::Readlane) { forward = chain_forward_readlane_kernel<false>; top = chain_forward_readlane_kernel<true>; top_back = chain_top_back_readlane_kernel; }
    }
  }
};

// Issues every launch of a plan (at least one) from its record.  a0: the factorisation, a1: the pivoted solve.
template <int N>
inline hipError_t chain_issue(const ChainLaunchPlan& pl, ChainArgs a0, ChainArgs a1, hipStream_t st, const AsmList& AL, const ChainSync& sync) {
  if (pl.launch[0].kernel != ChainKernel::Wave) {               // (the lane-per-node kernel takes no LDS)
    const hipError_t e = chain_allow_lds<N>();
    if (e != hipSuccess) return e;
  }
  auto set = [](ChainArgs& a, const ChainPass& ps) {
    a.level0 = ps.level0; a.m = ps.m; a.S = ps.S; a.first = ps.first; a.par = ps.par; a.lp_off = ps.lp_off;
  };
  a0.sync = a1.sync = nullptr; a0.sync_seq = a1.sync_seq = 0; a0.sync_fault = a1.sync_fault = sync.fault;
  const dim3 threads(pl.threads);
  for (int i = 0; i < pl.nlaunch; ++i) {
    const ChainLaunch& l = pl.launch[i];
    const ChainKernels<N> k(l.form);
    const dim3 grid(l.nb);
    const ChainPass& ps = pl.pass[l.pass];                      // (a Wave launch has none: the kernel runs the whole chain)
    if (l.kernel != ChainKernel::Wave) { set(a0, ps); set(a1, ps); }
    switch (l.kernel) {
      case ChainKernel::Wave:
        hipLaunchKernelGGL(chain_wave_kernel, grid, threads, 0, st, a0, a1, l.nb0, AL);
        break;
      case ChainKernel::Forward: {
        const auto forward = ps.top ? k.top : k.forward;
        hipLaunchKernelGGL(forward, grid, threads, l.lds, st, a0, a1, l.nb0, AL);
        break;
      }
      case ChainKernel::TopBack: {
        const ChainPass& pc = pl.pass[l.carried];
        const ChainPassDev cp{pc.level0, pc.m, pc.S, pc.first, pc.par, pc.lp_off};
        a0.sync = sync.words; a1.sync = sync.words + 1; a0.sync_seq = a1.sync_seq = sync.seq;
        hipLaunchKernelGGL(k.top_back, grid, threads, l.lds, st, a0, a1, l.nb0, AL, cp, l.nbt, l.nb0c);
        a0.sync = a1.sync = nullptr;
        break;
      }
      case ChainKernel::Backward:
        hipLaunchKernelGGL((chain_backward_kernel<N>), grid, threads, l.lds, st, a0, a1, l.nb0);
        break;
    }
  }
  return hipGetLastError();
}

// How chain_launch classified the launches that carried an assemble list, per process: [0] the batched load path (ASM_DENSE),
// [1] the generic set loop.  Read-only bookkeeping for the tests (gvi_debug_asm_launches); no kernel sees it.
inline std::atomic<long long>* chain_asm_launches() { static std::atomic<long long> c[2]; return c; }

// what chain_decide reads of an operation.  a: the arguments of an operation that is on (both run the same chain shape)
inline ChainFacts chain_facts(int n, const ChainArgs& a, bool on0, bool back0, bool on1, const AsmList* AL) {
  AsmSetFacts sets[2] = {};
  const int nsets = AL ? AL->nsets : 0;
  for (int i = 0; i < nsets && i < 2; ++i) sets[i] = {AL->s[i].K, AL->s[i].d, AL->s[i].nsp, AL->s[i].Vdmu && AL->s[i].Vddmu};
  return {a.T, n, on0, back0, on1, AL != nullptr, chain_asm_dense(sets, nsets, n)};
}

// on0: factorisation a0 (log-det; + selected inverse when a0.need_back); on1: pivoted solve a1.  Both: side by side in the
// same launches.  n: the caller's block size (a0.n / a1.n are set here).  AL: the factor sets of an assemble-on-load (a0.asm_on /
// a1.asm_on), else null.  sync: rules.merge holds only with its words.  Returns hipErrorInvalidValue, with nothing launched,
// when the plan refuses the shape (block size, or a pass that does not fit LDS).
inline hipError_t chain_launch(int n, ChainRules rules, ChainArgs a0, ChainArgs a1, bool on0, bool on1, hipStream_t st,
                               const AsmList* AL = nullptr, const ChainSync& sync = ChainSync{}) {
  rules.merge = rules.merge && sync.words;
  const ChainLaunchPlan pl = chain_decide(chain_facts(n, on0 ? a0 : a1, on0, on0 && a0.need_back, on1, AL), rules);
  if (pl.status != ChainStatus::Ok) return hipErrorInvalidValue;
  a0.n = a1.n = n;
  a0.pair = a1.pair = rules.pair ? 1 : 0;
  if (pl.assemble == ChainAsm::Off) a0.asm_on = a1.asm_on = 0;
  else {
    if (pl.assemble == ChainAsm::Dense) {          // the first pass's batched load path (kernels_chain.hpp, AsmDense)
      if (a0.asm_on) a0.asm_on = ASM_DENSE;
      if (a1.asm_on) a1.asm_on = ASM_DENSE;
    }
    ++chain_asm_launches()[pl.assemble == ChainAsm::Dense ? 0 : 1];
  }
  if (pl.nlaunch == 0) return hipSuccess;
  const AsmList none{};
  const AsmList& L = AL ? *AL : none;
  switch (chain_padded(n)) {
    case 1: return chain_issue<1>(pl, a0, a1, st, L, sync);
    case 2: return chain_issue<2>(pl, a0, a1, st, L, sync);
    case 3: return chain_issue<3>(pl, a0, a1, st, L, sync);
    case 4: return chain_issue<4>(pl, a0, a1, st, L, sync);
    case 6: return chain_issue<6>(pl, a0, a1, st, L, sync);
    case 8: return chain_issue<8>(pl, a0, a1, st, L, sync);
    case 12: return chain_issue<12>(pl, a0, a1, st, L, sync);
    case 16: return chain_issue<16>(pl, a0, a1, st, L, sync);
  }
  return hipErrorInvalidValue;
}

}  // namespace gvi
