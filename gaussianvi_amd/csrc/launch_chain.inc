// Launch helpers of the chain (block-tridiagonal) operations and of the per-set scatter / gather.  A fragment of the library's
// one translation unit (gvi_hip.hip); not a stand-alone header.
//
//   holds      ChainWs and ensure_chain_ws; TrialMix and make_chain_args; chain_rules; run_chain; run_bt_factor, run_bt_solve;
//              run_scatter, run_gather; check_pass_args
//   relies on  host_ctx.inc (gvi_ctx, FactorSet, DevMem, fail / HIPCK / GVICK, StageScope); chain_launch.hpp / chain_plan.hpp
//   defines    no entry point

namespace {

// workspace of one chain operation (kernels_chain.hpp); two operations are in flight together in the dual launches, so
// there are two: `which` = 0 (the factorisations, every stand-alone operation) or 1 (the parked gradient solve)
struct ChainWs { double* ws; int* wsi; };
gvi_status ensure_chain_ws(gvi_ctx* c, int which, ChainWs& w) {
  const int NP = chain_padded(c->n);
  if (!NP) return fail(c, GVI_ERR_UNSUPPORTED, "state_dim > 16");
  DevMem& Wb = which ? c->Wbuf2 : c->Wbuf;
  DevMem& Ib = which ? c->Ibuf2 : c->Ibuf;
  HIPCK(c, Wb.ensure(chain_ws_doubles(c->T, NP) * 8));
  HIPCK(c, Ib.ensure(chain_lp_entries(c->T) * sizeof(int)));
  w.ws = Wb.d();
  w.wsi = (int*)Ib.p;
  return GVI_OK;
}

// trial precision formed inside the first pass of a factorisation (see ChainArgs::mix*): out = chain + step (V - chain).
// V and out are [D | U] in one buffer each: the kernels derive the U parts.
struct TrialMix { const double* V; double* out; double step; };

ChainArgs make_chain_args(gvi_ctx* c, const ChainWs& w, const double* D, const double* U, const double* rhs, double scale, bool need_back,
                          double* SigD, double* SigU, double* x, double* hld, const TrialMix* mix = nullptr) {
  ChainArgs a{};
  a.T = c->T; a.n = c->n; a.need_back = need_back ? 1 : 0;
  a.D = D; a.U = U; a.rhs = rhs; a.rhs_scale = scale;
  a.ws = w.ws; a.wsi = w.wsi;
  a.SigD = SigD; a.SigU = SigU; a.x = x; a.hld = hld;
  a.pred = c->pipe.pred; a.pred_val = c->pipe.pred_val;
  a.mixV = mix ? mix->V : nullptr;
  a.mixOut = mix ? mix->out : nullptr; a.mix_step = mix ? mix->step : 0.0;
  return a;
}

// the chain's switches as this context set them (chain_plan.hpp); merge holds where the launch also gets hand-over words
ChainRules chain_rules(const gvi_ctx* c) { return {c->opt.chain_wave, c->opt.asm_dense, c->opt.chain_pair, c->opt.chain_merge}; }

gvi_status run_chain(gvi_ctx* c, const ChainArgs& a0, const ChainArgs& a1, bool on0, bool on1, const AsmList* AL = nullptr) {
  hipStream_t st = c->stream;
  StageScope scope(c, STAGE_CHAIN);
  ChainSync sy;
  if (c->opt.chain_merge) {
    constexpr unsigned RING = 64;
    if (!c->chain_sync.p) {
      HIPCK(c, c->chain_sync.ensure(RING * 2 * sizeof(unsigned)));
      // (once per context) on the launch stream, then waited for: the chain kernels run on a non-blocking stream, which a
      // clear on the null stream would not be ordered before
      HIPCK(c, hipMemsetAsync(c->chain_sync.p, 0, RING * 2 * sizeof(unsigned), st));
      HIPCK(c, hipStreamSynchronize(st));
    }
    if (++c->chain_seq == 0) ++c->chain_seq;       // 0 is the cleared state of a word
    sy.seq = c->chain_seq;
    sy.words = (unsigned*)c->chain_sync.p + 2 * (sy.seq % RING);
    sy.fault = c->opt.chain_merge_fault ? 0x40000000u : 0u;
  }
  const hipError_t e = chain_launch(c->n, chain_rules(c), a0, a1, on0, on1, st, AL, sy);
  if (e == hipErrorInvalidValue) return fail(c, GVI_ERR_UNSUPPORTED, "chain kernels: block size / LDS budget");
  HIPCK(c, e);
  return GVI_OK;
}

// log-det (+ optionally marginals) of the chain (D, U) device arrays
gvi_status run_bt_factor(gvi_ctx* c, const double* D, const double* U, double* SigD, double* SigU, double* hld) {
  ChainWs w;
  GVICK(ensure_chain_ws(c, 0, w));
  const ChainArgs a0 = make_chain_args(c, w, D, U, nullptr, 1.0, SigD != nullptr, SigD, SigU, nullptr, hld);
  return run_chain(c, a0, a0, true, false);
}

gvi_status run_bt_solve(gvi_ctx* c, const double* D, const double* U, const double* rhs, double scale, double* x, int ws = 0) {
  ChainWs w;
  GVICK(ensure_chain_ws(c, ws, w));
  const ChainArgs a1 = make_chain_args(c, w, D, U, rhs, scale, false, nullptr, nullptr, x, nullptr);
  return run_chain(c, a1, a1, false, true);
}

gvi_status run_scatter(gvi_ctx* c, FactorSet& s, const double* Vdmu, const double* Vddmu, double* g, double* D, double* U) {
  ScatterArgs a;
  a.T = c->T; a.n = c->n; a.d = s.d; a.K = s.K;
  a.start = s.dstart.i(); a.ptr = s.dptr.i(); a.idx = s.didx.i();
  a.Vdmu = Vdmu; a.Vddmu = Vddmu; a.g = g; a.D = D; a.U = U;
  const int64_t total = (int64_t)c->T * (c->n + 2 * c->n * c->n);
  hipLaunchKernelGGL(bt_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, a);
  HIPCK(c, hipGetLastError());
  return GVI_OK;
}

gvi_status run_gather(gvi_ctx* c, FactorSet& s, const double* mu, const double* SigD, const double* SigU,
                      double* mu_k, double* Sigma_k) {
  const int64_t total = (int64_t)s.K * (s.d + s.d * s.d);
  if (total == 0) return GVI_OK;
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, s.K, s.d, c->n,
                     s.dstart.i(), mu, SigD, SigU, mu_k, Sigma_k);
  HIPCK(c, hipGetLastError());
  return GVI_OK;
}

gvi_status check_pass_args(gvi_ctx* c, FactorSet* s, const void* mu, const void* Sigma) {
  if (!c) return GVI_ERR_ARG;
  if (!s) return fail(c, GVI_ERR_ARG, "bad set id");
  if (!mu || !Sigma) return fail(c, GVI_ERR_ARG, "mu / Sigma is NULL");
  return GVI_OK;
}

}  // namespace
