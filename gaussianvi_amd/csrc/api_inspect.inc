// Entry points that look into a context or switch it: counters, read-back of the iteration's state and gradients, profiles,
// options, debug logs.  A fragment of the library's one translation unit, included by gvi_hip.hip inside its extern "C"
// bracket; not a stand-alone header.
//
//   relies on  host_ctx.inc (grad_buf, StageScope's records, d2h / sync, get_set, ngd_invalidate); launch_factor.inc
//              (fused_launches, block3_launches); ngd_stage.inc (ngd_check); ngd_iter.inc (ngd_flush_assemble, ngd_join_solve);
//              options.hpp (option_set); routes.hpp (geometry_code, route_force_of_variant)
//   defines    gvi_ngd_counters; gvi_debug_asm_launches, gvi_debug_fused_launches, gvi_debug_block3_launches;
//              gvi_ngd_exchange, gvi_ngd_get_state, gvi_ngd_get_gradients; gvi_profile_enable / _last / _stages / _geometry;
//              gvi_set_option; gvi_debug_cost_log, gvi_debug_products; gvi_set_variant

gvi_status gvi_ngd_counters(gvi_ctx* ctx, int64_t* full_passes, int64_t* cost_passes, int reset) {
  if (!ctx) return GVI_ERR_ARG;
  if (full_passes) *full_passes = ctx->ngd.n_full_pass;
  if (cost_passes) *cost_passes = ctx->ngd.n_cost_pass;
  if (reset) ctx->ngd.n_full_pass = ctx->ngd.n_cost_pass = 0;
  return GVI_OK;
}

gvi_status gvi_debug_asm_launches(int64_t* dense, int64_t* generic) {
  if (dense) *dense = chain_asm_launches()[0].load();
  if (generic) *generic = chain_asm_launches()[1].load();
  return GVI_OK;
}

gvi_status gvi_debug_fused_launches(int64_t counts[3]) {
  if (!counts) return fail(nullptr, GVI_ERR_ARG, "NULL");
  for (int i = 0; i < 3; ++i) counts[i] = fused_launches()[i].load();
  return GVI_OK;
}

gvi_status gvi_debug_block3_launches(int64_t* count) {
  if (!count) return fail(nullptr, GVI_ERR_ARG, "NULL");
  *count = block3_launches().load();
  return GVI_OK;
}

gvi_status gvi_ngd_exchange(gvi_ctx* ctx, int which, void** dev_ptr, int64_t* count) {
  GVICK(ngd_check(ctx));
  if (!dev_ptr || !count) return fail(ctx, GVI_ERR_ARG, "NULL argument");
  GVICK(ngd_flush_assemble(ctx, 0));                    // the caller is going to read / reduce the buffers themselves
  GVICK(ngd_flush_assemble(ctx, 1));
  if (which == 0) { *dev_ptr = grad_buf(ctx, ctx->ngd.gcur).g; *count = (int64_t)((size_t)ctx->T * ctx->n + bt_count(ctx)); }
  else if (which == 1) { *dev_ptr = ctx->ngd.exch1.p; *count = 1; }
  else if (which == 2) { *dev_ptr = grad_buf(ctx, 1 - ctx->ngd.gcur).g; *count = (int64_t)((size_t)ctx->T * ctx->n + bt_count(ctx)); }
  else return fail(ctx, GVI_ERR_ARG, "which must be 0, 1 or 2");
  return GVI_OK;
}

gvi_status gvi_ngd_get_state(gvi_ctx* ctx, double* mu, double* D, double* U, double* SigD, double* SigU) {
  GVICK(ngd_check(ctx));
  HIPCK(ctx, hipSetDevice(ctx->device));
  NgdState& g = ctx->ngd;
  const size_t T = ctx->T, n = ctx->n, nn = n * n;
  const int i = g.cur;
  if (mu) GVICK(d2h(ctx, mu, g.mu[i].p, T * n * 8));
  if (D) GVICK(d2h(ctx, D, g.Lam[i].p, T * nn * 8));
  if (U && T > 1) GVICK(d2h(ctx, U, g.Lam[i].d() + T * nn, (T - 1) * nn * 8));
  if (SigD) GVICK(d2h(ctx, SigD, g.Sig[i].p, T * nn * 8));
  if (SigU && T > 1) GVICK(d2h(ctx, SigU, g.Sig[i].d() + T * nn, (T - 1) * nn * 8));
  return sync(ctx);
}

gvi_status gvi_ngd_get_gradients(gvi_ctx* ctx, double* dmu, double* dD, double* dU, double* gq, double* VD, double* VU) {
  GVICK(ngd_check(ctx));
  HIPCK(ctx, hipSetDevice(ctx->device));
  NgdState& g = ctx->ngd;
  const size_t T = ctx->T, n = ctx->n, nn = n * n, bt = bt_count(ctx);
  if (!(g.grad_valid)) return fail(ctx, GVI_ERR_STATE, "no gradients computed for the current proposal");
  GVICK(ngd_join_solve(ctx, g.gcur));
  if (dmu) GVICK(d2h(ctx, dmu, g.dmu2[g.gcur].p, T * n * 8));
  const GradBuf e = grad_buf(ctx, g.gcur);
  if (gq) GVICK(d2h(ctx, gq, e.g, T * n * 8));
  std::vector<double> V, L;
  if (dD || dU || VD || VU) {
    V.resize(bt);
    GVICK(d2h(ctx, V.data(), e.D, bt * 8));             // [V_D | V_U] in one copy
  }
  if (dD || dU) {
    L.resize(bt);
    GVICK(d2h(ctx, L.data(), g.Lam[g.cur].p, bt * 8));
  }
  GVICK(sync(ctx));
  if (VD) memcpy(VD, V.data(), T * nn * 8);
  if (VU && T > 1) memcpy(VU, V.data() + T * nn, (T - 1) * nn * 8);
  if (dD) for (size_t j = 0; j < T * nn; ++j) dD[j] = V[j] - L[j];          // dprecision = Vddmu - Lambda
  if (dU) for (size_t j = 0; j < (T - 1) * nn; ++j) dU[j] = V[T * nn + j] - L[T * nn + j];
  return GVI_OK;
}

gvi_status gvi_profile_enable(gvi_ctx* ctx, int on) {
  if (!ctx) return GVI_ERR_ARG;
  ctx->profile = on != 0;
  ctx->profile_all = on == 2;
  ctx->profile_every = on == 3 ? 8 : 1;
  ctx->ngd.profile_count = 0;
  for (auto& s : ctx->sets) s->ev_set[0] = s->ev_set[1] = false;
  return GVI_OK;
}

gvi_status gvi_profile_last(gvi_ctx* ctx, int set_id, int what, float* ms) {
  FactorSet* s = get_set(ctx, set_id);
  if (!s || !ms || what < 0 || what > 1) return GVI_ERR_ARG;
  if (!s->ev_set[what]) return fail(ctx, GVI_ERR_STATE, "no profiled launch recorded");
  HIPCK(ctx, hipEventSynchronize(s->ev[what][1]));
  HIPCK(ctx, hipEventElapsedTime(ms, s->ev[what][0], s->ev[what][1]));
  return GVI_OK;
}

gvi_status gvi_profile_stages(gvi_ctx* ctx, int on, float* mean_us, int* counts) {
  if (!ctx) return GVI_ERR_ARG;
  HIPCK(ctx, hipSetDevice(ctx->device));
  if (mean_us || counts) {
    GVICK(sync(ctx));
    double sum[STAGE_COUNT] = {0, 0, 0};
    int cnt[STAGE_COUNT] = {0, 0, 0};
    for (auto& r : ctx->stage_recs) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { sum[r.stage] += ms; ++cnt[r.stage]; }
    }
    for (int i = 0; i < STAGE_COUNT; ++i) {
      if (mean_us) mean_us[i] = cnt[i] ? (float)(1e3 * sum[i] / cnt[i]) : 0.f;
      if (counts) counts[i] = cnt[i];
    }
  }
  for (auto& r : ctx->stage_recs) { ctx->stage_pool.push_back(r.e0); ctx->stage_pool.push_back(r.e1); }
  ctx->stage_recs.clear();
  ctx->stage_prof = on != 0;
  return GVI_OK;
}

gvi_status gvi_profile_geometry(gvi_ctx* ctx, int set_id, int* variant, int* nchunk, int64_t* chunk) {
  FactorSet* s = get_set(ctx, set_id);
  if (!s) return GVI_ERR_ARG;
  if (variant) *variant = geometry_code(s->last.route, s->last.fused_pair, s->closed_form);
  if (nchunk) *nchunk = s->last.nchunk;
  if (chunk) *chunk = s->last.chunk;
  return GVI_OK;
}

gvi_status gvi_set_option(gvi_ctx* ctx, const char* name, int value) {
  if (!ctx || !name) return GVI_ERR_ARG;
  const std::string n(name);
  if (ctx->ngd.ready) { GVICK(ngd_flush_assemble(ctx, 0)); GVICK(ngd_flush_assemble(ctx, 1)); }
  if (n == "safe_publish") GVICK(sync(ctx));                   // nothing in flight publishes in the other form
  std::string why;
  if (!option_set(ctx->opt, name, value, &why)) return fail(ctx, GVI_ERR_ARG, why);
  // what a switch owes the context beyond its field
  if (n == "safe_publish") for (int q = 0; q < 16; ++q) ctx->host_slot[q] = 0.0;       // the two forms lay the slot out differently
  if (n == "chain_merge") ctx->opt.chain_merge_fault = value == 2;
  for (auto& s : ctx->sets) s->prep_slot = -1;
  ngd_invalidate(ctx);
  return GVI_OK;
}


gvi_status gvi_debug_cost_log(gvi_ctx* ctx, int entries, double* out, double* seq_now) {
  if (!ctx) return GVI_ERR_ARG;
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  if (entries > 0) {
    if (entries & (entries - 1)) return fail(ctx, GVI_ERR_ARG, "entries must be a power of two");
    HIPCK(ctx, ctx->dbg_log.ensure((size_t)entries * 8));
    HIPCK(ctx, hipMemset(ctx->dbg_log.p, 0, (size_t)entries * 8));
    ctx->dbg_mask = entries - 1;
    double* lg = ctx->dbg_log.d();
    HIPCK(ctx, hipMemcpyToSymbol(HIP_SYMBOL(gvi_dbg_mask), &ctx->dbg_mask, sizeof(int)));
    HIPCK(ctx, hipMemcpyToSymbol(HIP_SYMBOL(gvi_dbg_log), &lg, sizeof(double*)));
  } else if (entries == 0 && out) {
    if (!ctx->dbg_mask) return fail(ctx, GVI_ERR_STATE, "cost log not enabled");
    HIPCK(ctx, hipMemcpy(out, ctx->dbg_log.p, (size_t)(ctx->dbg_mask + 1) * 8, hipMemcpyDeviceToHost));
  } else {
    ctx->dbg_mask = 0;
    double* lg = nullptr;
    HIPCK(ctx, hipMemcpyToSymbol(HIP_SYMBOL(gvi_dbg_log), &lg, sizeof(double*)));
  }
  if (seq_now) *seq_now = ctx->seq;
  return GVI_OK;
}

gvi_status gvi_debug_products(gvi_ctx* ctx, int set_id, double* S, double* Sinv, double* Lam, double* H, double* u0) {
  if (!ctx) return GVI_ERR_ARG;
  FactorSet* s = get_set(ctx, set_id);
  if (!s) return GVI_ERR_ARG;
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  const size_t dd = (size_t)s->K * s->d * s->d * 8, md = (size_t)s->K * s->m * s->d * 8, mb = (size_t)s->K * s->m * 8;
  auto get = [&](double* out, const DevMem& src, size_t bytes) {
    if (!out || bytes == 0) return hipSuccess;
    if (!src.p || src.bytes < bytes) return hipErrorInvalidValue;
    return hipMemcpy(out, src.p, bytes, hipMemcpyDeviceToHost);
  };
  HIPCK(ctx, get(S, s->S, dd));
  HIPCK(ctx, get(Sinv, s->Sinv, dd));
  HIPCK(ctx, get(Lam, s->Lam, dd));
  HIPCK(ctx, get(H, s->H, md));
  HIPCK(ctx, get(u0, s->u0, mb));
  return GVI_OK;
}

gvi_status gvi_set_variant(gvi_ctx* ctx, int variant) {
  return ctx && route_force_of_variant(variant, &ctx->force) ? GVI_OK : GVI_ERR_ARG;
}
