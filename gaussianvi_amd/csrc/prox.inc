// The update rule of a context and the proximal (JKO) rule's gradients, trial and step.  A fragment of the library's one
// translation unit, included by gvi_hip.hip inside its extern "C" bracket; not a stand-alone header.
//
//   relies on  host_ctx.inc (grad_buf, ngd_invalidate); launch_factor.inc (launch_prep); ngd_stage.inc (ngd_check,
//              ngd_flush_gather, ngd_refresh, ngd_cost_local, ngd_cost_finish); ngd_iter.inc (ngd_moments_full, ngd_scatter,
//              gvi_ngd_cost, gvi_ngd_accept)
//   defines    gvi_ngd_set_update_rule; gvi_prox_gradients, gvi_prox_trial, gvi_prox_step; gvi_ngd_set_mode

gvi_status gvi_ngd_set_update_rule(gvi_ctx* ctx, int rule) {
  if (!ctx || (rule != GVI_RULE_NGD && rule != GVI_RULE_PROX_JKO)) return GVI_ERR_ARG;
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  ctx->update_rule = rule;
  for (auto& s : ctx->sets) { s->unit_temperature = rule == GVI_RULE_PROX_JKO; s->prep_slot = -1; }
  ngd_invalidate(ctx);
  return GVI_OK;
}

// factor-level JKO increments at step h for every set (moments at the current proposal), assembled into exch0[gcur]:
// g = joint dmu, [D | U] = joint dprecision (proxgd/ProxGVI-GH-impl.h:43-60: plain sums, no solve)
gvi_status gvi_prox_gradients(gvi_ctx* ctx, double h) {
  GVICK(ngd_check(ctx));
  if (ctx->update_rule != GVI_RULE_PROX_JKO) return fail(ctx, GVI_ERR_STATE, "call gvi_ngd_set_update_rule(GVI_RULE_PROX_JKO) first");
  if (!(h > 0.0)) return fail(ctx, GVI_ERR_ARG, "step must be positive");
  HIPCK(ctx, hipSetDevice(ctx->device));
  NgdState& g = ctx->ngd;
  g.grad_valid = false;
  GVICK(ngd_flush_gather(ctx, g.cur));
  GVICK(ngd_moments_full(ctx, g.cur));                    // Vdmu = b, Vddmu = S at unit temperature; f.Lam = Lam_k
  for (auto& sp : ctx->sets) {
    FactorSet& s = *sp;
    if (s.K == 0) continue;
    const size_t K = s.K, d = s.d, dd = d * d;
    HIPCK(ctx, s.jko_half.ensure(K * dd * 8));
    HIPCK(ctx, s.jko_S.ensure(K * dd * 8));
    HIPCK(ctx, s.jko_Sinv.ensure(K * dd * 8));
    HIPCK(ctx, s.jko_Lam.ensure(K * dd * 8));
    JkoArgs a;
    a.K = s.K; a.d = s.d; a.h = h; a.Vdmu = s.Vdmu.d(); a.Vddmu = s.Vddmu.d(); a.Sigma = s.Sigma_k[g.cur].d();
    a.Lam = s.Lam.d(); a.Shalf = s.jko_half.d(); a.LamNew = s.jko_Lam.d();
    hipLaunchKernelGGL(jko_half_kernel, dim3(s.K), dim3(64), jko_half_lds_bytes(s.d), ctx->stream, a);
    FactorDev f = s.dev(ctx->opt);                         // spectral map of Sig_half into scratch (no psi operands)
    f.m = 0; f.S = s.jko_S.d(); f.Sinv = s.jko_Sinv.d(); f.Lam = s.jko_Lam.d(); f.H = nullptr; f.Hq = nullptr; f.u0 = nullptr;
    f.jko_h = h;
    f.chol = 0;                                            // the JKO map is a function of the eigenvalues
    GVICK(launch_prep(ctx, f, nullptr, s.jko_half.d(), ctx->stream));
    hipLaunchKernelGGL(jko_finish_kernel, dim3((unsigned)((K * dd + 255) / 256)), dim3(256), 0, ctx->stream, a);
    HIPCK(ctx, hipGetLastError());
  }
  GVICK(ngd_scatter(ctx, g.cur, g.gcur));
  g.grad_valid = true;
  g.grad_slot = g.cur;
  return GVI_OK;
}

// trial of the proximal rule: mu + step dmu, Lam + step dprecision (proxgd/ProxGVI-GH-impl.h:24-41)
gvi_status gvi_prox_trial(gvi_ctx* ctx, double step, double* new_cost) {
  GVICK(ngd_check(ctx));
  if (ctx->update_rule != GVI_RULE_PROX_JKO) return fail(ctx, GVI_ERR_STATE, "call gvi_ngd_set_update_rule(GVI_RULE_PROX_JKO) first");
  HIPCK(ctx, hipSetDevice(ctx->device));
  NgdState& g = ctx->ngd;
  if (!(g.grad_valid && g.grad_slot == g.cur)) return fail(ctx, GVI_ERR_STATE, "call gvi_prox_gradients first");
  const size_t Tn = (size_t)ctx->T * ctx->n, bt = bt_count(ctx);
  const int c = g.cur, t = 1 - c;
  const GradBuf e = grad_buf(ctx, g.gcur);             // g = joint dmu, [D | U] = joint dprecision (gvi_prox_gradients)
  hipLaunchKernelGGL(trial_kernel, dim3((unsigned)((Tn + bt + 255) / 256)), dim3(256), 0, ctx->stream, (int64_t)Tn, (int64_t)bt,
                     step, g.mu[c].d(), e.g, g.Lam[c].d(), e.D, g.mu[t].d(), g.Lam[t].d(), 1);
  HIPCK(ctx, hipGetLastError());
  g.cost_valid[t] = false;
  GVICK(ngd_refresh(ctx, t));
  g.have_trial = true;
  GVICK(ngd_cost_local(ctx, t));
  return ngd_cost_finish(ctx, t, new_cost);
}

// ProxGVIGH::optimize body (proxgd/ProxGVI-GH-impl.h:121-202): gradients once at step = base, trial B uses base^B,
// the first decreasing trial is accepted; after max_backtrack failures the last trial is accepted anyway (:177-184)
gvi_status gvi_prox_step(gvi_ctx* ctx, double step_size_base, int max_backtrack, double* cost_iter, int* decreased,
                         double* new_cost, int* ntrials) {
  GVICK(ngd_check(ctx));
  if (ctx->update_rule != GVI_RULE_PROX_JKO) return fail(ctx, GVI_ERR_STATE, "call gvi_ngd_set_update_rule(GVI_RULE_PROX_JKO) first");
  double c0 = 0.0;
  GVICK(gvi_ngd_cost(ctx, &c0));
  if (cost_iter) *cost_iter = c0;
  GVICK(gvi_prox_gradients(ctx, step_size_base));
  int B = 1, cnt = 0, ok = 0;
  double c1 = c0;
  while (true) {
    GVICK(gvi_prox_trial(ctx, std::pow(step_size_base, B), &c1));
    ok = c1 < c0;
    if (!ok) { ++B; ++cnt; }
    if (ok || cnt > max_backtrack) { GVICK(gvi_ngd_accept(ctx)); break; }
  }
  if (decreased) *decreased = ok;
  if (new_cost) *new_cost = c1;
  if (ntrials) *ntrials = cnt + (ok ? 1 : 0);
  return GVI_OK;
}

gvi_status gvi_ngd_set_mode(gvi_ctx* ctx, int speculate, int fuse_trial) {
  if (!ctx) return GVI_ERR_ARG;
  if (fuse_trial < 0 || fuse_trial > 2) return fail(ctx, GVI_ERR_ARG, "fuse_trial must be 0, 1 or 2");
  ctx->speculate = speculate != 0;
  ctx->opt.fuse_trial = fuse_trial;
  ctx->ngd.last_first_accepted = true;
  return GVI_OK;
}
