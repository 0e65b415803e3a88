// Entry points of the stand-alone operators: one pass over one factor set, and the joint chain operations.  A fragment of the
// library's one translation unit, included by gvi_hip.hip inside its extern "C" bracket; not a stand-alone header.
//
//   holds      upload_pass_inputs; the staging helpers Region / carve, put_chain, stage_chain (posterior_host.inc stages
//              through them too)
//   relies on  host_ctx.inc (gvi_ctx, FactorSet, h2d / d2h / sync, get_set, bt_count, nn_); launch_factor.inc (run_prep,
//              run_moments, run_epilogue); launch_chain.inc (run_bt_factor, run_bt_solve, run_scatter, run_gather,
//              check_pass_args)
//   defines    gvi_moments_dev, gvi_costs_dev, gvi_moments, gvi_raw_moments, gvi_costs, gvi_expand, gvi_moments_from_psi;
//              gvi_bt_assemble, gvi_bt_solve, gvi_bt_logdet, gvi_bt_marginals, gvi_gather_marginals

// ---- per-pass factor operators ----
gvi_status gvi_moments_dev(gvi_ctx* ctx, int set_id, const double* mu, const double* Sigma, double* Ephi,
                           double* Vdmu, double* Vddmu) {
  FactorSet* s = get_set(ctx, set_id);
  GVICK(check_pass_args(ctx, s, mu, Sigma));
  if (psi_kind_is<PSI_NO_DEVICE>(s->kind)) return fail(ctx, GVI_ERR_ARG, "HOST_CALLBACK set: use gvi_expand + gvi_moments_from_psi");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(run_prep(ctx, *s, mu, Sigma));
  int nchunk = 1;
  GVICK(run_moments(ctx, *s, mu, nullptr, 1, &nchunk));
  return run_epilogue(ctx, *s, 1, nchunk, Ephi, nullptr, Vdmu, Vddmu, nullptr, nullptr);
}

gvi_status gvi_costs_dev(gvi_ctx* ctx, int set_id, const double* mu, const double* Sigma, double* cost) {
  FactorSet* s = get_set(ctx, set_id);
  GVICK(check_pass_args(ctx, s, mu, Sigma));
  if (psi_kind_is<PSI_NO_DEVICE>(s->kind)) return fail(ctx, GVI_ERR_ARG, "HOST_CALLBACK set has no device psi");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(run_prep(ctx, *s, mu, Sigma));
  int nchunk = 1;
  GVICK(run_moments(ctx, *s, mu, nullptr, 0, &nchunk));
  return run_epilogue(ctx, *s, 0, nchunk, nullptr, cost, nullptr, nullptr, nullptr, nullptr);
}

static gvi_status upload_pass_inputs(gvi_ctx* ctx, FactorSet* s, const double* mu, const double* Sigma) {
  HIPCK(ctx, s->in_mu.ensure((size_t)s->K * s->d * 8));
  HIPCK(ctx, s->in_Sigma.ensure((size_t)s->K * s->d * s->d * 8));
  GVICK(h2d(ctx, s->in_mu.p, mu, (size_t)s->K * s->d * 8));
  return h2d(ctx, s->in_Sigma.p, Sigma, (size_t)s->K * s->d * s->d * 8);
}

gvi_status gvi_moments(gvi_ctx* ctx, int set_id, const double* mu, const double* Sigma, double* Ephi,
                       double* Vdmu, double* Vddmu) {
  FactorSet* s = get_set(ctx, set_id);
  GVICK(check_pass_args(ctx, s, mu, Sigma));
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(upload_pass_inputs(ctx, s, mu, Sigma));
  GVICK(gvi_moments_dev(ctx, set_id, s->in_mu.d(), s->in_Sigma.d(), s->Ephi.d(), s->Vdmu.d(), s->Vddmu.d()));
  if (Ephi) GVICK(d2h(ctx, Ephi, s->Ephi.p, (size_t)s->K * 8));
  if (Vdmu) GVICK(d2h(ctx, Vdmu, s->Vdmu.p, (size_t)s->K * s->d * 8));
  if (Vddmu) GVICK(d2h(ctx, Vddmu, s->Vddmu.p, (size_t)s->K * s->d * s->d * 8));
  return sync(ctx);
}

gvi_status gvi_raw_moments(gvi_ctx* ctx, int set_id, const double* mu, const double* Sigma, double* E_phi,
                           double* E_xmuphi, double* E_xxphi) {
  FactorSet* s = get_set(ctx, set_id);
  GVICK(check_pass_args(ctx, s, mu, Sigma));
  if (psi_kind_is<PSI_NO_DEVICE>(s->kind)) return fail(ctx, GVI_ERR_ARG, "HOST_CALLBACK set has no device psi");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(upload_pass_inputs(ctx, s, mu, Sigma));
  HIPCK(ctx, s->raw1.ensure((size_t)s->K * s->d * 8));
  HIPCK(ctx, s->raw2.ensure((size_t)s->K * s->d * s->d * 8));
  GVICK(run_prep(ctx, *s, s->in_mu.d(), s->in_Sigma.d()));
  int nchunk = 1;
  GVICK(run_moments(ctx, *s, s->in_mu.d(), nullptr, 1, &nchunk));
  GVICK(run_epilogue(ctx, *s, 1, nchunk, s->Ephi.d(), nullptr, nullptr, nullptr, s->raw1.d(), s->raw2.d()));
  if (E_phi) GVICK(d2h(ctx, E_phi, s->Ephi.p, (size_t)s->K * 8));
  if (E_xmuphi) GVICK(d2h(ctx, E_xmuphi, s->raw1.p, (size_t)s->K * s->d * 8));
  if (E_xxphi) GVICK(d2h(ctx, E_xxphi, s->raw2.p, (size_t)s->K * s->d * s->d * 8));
  return sync(ctx);
}

gvi_status gvi_costs(gvi_ctx* ctx, int set_id, const double* mu, const double* Sigma, double* cost) {
  FactorSet* s = get_set(ctx, set_id);
  GVICK(check_pass_args(ctx, s, mu, Sigma));
  if (!cost) return fail(ctx, GVI_ERR_ARG, "cost is NULL");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(upload_pass_inputs(ctx, s, mu, Sigma));
  GVICK(gvi_costs_dev(ctx, set_id, s->in_mu.d(), s->in_Sigma.d(), s->cost.d()));
  GVICK(d2h(ctx, cost, s->cost.p, (size_t)s->K * 8));
  return sync(ctx);
}

gvi_status gvi_expand(gvi_ctx* ctx, int set_id, const double* mu, const double* Sigma, double* X) {
  FactorSet* s = get_set(ctx, set_id);
  GVICK(check_pass_args(ctx, s, mu, Sigma));
  if (!X) return fail(ctx, GVI_ERR_ARG, "X is NULL");
  if (s->K == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(upload_pass_inputs(ctx, s, mu, Sigma));
  const size_t bytes = (size_t)s->K * s->d * s->table->N * 8;
  HIPCK(ctx, s->X.ensure(bytes));
  s->force_sym = true;                                       // the caller sees the nodes: the reference's symmetric root
  const gvi_status pst = run_prep(ctx, *s, s->in_mu.d(), s->in_Sigma.d());
  s->force_sym = false;
  GVICK(pst);
  hipLaunchKernelGGL(expand_kernel, dim3((unsigned)((s->table->N + 255) / 256), s->K), dim3(256), 0, ctx->stream,
                     s->dev(ctx->opt), s->in_mu.d(), s->X.d());
  HIPCK(ctx, hipGetLastError());
  GVICK(d2h(ctx, X, s->X.p, bytes));
  return sync(ctx);
}

gvi_status gvi_moments_from_psi(gvi_ctx* ctx, int set_id, const double* mu, const double* Sigma, const double* psi,
                                double* Ephi, double* Vdmu, double* Vddmu) {
  FactorSet* s = get_set(ctx, set_id);
  GVICK(check_pass_args(ctx, s, mu, Sigma));
  if (!psi) return fail(ctx, GVI_ERR_ARG, "psi is NULL");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(upload_pass_inputs(ctx, s, mu, Sigma));
  const size_t bytes = (size_t)s->K * s->table->N * 8;
  HIPCK(ctx, s->psi_ext.ensure(bytes));
  GVICK(h2d(ctx, s->psi_ext.p, psi, bytes));
  s->force_sym = true;                                       // psi was evaluated at the reference's nodes (gvi_expand)
  gvi_status pst = run_prep(ctx, *s, s->in_mu.d(), s->in_Sigma.d());
  int nchunk = 1;
  if (pst == GVI_OK) pst = run_moments(ctx, *s, s->in_mu.d(), s->psi_ext.d(), 1, &nchunk);
  if (pst == GVI_OK) pst = run_epilogue(ctx, *s, 1, nchunk, s->Ephi.d(), nullptr, s->Vdmu.d(), s->Vddmu.d(), nullptr, nullptr);
  s->force_sym = false;
  GVICK(pst);
  if (Ephi) GVICK(d2h(ctx, Ephi, s->Ephi.p, (size_t)s->K * 8));
  if (Vdmu) GVICK(d2h(ctx, Vdmu, s->Vdmu.p, (size_t)s->K * s->d * 8));
  if (Vddmu) GVICK(d2h(ctx, Vddmu, s->Vddmu.p, (size_t)s->K * s->d * s->d * 8));
  return sync(ctx);
}

// ---- joint operators (host-pointer forms stage through the scratch buffer) ----
gvi_status gvi_bt_assemble(gvi_ctx* ctx, int nsets, const int* set_ids, const double* const* Vdmu,
                           const double* const* Vddmu, double* g, double* D, double* U) {
  if (!ctx) return GVI_ERR_ARG;
  if (nsets < 1 || !set_ids || !Vdmu || !Vddmu || !g || !D || !U) return fail(ctx, GVI_ERR_ARG, "NULL argument");
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t T = ctx->T, n = ctx->n, nn = n * n, tot = T * n + bt_count(ctx);
  HIPCK(ctx, ctx->scratch.ensure(tot * 8));
  double* dg = ctx->scratch.d();
  double* dD = dg + T * n;
  double* dU = dD + T * nn;
  HIPCK(ctx, hipMemsetAsync(dg, 0, tot * 8, ctx->stream));
  for (int i = 0; i < nsets; ++i) {
    FactorSet* s = get_set(ctx, set_ids[i]);
    if (!s) return fail(ctx, GVI_ERR_ARG, "bad set id");
    GVICK(h2d(ctx, s->Vdmu.p, Vdmu[i], (size_t)s->K * s->d * 8));
    GVICK(h2d(ctx, s->Vddmu.p, Vddmu[i], (size_t)s->K * s->d * s->d * 8));
    GVICK(run_scatter(ctx, *s, s->Vdmu.d(), s->Vddmu.d(), dg, dD, dU));
  }
  GVICK(d2h(ctx, g, dg, T * n * 8));
  GVICK(d2h(ctx, D, dD, T * nn * 8));
  if (T > 1) GVICK(d2h(ctx, U, dU, (T - 1) * nn * 8));
  return sync(ctx);
}

// Staging: the ONE place a buffer of doubles is sized and cut.  ensure() on the sum of the regions, then every region's pointer,
// in the order given -- the size and the carve cannot disagree.  An empty region gets the pointer of the next one.
struct Region { double** at; size_t doubles; };
static gvi_status carve(gvi_ctx* ctx, DevMem& buf, std::initializer_list<Region> regions) {
  size_t total = 0;
  for (const Region& r : regions) total += r.doubles;
  HIPCK(ctx, buf.ensure(total * 8));
  double* p = buf.d();
  for (const Region& r : regions) { *r.at = p; p += r.doubles; }
  return GVI_OK;
}

// (D, U) of a host-pointer call into their regions, on the context stream; a single-state chain has no U
static gvi_status put_chain(gvi_ctx* ctx, double* dD, double* dU, const double* D, const double* U) {
  const size_t T = ctx->T, nn = nn_(ctx);
  GVICK(h2d(ctx, dD, D, T * nn * 8));
  if (T > 1) GVICK(h2d(ctx, dU, U, (T - 1) * nn * 8));
  return GVI_OK;
}

static gvi_status stage_chain(gvi_ctx* ctx, const double* D, const double* U, size_t extra, double** dD, double** dU,
                              double** dextra) {
  const size_t T = ctx->T, nn = nn_(ctx);
  GVICK(carve(ctx, ctx->scratch, {{dD, T * nn}, {dU, (T - 1) * nn}, {dextra, extra}}));
  return put_chain(ctx, *dD, *dU, D, U);
}

gvi_status gvi_bt_solve(gvi_ctx* ctx, const double* D, const double* U, const double* rhs, double* x) {
  if (!ctx) return GVI_ERR_ARG;
  if (!D || (!U && ctx->T > 1) || !rhs || !x) return fail(ctx, GVI_ERR_ARG, "NULL argument");
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t Tn = (size_t)ctx->T * ctx->n;
  double *dD, *dU, *ex;
  GVICK(stage_chain(ctx, D, U, 2 * Tn, &dD, &dU, &ex));
  GVICK(h2d(ctx, ex, rhs, Tn * 8));
  GVICK(run_bt_solve(ctx, dD, dU, ex, 1.0, ex + Tn));
  GVICK(d2h(ctx, x, ex + Tn, Tn * 8));
  return sync(ctx);
}

gvi_status gvi_bt_logdet(gvi_ctx* ctx, const double* D, const double* U, double* half_logdet) {
  if (!ctx) return GVI_ERR_ARG;
  if (!D || (!U && ctx->T > 1) || !half_logdet) return fail(ctx, GVI_ERR_ARG, "NULL argument");
  HIPCK(ctx, hipSetDevice(ctx->device));
  double *dD, *dU, *ex;
  GVICK(stage_chain(ctx, D, U, 1, &dD, &dU, &ex));
  GVICK(run_bt_factor(ctx, dD, dU, nullptr, nullptr, ex));
  GVICK(d2h(ctx, half_logdet, ex, 8));
  return sync(ctx);
}

gvi_status gvi_bt_marginals(gvi_ctx* ctx, const double* D, const double* U, double* SigD, double* SigU) {
  if (!ctx) return GVI_ERR_ARG;
  if (!D || (!U && ctx->T > 1) || !SigD || (!SigU && ctx->T > 1)) return fail(ctx, GVI_ERR_ARG, "NULL argument");
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t T = ctx->T, nn = nn_(ctx);
  double *dD, *dU, *ex;
  GVICK(stage_chain(ctx, D, U, bt_count(ctx) + 1, &dD, &dU, &ex));
  double* sD = ex;
  double* sU = sD + T * nn;
  GVICK(run_bt_factor(ctx, dD, dU, sD, sU, sU + (T - 1) * nn));
  GVICK(d2h(ctx, SigD, sD, T * nn * 8));
  if (T > 1) GVICK(d2h(ctx, SigU, sU, (T - 1) * nn * 8));
  return sync(ctx);
}

gvi_status gvi_gather_marginals(gvi_ctx* ctx, int set_id, const double* mu, const double* SigD, const double* SigU,
                                double* mu_k, double* Sigma_k) {
  FactorSet* s = get_set(ctx, set_id);
  if (!s) return fail(ctx, GVI_ERR_ARG, "bad set id");
  if (!mu || !SigD || (!SigU && ctx->T > 1) || !mu_k || !Sigma_k) return fail(ctx, GVI_ERR_ARG, "NULL argument");
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t T = ctx->T, n = ctx->n, nn = n * n;
  HIPCK(ctx, ctx->scratch.ensure((T * n + bt_count(ctx)) * 8));
  double* dmu = ctx->scratch.d();
  double* sD = dmu + T * n;
  double* sU = sD + T * nn;
  GVICK(h2d(ctx, dmu, mu, T * n * 8));
  GVICK(h2d(ctx, sD, SigD, T * nn * 8));
  if (T > 1) GVICK(h2d(ctx, sU, SigU, (T - 1) * nn * 8));
  HIPCK(ctx, s->in_mu.ensure((size_t)s->K * s->d * 8));
  HIPCK(ctx, s->in_Sigma.ensure((size_t)s->K * s->d * s->d * 8));
  GVICK(run_gather(ctx, *s, dmu, sD, sU, s->in_mu.d(), s->in_Sigma.d()));
  GVICK(d2h(ctx, mu_k, s->in_mu.p, (size_t)s->K * s->d * 8));
  GVICK(d2h(ctx, Sigma_k, s->in_Sigma.p, (size_t)s->K * s->d * s->d * 8));
  return sync(ctx);
}
