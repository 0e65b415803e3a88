// The resident iteration's stages over ALL sets: prep, epilogue, refresh and gather of a slot, and the cost of a slot from
// the local sum to the host's wait.  A fragment of the library's one translation unit, included by gvi_hip.hip inside its
// extern "C" bracket; not a stand-alone header.
//
//   holds      ngd_check; make_set_list; ngd_flush_gather; ngd_prep_all; make_epi_list, ngd_epilogue_all; ngd_refresh_factor,
//              ngd_gather_now, ngd_gather_with_prep, ngd_refresh; ngd_cost_local / _publish / _wait / _finish; cpu_relax.
//              Declares plan_sets and ngd_moments_launch ahead of their definitions in ngd_iter.inc
//   relies on  host_ctx.inc (gvi_ctx, NgdState, pub_slot); launch_factor.inc (MomPlan / PassPlan, warm_start_of, take_gather,
//              fill_epi_tail); launch_chain.inc (run_bt_factor); routes.hpp (with_prep_instance)
//   defines    no entry point

// ---- device-resident NGD iteration ----
static gvi_status ngd_check(gvi_ctx* ctx) {
  if (!ctx) return GVI_ERR_ARG;
  if (!ctx->ngd.ready) return fail(ctx, GVI_ERR_STATE, "call gvi_ngd_init first");
  return GVI_OK;
}

static SetList make_set_list(gvi_ctx* ctx, int slot) {
  SetList L;
  L.nsets = (int)ctx->sets.size();
  for (int i = 0; i < L.nsets; ++i) {
    FactorSet& s = *ctx->sets[i];
    SetDesc& d = L.s[i];
    d.K = s.K; d.d = s.d;
    d.start = s.dstart.i(); d.ptr = s.dptr.i(); d.idx = s.didx.i();
    d.Vdmu = s.Vdmu.d(); d.Vddmu = s.Vddmu.d();
    d.mu_k = s.mu_k[slot].d(); d.Sigma_k = s.Sigma_k[slot].d();
    d.cost = s.cost.d();
  }
  return L;
}

static gvi_status ngd_gather_now(gvi_ctx* ctx, int i, const double* mu_from, const double* dmu, double step);

// stand-alone gather of a slot whose gather was left to the next prep (consumers other than prep call this)
static gvi_status ngd_flush_gather(gvi_ctx* ctx, int i) {
  const NgdState::GatherPending p = ctx->ngd.gpend[i];
  if (!p.on) return GVI_OK;
  return ngd_gather_now(ctx, i, p.mu_from, p.dmu, p.step);
}

// prep of every set whose per-pass products are not those of NGD slot i -- one launch
static gvi_status ngd_prep_all(gvi_ctx* ctx, int i) {
  NgdState& g = ctx->ngd;
  PrepList L;
  L.nsets = 0;
  L.koff[0] = 0;
  L.gather = 0;
  L.pred = ctx->pipe.pred; L.pred_val = ctx->pipe.pred_val;
  int dmax = 0;
  bool all = true;
  for (auto& s : ctx->sets) {
    if (psi_kind_is<PSI_NO_DEVICE>(s->kind)) return fail(ctx, GVI_ERR_UNSUPPORTED, "resident NGD needs device psi kinds");
    if (s->prep_slot == i) { all = false; break; }
  }
  if (g.gpend[i].on && !all) GVICK(ngd_flush_gather(ctx, i));      // cannot happen (a pending gather resets every prep_slot)
  for (auto& s : ctx->sets) {
    if (s->prep_slot == i) continue;
    s->prep_slot = i;
    L.f[L.nsets] = s->dev(ctx->opt);
    GVICK(warm_start_of(ctx, *s, L.f[L.nsets]));
    L.mu[L.nsets] = s->mu_k[i].d();
    L.Sigma[L.nsets] = s->Sigma_k[i].d();
    L.start[L.nsets] = (const int32_t*)s->dstart.p;
    L.mu_k[L.nsets] = s->mu_k[i].d();
    L.Sigma_k[L.nsets] = s->Sigma_k[i].d();
    L.koff[L.nsets + 1] = L.koff[L.nsets] + s->K;
    dmax = std::max(dmax, s->d);
    ++L.nsets;
  }
  if (L.nsets == 0) return GVI_OK;
  const unsigned extra = take_gather(ctx, i, L, 64);
  const size_t lds = prep_all_lds_bytes(dmax);
  const dim3 grid(L.koff[L.nsets] + extra);
  if (grid.x == 0) return GVI_OK;                                     // only empty shards
  auto launch = [&](auto rowb) {                                      // rowb: the row-broadcast Cholesky, as a type
    return with_prep_instance(dmax, [&]<int EPLP>(PrepInst<EPLP>) {
      hipLaunchKernelGGL((prep_all_kernel<EPLP, decltype(rowb)::value>), grid, dim3(64), lds, ctx->stream, L);
    });
  };
  if (!(ctx->opt.chol_rowb ? launch(std::true_type{}) : launch(std::false_type{})))
    return fail(ctx, GVI_ERR_UNSUPPORTED, "factor dimension > 32");
  HIPCK(ctx, hipGetLastError());
  return GVI_OK;
}

// epilogue of every set -- one launch (full: Vdmu / Vddmu / Ephi / cost; else cost only)
// P: the plans of the pass it reduces
static EpiList make_epi_list(gvi_ctx* ctx, int full, const MomPlan* P, int* dmax_out) {
  EpiList L;
  L.nsets = (int)ctx->sets.size();
  L.koff[0] = 0;
  int dmax = 0;
  for (int si = 0; si < L.nsets; ++si) {
    FactorSet& s = *ctx->sets[si];
    EpiArgs& e = L.e[si];
    e.f = s.dev(ctx->opt); e.partial = s.partial.d(); e.nchunk = P[si].nchunk; e.full = full;
    e.Ephi = full ? s.Ephi.d() : nullptr; e.cost = s.cost.d();
    e.Vdmu = full ? s.Vdmu.d() : nullptr; e.Vddmu = full ? s.Vddmu.d() : nullptr;
    e.E_xmuphi = nullptr; e.E_xxphi = nullptr;
    L.koff[si + 1] = L.koff[si] + s.K;
    dmax = std::max(dmax, s.d);
  }
  if (dmax_out) *dmax_out = dmax;
  return L;
}

// publish_slot >= 0: the launch also sums the factor costs and publishes the cost of NGD slot `publish_slot` (EpiTail)
static gvi_status ngd_epilogue_all(gvi_ctx* ctx, int full, const MomPlan* P, int publish_slot = -1) {
  int dmax = 0;
  const EpiList L = make_epi_list(ctx, full, P, &dmax);
  const size_t lds = epilogue_all_lds_doubles(dmax) * 8;
  if (L.koff[L.nsets] == 0) return GVI_OK;
  EpiTail tail;
  GVICK(fill_epi_tail(ctx, L.koff[L.nsets], publish_slot, &tail));
  CostList cl{};
  cl.nsets = L.nsets;
  for (int si = 0; si < L.nsets; ++si) { cl.cost[si] = L.e[si].cost; cl.K[si] = L.e[si].f.K; }
  hipLaunchKernelGGL(epilogue_all_kernel, dim3(L.koff[L.nsets]), dim3(64), lds, ctx->stream, L, tail, cl);
  HIPCK(ctx, hipGetLastError());
  return GVI_OK;
}

// marginals + log-det of Lam[i], then gather every set's (mu_k, Sigma_k) into slot i (one launch)
static gvi_status ngd_refresh_factor(gvi_ctx* ctx, int i) {
  NgdState& g = ctx->ngd;
  const size_t T = ctx->T, nn = nn_(ctx);
  double* D = g.Lam[i].d();
  double* U = D + T * nn;
  double* sD = g.Sig[i].d();
  double* sU = sD + T * nn;
  return run_bt_factor(ctx, D, U, sD, sU, g.hld[i].d());
}

// gather every set's (mu_k, Sigma_k) into slot i, launched now (one launch).
// mu_from / dmu / step: form mu[i] = mu_from + step dmu inside the gather launch (trial state); null: mu[i] is current
static gvi_status ngd_gather_now(gvi_ctx* ctx, int i, const double* mu_from, const double* dmu, double step) {
  NgdState& g = ctx->ngd;
  g.gpend[i].on = false;
  const size_t T = ctx->T, nn = nn_(ctx);
  const int64_t nmu = (int64_t)T * ctx->n;
  double* sD = g.Sig[i].d();
  double* sU = sD + T * nn;
  if (ctx->sets.empty()) {
    if (dmu) hipLaunchKernelGGL(trial_kernel, dim3((unsigned)((nmu + 255) / 256)), dim3(256), 0, ctx->stream, nmu, (int64_t)0, step,
                                mu_from, dmu, (const double*)nullptr, (const double*)nullptr, g.mu[i].d(), (double*)nullptr);
    return GVI_OK;
  }
  if ((int)ctx->sets.size() > MAX_SETS) return fail(ctx, GVI_ERR_UNSUPPORTED, "more than 8 factor sets");
  int64_t maxwork = dmu ? nmu : 0;
  for (auto& s : ctx->sets) {
    if (s->prep_slot == i) s->prep_slot = -1;
    maxwork = std::max<int64_t>(maxwork, (int64_t)s->K * (s->d + s->d * s->d));
  }
  hipLaunchKernelGGL(gather_all_kernel, dim3((unsigned)std::max<int64_t>(1, (maxwork + 255) / 256), (unsigned)ctx->sets.size() + (dmu ? 1u : 0u)),
                     dim3(256), 0, ctx->stream, make_set_list(ctx, i), ctx->n, dmu ? mu_from : g.mu[i].d(), sD, sU, dmu, step,
                     g.mu[i].d(), nmu);
  HIPCK(ctx, hipGetLastError());
  return GVI_OK;
}

// the same gather left to the prep launch of slot i that follows (trial state: a cost or full pass of the slot always does;
// any other reader flushes it, ngd_flush_gather); option fuse_gather = 0: launched now
static gvi_status ngd_gather_with_prep(gvi_ctx* ctx, int i, const double* mu_from, const double* dmu, double step) {
  if (!ctx->opt.fuse_gather || ctx->sets.empty()) return ngd_gather_now(ctx, i, mu_from, dmu, step);
  for (auto& s : ctx->sets) if (s->prep_slot == i) s->prep_slot = -1;
  ctx->ngd.gpend[i] = {true, mu_from, dmu, step};
  return GVI_OK;
}

static gvi_status ngd_refresh(gvi_ctx* ctx, int i) {
  GVICK(ngd_refresh_factor(ctx, i));
  return ngd_gather_now(ctx, i, nullptr, nullptr, 0.0);
}

// sum over sets of sum_k E[psi]/T_k at slot i -> exch1[0].  Everything stays on ONE stream: side streams
// share the hardware queue on this part and every cross-stream dependency costs a 6-30 us barrier
// packet (profiles/r01_d_*); the small sets ride along inside the fused prep / epilogue launches.
static gvi_status plan_sets(gvi_ctx* ctx, int slot, int full, PassPlan* pp);
static gvi_status ngd_moments_launch(gvi_ctx* ctx, int full, const PassPlan& pp);

// publish = true (single-process iteration): the same launch also writes {cost, half log-det, sequence} to the
// host-mapped slot, so no separate publish_kernel follows
static gvi_status ngd_cost_local(gvi_ctx* ctx, int i, bool publish = false) {
  NgdState& g = ctx->ngd;
  if (ctx->sets.empty()) {
    HIPCK(ctx, hipMemsetAsync(g.exch1.p, 0, 8, ctx->stream));
    if (publish) {
      ctx->seq += 1.0;
      hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, ctx->stream, g.exch1.d(), g.hld[i].d(), pub_slot(ctx), ctx->seq);
      HIPCK(ctx, hipGetLastError());
    }
    return GVI_OK;
  }
  if ((int)ctx->sets.size() > MAX_SETS) return fail(ctx, GVI_ERR_UNSUPPORTED, "more than 8 factor sets");
  GVICK(ngd_prep_all(ctx, i));
  PassPlan pp;
  GVICK(plan_sets(ctx, i, 0, &pp));
  GVICK(ngd_moments_launch(ctx, 0, pp));
  if (publish) ctx->seq += 1.0;
  if (!ctx->tail_counter.p) {
    HIPCK(ctx, ctx->tail_counter.ensure(8));
    HIPCK(ctx, hipMemsetAsync(ctx->tail_counter.p, 0, 8, ctx->stream));
  }
  int64_t nfac = 0;
  for (auto& s : ctx->sets) nfac = std::max<int64_t>(nfac, s->K);
  const unsigned nblk = (unsigned)std::min<int64_t>(32, std::max<int64_t>(1, (nfac + 255) / 256));
  hipLaunchKernelGGL(cost_tail_kernel, dim3(nblk), dim3(256), 0, ctx->stream, make_epi_list(ctx, 0, pp.P, nullptr), g.exch1.d(),
                     g.hld[i].d(), publish ? pub_slot(ctx) : nullptr, ctx->seq, (unsigned*)ctx->tail_counter.p);
  HIPCK(ctx, hipGetLastError());
  return GVI_OK;
}

static gvi_status ngd_cost_publish(gvi_ctx* ctx, int i) {
  NgdState& g = ctx->ngd;
  ctx->seq += 1.0;
  hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, ctx->stream, g.exch1.d(), g.hld[i].d(),
                     pub_slot(ctx), ctx->seq);
  HIPCK(ctx, hipGetLastError());
  return GVI_OK;
}

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield" ::: "memory");
#else
  asm volatile("" ::: "memory");
#endif
}

static gvi_status ngd_cost_wait(gvi_ctx* ctx, int i, double* out, double seq_expected = -1.0, int ring = -1) {
  NgdState& g = ctx->ngd;
  const double want = seq_expected >= 0.0 ? seq_expected : ctx->seq;
  const int rg = ring >= 0 ? ring : ctx->pipe.pub_ring;
  // Spin on the host-mapped sequence word: a blocking stream sync costs tens of us of wake-up latency and would
  // also wait for the speculative work queued behind the publish.  The spin is bounded by WALL TIME (2 ms -- an
  // iteration is < 1 ms); past that the wait sleeps between polls (below).
  // {value, sequence} is ONE 16-byte device store (publish_to_host) and is read here with ONE 16-byte load (movdqa: a single
  // access on every AVX-capable x86), so value and sequence always belong to the same publish -- no "new sequence, old value"
  // window between two 8-byte loads (ADVICE r2)
  const double* slot = ctx->host_slot + 4 * rg;
  typedef double v2d __attribute__((vector_size(16), aligned(16)));
  const bool safe = ctx->opt.safe_publish;
  auto poll = [&](double* val) {
    if (safe) {
      // checked form [sequence | value | value | sequence]: taken only when both sequence words and both copies agree
      const volatile double* vs = slot;
      const double s0 = vs[0];
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      const double v1 = vs[1], v2 = vs[2];
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      const double s3 = vs[3];
      *val = v1;
      return s0 == want && s3 == want && std::memcmp(&v1, &v2, 8) == 0;
    }
    const v2d both = *(const volatile v2d*)(const void*)slot;        // (volatile: re-read at every poll)
    *val = both[0];
    return both[1] == want;
  };
  bool seen = false;
  double v = 0.0;
  const auto t0 = std::chrono::steady_clock::now();
  for (long spins = 0;; ++spins) {
    if (poll(&v)) { seen = true; break; }
    cpu_relax();
    if ((spins & 1023) == 1023 &&
        std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(ctx->opt.spin_ms)) break;
  }
  if (!seen) {
    // long passes (config 5: seconds per pass): sleep-poll the word and, every millisecond, the stream itself, so a
    // device fault or a drained stream without a publish ends the wait with an error instead of spinning
    for (long polls = 0;; ++polls) {
      if (poll(&v)) { seen = true; break; }
      std::this_thread::sleep_for(std::chrono::microseconds(20));
      if ((polls & 63) == 63) {
        const hipError_t q = hipStreamQuery(ctx->stream);
        if (q == hipSuccess) break;                       // everything queued has run
        if (q != hipErrorNotReady) return fail(ctx, GVI_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(q));
      }
    }
    if (!seen && !poll(&v))
      return fail(ctx, GVI_ERR_STATE, "cost publish did not arrive (sequence word stale after the stream drained)");
  }
  __sync_synchronize();
  g.cost[i] = v;                                     // cost_value = sum of factor costs + 1/2 log det (added on the device)
  g.cost_valid[i] = true;
  if (out) *out = v;
  return GVI_OK;
}

static gvi_status ngd_cost_finish(gvi_ctx* ctx, int i, double* out) {
  GVICK(ngd_cost_publish(ctx, i));
  return ngd_cost_wait(ctx, i, out);
}
