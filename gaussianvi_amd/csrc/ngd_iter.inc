// One iteration of the resident natural-gradient descent: cost and gradients at the current state, the trial state, the line
// search.  A fragment of the library's one translation unit, included by gvi_hip.hip inside its extern "C" bracket; not a
// stand-alone header.
//
//   holds      decide_sets, bind_sets, plan_sets; ngd_moments_launch; ngd_fused_full, ngd_block3_full, ngd_moments_full;
//              dual_solve, asm_on_load_ok, make_asm_list; ngd_scatter, ngd_flush_assemble, ngd_scatter_now; ngd_grad_local,
//              ngd_grad_finish, ngd_join_solve; ngd_trial_state; take_spec_gradients; ngd_iteration_entry; ngd_linesearch
//   relies on  host_ctx.inc; launch_factor.inc (bind_plan, launch_single, launch_orbit_pair, launch_fused_t, orbit_args,
//              ProfBracket ...); launch_chain.inc (run_chain, run_bt_solve, make_chain_args); api_operators.inc
//              (gvi_costs_dev); ngd_stage.inc; ngd_dist.inc
//   defines    gvi_ngd_init; gvi_ngd_cost, gvi_ngd_cost_local, gvi_ngd_cost_finish, gvi_ngd_factor_costs;
//              gvi_ngd_gradients, gvi_ngd_gradients_local, gvi_ngd_gradients_finish; gvi_ngd_trial, gvi_ngd_trial_local,
//              gvi_ngd_trial_finish, gvi_ngd_trial_publish, gvi_ngd_trial_wait; gvi_ngd_spec_gradients_local / _finish;
//              gvi_ngd_accept, gvi_ngd_accept_spec; gvi_ngd_step

gvi_status gvi_ngd_init(gvi_ctx* ctx, const double* mu, const double* D, const double* U) {
  if (!ctx) return GVI_ERR_ARG;
  if (ctx->T < 1) return fail(ctx, GVI_ERR_STATE, "call gvi_chain_set first");
  if (!mu || !D || (!U && ctx->T > 1)) return fail(ctx, GVI_ERR_ARG, "NULL argument");
  HIPCK(ctx, hipSetDevice(ctx->device));
  NgdState& g = ctx->ngd;
  const size_t T = ctx->T, n = ctx->n, nn = n * n, bt = bt_count(ctx);
  for (int i = 0; i < 2; ++i) {
    HIPCK(ctx, g.mu[i].ensure(T * n * 8));
    HIPCK(ctx, g.Lam[i].ensure(bt * 8));
    HIPCK(ctx, g.Sig[i].ensure(bt * 8));
    HIPCK(ctx, g.hld[i].ensure(8));
  }
  for (int i = 0; i < 2; ++i) {
    HIPCK(ctx, g.exch0[i].ensure((T * n + bt) * 8));
    HIPCK(ctx, g.dmu2[i].ensure(T * n * 8));
  }
  g.gcur = 0; g.grad_valid = false; g.grad_slot = -1;
  ctx->ngd.solve_deferred[0] = ctx->ngd.solve_deferred[1] = false;
  ctx->ngd.asm_pending[0] = ctx->ngd.asm_pending[1] = false;
  ctx->ngd.last_first_accepted = true;             // adaptive fusing starts afresh: the pass order of a run must not depend on the previous problem
  HIPCK(ctx, g.exch1.ensure(8));
  HIPCK(ctx, g.dmu.ensure(T * n * 8));
  HIPCK(ctx, g.dLam.ensure(bt * 8));
  HIPCK(ctx, g.total.ensure(8));
  for (auto& s : ctx->sets) GVICK(ensure_set_buffers(ctx, *s));
  g.cur = 0; g.have_trial = false;
  for (auto& s : ctx->sets) { s->prep_slot = -1; s->warm_count = 0; }
  g.cost_valid[0] = g.cost_valid[1] = false;
  GVICK(h2d(ctx, g.mu[0].p, mu, T * n * 8));
  GVICK(h2d(ctx, g.Lam[0].p, D, T * nn * 8));
  if (T > 1) GVICK(h2d(ctx, g.Lam[0].d() + T * nn, U, (T - 1) * nn * 8));
  GVICK(sync(ctx));                                // the caller's buffers are free on return
  GVICK(ngd_refresh(ctx, 0));                      // stream-ordered before everything that follows: not waited for
  HIPCK(ctx, hipGetLastError());
  g.ready = true;
  return GVI_OK;
}

gvi_status gvi_ngd_cost(gvi_ctx* ctx, double* cost) {
  GVICK(ngd_check(ctx));
  HIPCK(ctx, hipSetDevice(ctx->device));
  NgdState& g = ctx->ngd;
  if (!g.cost_valid[g.cur]) {
    GVICK(ngd_cost_local(ctx, g.cur));
    GVICK(dist_exchange1(ctx));
    GVICK(ngd_cost_finish(ctx, g.cur, nullptr));
  }
  if (cost) *cost = g.cost[g.cur];
  return GVI_OK;
}

gvi_status gvi_ngd_cost_local(gvi_ctx* ctx) {
  GVICK(ngd_check(ctx));
  HIPCK(ctx, hipSetDevice(ctx->device));
  return ngd_cost_local(ctx, ctx->ngd.cur);
}

gvi_status gvi_ngd_cost_finish(gvi_ctx* ctx, double* cost) {
  GVICK(ngd_check(ctx));
  HIPCK(ctx, hipSetDevice(ctx->device));
  return ngd_cost_finish(ctx, ctx->ngd.cur, cost);
}

gvi_status gvi_ngd_factor_costs(gvi_ctx* ctx, int set_id, double* costs) {
  GVICK(ngd_check(ctx));
  FactorSet* s = get_set(ctx, set_id);
  if (!s || !costs) return fail(ctx, GVI_ERR_ARG, "bad set id / NULL");
  HIPCK(ctx, hipSetDevice(ctx->device));
  const int i = ctx->ngd.cur;
  GVICK(ngd_flush_gather(ctx, i));
  GVICK(gvi_costs_dev(ctx, set_id, s->mu_k[i].d(), s->Sigma_k[i].d(), s->cost.d()));
  GVICK(d2h(ctx, costs, s->cost.p, (size_t)s->K * 8));
  return sync(ctx);
}

// every set's decision for a pass of the resident iteration
static gvi_status decide_sets(gvi_ctx* ctx, int full, PassPlan* pp) {
  if ((int)ctx->sets.size() > MAX_SETS) return fail(ctx, GVI_ERR_UNSUPPORTED, "more than 8 factor sets");
  const RouteRules r = rules_of(ctx);
  for (size_t i = 0; i < ctx->sets.size(); ++i) {
    pp->F[i] = route_facts(*ctx->sets[i], false);
    pp->D[i] = decide_route(pp->F[i], r, full);
    if (pp->D[i].status != GVI_OK) return fail(ctx, pp->D[i].status, pp->D[i].why);
  }
  return GVI_OK;
}

// ... bound at NGD slot `slot`: the sets' launches exactly as they would go out on their own (chunking, table pointers,
// partial buffers)
static gvi_status bind_sets(gvi_ctx* ctx, int slot, int full, PassPlan* pp) {
  for (size_t i = 0; i < ctx->sets.size(); ++i)
    GVICK(bind_plan(ctx, *ctx->sets[i], pp->D[i], ctx->sets[i]->mu_k[slot].d(), nullptr, full, &pp->P[i]));
  return GVI_OK;
}

static gvi_status plan_sets(gvi_ctx* ctx, int slot, int full, PassPlan* pp) {
  GVICK(decide_sets(ctx, full, pp));
  return bind_sets(ctx, slot, full, pp);
}

// All sets' moments (full = 1) or cost (full = 0) launches of a planned pass: decide_fuse (routes.hpp) says which plans go out
// as ONE launch; every other combination is one launch per set.
static gvi_status ngd_moments_launch(gvi_ctx* ctx, int full, const PassPlan& pp) {
  if (full) ++ctx->ngd.n_full_pass; else ++ctx->ngd.n_cost_pass;
  const MomPlan* P = pp.P;
  const int ns = (int)ctx->sets.size();
  ProfBracket b;
  switch (decide_fuse(ns, pp.F, pp.D, rules_of(ctx), ctx->profile_all, full)) {
    case Fuse::OrbitPair: {
      FactorSet &s0 = *ctx->sets[0], &s1 = *ctx->sets[1];
      GVICK(prof_open(ctx, s0, 0, full != 0, false, ctx->stream, &b));
      launch_orbit_pair(P[0].oa, P[1].oa, s0.m, std::max(P[0].smax, P[1].smax), full != 0, ctx->stream, b.e0, b.e1);
      HIPCK(ctx, hipGetLastError());
      record_plan(s0, P[0], true);
      record_plan(s1, P[1], true);
      return prof_close(ctx, b);
    }
    case Fuse::SregPair:
    case Fuse::ScostPair: {
      FactorSet &s0 = *ctx->sets[0], &s1 = *ctx->sets[1];
      const MomArgs &a0 = P[0].a, &a1 = P[1].a;
      const int nbx0 = (int)P[0].grid.x, nbx1 = (int)P[1].grid.x;
      const int nb0 = nbx0 * (int)P[0].grid.y, nb1 = nbx1 * (int)P[1].grid.y;
      GVICK(prof_open(ctx, s0, 0, full != 0, true, ctx->stream, &b));
      if (full && P[0].pipe && P[1].pipe)                    // every block: one prior item + strided unary items
        hipLaunchKernelGGL((moments_sreg_pair_kernel<12, 6, 6, 6, true, true>), dim3(std::max(nb0, nb1)), dim3(256), 0, ctx->stream,
                           a0, a1, nbx0, nb0, nbx1);
      else if (full)
        hipLaunchKernelGGL((moments_sreg_pair_kernel<12, 6, 6, 6, true>), dim3(nb0 + nb1), dim3(256), 0, ctx->stream, a0, a1, nbx0, nb0, nbx1);
      else
        hipLaunchKernelGGL((moments_scost_pair_kernel<12, 6, 6, 6, 2>), dim3(nb0 + nb1), dim3(256), 0, ctx->stream, a0, a1, nbx0, nb0, nbx1);
      HIPCK(ctx, hipGetLastError());
      record_plan(s0, P[0], true);
      record_plan(s1, P[1], true);
      return prof_close(ctx, b);
    }
    case Fuse::Planar3: {
      int nbx[3], nb[3];
      for (int q = 0; q < 3; ++q) {
        nbx[q] = (ctx->sets[q]->K + 3) / 4;
        nb[q] = nbx[q] * P[q].nchunk;
      }
      GVICK(prof_open(ctx, *ctx->sets[1], 0, full != 0, true, ctx->stream, &b));   // booked on the obstacle set (the dominant one)
      if (full)
        hipLaunchKernelGGL((moments_planar3_kernel<true>), dim3(nb[0] + nb[1] + nb[2]), dim3(256), 0, ctx->stream, P[0].a, P[1].a, P[2].a,
                           nbx[0], nb[0], nbx[1], nb[1], nbx[2], P[0].pipe ? 1 : 0);
      else
        hipLaunchKernelGGL((moments_planar3_kernel<false>), dim3(nb[0] + nb[1] + nb[2]), dim3(256), 0, ctx->stream, P[0].a, P[1].a, P[2].a,
                           nbx[0], nb[0], nbx[1], nb[1], nbx[2], 0);
      HIPCK(ctx, hipGetLastError());
      for (int q = 0; q < 3; ++q) record_plan(*ctx->sets[q], P[q], false);
      return prof_close(ctx, b);
    }
    case Fuse::None:
      break;
  }
  for (int i = 0; i < ns; ++i) GVICK(launch_single(ctx, *ctx->sets[i], P[i], ctx->stream));
  return GVI_OK;
}

// ---- the full pass as ONE launch (kernels_fused.hpp), where decide_full says Fused ----
// It chunks by its own rule: four chunks per factor, one per wave.
static gvi_status ngd_fused_full(gvi_ctx* ctx, int slot, int publish_slot, const PassPlan& pp) {
  constexpr int fused_chunks = 4;
  FusedArgs A{};
  A.nsets = (int)ctx->sets.size();
  A.koff[0] = 0;
  int dmax = 0, copies = 1;
  const FusedKey key = fused_key(A.nsets, pp.F);
  A.nblk = fused_nblk(pp.F[0].K, A.nsets > 1 ? pp.F[1].K : 0, FUSED_MAX_ITEMS);
  for (int si = 0; si < A.nsets; ++si) {
    FactorSet& s = *ctx->sets[si];
    FusedSet& F = A.s[si];
    s.prep_slot = -1;                      // the fused pass keeps its products in LDS: nothing resident for a later pass
    F.f = s.dev(ctx->opt);
    GVICK(warm_start_of(ctx, s, F.f));     // (symmetric-root sets only; the Cholesky route ignores it)
    GVICK(orbit_args(ctx, s, fused_chunks, &F.oa));
    F.oa.partial = nullptr;
    F.mu = s.mu_k[slot].d(); F.Sigma = s.Sigma_k[slot].d();
    F.start = s.chain_structured ? nullptr : (const int32_t*)s.dstart.p;      // null: start[k] == k, one dependent load less
    F.mu_k = s.mu_k[slot].d(); F.Sigma_k = s.Sigma_k[slot].d();
    F.Ephi = s.Ephi.d(); F.cost = s.cost.d(); F.Vdmu = s.Vdmu.d(); F.Vddmu = s.Vddmu.d();
    A.koff[si + 1] = A.koff[si] + s.K;
    A.cl.cost[si] = s.cost.d(); A.cl.K[si] = s.K;
    dmax = std::max(dmax, s.d);
    copies = std::max(copies, F.oa.copies);
    Table& t = *s.table;                   // the walk's priority bands: costs of the table's four chunks, made once
    if (!t.orb_walk_prio) t.orb_walk_prio = std::make_unique<WalkPrioSet>(walk_prio_costs(t.orb, orbit_chunk_bounds(t.orb, fused_chunks)));
    A.wp[si] = *t.orb_walk_prio;
  }
  A.walk_prio = ctx->opt.walk_prio ? 1 : 0;   // (launch_fused_t: only where the item blocks fit one residency round)
  // (the walk regions are sized for the widest set with the most accumulator copies: an upper bound for every set)
  const int items = 1 + (A.nsets > 1 ? (ctx->sets[1]->K + A.nblk - 1) / A.nblk : 0);      // most items of a block
  const size_t lds = fused_lds_doubles(dmax, key.m, copies, items) * 8;
  if (lds > 160 * 1024) return fail(ctx, GVI_ERR_UNSUPPORTED, "fused pass: LDS budget");
  A.cl.nsets = A.nsets;
  if (A.nsets == 1) A.koff[2] = A.koff[1];
  const unsigned extra = take_gather(ctx, slot, A, 256);
  GVICK(fill_epi_tail(ctx, A.koff[A.nsets], publish_slot, &A.tail));
  ++ctx->ngd.n_full_pass;
  ProfBracket b;
  GVICK(prof_open(ctx, *ctx->sets[0], 0, true, false, ctx->stream, &b));
  const unsigned grid = (unsigned)A.nblk + extra;
  gvi_status rc = GVI_OK;
  if (!with_fused_instance(key.m, key.smax, key.d0, key.d1, [&]<int M, int SMAX, int WAVES, int D0, int D1>(FusedInst<M, SMAX, WAVES, D0, D1>) {
        rc = launch_fused_t<M, SMAX, WAVES, D0, D1>(ctx, A, grid, lds, dmax, copies, items, b.e0, b.e1);
      }))
    return fail(ctx, GVI_ERR_UNSUPPORTED, "fused pass: shape not instantiated");
  GVICK(rc);
  HIPCK(ctx, hipGetLastError());
  for (auto& s : ctx->sets) record_pass(s->last, Route::Orbit, true, fused_chunks, s->table->Np);
  return prof_close(ctx, b);
}

// ---- the planning graph's full pass as ONE launch (kernels_block.hpp), where decide_full says Block3 ----
// The sets' moments launches exactly as they would go out on their own (pp), taken by one kernel with prep and epilogue.
static gvi_status ngd_block3_full(gvi_ctx* ctx, int slot, int publish_slot, const PassPlan& pp) {
  const MomPlan* P = pp.P;
  ++ctx->ngd.n_full_pass;
  Block3Args A{};
  A.nitems = ctx->sets[0]->K + ctx->sets[1]->K + ctx->sets[2]->K;
  A.pipe = P[0].pipe ? 1 : 0;
  unsigned nblk = 0;
  for (int q = 0; q < 3; ++q) {
    FactorSet& s = *ctx->sets[q];
    BlockSet& B = A.s[q];
    B.a = P[q].a;
    GVICK(warm_start_of(ctx, s, B.a.f));       // warm-started Jacobi of the symmetric-root sets, as ngd_prep_all
    B.start = (const int32_t*)s.dstart.p;
    B.mu_k = s.mu_k[slot].d(); B.Sigma_k = s.Sigma_k[slot].d();
    B.Ephi = s.Ephi.d(); B.cost = s.cost.d(); B.Vdmu = s.Vdmu.d(); B.Vddmu = s.Vddmu.d();
    A.cl.cost[q] = s.cost.d(); A.cl.K[q] = s.K;
    nblk += (unsigned)block3_blocks(s.K, P[q].nchunk);
    s.prep_slot = slot;                        // the products go to memory as prep_all_kernel leaves them
  }
  A.cl.nsets = 3;
  const unsigned extra = take_gather(ctx, slot, A, 256);
  GVICK(fill_epi_tail(ctx, A.nitems, publish_slot, &A.tail));
  ProfBracket b;                               // the bracket is booked on the obstacle set (the dominant one)
  GVICK(prof_open(ctx, *ctx->sets[1], 0, true, true, ctx->stream, &b));
  hipLaunchKernelGGL(factor_block3_kernel, dim3(nblk + extra), dim3(256), 4 * block3_lds_doubles() * 8, ctx->stream, A);
  ++block3_launches();
  HIPCK(ctx, hipGetLastError());
  for (int q = 0; q < 3; ++q) record_plan(*ctx->sets[q], P[q], false);
  return prof_close(ctx, b);
}

// the full pass at NGD slot `slot`: decide every set, decide_full, then one switch that launches
static gvi_status ngd_moments_full(gvi_ctx* ctx, int slot, int publish_slot = -1) {
  for (auto& s : ctx->sets)
    if (psi_kind_is<PSI_NO_DEVICE>(s->kind)) return fail(ctx, GVI_ERR_UNSUPPORTED, "resident NGD needs device psi kinds");
  StageScope scope(ctx, STAGE_FACTORS);
  PassPlan pp;
  GVICK(decide_sets(ctx, 1, &pp));
  const int ns = (int)ctx->sets.size();
  bool resident[MAX_SETS];                     // products of this state already there: the plain route skips the prep
  for (int i = 0; i < ns; ++i) resident[i] = ctx->sets[i]->prep_slot == slot;
  switch (decide_full(ns, pp.F, pp.D, resident, rules_of(ctx), ctx->profile_all, ctx->update_rule == GVI_RULE_NGD, FUSED_MAX_ITEMS)) {
    case FullFuse::Fused:
      return ngd_fused_full(ctx, slot, publish_slot, pp);
    case FullFuse::Block3:
      GVICK(bind_sets(ctx, slot, 1, &pp));
      return ngd_block3_full(ctx, slot, publish_slot, pp);
    case FullFuse::Separate:
      break;
  }
  GVICK(ngd_prep_all(ctx, slot));
  GVICK(bind_sets(ctx, slot, 1, &pp));
  GVICK(ngd_moments_launch(ctx, 1, pp));
  return ngd_epilogue_all(ctx, 1, pp.P, publish_slot);
}

// the gradient solve is parked and goes out beside the next trial factorisation, as the dual launch (ngd_trial_state);
// else (option side_solve = 0, a one-state chain) it is launched at once
static bool dual_solve(const gvi_ctx* ctx) { return ctx->opt.side_solve && chain_supported(ctx->n) && ctx->T > 1; }

// assemble-on-load applies: every set chain-structured, the solve of this buffer will go out through the dual launch (or
// the flushing solve), nobody needs [g | V_D | V_U] in memory before that
static bool asm_on_load_ok(const gvi_ctx* ctx) {
  if (!ctx->opt.asm_on_load || dist_on(ctx) || ctx->update_rule != GVI_RULE_NGD || ctx->sets.empty()) return false;
  if (!dual_solve(ctx)) return false;
  for (auto& s : ctx->sets)
    if (!s->chain_structured && !(s->d == ctx->n && s->K <= ASM_SPARSE_MAX)) return false;    // (sparse unary sets: AsmSet::sp)
  return true;
}

static AsmList make_asm_list(gvi_ctx* ctx) {
  AsmList L{};
  L.nsets = (int)ctx->sets.size();
  for (int i = 0; i < L.nsets; ++i) {
    FactorSet& s = *ctx->sets[i];
    L.s[i].K = s.K; L.s[i].d = s.d; L.s[i].Vdmu = s.Vdmu.d(); L.s[i].Vddmu = s.Vddmu.d();
    L.s[i].nsp = 0;
    if (!s.chain_structured) {
      L.s[i].nsp = s.K;
      for (int k = 0; k < s.K && k < ASM_SPARSE_MAX; ++k) L.s[i].sp[k] = s.start[k];
    }
  }
  return L;
}

static gvi_status ngd_scatter_now(gvi_ctx* ctx, int slot, int gb);

// ordered assemble of the per-factor results into gradient buffer `gb` -- launched now, or left to the first pass of the
// chain operations that consume the buffer (assemble-on-load)
static gvi_status ngd_scatter(gvi_ctx* ctx, int slot, int gb) {
  if ((int)ctx->sets.size() <= MAX_SETS && asm_on_load_ok(ctx)) {
    ctx->ngd.asm_pending[gb] = true;
    ctx->ngd.asm_pending[1 - gb] = false;               // its source (the sets' Vdmu / Vddmu) has just been overwritten
    return GVI_OK;
  }
  ctx->ngd.asm_pending[gb] = false;
  return ngd_scatter_now(ctx, slot, gb);
}

// stand-alone assemble of a buffer whose assemble was left pending (consumers other than the chain launches)
static gvi_status ngd_flush_assemble(gvi_ctx* ctx, int gb) {
  if (!ctx->ngd.asm_pending[gb]) return GVI_OK;
  ctx->ngd.asm_pending[gb] = false;
  return ngd_scatter_now(ctx, ctx->ngd.cur, gb);
}

static gvi_status ngd_scatter_now(gvi_ctx* ctx, int slot, int gb) {
  const size_t T = ctx->T, n = ctx->n, nn = n * n;
  const GradBuf e = grad_buf(ctx, gb);
  const int64_t total = (int64_t)T * (n + 2 * nn);
  StageScope scope(ctx, STAGE_ASSEMBLE);
  double* rec = nullptr;                                     // sharded: the assemble writes this rank's exchange records too
  int rlo = 0, rlen = 0;
  if (dist_on(ctx)) {
    GVICK(dist_ranges(ctx));
    rec = ctx->dist.send.d(); rlo = ctx->dist.lo[ctx->dist.rank]; rlen = ctx->dist.hi[ctx->dist.rank] - rlo + 1;
  }
  hipLaunchKernelGGL(bt_scatter_all_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                     make_set_list(ctx, slot), ctx->T, ctx->n, e.g, e.D, e.U, ctx->pipe.pred, ctx->pipe.pred_val, rec, rlo, rlen);
  HIPCK(ctx, hipGetLastError());
  if (rec) ctx->dist.rec_fresh = true;
  return GVI_OK;
}

static gvi_status ngd_grad_local(gvi_ctx* ctx, int slot, int gb) {
  ctx->ngd.solve_deferred[gb] = false;                      // a parked solve of this buffer's previous contents is moot
  GVICK(ngd_moments_full(ctx, slot));
  return ngd_scatter(ctx, slot, gb);
}

// dmu = Vddmu^-1 (-Vdmu) from gradient buffer `gb` (dprecision = V - Lambda is formed inside the trial)
static gvi_status ngd_grad_finish(gvi_ctx* ctx, int gb) {
  NgdState& g = ctx->ngd;
  if (dual_solve(ctx)) {
    g.solve_deferred[gb] = true;                        // goes out with the next trial factorisation (ngd_trial_state)
    return GVI_OK;
  }
  GVICK(ngd_flush_assemble(ctx, gb));
  const GradBuf e = grad_buf(ctx, gb);
  return run_bt_solve(ctx, e.D, e.U, e.g, -1.0, g.dmu2[gb].d());
}

// a reader of dmu / [g | V_D | V_U] of gradient buffer gb other than the next trial: a parked solve that nobody fused with a
// factorisation runs now, in stream order, on the second workspace; a pending assemble goes with it, or alone
static gvi_status ngd_join_solve(gvi_ctx* ctx, int gb) {
  NgdState& g = ctx->ngd;
  if (!g.solve_deferred[gb]) return ngd_flush_assemble(ctx, gb);
  g.solve_deferred[gb] = false;
  const GradBuf e = grad_buf(ctx, gb);
  if (!g.asm_pending[gb]) return run_bt_solve(ctx, e.D, e.U, e.g, -1.0, g.dmu2[gb].d(), 1);
  g.asm_pending[gb] = false;
  ChainWs w;
  GVICK(ensure_chain_ws(ctx, 1, w));
  ChainArgs a1 = make_chain_args(ctx, w, e.D, e.U, e.g, -1.0, false, nullptr, nullptr, g.dmu2[gb].d(), nullptr);
  a1.asm_on = 1; a1.asmG = e.g; a1.asmD = e.D; a1.asmU = e.U;
  const AsmList AL = make_asm_list(ctx);
  return run_chain(ctx, a1, a1, false, true, &AL);
}

gvi_status gvi_ngd_gradients_local(gvi_ctx* ctx) {
  GVICK(ngd_check(ctx));
  HIPCK(ctx, hipSetDevice(ctx->device));
  ctx->ngd.grad_valid = false;
  return ngd_grad_local(ctx, ctx->ngd.cur, ctx->ngd.gcur);
}

gvi_status gvi_ngd_gradients_finish(gvi_ctx* ctx) {
  GVICK(ngd_check(ctx));
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(ngd_grad_finish(ctx, ctx->ngd.gcur));
  ctx->ngd.grad_valid = true;
  ctx->ngd.grad_slot = ctx->ngd.cur;
  return GVI_OK;
}

gvi_status gvi_ngd_gradients(gvi_ctx* ctx) {
  GVICK(gvi_ngd_gradients_local(ctx));
  GVICK(dist_exchange0(ctx, ctx->ngd.gcur));
  return gvi_ngd_gradients_finish(ctx);
}

// trial proposal into the other slot: state, chain factorisation (log-det + marginals), gather
static gvi_status ngd_trial_state(gvi_ctx* ctx, double step) {
  NgdState& g = ctx->ngd;
  if (!(g.grad_valid && g.grad_slot == g.cur)) return fail(ctx, GVI_ERR_STATE, "call gvi_ngd_gradients first");
  const size_t Tn = (size_t)ctx->T * ctx->n, bt = bt_count(ctx);
  const int c = g.cur, t = 1 - c;
  const GradBuf e = grad_buf(ctx, g.gcur);
  g.cost_valid[t] = false;
  g.spec_ready = false;
  if (g.solve_deferred[g.gcur]) {
    // Lam_trial formed and factorised (log-det + marginals) and the parked gradient solve, side by side in three launches.
    // Lam_trial = Lam + step (V - Lam) is formed by the first pass of the factorisation while it loads the chain (and written
    // to Lam[t] there): "Lam[c] mixed with V" is factorised, no trial_kernel goes first.
    const size_t T = ctx->T, Tnn = T * nn_(ctx);
    const TrialMix mix{e.D, g.Lam[t].d(), step};
    ChainWs w0, w1;
    GVICK(ensure_chain_ws(ctx, 0, w0));
    GVICK(ensure_chain_ws(ctx, 1, w1));
    double* sD = g.Sig[t].d();
    ChainArgs a0 = make_chain_args(ctx, w0, g.Lam[c].d(), g.Lam[c].d() + Tnn, nullptr, 1.0, true, sD, sD + Tnn, nullptr, g.hld[t].d(), &mix);
    ChainArgs a1 = make_chain_args(ctx, w1, e.D, e.U, e.g, -1.0, false, nullptr, nullptr, g.dmu2[g.gcur].d(), nullptr);
    if (g.asm_pending[g.gcur]) {
      // the assemble of this gradient buffer was left to these launches: both operations form V from the per-factor
      // results while they load, the solve leaves [g | V_D | V_U] in the buffer (later trials of this iteration read it)
      g.asm_pending[g.gcur] = false;
      a0.asm_on = a1.asm_on = 1;
      a1.asmG = e.g; a1.asmD = e.D; a1.asmU = e.U;
      const AsmList AL = make_asm_list(ctx);
      GVICK(run_chain(ctx, a0, a1, true, true, &AL));
    } else GVICK(run_chain(ctx, a0, a1, true, true));
    g.solve_deferred[g.gcur] = false;
    // mu_trial and the gather ride in the prep launch of the cost pass
    GVICK(ngd_gather_with_prep(ctx, t, g.mu[c].d(), g.dmu2[g.gcur].d(), step));
  } else {
    hipLaunchKernelGGL(trial_kernel, dim3((unsigned)((Tn + bt + 255) / 256)), dim3(256), 0, ctx->stream, (int64_t)Tn,
                       (int64_t)bt, step, g.mu[c].d(), g.dmu2[g.gcur].d(), g.Lam[c].d(), e.D,
                       g.mu[t].d(), g.Lam[t].d());
    HIPCK(ctx, hipGetLastError());
    GVICK(ngd_refresh(ctx, t));
  }
  g.have_trial = true;
  return GVI_OK;
}

gvi_status gvi_ngd_trial_local(gvi_ctx* ctx, double step) {
  GVICK(ngd_check(ctx));
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(ngd_trial_state(ctx, step));
  return ngd_cost_local(ctx, 1 - ctx->ngd.cur);
}

gvi_status gvi_ngd_trial_finish(gvi_ctx* ctx, double* new_cost) {
  GVICK(ngd_check(ctx));
  if (!ctx->ngd.have_trial) return fail(ctx, GVI_ERR_STATE, "no trial pending");
  HIPCK(ctx, hipSetDevice(ctx->device));
  return ngd_cost_finish(ctx, 1 - ctx->ngd.cur, new_cost);
}

gvi_status gvi_ngd_trial(gvi_ctx* ctx, double step, double* new_cost) {
  GVICK(gvi_ngd_trial_local(ctx, step));
  GVICK(dist_exchange1(ctx));
  return gvi_ngd_trial_finish(ctx, new_cost);
}

// ---- split / speculative forms for the sharded driver: publish the (all-reduced) trial cost without waiting, queue the
// NEXT iteration's gradients at the trial state into the other gradient buffer behind it, then wait and decide ----
gvi_status gvi_ngd_trial_publish(gvi_ctx* ctx) {
  GVICK(ngd_check(ctx));
  if (!ctx->ngd.have_trial) return fail(ctx, GVI_ERR_STATE, "no trial pending");
  HIPCK(ctx, hipSetDevice(ctx->device));
  return ngd_cost_publish(ctx, 1 - ctx->ngd.cur);
}

gvi_status gvi_ngd_trial_wait(gvi_ctx* ctx, double* new_cost) {
  GVICK(ngd_check(ctx));
  if (!ctx->ngd.have_trial) return fail(ctx, GVI_ERR_STATE, "no trial pending");
  return ngd_cost_wait(ctx, 1 - ctx->ngd.cur, new_cost);
}

gvi_status gvi_ngd_spec_gradients_local(gvi_ctx* ctx) {
  GVICK(ngd_check(ctx));
  if (!ctx->ngd.have_trial) return fail(ctx, GVI_ERR_STATE, "no trial pending");
  HIPCK(ctx, hipSetDevice(ctx->device));
  ctx->ngd.spec_ready = false;
  return ngd_grad_local(ctx, 1 - ctx->ngd.cur, 1 - ctx->ngd.gcur);
}

gvi_status gvi_ngd_spec_gradients_finish(gvi_ctx* ctx) {
  GVICK(ngd_check(ctx));
  if (!ctx->ngd.have_trial) return fail(ctx, GVI_ERR_STATE, "no trial pending");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(ngd_grad_finish(ctx, 1 - ctx->ngd.gcur));
  ctx->ngd.spec_ready = true;
  return GVI_OK;
}

// after an accept: the gradients queued at the trial state (the other buffer) are those of the current state
static void take_spec_gradients(NgdState& g) { g.gcur = 1 - g.gcur; g.grad_valid = true; g.grad_slot = g.cur; }

gvi_status gvi_ngd_accept_spec(gvi_ctx* ctx) {
  GVICK(ngd_check(ctx));
  if (!ctx->ngd.spec_ready) return fail(ctx, GVI_ERR_STATE, "no speculative gradients at the trial state");
  GVICK(gvi_ngd_accept(ctx));
  take_spec_gradients(ctx->ngd);
  ctx->ngd.spec_ready = false;
  return GVI_OK;
}

gvi_status gvi_ngd_accept(gvi_ctx* ctx) {
  GVICK(ngd_check(ctx));
  if (!ctx->ngd.have_trial) return fail(ctx, GVI_ERR_STATE, "no trial pending");
  GVICK(ngd_flush_gather(ctx, 1 - ctx->ngd.cur));      // no-op once the trial's cost pass has run
  ctx->ngd.cur = 1 - ctx->ngd.cur;
  ctx->ngd.have_trial = false;
  ctx->ngd.grad_valid = false;
  return GVI_OK;
}

// Cost and gradients at the current state for the start of an iteration.  When NEITHER is there yet (first iteration after
// gvi_ngd_init) one full moments pass serves both -- its m0 column is the cost, exactly as in a fused trial -- instead of a
// cost-only pass followed by the gradient pass.
static gvi_status ngd_iteration_entry(gvi_ctx* ctx, double* c0) {
  NgdState& g = ctx->ngd;
  const bool have_grad = g.grad_valid && g.grad_slot == g.cur;
  if (!g.cost_valid[g.cur] && !have_grad && ctx->opt.fuse_trial != 0 && !dist_on(ctx) && !ctx->sets.empty()) {
    ctx->ngd.solve_deferred[g.gcur] = false;
    GVICK(ngd_moments_full(ctx, g.cur, g.cur));          // epilogue + ordered cost sum + publish in one launch
    GVICK(ngd_scatter(ctx, g.cur, g.gcur));
    GVICK(ngd_grad_finish(ctx, g.gcur));
    g.grad_valid = true; g.grad_slot = g.cur;
    return ngd_cost_wait(ctx, g.cur, c0);
  }
  GVICK(gvi_ngd_cost(ctx, c0));
  if (!have_grad) GVICK(gvi_ngd_gradients(ctx));         // else: computed speculatively
  return GVI_OK;
}

// The backtracking loop of one iteration from trial number `cnt` on (step = the step of the LAST trial taken, or the base
// before the first): step *= 0.75 per trial, first decrease accepted, give up after max_backtrack + 1 trials.
static gvi_status ngd_linesearch(gvi_ctx* ctx, double c0, double step, int cnt, int max_backtrack, double* c1_out, int* ok_out,
                                 int* cnt_out) {
  NgdState& g = ctx->ngd;
  double c1 = c0;
  int ok = 0;
  while (true) {
    step *= 0.75;                                  // gvibase/GVI-GH-impl.h:83
    const int t = 1 - g.cur;
    const bool spec = cnt == 0 && ctx->speculate;
    GVICK(ngd_trial_state(ctx, step));
    const bool fuse = spec && (ctx->opt.fuse_trial == 1 || (ctx->opt.fuse_trial == 2 && ctx->ngd.last_first_accepted));
    if (fuse) {
      // Fused form: ONE full moments pass at the trial point serves both the trial cost (its m0 column)
      // and -- if the trial is accepted -- the next iteration's gradients.  Same numbers, one psi pass
      // less per accepted iteration; a rejected first trial wasted the moment accumulation.
      if (dist_on(ctx)) {
        // sharded: the local cost sum and the local [g | D | U] go through the two exchanges before publish / solve
        // (ONE all-gather: the partial cost sum rides with the gradient records; the publish follows it)
        GVICK(ngd_moments_full(ctx, t));
        GVICK(dist_ranges(ctx));
        hipLaunchKernelGGL(cost_sum_all_kernel, dim3(1), dim3(256), 0, ctx->stream, make_set_list(ctx, t), g.exch1.d(),
                           ctx->dist.send.d() + (size_t)ctx->dist.maxlen * (ctx->n + 2 * nn_(ctx)));
        HIPCK(ctx, hipGetLastError());
        GVICK(ngd_scatter(ctx, t, 1 - g.gcur));               // also writes this rank's records
        GVICK(dist_exchange0(ctx, 1 - g.gcur, true, t));      // all-gather, fold, ordered cost total, publish
        GVICK(ngd_grad_finish(ctx, 1 - g.gcur));
      } else if (ctx->sets.empty()) {
        HIPCK(ctx, hipMemsetAsync(g.exch1.p, 0, 8, ctx->stream));
        GVICK(ngd_cost_publish(ctx, t));
      } else {
        GVICK(ngd_moments_full(ctx, t, t));           // epilogue + ordered cost sum + publish in one launch
      }
      if (!dist_on(ctx)) {
        GVICK(ngd_scatter(ctx, t, 1 - g.gcur));
        GVICK(ngd_grad_finish(ctx, 1 - g.gcur));
      }
    } else {
      if (dist_on(ctx)) {
        GVICK(ngd_cost_local(ctx, t, false));
        GVICK(dist_exchange1(ctx));
        GVICK(ngd_cost_publish(ctx, t));
      } else {
        GVICK(ngd_cost_local(ctx, t, true));        // cost tail publishes in the same launch
      }
      // Speculation: the first trial is accepted in the common case, and then the next iteration starts
      // with the gradients at exactly this trial state.  Queue them BEHIND the publish, into the other
      // gradient buffer, so the device never idles while the host reads the cost and decides.  A rejected
      // trial just leaves that buffer unused (same numbers either way).
      if (spec) {
        GVICK(ngd_grad_local(ctx, t, 1 - g.gcur));
        GVICK(dist_exchange0(ctx, 1 - g.gcur));
        GVICK(ngd_grad_finish(ctx, 1 - g.gcur));
      }
    }
    GVICK(ngd_cost_wait(ctx, t, &c1));
    ++cnt;
    if (cnt == 1) ctx->ngd.last_first_accepted = c1 < c0;
    if (c1 < c0) {                                 // NaN compares false -> rejected
      GVICK(gvi_ngd_accept(ctx));
      if (spec) take_spec_gradients(g);
      ok = 1;
      break;
    }
    if (cnt > max_backtrack) break;
  }
  *c1_out = c1; *ok_out = ok; *cnt_out = cnt;
  return GVI_OK;
}

gvi_status gvi_ngd_step(gvi_ctx* ctx, double step_size_base, int max_backtrack, double* cost_iter, int* accepted,
                        double* new_cost, int* ntrials) {
  GVICK(ngd_check(ctx));
  if (ctx->update_rule != GVI_RULE_NGD) return fail(ctx, GVI_ERR_STATE, "proximal rule selected: use gvi_prox_step");
  HIPCK(ctx, hipSetDevice(ctx->device));
  double c0 = 0.0;
  GVICK(ngd_iteration_entry(ctx, &c0));
  if (cost_iter) *cost_iter = c0;
  double c1 = c0;
  int cnt = 0, ok = 0;
  GVICK(ngd_linesearch(ctx, c0, step_size_base, 0, max_backtrack, &c1, &ok, &cnt));
  if (accepted) *accepted = ok;
  if (new_cost) *new_cost = ok ? c1 : c0;
  if (ntrials) *ntrials = cnt;
  return GVI_OK;
}
