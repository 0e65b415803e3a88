// gvi_ngd_run: the iteration loop, pipelined one iteration deep.  A fragment of the library's one translation unit, included
// by gvi_hip.hip inside its extern "C" bracket; not a stand-alone header.
//
//   holds      PipeSnapshot with pipe_save / pipe_restore; PipeWindowScope; pipe_ok; pipe_enqueue
//   relies on  host_ctx.inc (gvi_ctx::PipeWindow, NgdBook); ngd_stage.inc (ngd_cost_wait); ngd_dist.inc (dist_on); ngd_iter.inc
//              (ngd_iteration_entry, ngd_trial_state, ngd_moments_full, ngd_scatter, ngd_grad_finish, ngd_linesearch,
//              take_spec_gradients, dual_solve, gvi_ngd_step, gvi_ngd_accept)
//   defines    gvi_ngd_run

// ---- gvi_ngd_run: the iteration loop, pipelined one iteration deep ----
// gvi_ngd_step queues an iteration, waits for its trial cost on the host, decides, and only then queues the next one: the
// device idles for the host's wake-up + launch latency (4-7 us of a 0.14 ms iteration in the kernel trace).  Here the launches
// of iteration i + 1 are queued BEFORE the host has read the cost of iteration i, assuming its first trial is accepted (it
// is, in the steady state); they are PREDICATED on a device word that the tail of iteration i sets only if its cost
// decreased (same comparison, same doubles as the host's), so a rejected trial turns them into no-ops, the host rolls its
// bookkeeping back and continues that iteration's backtracking exactly as gvi_ngd_step would.  Same numbers either way
// (tests/test_gpu_parity.py::test_ngd_run_equals_the_same_sequence_of_steps, with rejected first trials).
namespace {
struct PipeSnapshot {
  NgdBook book;
  std::vector<int> prep_slot, warm_count;
};

void pipe_save(const gvi_ctx* c, PipeSnapshot& p) {
  p.book = c->ngd;
  p.prep_slot.clear(); p.warm_count.clear();
  for (const auto& s : c->sets) { p.prep_slot.push_back(s->prep_slot); p.warm_count.push_back(s->warm_count); }
}

void pipe_restore(gvi_ctx* c, const PipeSnapshot& p) {
  static_cast<NgdBook&>(c->ngd) = p.book;
  for (size_t i = 0; i < c->sets.size(); ++i) { c->sets[i]->prep_slot = p.prep_slot[i]; c->sets[i]->warm_count = p.warm_count[i]; }
}

// the pipelined run's window (gvi_ctx::PipeWindow) for the launches queued during the lifetime; the plain iteration again on
// every way out
struct PipeWindowScope {
  gvi_ctx* c;
  PipeWindowScope(gvi_ctx* ctx, const gvi_ctx::PipeWindow& w) : c(ctx) { c->pipe = w; }
  ~PipeWindowScope() { c->pipe = gvi_ctx::PipeWindow(); }
  PipeWindowScope(const PipeWindowScope&) = delete;
  PipeWindowScope& operator=(const PipeWindowScope&) = delete;
};

// every launch of a queued iteration must be one of the predicated kernels: the dual chain launches, the fused factor pass or
// the prep launch with the fused gather + the sets' moments launches (every MomArgs / OrbitArgs kernel) + the epilogue with its
// tail, the assemble
bool pipe_ok(const gvi_ctx* c) {
  if (!c->opt.pipeline || dist_on(c) || c->update_rule != GVI_RULE_NGD || !c->speculate || c->opt.fuse_trial == 0) return false;
  if (!dual_solve(c)) return false;
  if (!c->opt.fuse_gather || !c->opt.pair_fuse || c->profile_all || c->sets.empty() || (int)c->sets.size() > MAX_SETS) return false;
  for (const auto& s : c->sets)
    if (s->K <= 0 || psi_kind_is<PSI_NO_DEVICE>(s->kind)) return false;       // (host-evaluated psi: the host is in the loop anyway)
  return true;
}
}  // namespace

// one iteration's launches with a fused first trial (the non-sharded branch of ngd_linesearch, first trial), queued in
// the window w
static gvi_status pipe_enqueue(gvi_ctx* ctx, double step, const gvi_ctx::PipeWindow& w) {
  PipeWindowScope window(ctx, w);
  NgdState& g = ctx->ngd;
  const int t = 1 - g.cur;
  GVICK(ngd_trial_state(ctx, step));
  GVICK(ngd_moments_full(ctx, t, t));
  GVICK(ngd_scatter(ctx, t, 1 - g.gcur));
  return ngd_grad_finish(ctx, 1 - g.gcur);
}

gvi_status gvi_ngd_run(gvi_ctx* ctx, int max_iters, double step_size_base, int max_backtrack, double* cost_iter,
                       int* accepted, double* new_cost, int* ntrials, int* iters_done) {
  GVICK(ngd_check(ctx));
  if (max_iters < 0) return fail(ctx, GVI_ERR_ARG, "max_iters < 0");
  if (ctx->update_rule != GVI_RULE_NGD) return fail(ctx, GVI_ERR_STATE, "proximal rule selected: use gvi_prox_step");
  HIPCK(ctx, hipSetDevice(ctx->device));
  NgdState& g = ctx->ngd;
  int done = 0;
  auto record = [&](double c0, int ok, double c1, int nt) {
    if (cost_iter) cost_iter[done] = c0;
    if (accepted) accepted[done] = ok;
    if (new_cost) new_cost[done] = c1;
    if (ntrials) ntrials[done] = nt;
    ++done;
  };
  auto finish = [&](gvi_status st) {
    if (iters_done) *iters_done = done;
    return st;
  };
  gvi_status plain_st = GVI_OK;
  auto plain_iteration = [&]() {     // one gvi_ngd_step, recorded; false: the run ends here (plain_st)
    double c0 = 0.0, c1 = 0.0;
    int ok = 0, nt = 0;
    plain_st = gvi_ngd_step(ctx, step_size_base, max_backtrack, &c0, &ok, &c1, &nt);
    if (plain_st != GVI_OK) return false;
    record(c0, ok, c1, nt);
    return ok != 0;
  };
  bool pending = false;          // the launches of iteration `done` are already queued (speculatively; their predicate held)
  double pend_seq = 0.0;
  int pend_ring = 0;
  const double step1 = step_size_base * 0.75;
  while (done < max_iters) {
    const bool fused_first = ctx->opt.fuse_trial == 1 || (ctx->opt.fuse_trial == 2 && g.last_first_accepted);
    if (!pending && !(pipe_ok(ctx) && fused_first)) {
      if (!plain_iteration()) return finish(plain_st);
      continue;
    }
    double c0 = 0.0, seq_i = 0.0;
    int ring_i = 0;
    if (!pending) {
      gvi_status st = ngd_iteration_entry(ctx, &c0);
      if (st != GVI_OK) return finish(st);
      if (!g.solve_deferred[g.gcur]) {                          // not in the dual-launch state
        if (!plain_iteration()) return finish(plain_st);
        continue;
      }
      if (!ctx->pipe_dev.p) {
        HIPCK(ctx, ctx->pipe_dev.ensure(64));
        HIPCK(ctx, hipMemsetAsync(ctx->pipe_dev.p, 0, 64, ctx->stream));
      }
      gvi_ctx::PipeWindow w;
      w.tail = true; w.c0 = c0;                                 // unpredicated, the current cost as an immediate, ring slot 0
      st = pipe_enqueue(ctx, step1, w);
      if (st != GVI_OK) return finish(st);
      seq_i = ctx->seq; ring_i = 0;
    } else {
      c0 = g.cost[g.cur]; seq_i = pend_seq; ring_i = pend_ring;
    }
    // queue iteration i + 1 behind it, predicated on the acceptance of trial i
    const bool spec_next = done + 1 < max_iters;
    PipeSnapshot snap;
    double seq_n = 0.0;
    if (spec_next) {
      pipe_save(ctx, snap);
      gvi_status st = gvi_ngd_accept(ctx);                      // provisional: cur <- trial slot
      if (st != GVI_OK) { pipe_restore(ctx, snap); return finish(st); }
      take_spec_gradients(g);
      g.last_first_accepted = true;
      // (the accept words alternate like the host slots: this iteration's own tail writes the OTHER word, so its assemble,
      // which runs after that tail, still sees the predicate it was queued under)
      gvi_ctx::PipeWindow w;
      w.pred = ctx->pipe_dev.d() + ring_i; w.pred_val = seq_i;
      w.tail = true; w.c0_imm = false; w.pub_ring = 1 - ring_i;
      st = pipe_enqueue(ctx, step1, w);
      if (st != GVI_OK) { pipe_restore(ctx, snap); return finish(st); }   // undo the provisional accept (cur / gcur flipped)
      seq_n = ctx->seq;
    }
    const int ti = spec_next ? g.cur : 1 - g.cur;                // NGD slot of trial i
    double c1 = 0.0;
    {
      const gvi_status st = ngd_cost_wait(ctx, ti, &c1, seq_i, ring_i);
      if (st != GVI_OK) { if (spec_next) pipe_restore(ctx, snap); return finish(st); }
    }
    if (c1 < c0) {                                               // accepted (NaN compares false)
      g.last_first_accepted = true;
      if (!spec_next) {
        const gvi_status st = gvi_ngd_accept(ctx);
        if (st != GVI_OK) return finish(st);
        take_spec_gradients(g);
      }
      record(c0, 1, c1, 1);
      pending = spec_next; pend_seq = seq_n; pend_ring = 1 - ring_i;
      continue;
    }
    // first trial rejected: the device skipped everything queued for iteration i + 1
    if (spec_next) pipe_restore(ctx, snap);
    pending = false;
    g.last_first_accepted = false;
    double c1b = c0;
    int ok = 0, cnt = 1;
    if (cnt <= max_backtrack) {
      const gvi_status st = ngd_linesearch(ctx, c0, step1, 1, max_backtrack, &c1b, &ok, &cnt);
      if (st != GVI_OK) return finish(st);
    }
    record(c0, ok, ok ? c1b : c0, cnt);
    if (!ok) break;
  }
  return finish(GVI_OK);
}
