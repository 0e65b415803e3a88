// Posterior queries of the C ABI (include/gvi_hip.h): samples and log-density of q, many right-hand sides and covariance
// columns, the dense-time posterior, costs of sampled trajectories.  Host code only, included once by gvi_hip.hip behind its
// own entry points; the state lives in gvi_ctx::post.  The entry points are declared extern "C" by the header.
//
// Every query entry is written against two rules (DESIGN.md section 10.1):
//   checks   its preconditions are a Query, evaluated by query_check in ONE order; a host call and its _dev twin share a body
//   staging  a buffer is sized and cut by carve() alone; (D, U) go up through put_chain(); results come back through copy_out()

static const char MSG_NULL[] = "NULL argument";
static const char MSG_NMAX[] = "state_dim > 16";
static_assert(SAMPLE_NMAX == 16 && SOLVE_NMAX == 16 && INTERP_NMAX == 16, "one state_dim rule for every query");

// ---- the check order ----
static gvi_status scost_check_set(gvi_ctx* ctx, const FactorSet& s, bool clearance) {
  if (psi_kind_is<PSI_NO_DEVICE>(s.kind)) return fail(ctx, GVI_ERR_UNSUPPORTED, "a PSI_HOST_CALLBACK set has no device psi");
  if (clearance && !psi_kind_is<PSI_CLEARANCE>(s.kind)) return fail(ctx, GVI_ERR_UNSUPPORTED, "clearance needs a hinge-on-SDF set");   // text kept for its callers; HINGE_BOX and HINGE_HALFSPACE sets pass too
  if (psi_kind_is<PSI_SUMSQ>(s.kind) && s.d > SCOST_DMAX) return fail(ctx, GVI_ERR_UNSUPPORTED, "factor dimension > 32");
  if (psi_kind_is<PSI_ARM>(s.kind) && !s.arm.p)
    return fail(ctx, GVI_ERR_STATE, "HINGE_SDF_3D_ARM set without an arm model: call gvi_factors_set_arm");
  if (psi_kind_is<PSI_SDF>(s.kind) && s.sdf_rows == 0)
    return fail(ctx, GVI_ERR_STATE, "HINGE_SDF set without a grid: call gvi_factors_set_sdf2d / gvi_factors_set_sdf3d");
  return GVI_OK;
}

// every set of the context can be evaluated on the device (gvi_sample_costs / gvi_ngd_sample_costs)
static gvi_status scost_check_all(gvi_ctx* ctx, int clearance_set) {
  if ((int)ctx->sets.size() > MAX_SETS) return fail(ctx, GVI_ERR_UNSUPPORTED, "more than 8 factor sets");
  for (int i = 0; i < (int)ctx->sets.size(); ++i) GVICK(scost_check_set(ctx, *ctx->sets[i], i == clearance_set));
  return GVI_OK;
}

// What a query call requires, in the order query_check evaluates it.  A field left at its default is no requirement.
enum Eval { EVAL_NONE, EVAL_SET, EVAL_ALL };
struct Query {
  const char* count_name = nullptr;   // "S" / "R" / "ncols": `count` may not be negative
  int count = 0;
  bool ptrs = true;                   // every required pointer was given ...
  bool chain = false;                 // ... and the call takes (D, U): U may be NULL on a single-state chain only
  const void* U = nullptr;
  int64_t first = 0;
  bool set_required = false;          // `set` names a set; otherwise a negative `set` means none
  int set = -1;
  bool ngd = false;                   // resident state
  bool nmax = false;                  // state_dim <= 16
  const int32_t* nodes = nullptr;     // `count` nodes inside [0, T)
  bool interp = false;                // a query set is held
  Eval eval = EVAL_NONE;              // `set` (as a cost or as a clearance set) / every set can be evaluated on the device
  bool clearance = false;
};

// OK: the caller returns at once on a zero count (the last rule of the order) and otherwise goes to work
static gvi_status query_check(gvi_ctx* ctx, const Query& q) {
  if (!ctx) return GVI_ERR_ARG;
  if (q.count < 0) return fail(ctx, GVI_ERR_ARG, std::string(q.count_name) + " < 0");
  if (ctx->T < 1) return fail(ctx, GVI_ERR_STATE, "call gvi_chain_set first");
  if (!q.ptrs || (q.chain && !q.U && ctx->T > 1)) return fail(ctx, GVI_ERR_ARG, MSG_NULL);
  if (q.first < 0) return fail(ctx, GVI_ERR_ARG, "first < 0");
  if (q.set >= (int)ctx->sets.size() || (q.set_required && q.set < 0)) return fail(ctx, GVI_ERR_ARG, "bad set id");
  if (q.ngd) GVICK(ngd_check(ctx));
  if (q.nmax && ctx->n > SAMPLE_NMAX) return fail(ctx, GVI_ERR_UNSUPPORTED, MSG_NMAX);
  if (q.nodes) {
    for (int c = 0; c < q.count; ++c)
      if (q.nodes[c] < 0 || q.nodes[c] >= ctx->T) return fail(ctx, GVI_ERR_ARG, "node outside [0, T)");
    if ((int64_t)q.count * ctx->n > INT32_MAX) return fail(ctx, GVI_ERR_ARG, "ncols * state_dim exceeds 2^31 - 1");
  }
  if (q.interp && ctx->post.itp_Q < 1) return fail(ctx, GVI_ERR_STATE, "call gvi_interp_set first");
  if (q.eval == EVAL_SET) return scost_check_set(ctx, *ctx->sets[q.set], q.clearance);
  if (q.eval == EVAL_ALL) return scost_check_all(ctx, q.set);
  return GVI_OK;
}

// ---- staging (carve / put_chain: gvi_hip.hip) ----
static size_t Tn_(const gvi_ctx* c) { return (size_t)c->T * c->n; }
static size_t Tnn_(const gvi_ctx* c) { return (size_t)c->T * nn_(c); }

// results of a host call back to the caller (a NULL host pointer: not asked for), then the closing synchronisation
struct Out { void* host; const double* dev; size_t doubles; };
static gvi_status copy_out(gvi_ctx* ctx, std::initializer_list<Out> outs) {
  for (const Out& o : outs)
    if (o.host) GVICK(d2h(ctx, o.host, o.dev, o.doubles * 8));
  return sync(ctx);
}

// the resident state the gvi_ngd_* queries read; it never leaves HBM, no ChainArgs is built and nothing the iteration reads
// is written
struct Resident { const double *D, *U, *mu, *SigD, *SigU; };
static Resident resident(const gvi_ctx* ctx) {
  const NgdState& g = ctx->ngd;
  const size_t Tnn = Tnn_(ctx);
  return {g.Lam[g.cur].d(), g.Lam[g.cur].d() + Tnn, g.mu[g.cur].d(), g.Sig[g.cur].d(), g.Sig[g.cur].d() + Tnn};
}

// ---- launch plan of the per-sample / per-right-hand-side sweeps (kernels_sample.hpp, kernels_solve.hpp) ----
static_assert(SAMPLE_LDS_BYTES == SOLVE_LDS_BYTES && SAMPLE_TILE_MAX == SOLVE_TILE_MAX && SAMPLE_SWEEP_THREADS == SOLVE_SWEEP_THREADS,
              "sweep_plan serves the sample sweep and the solve sweep");
struct SweepPlan { bool lds; int tile; unsigned grid; size_t ldsb; };
static SweepPlan sweep_plan(int count, int T, int n, bool lds_allowed) {
  const size_t rowb = (size_t)T * n * 8;
  SweepPlan p;
  p.lds = lds_allowed && rowb <= (size_t)SAMPLE_LDS_BYTES;
  const int cap = p.lds ? std::min<int>(SAMPLE_TILE_MAX, (int)(SAMPLE_LDS_BYTES / rowb)) : SAMPLE_TILE_MAX;
  p.tile = std::max(1, std::min(cap, (count + 511) / 512));     // >= 512 workgroups while the count allows, then longer tiles
  p.grid = (unsigned)((count + p.tile - 1) / p.tile);
  p.ldsb = p.lds ? (size_t)p.tile * rowb : 0;
  return p;
}

// the sweeps are instantiated for state dimensions up to 4, 8 and 16: f(std::integral_constant<int, N>)
template <class F>
static gvi_status by_state_dim(int n, F&& f) {
  if (n <= 4) return f(std::integral_constant<int, 4>{});
  if (n <= 8) return f(std::integral_constant<int, 8>{});
  return f(std::integral_constant<int, 16>{});
}

template <class Kernel, class Args>
static gvi_status launch_sweep(gvi_ctx* c, const SweepPlan& p, Kernel kern, const Args& a) {
  if (p.lds) GVICK(allow_lds(c, (const void*)kern, SAMPLE_LDS_BYTES));
  hipLaunchKernelGGL(kern, dim3(p.grid), dim3(SAMPLE_SWEEP_THREADS), p.ldsb, c->stream, a);
  HIPCK(c, hipGetLastError());
  return GVI_OK;
}

// ---- sampling and log-density of q = N(mu, Lambda^-1) (kernels_sample.hpp) ----
// Factorisation of Lambda = (D, U) on the context stream: every node's R, GA, GB and the half log-det, left in smp_ws
// (fa says where).  One launch of sample_factor_kernel per level.  Shared by the samplers and the multi-solve.
static gvi_status run_sample_factor(gvi_ctx* c, const double* D, const double* U, SampleFactorArgs& fa) {
  const int T = c->T, n = c->n, L = chain_levels(T);
  const size_t Tnn = Tnn_(c);
  fa = SampleFactorArgs{};
  fa.T = T; fa.n = n; fa.L = L; fa.D = D; fa.U = U;
  double *Db[2], *Cb[2];
  GVICK(carve(c, c->post.smp_ws, {{&Db[0], Tnn}, {&Db[1], Tnn}, {&Cb[0], Tnn}, {&Cb[1], Tnn}, {&fa.R, Tnn}, {&fa.GA, Tnn}, {&fa.GB, Tnn},
                                  {&fa.lp, (size_t)T}, {&fa.hld, 1}}));
  for (int l = 0; l <= L; ++l) {
    fa.level = l;
    fa.Dr = Db[(l + 1) & 1]; fa.Cr = Cb[(l + 1) & 1];
    fa.Dw = Db[l & 1]; fa.Cw = Cb[l & 1];
    const int alive = (int)(((int64_t)T + (1 << l) - 1) >> l);
    hipLaunchKernelGGL(sample_factor_kernel, dim3(alive), dim3(64), 0, c->stream, fa);
  }
  HIPCK(c, hipGetLastError());
  return GVI_OK;
}

// Factorisation and sweep of S > 0 samples into the device buffer X, all on the context stream.
// Chain arguments of its own: no fused trial precision, no accept predicate, no selected inverse.
static gvi_status run_sample(gvi_ctx* c, const double* D, const double* U, const double* mu, int S, uint64_t seed, int64_t first,
                             const double* eps, double* X) {
  const int T = c->T, n = c->n;
  SampleFactorArgs fa;
  GVICK(run_sample_factor(c, D, U, fa));
  if (!c->opt.sample_sweep) return GVI_OK;
  const SweepPlan p = sweep_plan(S, T, n, true);
  SampleSweepArgs sa{};
  sa.T = T; sa.n = n; sa.L = fa.L; sa.S = S; sa.seed = seed; sa.first = first; sa.eps = eps;
  sa.R = fa.R; sa.GA = fa.GA; sa.GB = fa.GB; sa.mu = mu; sa.hld = fa.hld; sa.X = X; sa.tile = p.tile;
  return by_state_dim(n, [&](auto N) {
    constexpr int NB = decltype(N)::value;
    return p.lds ? launch_sweep(c, p, sample_sweep_kernel<NB, true>, sa) : launch_sweep(c, p, sample_sweep_kernel<NB, false>, sa);
  });
}

gvi_status gvi_randn(gvi_ctx* ctx, uint64_t seed, int64_t first, int64_t count, double* out) {
  if (!ctx) return GVI_ERR_ARG;
  if (count < 0 || first < 0) return fail(ctx, GVI_ERR_ARG, "count < 0 or first < 0");
  if (!out) return fail(ctx, GVI_ERR_ARG, MSG_NULL);
  if (count == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  double* dz;
  GVICK(carve(ctx, ctx->post.smp_io, {{&dz, (size_t)count}}));
  const int64_t pairs = ((first + count - 1) >> 1) - (first >> 1) + 1;
  hipLaunchKernelGGL(randn_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, ctx->stream, seed, first, count, dz);
  HIPCK(ctx, hipGetLastError());
  return copy_out(ctx, {{out, dz, (size_t)count}});
}

gvi_status gvi_bt_sample(gvi_ctx* ctx, const double* D, const double* U, const double* mu, int S, uint64_t seed, int64_t first,
                         const double* eps, double* X) {
  GVICK(query_check(ctx, {.count_name = "S", .count = S, .ptrs = D && mu && X, .chain = true, .U = U, .first = first, .nmax = true}));
  if (S == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t Tnn = Tnn_(ctx), Tn = Tn_(ctx), SX = (size_t)S * Tn;
  double *dD, *dU, *dmu, *dX, *deps;
  GVICK(carve(ctx, ctx->post.smp_io, {{&dD, Tnn}, {&dU, Tnn - nn_(ctx)}, {&dmu, Tn}, {&dX, SX}, {&deps, eps ? SX : 0}}));
  GVICK(put_chain(ctx, dD, dU, D, U));
  GVICK(h2d(ctx, dmu, mu, Tn * 8));
  if (eps) GVICK(h2d(ctx, deps, eps, SX * 8));
  GVICK(run_sample(ctx, dD, dU, dmu, S, seed, first, eps ? deps : nullptr, dX));
  return copy_out(ctx, {{X, dX, SX}});
}

// host call (X: host, staged) and _dev twin (X: device, asynchronous) of the resident sampler
static gvi_status ngd_sample(gvi_ctx* ctx, int S, uint64_t seed, int64_t first, double* X, bool host) {
  GVICK(query_check(ctx, {.count_name = "S", .count = S, .ptrs = X != nullptr, .first = first, .ngd = true, .nmax = true}));
  if (S == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t SX = (size_t)S * Tn_(ctx);
  double* dX = X;
  if (host) GVICK(carve(ctx, ctx->post.smp_io, {{&dX, SX}}));
  const Resident r = resident(ctx);
  GVICK(run_sample(ctx, r.D, r.U, r.mu, S, seed, first, nullptr, dX));
  return host ? copy_out(ctx, {{X, dX, SX}}) : GVI_OK;
}

gvi_status gvi_ngd_sample(gvi_ctx* ctx, int S, uint64_t seed, int64_t first, double* X) {
  return ngd_sample(ctx, S, seed, first, X, true);
}

gvi_status gvi_ngd_sample_dev(gvi_ctx* ctx, int S, uint64_t seed, int64_t first, double* X_dev) {
  return ngd_sample(ctx, S, seed, first, X_dev, false);
}

// logq [S] (device) of the device samples X under N(mu, (D, U)^-1), on the context stream: the chain kernels' half log-det
// (arguments and a workspace of its own: no mix, no predicate, no back pass) into dh [1], the quadratic forms into dQ [S][T]
static gvi_status run_logpdf(gvi_ctx* ctx, const double* dD, const double* dU, const double* dmu, int S, const double* dX,
                             double* dQ, double* dh, double* dl) {
  const int T = ctx->T, n = ctx->n, NP = chain_padded(n);
  HIPCK(ctx, ctx->post.smp_cws.ensure(chain_ws_doubles(T, NP) * 8));
  HIPCK(ctx, ctx->post.smp_cwsi.ensure(chain_lp_entries(T) * sizeof(int)));
  ChainArgs a{};
  a.T = T; a.n = n; a.need_back = 0;
  a.D = dD; a.U = dU; a.rhs_scale = 1.0;
  a.ws = ctx->post.smp_cws.d(); a.wsi = (int*)ctx->post.smp_cwsi.p; a.hld = dh;
  const hipError_t e = chain_launch(n, chain_rules(ctx), a, a, true, false, ctx->stream);
  if (e == hipErrorInvalidValue) return fail(ctx, GVI_ERR_UNSUPPORTED, "chain kernels: block size / LDS budget");
  HIPCK(ctx, e);
  const int64_t items = (int64_t)S * T;
  hipLaunchKernelGGL(logpdf_quad_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, ctx->stream, T, n, S, dD, dU, dmu, dX, dQ);
  hipLaunchKernelGGL(logpdf_reduce_kernel, dim3(S), dim3(256), 0, ctx->stream, T, n, dQ, dh, dl);
  HIPCK(ctx, hipGetLastError());
  return GVI_OK;
}

gvi_status gvi_bt_logpdf(gvi_ctx* ctx, const double* D, const double* U, const double* mu, int S, const double* X, double* logq) {
  GVICK(query_check(ctx, {.count_name = "S", .count = S, .ptrs = D && mu && X && logq, .chain = true, .U = U, .nmax = true}));
  if (S == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t Tnn = Tnn_(ctx), Tn = Tn_(ctx), SX = (size_t)S * Tn;
  double *dD, *dU, *dmu, *dX, *dQ, *dl, *dh;
  GVICK(carve(ctx, ctx->post.smp_io, {{&dD, Tnn}, {&dU, Tnn - nn_(ctx)}, {&dmu, Tn}, {&dX, SX}, {&dQ, (size_t)S * ctx->T},
                                      {&dl, (size_t)S}, {&dh, 1}}));
  GVICK(put_chain(ctx, dD, dU, D, U));
  GVICK(h2d(ctx, dmu, mu, Tn * 8));
  GVICK(h2d(ctx, dX, X, SX * 8));
  GVICK(run_logpdf(ctx, dD, dU, dmu, S, dX, dQ, dh, dl));
  return copy_out(ctx, {{logq, dl, (size_t)S}});
}


// ---- multi-right-hand-side solve and block columns of Lambda^-1 (kernels_solve.hpp) ----
// Factorisation (run_sample_factor) and sweep of R > 0 right-hand sides into the device buffer X, all on the context stream.
// B ([R][T][n], device) or, with B null, the unit columns of the device node list (R = ncols n, X = C[ncols][T][n][n]).
// Like run_sample it builds no ChainArgs.
static gvi_status run_solve(gvi_ctx* c, const double* D, const double* U, int R, const double* B, const int32_t* nodes, double* X) {
  const int T = c->T, n = c->n;
  SampleFactorArgs fa;
  GVICK(run_sample_factor(c, D, U, fa));
  if (!c->opt.sample_sweep) return GVI_OK;
  const SweepPlan p = sweep_plan(R, T, n, c->opt.solve_lds);
  SolveSweepArgs sa{};
  sa.T = T; sa.n = n; sa.L = fa.L; sa.R = R; sa.B = B; sa.nodes = nodes;
  sa.Rf = fa.R; sa.GA = fa.GA; sa.GB = fa.GB; sa.hld = fa.hld; sa.X = X; sa.tile = p.tile;
  return by_state_dim(n, [&](auto N) {
    constexpr int NB = decltype(N)::value;
    return p.lds ? launch_sweep(c, p, solve_sweep_kernel<NB, true>, sa) : launch_sweep(c, p, solve_sweep_kernel<NB, false>, sa);
  });
}

gvi_status gvi_bt_solve_multi(gvi_ctx* ctx, const double* D, const double* U, int R, const double* B, double* X) {
  GVICK(query_check(ctx, {.count_name = "R", .count = R, .ptrs = D && B && X, .chain = true, .U = U, .nmax = true}));
  if (R == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t Tnn = Tnn_(ctx), RX = (size_t)R * Tn_(ctx);
  double *dD, *dU, *dB, *dX;
  GVICK(carve(ctx, ctx->post.smp_io, {{&dD, Tnn}, {&dU, Tnn - nn_(ctx)}, {&dB, RX}, {&dX, RX}}));
  GVICK(put_chain(ctx, dD, dU, D, U));
  GVICK(h2d(ctx, dB, B, RX * 8));
  GVICK(run_solve(ctx, dD, dU, R, dB, nullptr, dX));
  return copy_out(ctx, {{X, dX, RX}});
}

// the columns of ncols > 0 nodes (host list, sent to slv_idx) of (D, U)^-1 (device) into the device buffer C
static gvi_status run_cov_columns(gvi_ctx* ctx, const double* D, const double* U, int ncols, const int32_t* nodes, double* C) {
  HIPCK(ctx, ctx->post.slv_idx.ensure((size_t)ncols * sizeof(int32_t)));
  GVICK(h2d(ctx, ctx->post.slv_idx.p, nodes, (size_t)ncols * sizeof(int32_t)));
  return run_solve(ctx, D, U, ncols * ctx->n, nullptr, ctx->post.slv_idx.i(), C);
}

gvi_status gvi_bt_cov_columns(gvi_ctx* ctx, const double* D, const double* U, int ncols, const int32_t* nodes, double* C) {
  GVICK(query_check(ctx, {.count_name = "ncols", .count = ncols, .ptrs = D && nodes && C, .chain = true, .U = U, .nmax = true,
                          .nodes = nodes}));
  if (ncols == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t Tnn = Tnn_(ctx), CX = (size_t)ncols * Tnn;
  double *dD, *dU, *dC;
  GVICK(carve(ctx, ctx->post.smp_io, {{&dD, Tnn}, {&dU, Tnn - nn_(ctx)}, {&dC, CX}}));
  GVICK(put_chain(ctx, dD, dU, D, U));
  GVICK(run_cov_columns(ctx, dD, dU, ncols, nodes, dC));
  return copy_out(ctx, {{C, dC, CX}});
}

static gvi_status ngd_cov_columns(gvi_ctx* ctx, int ncols, const int32_t* nodes, double* C, bool host) {
  GVICK(query_check(ctx, {.count_name = "ncols", .count = ncols, .ptrs = nodes && C, .ngd = true, .nmax = true, .nodes = nodes}));
  if (ncols == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t CX = (size_t)ncols * Tnn_(ctx);
  double* dC = C;
  if (host) GVICK(carve(ctx, ctx->post.smp_io, {{&dC, CX}}));
  const Resident r = resident(ctx);
  GVICK(run_cov_columns(ctx, r.D, r.U, ncols, nodes, dC));
  return host ? copy_out(ctx, {{C, dC, CX}}) : GVI_OK;
}

gvi_status gvi_ngd_cov_columns(gvi_ctx* ctx, int ncols, const int32_t* nodes, double* C) {
  return ngd_cov_columns(ctx, ncols, nodes, C, true);
}

gvi_status gvi_ngd_cov_columns_dev(gvi_ctx* ctx, int ncols, const int32_t* nodes, double* C_dev) {
  return ngd_cov_columns(ctx, ncols, nodes, C_dev, false);
}

// ---- dense-time posterior: moments and samples between the support states (kernels_interp.hpp) ----
gvi_status gvi_interp_set(gvi_ctx* ctx, int Q, const int32_t* idx, const double* A, const double* B, const double* c,
                          const double* Qt) {
  if (!ctx) return GVI_ERR_ARG;
  if (Q < 0) return fail(ctx, GVI_ERR_ARG, "Q < 0");
  if (ctx->T < 1) return fail(ctx, GVI_ERR_STATE, "call gvi_chain_set first");
  if (Q > 0 && (!idx || !A || !B)) return fail(ctx, GVI_ERR_ARG, MSG_NULL);
  if (ctx->n > INTERP_NMAX) return fail(ctx, GVI_ERR_UNSUPPORTED, MSG_NMAX);
  for (int q = 0; q < Q; ++q)
    if (idx[q] < 0 || idx[q] > ctx->T - 2) return fail(ctx, GVI_ERR_ARG, "idx outside [0, T - 2]");
  if ((int64_t)Q * ctx->n > INT32_MAX) return fail(ctx, GVI_ERR_ARG, "Q * state_dim exceeds 2^31 - 1");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));                       // a queued _dev call may still read the set being replaced
  Posterior& P = ctx->post;
  P.clear_interp();
  if (Q == 0) return GVI_OK;
  const size_t n = ctx->n, Qnn = (size_t)Q * n * n, Qn = (size_t)Q * n;
  DevMem raw;                             // A | B | c: only the packed form is kept
  double *dA, *dB, *dc;
  GVICK(carve(ctx, raw, {{&dA, Qnn}, {&dB, Qnn}, {&dc, Qn}}));
  HIPCK(ctx, P.itp_ops.ensure(Qn * (3 * n + 1) * 8));
  HIPCK(ctx, P.itp_idx.ensure((size_t)Q * sizeof(int32_t)));
  HIPCK(ctx, P.itp_bad.ensure((size_t)Q * sizeof(int32_t)));
  if (Qt) HIPCK(ctx, P.itp_qt.ensure(Qnn * 8));
  GVICK(h2d(ctx, dA, A, Qnn * 8));
  GVICK(h2d(ctx, dB, B, Qnn * 8));
  if (c) GVICK(h2d(ctx, dc, c, Qn * 8));
  if (Qt) GVICK(h2d(ctx, P.itp_qt.p, Qt, Qnn * 8));
  GVICK(h2d(ctx, P.itp_idx.p, idx, (size_t)Q * sizeof(int32_t)));
  InterpPrepArgs pa{};
  pa.Q = Q; pa.n = (int)n; pa.A = dA; pa.B = dB; pa.c = c ? dc : nullptr; pa.Qt = Qt ? P.itp_qt.d() : nullptr;
  pa.ops = P.itp_ops.d(); pa.bad = P.itp_bad.i();
  hipLaunchKernelGGL(interp_prepare_kernel, dim3(Q), dim3(64), 0, ctx->stream, pa);
  HIPCK(ctx, hipGetLastError());
  std::vector<int32_t> bad(Q);
  GVICK(d2h(ctx, bad.data(), P.itp_bad.p, (size_t)Q * sizeof(int32_t)));
  GVICK(sync(ctx));                       // raw is released on return
  int nbad = 0;
  for (int q = 0; q < Q; ++q) nbad += bad[q] != 0;
  P.itp_Q = Q; P.itp_nbad = nbad; P.itp_noise = Qt != nullptr;
  return GVI_OK;
}

gvi_status gvi_interp_info(gvi_ctx* ctx, int* Q, int* nbad) {
  if (!ctx) return GVI_ERR_ARG;
  if (Q) *Q = ctx->post.itp_Q;
  if (nbad) *nbad = ctx->post.itp_nbad;
  return GVI_OK;
}

// mean_q / cov_q (device, either may be null) of the prepared set from device (mu, SigD, SigU), on the context stream
static gvi_status run_interp_moments(gvi_ctx* c, const double* mu, const double* SigD, const double* SigU, double* mean_q,
                                     double* cov_q) {
  const Posterior& P = c->post;
  InterpMomArgs ma{};
  ma.Q = P.itp_Q; ma.n = c->n; ma.idx = P.itp_idx.i(); ma.ops = P.itp_ops.d();
  ma.Qt = P.itp_noise ? P.itp_qt.d() : nullptr;
  ma.mu = mu; ma.SigD = SigD; ma.SigU = SigU; ma.mean = mean_q; ma.cov = cov_q;
  hipLaunchKernelGGL(interp_moments_kernel, dim3(P.itp_Q), dim3(64), 0, c->stream, ma);
  HIPCK(c, hipGetLastError());
  return GVI_OK;
}

// samples per workgroup of the sweep: a power of two <= INTERP_TILE_MAX, grown only while the grid keeps INTERP_TARGET_BLOCKS
static int interp_tile(int S, int Q, int n) {
  const int64_t qblocks = ((int64_t)Q + INTERP_SWEEP_WAVES * (64 / n) - 1) / (INTERP_SWEEP_WAVES * (64 / n));
  int tile = 1;
  while (tile < INTERP_TILE_MAX && qblocks * ((S + 2 * tile - 1) / (2 * tile)) >= INTERP_TARGET_BLOCKS) tile *= 2;
  return tile;
}

// Xq [S][Q][n] (device) from X [S][T][n] (device), on the context stream
static gvi_status run_interp_sweep(gvi_ctx* c, int S, const double* X, uint64_t noise_seed, int64_t first, const double* eps,
                                   double* Xq) {
  const Posterior& P = c->post;
  const int n = c->n, Q = P.itp_Q;
  InterpSweepArgs sa{};
  sa.T = c->T; sa.n = n; sa.Q = Q; sa.S = S; sa.tile = interp_tile(S, Q, n);
  sa.noise = P.itp_noise ? 1 : 0; sa.noise_seed = noise_seed; sa.first = first;
  sa.idx = P.itp_idx.i(); sa.ops = P.itp_ops.d(); sa.bad = P.itp_bad.i(); sa.eps = eps; sa.X = X; sa.Xq = Xq;
  const int qpb = INTERP_SWEEP_WAVES * (64 / n);
  const dim3 grid((unsigned)((Q + qpb - 1) / qpb), (unsigned)((S + sa.tile - 1) / sa.tile)), blk(INTERP_SWEEP_WAVES * 64);
  if (grid.y > 65535u) return fail(c, GVI_ERR_ARG, "S exceeds 65535 sample tiles");
  return by_state_dim(n, [&](auto N) -> gvi_status {
    hipLaunchKernelGGL(interp_sweep_kernel<decltype(N)::value>, grid, blk, 0, c->stream, sa);
    HIPCK(c, hipGetLastError());
    return GVI_OK;
  });
}

gvi_status gvi_bt_interp(gvi_ctx* ctx, const double* mu, const double* SigD, const double* SigU, double* mean_q, double* cov_q) {
  GVICK(query_check(ctx, {.ptrs = mu && SigD && SigU && mean_q && cov_q, .interp = true}));
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t Tnn = Tnn_(ctx), Tn = Tn_(ctx), Qn = (size_t)ctx->post.itp_Q * ctx->n, Qnn = Qn * ctx->n;
  double *dmu, *dSD, *dSU, *dm, *dc;
  GVICK(carve(ctx, ctx->post.smp_io, {{&dmu, Tn}, {&dSD, Tnn}, {&dSU, Tnn - nn_(ctx)}, {&dm, Qn}, {&dc, Qnn}}));
  GVICK(h2d(ctx, dmu, mu, Tn * 8));
  GVICK(put_chain(ctx, dSD, dSU, SigD, SigU));
  GVICK(run_interp_moments(ctx, dmu, dSD, dSU, dm, dc));
  return copy_out(ctx, {{mean_q, dm, Qn}, {cov_q, dc, Qnn}});
}

static gvi_status ngd_interp(gvi_ctx* ctx, double* mean_q, double* cov_q, bool host) {
  GVICK(query_check(ctx, {.ptrs = mean_q && cov_q, .ngd = true, .interp = true}));
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t Qn = (size_t)ctx->post.itp_Q * ctx->n, Qnn = Qn * ctx->n;
  double *dm = mean_q, *dc = cov_q;
  if (host) GVICK(carve(ctx, ctx->post.smp_io, {{&dm, Qn}, {&dc, Qnn}}));
  const Resident r = resident(ctx);
  GVICK(run_interp_moments(ctx, r.mu, r.SigD, r.SigU, dm, dc));
  return host ? copy_out(ctx, {{mean_q, dm, Qn}, {cov_q, dc, Qnn}}) : GVI_OK;
}

gvi_status gvi_ngd_interp(gvi_ctx* ctx, double* mean_q, double* cov_q) { return ngd_interp(ctx, mean_q, cov_q, true); }

gvi_status gvi_ngd_interp_dev(gvi_ctx* ctx, double* mean_q_dev, double* cov_q_dev) {
  return ngd_interp(ctx, mean_q_dev, cov_q_dev, false);
}

gvi_status gvi_bt_interp_samples(gvi_ctx* ctx, int S, const double* X, uint64_t noise_seed, int64_t first, const double* eps,
                                 double* Xq) {
  GVICK(query_check(ctx, {.count_name = "S", .count = S, .ptrs = X && Xq, .first = first, .interp = true}));
  if (S == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t SX = (size_t)S * Tn_(ctx), SQ = (size_t)S * ctx->post.itp_Q * ctx->n;
  double *dX, *dXq, *deps;
  GVICK(carve(ctx, ctx->post.smp_io, {{&dX, SX}, {&dXq, SQ}, {&deps, eps ? SQ : 0}}));
  GVICK(h2d(ctx, dX, X, SX * 8));
  if (eps) GVICK(h2d(ctx, deps, eps, SQ * 8));
  GVICK(run_interp_sweep(ctx, S, dX, noise_seed, first, eps ? deps : nullptr, dXq));
  return copy_out(ctx, {{Xq, dXq, SQ}});
}

// X is optional in both variants: a _dev call that does not ask for the support samples keeps them in the staging buffer
static gvi_status ngd_sample_interp(gvi_ctx* ctx, int S, uint64_t seed, uint64_t noise_seed, int64_t first, double* X, double* Xq,
                                    bool host) {
  GVICK(query_check(ctx, {.count_name = "S", .count = S, .ptrs = Xq != nullptr, .first = first, .ngd = true, .nmax = true,
                          .interp = true}));
  if (S == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t SX = (size_t)S * Tn_(ctx), SQ = (size_t)S * ctx->post.itp_Q * ctx->n;
  double *dX = X, *dXq = Xq;
  if (host) GVICK(carve(ctx, ctx->post.smp_io, {{&dX, SX}, {&dXq, SQ}}));
  else if (!X) GVICK(carve(ctx, ctx->post.smp_io, {{&dX, SX}}));
  const Resident r = resident(ctx);
  GVICK(run_sample(ctx, r.D, r.U, r.mu, S, seed, first, nullptr, dX));
  if (!ctx->opt.sample_sweep) return host ? sync(ctx) : GVI_OK;
  GVICK(run_interp_sweep(ctx, S, dX, noise_seed, first, nullptr, dXq));
  return host ? copy_out(ctx, {{X, dX, SX}, {Xq, dXq, SQ}}) : GVI_OK;
}

gvi_status gvi_ngd_sample_interp(gvi_ctx* ctx, int S, uint64_t seed, uint64_t noise_seed, int64_t first, double* X, double* Xq) {
  return ngd_sample_interp(ctx, S, seed, noise_seed, first, X, Xq, true);
}

gvi_status gvi_ngd_sample_interp_dev(gvi_ctx* ctx, int S, uint64_t seed, uint64_t noise_seed, int64_t first, double* X_dev,
                                     double* Xq_dev) {
  return ngd_sample_interp(ctx, S, seed, noise_seed, first, X_dev, Xq_dev, false);
}

// ---- costs of sampled trajectories (kernels_sample_cost.hpp) ----
static int64_t scost_total_factors(const gvi_ctx* ctx) {
  int64_t K = 0;
  for (auto& s : ctx->sets) K += s->K;
  return K;
}

// ONE launch over the sets [lo, hi): cost (device, or null) is [S][ld] with the sets' columns side by side from column 0;
// clr (device, or null) is [S][ld_clr] of set clr_set.  X is a device buffer; everything on the context stream.
static gvi_status run_sample_cost(gvi_ctx* c, int lo, int hi, int S, const double* X, double* cost, int64_t ld, int clr_set,
                                  double* clr, int64_t ld_clr) {
  SampleCostList L{};
  L.T = c->T; L.n = c->n; L.S = S; L.X = X;
  int64_t nb = 0, koff = 0;
  int dmax = 0;
  for (int i = lo; i < hi; ++i) {
    FactorSet& s = *c->sets[i];
    double* cp = cost ? cost + koff : nullptr;
    double* kp = i == clr_set ? clr : nullptr;
    koff += s.K;
    if (s.K == 0 || (!cp && !kp)) continue;
    const int j = L.nsets++;
    L.f[j] = s.dev(c->opt); L.start[j] = s.dstart.i();
    L.cost[j] = cp; L.clr[j] = kp; L.ld_cost[j] = ld; L.ld_clr[j] = ld_clr;
    L.boff[j] = (int)nb;
    if (psi_kind_is<PSI_SUMSQ>(s.kind)) {
      // tiles of 4 G factors; the samples are cut into chunks only as far as the grid needs them (a block loads its rows of A once)
      const int F = SCOST_WAVES * (64 / scost_group(s.m));
      const int ft = (s.K + F - 1) / F;
      const int nsc = std::max(1, std::min(S, (SCOST_TARGET_BLOCKS + ft - 1) / ft));
      L.ftiles[j] = ft;
      L.schunk[j] = (S + nsc - 1) / nsc;
      nb += (int64_t)ft * ((S + L.schunk[j] - 1) / L.schunk[j]);
      dmax = std::max(dmax, s.d);
    } else {
      nb += ((int64_t)s.K * S + SCOST_THREADS - 1) / SCOST_THREADS;
    }
    if (nb > 0x7fffffffLL) return fail(c, GVI_ERR_ARG, "S * K exceeds the grid");
  }
  L.boff[L.nsets] = (int)nb;
  if (L.nsets == 0) return GVI_OK;
  const dim3 grid((unsigned)nb), blk(SCOST_THREADS);
  if (dmax <= 4) hipLaunchKernelGGL(sample_cost_kernel<4>, grid, blk, 0, c->stream, L);
  else if (dmax <= 8) hipLaunchKernelGGL(sample_cost_kernel<8>, grid, blk, 0, c->stream, L);
  else if (dmax <= 12) hipLaunchKernelGGL(sample_cost_kernel<12>, grid, blk, 0, c->stream, L);
  else if (dmax <= 16) hipLaunchKernelGGL(sample_cost_kernel<16>, grid, blk, 0, c->stream, L);
  else if (dmax <= 24) hipLaunchKernelGGL(sample_cost_kernel<24>, grid, blk, 0, c->stream, L);
  else hipLaunchKernelGGL(sample_cost_kernel<32>, grid, blk, 0, c->stream, L);
  HIPCK(c, hipGetLastError());
  return GVI_OK;
}

// scost_ws of the total-cost calls.  A host call stages its results in front (J; the resident call logq and clr_min too); then
// the cost matrix [S][all factors], the clearance matrix [S][K of clr_set] and, for the resident call, the log-density's
// quadratic forms [S][T] and half log-det.
struct CostWs { double *J, *logq, *clr, *cost_m, *clr_m, *Q, *hld; };
static gvi_status cost_ws(gvi_ctx* c, int S, int clr_set, bool resident_call, bool host, CostWs& w) {
  const size_t s = S, res = host ? s : 0, res2 = resident_call ? res : 0, one = resident_call ? 1 : 0;
  const size_t Kt = scost_total_factors(c), Kc = clr_set >= 0 ? c->sets[clr_set]->K : 0;
  return carve(c, c->post.scost_ws, {{&w.J, res}, {&w.logq, res2}, {&w.clr, res2}, {&w.cost_m, s * Kt}, {&w.clr_m, s * Kc},
                                     {&w.Q, one * s * c->T}, {&w.hld, one}});
}

// J [S] and, for clr_set >= 0, clr_min [S] (device buffers) of the device samples X: the launch over every set into the
// matrices of w, then the ordered reduction
static gvi_status run_sample_costs_total(gvi_ctx* c, int S, const double* X, double* J, int clr_set, double* clr_min, const CostWs& w) {
  const bool want_clr = clr_set >= 0 && clr_min;
  const int64_t Kt = scost_total_factors(c), Kc = want_clr ? c->sets[clr_set]->K : 0;
  GVICK(run_sample_cost(c, 0, (int)c->sets.size(), S, X, w.cost_m, Kt, want_clr ? clr_set : -1, w.clr_m, Kc));
  SampleCostReduceArgs ra{};
  ra.Kt = (int)Kt; ra.Kc = (int)Kc; ra.cost = w.cost_m; ra.clr = want_clr ? w.clr_m : nullptr; ra.J = J; ra.clr_min = clr_min;
  hipLaunchKernelGGL(sample_cost_reduce_kernel, dim3(S), dim3(256), 0, c->stream, ra);
  HIPCK(c, hipGetLastError());
  return GVI_OK;
}

// cost / clearance matrix [S][K] of one set: host call (X, out: host, staged) and _dev twin
static gvi_status sample_set_matrix(gvi_ctx* ctx, int set_id, int S, const double* X, double* out, bool clearance, bool host) {
  GVICK(query_check(ctx, {.count_name = "S", .count = S, .ptrs = X && out, .set_required = true, .set = set_id, .eval = EVAL_SET,
                          .clearance = clearance}));
  const size_t K = ctx->sets[set_id]->K, SX = (size_t)S * Tn_(ctx);
  if (S == 0 || K == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const double* dX = X;
  double* dm = out;
  if (host) {
    double* in;
    GVICK(carve(ctx, ctx->post.smp_io, {{&in, SX}}));
    GVICK(carve(ctx, ctx->post.scost_ws, {{&dm, (size_t)S * K}}));
    GVICK(h2d(ctx, in, X, SX * 8));
    dX = in;
  }
  GVICK(run_sample_cost(ctx, set_id, set_id + 1, S, dX, clearance ? nullptr : dm, (int64_t)K, clearance ? set_id : -1, dm, (int64_t)K));
  return host ? copy_out(ctx, {{out, dm, (size_t)S * K}}) : GVI_OK;
}

gvi_status gvi_sample_factor_costs(gvi_ctx* ctx, int set_id, int S, const double* X, double* cost) {
  return sample_set_matrix(ctx, set_id, S, X, cost, false, true);
}

gvi_status gvi_sample_clearance(gvi_ctx* ctx, int set_id, int S, const double* X, double* clr) {
  return sample_set_matrix(ctx, set_id, S, X, clr, true, true);
}

gvi_status gvi_sample_clearance_dev(gvi_ctx* ctx, int set_id, int S, const double* X_dev, double* clr_dev) {
  return sample_set_matrix(ctx, set_id, S, X_dev, clr_dev, true, false);
}

static gvi_status sample_costs(gvi_ctx* ctx, int S, const double* X, double* J, bool host) {
  GVICK(query_check(ctx, {.count_name = "S", .count = S, .ptrs = X && J, .eval = EVAL_ALL}));
  if (S == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const size_t SX = (size_t)S * Tn_(ctx);
  CostWs w;
  GVICK(cost_ws(ctx, S, -1, false, host, w));
  const double* dX = X;
  if (host) {
    double* in;
    GVICK(carve(ctx, ctx->post.smp_io, {{&in, SX}}));
    GVICK(h2d(ctx, in, X, SX * 8));
    dX = in;
  }
  GVICK(run_sample_costs_total(ctx, S, dX, host ? w.J : J, -1, nullptr, w));
  return host ? copy_out(ctx, {{J, w.J, (size_t)S}}) : GVI_OK;
}

gvi_status gvi_sample_costs(gvi_ctx* ctx, int S, const double* X, double* J) { return sample_costs(ctx, S, X, J, true); }

gvi_status gvi_sample_costs_dev(gvi_ctx* ctx, int S, const double* X_dev, double* J_dev) {
  return sample_costs(ctx, S, X_dev, J_dev, false);
}

// sampler -> cost launch + reduction -> log-density, all on the context stream and on device buffers.  X, logq and clr_min are
// optional in both variants; a _dev call that does not ask for the samples keeps them in the staging buffer.
static gvi_status ngd_sample_costs(gvi_ctx* ctx, int S, uint64_t seed, int64_t first, int clearance_set, double* X, double* J,
                                   double* logq, double* clr_min, bool host) {
  GVICK(query_check(ctx, {.count_name = "S", .count = S, .ptrs = J != nullptr, .first = first, .set = clearance_set, .ngd = true,
                          .nmax = true, .eval = EVAL_ALL}));
  if (S == 0) return GVI_OK;
  HIPCK(ctx, hipSetDevice(ctx->device));
  const int cs = (clearance_set >= 0 && clr_min) ? clearance_set : -1;
  const size_t SX = (size_t)S * Tn_(ctx);
  double* dX = X;
  if (host || !X) GVICK(carve(ctx, ctx->post.smp_io, {{&dX, SX}}));
  CostWs w;
  GVICK(cost_ws(ctx, S, cs, true, host, w));
  double* dJ = host ? w.J : J;
  double* dl = !logq ? nullptr : host ? w.logq : logq;
  double* dc = cs < 0 ? nullptr : host ? w.clr : clr_min;
  const Resident r = resident(ctx);
  GVICK(run_sample(ctx, r.D, r.U, r.mu, S, seed, first, nullptr, dX));
  if (!ctx->opt.sample_sweep) return host ? sync(ctx) : GVI_OK;
  GVICK(run_sample_costs_total(ctx, S, dX, dJ, cs, dc, w));
  if (dl) GVICK(run_logpdf(ctx, r.D, r.U, r.mu, S, dX, w.Q, w.hld, dl));
  if (!host) return GVI_OK;
  return copy_out(ctx, {{X, dX, SX}, {J, dJ, (size_t)S}, {logq, dl, (size_t)S}, {cs < 0 ? nullptr : clr_min, dc, (size_t)S}});
}

gvi_status gvi_ngd_sample_costs(gvi_ctx* ctx, int S, uint64_t seed, int64_t first, int clearance_set, double* X, double* J,
                                double* logq, double* clr_min) {
  return ngd_sample_costs(ctx, S, seed, first, clearance_set, X, J, logq, clr_min, true);
}

gvi_status gvi_ngd_sample_costs_dev(gvi_ctx* ctx, int S, uint64_t seed, int64_t first, int clearance_set, double* X_dev,
                                    double* J_dev, double* logq_dev, double* clr_min_dev) {
  return ngd_sample_costs(ctx, S, seed, first, clearance_set, X_dev, J_dev, logq_dev, clr_min_dev, false);
}
