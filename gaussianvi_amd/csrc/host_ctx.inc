// The types every host file works on, and the small helpers beside them.  A fragment of the library's one translation unit
// (gvi_hip.hip includes it first, behind the kernel and plan headers); not a stand-alone header.
//
//   holds      DevMem; Table and upload_table; FactorSet (and FactorSet::dev, the kernels' view of a set); NgdBook / NgdState and
//              grad_buf, the resident iteration's bookkeeping and buffers; Posterior; gvi_ctx itself; fail / HIPCK / GVICK;
//              allow_lds; StageScope; bt_count / nn_; the copies h2d / d2h and sync; pub_slot; get_set; ngd_invalidate
//   relies on  the headers gvi_hip.hip includes (FactorDev, OrbitHost, WalkPrioSet, PassRecord, Options, RouteForce ...)
//   defines    no entry point

namespace {

struct DevMem {
  void* p = nullptr;
  size_t bytes = 0;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { release(); }
  void release() { if (p) { (void)hipFree(p); p = nullptr; bytes = 0; } }
  hipError_t ensure(size_t n) {
    if (n <= bytes) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, n ? n : 8);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  double* d() const { return (double*)p; }
  int32_t* i() const { return (int32_t*)p; }
};

struct Table {
  int d = 0, p = 0;
  int64_t N = 0, Np = 0;
  DevMem Zt, w;
  DevMem Zq;               // tile-major copy [Np / 64][d + 1][64] (row d = w) read by the hand-pipelined kernels
  DevMem Zm;               // mirror-half tile-major table (one representative per +-pair), empty if the table is not symmetric
  int64_t Nm = 0, Nmp = 0;
  DevMem codes, lut;       // 8-bit node codes [d/4][Np] + value look-up (moments_split_kernel); empty when not coded
  bool coded = false;
  // sign-orbit form (orbits.hpp; moments_orbit_kernel): host copy keeps only the tile lists, the rest lives on the device
  OrbitHost orb;
  DevMem orb_cpk, orb_rpk, orb_mag, orb_w, orb_tau2;
  std::map<int, std::unique_ptr<DevMem>> orb_bounds;   // nchunk -> [nchunk + 1] tile bounds
  std::unique_ptr<WalkPrioSet> orb_walk_prio;          // costs of the four-chunk split (fused pass; made on first use)
};

struct FactorSet {
  int K = 0, d = 0, p = 0, m = 0, kind = 0, raw_stride = 0;
  std::vector<int32_t> start;
  std::shared_ptr<Table> table;
  DevMem dstart, dptr, didx, A, b, sgn, raw, temperature;
  DevMem S, Sinv, Lam, H, Hq, u0;     // per-pass products
  DevMem ones;                        // [K] unit temperatures (proximal rule: the reference's prox classes never divide by T)
  bool unit_temperature = false;
  DevMem jko_half, jko_S, jko_Sinv, jko_Lam;   // scratch of the JKO map
  DevMem sdf;                         // HINGE_SDF_* grid
  DevMem arm;                         // HINGE_SDF_3D_ARM: DH chain + collision spheres
  int sdf_rows = 0, sdf_cols = 0, sdf_nz = 1;
  double sdf_ox = 0, sdf_oy = 0, sdf_oz = 0, sdf_cell = 1;
  DevMem Vws;                         // eigenvectors of the last resident-NGD prep (Jacobi warm start)
  int warm_count = 0;                 // preps since the last cold start
  DevMem partial;
  PassRecord last;                    // the set's last moments / cost launch (routes.hpp; gvi_profile_geometry)
  int arm_ndof = 0;
  int seg_J = 0;                      // HINGE_SDF_*_SEG: check points per factor; HINGE_HALFSPACE: rows per factor
  bool closed_form = false;           // no sigma points: NGDFactorizedLinear route (sum-of-squares kinds), box_moments.hpp (HINGE_BOX, its default), halfspace_moments.hpp (HINGE_HALFSPACE, its default)
  int readout_order = 0;              // > 0: moments by the read-out-space rule of this order (gvi_factors_set_readout_rule; PSI_READOUT kinds)
  DevMem readout_rule;                // its 1-D rule [nodes (order) | weights (order)]
  bool chain_structured = false;      // start[k] == k (factor k on state k / states k, k + 1): assemble-on-load needs no CSR
  bool all_pos = false;               // every residual row has sgn = +1 (positive-definite weight)
  bool force_sym = false;             // set around passes whose caller sees the sigma points
  int prep_slot = -1;                 // NGD slot whose (mu_k, Sigma_k) the per-pass products belong to
  hipStream_t st = nullptr;           // the set's own stream: prep -> moments -> epilogue overlap across sets
  hipEvent_t done = nullptr;
  // operator outputs / NGD per-set state
  DevMem mu_k[2], Sigma_k[2], Ephi, cost, Vdmu, Vddmu, raw1, raw2, X, psi_ext;
  DevMem in_mu, in_Sigma;             // staging of the host-pointer API (never aliases NGD state)
  hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [moments|cost][start|stop]
  bool ev_set[2] = {false, false};
  ~FactorSet() {
    for (auto& a : ev) for (auto& e : a) if (e) (void)hipEventDestroy(e);
    if (done) (void)hipEventDestroy(done);
    if (st) (void)hipStreamDestroy(st);
  }
  FactorDev dev(const Options& opt) const {
    FactorDev f;
    f.K = K; f.d = d; f.m = m; f.kind = kind;
    f.N = table->N; f.Np = table->Np;
    f.Zt = table->Zt.d(); f.w = table->w.d();
    f.Zq = table->Zq.p ? table->Zq.d() : nullptr; f.all_pos = all_pos ? 1 : 0;
    f.Zm = (table->Zm.p && opt.mirror) ? table->Zm.d() : nullptr; f.Nm = table->Nm; f.Nmp = table->Nmp;
    f.codes = table->coded ? (const uint32_t*)table->codes.p : nullptr; f.lut = table->coded ? table->lut.d() : nullptr;
    f.A = A.d(); f.b = b.d(); f.sgn = sgn.d(); f.raw = raw.d(); f.raw_stride = raw_stride;
    f.temperature = unit_temperature ? ones.d() : temperature.d();
    f.S = S.d(); f.Sinv = Sinv.d(); f.Lam = Lam.d(); f.H = H.d(); f.Hq = Hq.p ? Hq.d() : nullptr; f.u0 = u0.d();
    f.Vws = nullptr; f.warm = 0; f.seg_J = seg_J; f.jko_h = 0.0; f.jtol = opt.jacobi_tol;
    f.chol = chol_products(kind, d, table->p, opt.chol_sqrt, force_sym) ? 1 : 0;
    f.sdf = sdf.d(); f.sdf_rows = sdf_rows; f.sdf_cols = sdf_cols; f.sdf_ox = sdf_ox; f.sdf_oy = sdf_oy; f.sdf_cell = sdf_cell; f.sdf_inv_cell = 1.0 / sdf_cell; f.sdf_nz = sdf_nz; f.sdf_oz = sdf_oz; f.arm = arm.p ? arm.d() : nullptr;
    return f;
  }
};

// The host's bookkeeping of the resident iteration: what is where, what is valid, what is parked.  One plain value, so that
// the pipelined run (gvi_ngd_run) takes it back after a rejected first trial by assignment: a field added here is rolled back
// with the rest.  (The sets' prep_slot / warm_count are the other part of that snapshot.)
struct NgdBook {
  int cur = 0;
  int gcur = 0;                           // gradient buffer holding the gradients of `grad_slot`
  bool grad_valid = false;
  int grad_slot = -1;
  bool cost_valid[2] = {false, false};
  double cost[2] = {0, 0};
  bool have_trial = false;
  bool spec_ready = false;            // gradients at the TRIAL state sit in exch0[1 - gcur] / dmu2[1 - gcur]
  // gather of slot i deferred into the next prep launch of that slot (ngd_prep_all) -- see PrepList
  struct GatherPending { bool on = false; const double* mu_from = nullptr; const double* dmu = nullptr; double step = 0.0; };
  GatherPending gpend[2];
  // solve_deferred[gb]: the solve of gradient buffer gb is not launched yet -- it goes out fused with the next trial
  // factorisation (the dual launch of ngd_trial_state: same three launches, no second stream), or with its first other reader
  bool solve_deferred[2] = {false, false};
  bool asm_pending[2] = {false, false};   // gradient buffer gb is NOT assembled yet (assemble-on-load, see Options::asm_on_load)
  bool last_first_accepted = true;        // adaptive fusing (Options::fuse_trial = 2)
  int64_t n_full_pass = 0, n_cost_pass = 0;   // psi passes launched over all sets (gvi_ngd_counters)
  long profile_count = 0;                 // eligible launches seen by the profile sampling (gvi_ctx::profile_every)
};
static_assert(std::is_trivially_copyable<NgdBook>::value, "the pipelined run snapshots the bookkeeping by assignment");

// Outside NgdBook, deliberately never rolled back: the device buffers (the predicated launches of a rejected iteration wrote
// nothing), and in gvi_ctx the publish sequence `seq` and the chain hand-over `chain_seq` (their numbers were handed to
// launches that stay queued, so they only ever grow) and the options (only gvi_ctx_create and the setters write them).
struct NgdState : NgdBook {
  bool ready = false;
  DevMem mu[2], Lam[2], Sig[2], hld[2];   // Lam = [D | U], Sig = [SigD | SigU]
  DevMem exch0[2], exch1;                 // gradient buffers [g | VD | VU] (double-buffered for speculation), [cost partial sum]
  DevMem dmu2[2];
  DevMem dmu, dLam, total;
};

// The three parts of a gradient buffer exch0[gb], [g (T n) | V_D (T n n) | V_U ((T - 1) n n)]: the ONE place the buffer is cut
// (grad_buf below, behind gvi_ctx, which holds T and n).  [D | U] is one block of bt_count doubles from D on.
struct GradBuf { double *g, *D, *U; };

// State of the posterior queries (posterior_host.inc)
struct Posterior {
  // samplers / log-density (kernels_sample.hpp): workspaces of their own, so that a call between NGD steps touches nothing
  // the iteration reads or writes
  DevMem smp_ws, smp_io, smp_cws, smp_cwsi;
  // multi-right-hand-side solve / covariance columns (kernels_solve.hpp): the sampler's factor workspace (smp_ws) and staging
  // (smp_io), plus the node list of the columns
  DevMem slv_idx;
  // dense-time queries (kernels_interp.hpp): the prepared set of gvi_interp_set in buffers of its own -- the samplers and the
  // solves overwrite smp_ws / smp_io, which only stage the inputs and outputs of a call here
  DevMem itp_ops, itp_qt, itp_idx, itp_bad;
  int itp_Q = 0, itp_nbad = 0;
  bool itp_noise = false;             // the set was given a Qt array
  // costs of sampled trajectories (kernels_sample_cost.hpp): the per-factor cost / clearance matrices and the staged results
  DevMem scost_ws;
  void clear_interp() { itp_Q = 0; itp_nbad = 0; itp_noise = false; }
};

}  // namespace

struct gvi_ctx {
  int device = 0, dtype = GVI_F64;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  int T = 0, n = 0;
  std::vector<std::unique_ptr<FactorSet>> sets;
  std::vector<std::shared_ptr<Table>> tables;
  NgdState ngd;
  DevMem Wbuf, Ibuf, vbuf, scratch, hldtmp;
  std::string err;
  Options opt;                        // every switch of gvi_set_option / the environment (options.hpp)
  RouteForce force = RouteForce::Auto;   // gvi_set_variant
  bool speculate = true;              // gvi_ngd_step: queue the next gradients behind the first trial (gvi_ngd_set_mode)
  bool profile = false;
  bool profile_all = false;           // events around every moments / cost launch (else: set 0, full pass only)
  int profile_every = 1;              // on = 3: bracket only every 8th dominant launch (an event pair costs ~14 us of queue gaps)
  int update_rule = 0;                // 0 natural gradient (NGD-GH), 1 proximal / JKO (ProxGVI-GH)
  DevMem Wbuf2, Ibuf2;                // second BCR workspace (the two chains are in flight together)
  // merged top + backward launch of the chain (chain_launch.hpp::ChainSync): a ring of word pairs, one pair per launch
  DevMem chain_sync;
  unsigned chain_seq = 0;
  DevMem tail_counter;                // arrival counter of cost_tail_kernel (last block reduces)
  DevMem epi_counter;                 // two-level arrival counters of epilogue_all_kernel's tail
  // ---- sharded factors (one process per GPU): the exchange steps run inside the library, on the context stream ----
  struct Dist {
    int rank = 0, world = 1;
    // all-gather of `count` doubles per rank: send [count] -> recv [world][count], ordered after / before the work on `stream`
    gvi_allgather_fn fn = nullptr;       // host-supplied collective (tests: gloo; hosts with their own transport: MPI ...)
    void* user = nullptr;
    void* rccl_lib = nullptr;            // dlopen handle; the default transport
    void* comm = nullptr;                // ncclComm_t
    int (*ncclAllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*ncclCommDestroy)(void*) = nullptr;
    DevMem send, recv, ranges;           // packed state records; [world][2] state ranges (device); cost scratch
    std::vector<int32_t> lo, hi;         // owned state range [lo, hi] of every rank (records sent)
    int maxlen = 0;
    bool rec_fresh = false;           // the last assemble wrote this rank's exchange records itself (no pack launch)
    bool ranges_valid = false;
  } dist;
  // pipelined iterations (gvi_ngd_run): what holds for EVERY launch queued while an iteration is being queued ahead -- its
  // predicate, the device-side accept decision of the tails, the ring of two host slots (a speculatively queued iteration
  // publishes into the other one).  The default value is the plain iteration; only PipeWindowScope sets another.
  struct PipeWindow {
    const double* pred = nullptr;     // predicate of the launches being queued
    double pred_val = 0.0;
    bool tail = false;                // tails take the accept decision on the device
    bool c0_imm = true;               // current cost as an immediate (known to the host) or from pipe_dev
    double c0 = 0.0;
    int pub_ring = 0;                 // host slot the next publish goes to
  } pipe;
  DevMem pipe_dev;                    // doubles: [0..1] accept words (ring), [2..3] cost of the state in NGD slot 0 / 1
  double* host_slot = nullptr;        // host-mapped {cost value, sequence}: one 16-byte device store (publish_to_host)
  // kernels whose dynamic-LDS limit was raised on THIS context's device (the attribute is per device, and a
  // process may hold contexts on several devices)
  std::set<const void*> lds_attr_done;
  // blocks of a fused instance the device holds at once, by (kernel, dynamic LDS): asked of the occupancy API once
  // (fused_round_blocks)
  std::map<std::pair<const void*, size_t>, int> fused_round;
  double seq = 0.0;
  // stage timing (gvi_profile_stages): event pairs around the chain launches / the factor pass / the assemble of the
  // resident iteration.  A pair costs ~14 us of queue gaps, so it is switched on for a few iterations OUTSIDE any timed region.
  bool stage_prof = false;
  struct StageRec { int stage; hipEvent_t e0, e1; };
  std::vector<StageRec> stage_recs;
  std::vector<hipEvent_t> stage_pool;
  double* host_slot_dev = nullptr;
  DevMem dbg_log;                     // gvi_debug_cost_log: ring of the costs the epilogue tails published, indexed by sequence
  int dbg_mask = 0;
  Posterior post;                     // state of the posterior queries (posterior_host.inc)
};

namespace {

thread_local std::string g_noctx_err;

gvi_status fail(gvi_ctx* c, gvi_status s, const std::string& msg) {
  if (c) c->err = msg; else g_noctx_err = msg;
  return s;
}

#define HIPCK(ctx, expr)                                                                       \
  do {                                                                                         \
    hipError_t e__ = (expr);                                                                   \
    if (e__ != hipSuccess)                                                                     \
      return fail(ctx, GVI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));       \
  } while (0)
#define GVICK(expr)                          \
  do {                                       \
    gvi_status s__ = (expr);                 \
    if (s__ != GVI_OK) return s__;           \
  } while (0)

// raise a kernel's dynamic-LDS limit once per context (= per device)
gvi_status allow_lds(gvi_ctx* c, const void* func, int bytes) {
  if (c->lds_attr_done.count(func)) return GVI_OK;
  HIPCK(c, hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  c->lds_attr_done.insert(func);
  return GVI_OK;
}

// stage timing: StageScope brackets the launches queued during its lifetime with an event pair (no-op unless switched on)
enum { STAGE_CHAIN = 0, STAGE_FACTORS = 1, STAGE_ASSEMBLE = 2, STAGE_COUNT = 3 };
struct StageScope {
  gvi_ctx* c;
  int idx = -1;
  StageScope(gvi_ctx* ctx, int stage) : c(ctx) {
    if (!c->stage_prof || c->stage_recs.size() >= 512) return;
    auto get = [&]() {
      hipEvent_t e = nullptr;
      if (!c->stage_pool.empty()) { e = c->stage_pool.back(); c->stage_pool.pop_back(); }
      else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
      return e;
    };
    gvi_ctx::StageRec r{stage, get(), get()};
    if (!r.e0 || !r.e1) return;
    (void)hipEventRecord(r.e0, c->stream);
    c->stage_recs.push_back(r);
    idx = (int)c->stage_recs.size() - 1;
  }
  ~StageScope() { if (idx >= 0) (void)hipEventRecord(c->stage_recs[idx].e1, c->stream); }
};

size_t bt_count(const gvi_ctx* c) { return (size_t)(2 * c->T - 1) * c->n * c->n; }   // [D | U]
size_t nn_(const gvi_ctx* c) { return (size_t)c->n * c->n; }
GradBuf grad_buf(const gvi_ctx* c, int gb) {
  double* g = c->ngd.exch0[gb].d();
  double* D = g + (size_t)c->T * c->n;
  return {g, D, D + (size_t)c->T * nn_(c)};
}

gvi_status h2d(gvi_ctx* c, void* dst, const void* src, size_t bytes) {
  HIPCK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  return GVI_OK;
}
gvi_status d2h(gvi_ctx* c, void* dst, const void* src, size_t bytes) {
  HIPCK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  return GVI_OK;
}
gvi_status sync(gvi_ctx* c) {
  // polled for a while before the blocking wait: a blocked hipStreamSynchronize wakes up 50-70 us after the stream has drained
  // (bench.py, closing synchronisation of a 2 ms timed region), a poll within a few
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipStreamQuery(c->stream);
  while (e == hipErrorNotReady && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(2)) e = hipStreamQuery(c->stream);
  if (e != hipSuccess && e != hipErrorNotReady) HIPCK(c, e);
  HIPCK(c, hipStreamSynchronize(c->stream));
  return GVI_OK;
}

gvi_status upload_table(gvi_ctx* c, Table& t, int d, int p, int64_t N, const double* Z, const double* w) {
  t.d = d; t.p = p; t.N = N; t.Np = (N + 255) / 256 * 256;   // tile kernels walk 256-point tiles
  std::vector<double> zt((size_t)d * t.Np, 0.0), wp(t.Np, 0.0);
  for (int64_t i = 0; i < N; ++i) {
    wp[i] = w[i];
    for (int a = 0; a < d; ++a) zt[(size_t)a * t.Np + i] = Z[(size_t)i * d + a];
  }
  HIPCK(c, t.Zt.ensure(zt.size() * 8));
  HIPCK(c, t.w.ensure(wp.size() * 8));
  HIPCK(c, hipMemcpy(t.Zt.p, zt.data(), zt.size() * 8, hipMemcpyHostToDevice));
  HIPCK(c, hipMemcpy(t.w.p, wp.data(), wp.size() * 8, hipMemcpyHostToDevice));
  if (d <= 12) {                          // shapes of the sreg kernels
    const size_t ntile = (size_t)t.Np / 64, rows = (size_t)d + 1;
    std::vector<double> zq(ntile * rows * 64, 0.0);
    for (int64_t i = 0; i < N; ++i) {
      const size_t base = ((size_t)i / 64) * rows * 64 + (size_t)i % 64;
      for (int a = 0; a < d; ++a) zq[base + (size_t)a * 64] = Z[(size_t)i * d + a];
      zq[base + (size_t)d * 64] = w[i];
    }
    HIPCK(c, t.Zq.ensure(zq.size() * 8));
    HIPCK(c, hipMemcpy(t.Zq.p, zq.data(), zq.size() * 8, hipMemcpyHostToDevice));
    // Mirror-half table.  Rows are in ascending lexicographic order, so the mirror image of row i is row N - 1 - i; the
    // grid of nwspgr (sym = 1: every non-zero coordinate reflected with the weight copied, nwspgr.m:108-126) is exactly
    // symmetric.  A caller-supplied table that is not keeps the unpaired kernels.
    bool sym = true;
    for (int64_t i = 0; i < N / 2 && sym; ++i) {
      sym = w[i] == w[N - 1 - i];
      for (int a = 0; a < d && sym; ++a) sym = Z[(size_t)i * d + a] == -Z[(size_t)(N - 1 - i) * d + a];
    }
    if (sym && (N & 1))
      for (int a = 0; a < d; ++a) sym = sym && Z[(size_t)(N / 2) * d + a] == 0.0;
    t.Nm = t.Nmp = 0;
    t.Zm.release();
    if (sym) {
      t.Nm = N - N / 2;                                   // upper half (first non-zero coordinate positive) + the origin
      t.Nmp = (t.Nm + 63) / 64 * 64;
      std::vector<double> zm((size_t)t.Nmp / 64 * rows * 64, 0.0);
      for (int64_t j = 0; j < t.Nm; ++j) {
        const int64_t i = N / 2 + j;                      // j = 0 is the origin when N is odd
        const size_t base = ((size_t)j / 64) * rows * 64 + (size_t)j % 64;
        for (int a = 0; a < d; ++a) zm[base + (size_t)a * 64] = Z[(size_t)i * d + a];
        zm[base + (size_t)d * 64] = ((N & 1) && j == 0) ? 0.5 * w[i] : w[i];   // the origin is its own mirror image
      }
      HIPCK(c, t.Zm.ensure(zm.size() * 8));
      HIPCK(c, hipMemcpy(t.Zm.p, zm.data(), zm.size() * 8, hipMemcpyHostToDevice));
    }
  }
  // 8-bit node codes for the split kernel: a Smolyak table has a few dozen distinct node values
  t.coded = false;
  if (d >= 16 && d % 4 == 0) {
    std::vector<double> vals{0.0};                                  // sorted distinct values
    bool ok = true;
    std::vector<uint32_t> packed((size_t)(d / 4) * t.Np, 0u);
    // pass 1: distinct values
    double last = 0.0;
    for (size_t e = 0; e < (size_t)N * d && ok; ++e) {
      const double v = Z[e];
      if (v == last) continue;
      last = v;
      auto it = std::lower_bound(vals.begin(), vals.end(), v);
      if (it == vals.end() || *it != v) {
        if (vals.size() >= 256) ok = false;
        else vals.insert(it, v);
      }
    }
    if (ok) {
      const uint32_t zero_code = (uint32_t)(std::lower_bound(vals.begin(), vals.end(), 0.0) - vals.begin());
      uint32_t zero_word = zero_code | zero_code << 8 | zero_code << 16 | zero_code << 24;
      std::fill(packed.begin(), packed.end(), zero_word);          // pad points decode to z = 0
      for (int64_t i = 0; i < N; ++i)
        for (int a = 0; a < d; ++a) {
          const uint32_t code = (uint32_t)(std::lower_bound(vals.begin(), vals.end(), Z[(size_t)i * d + a]) - vals.begin());
          uint32_t& word = packed[(size_t)(a / 4) * t.Np + i];
          word = (word & ~(255u << (8 * (a % 4)))) | code << (8 * (a % 4));
        }
      vals.resize(256, 0.0);
      HIPCK(c, t.codes.ensure(packed.size() * 4));
      HIPCK(c, t.lut.ensure(256 * 8));
      HIPCK(c, hipMemcpy(t.codes.p, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
      HIPCK(c, hipMemcpy(t.lut.p, vals.data(), 256 * 8, hipMemcpyHostToDevice));
      t.coded = true;
    }
  }
  // sign-orbit form: every table whose points come in complete sign orbits with one weight (nwspgr's do by construction)
  t.orb = OrbitHost();
  t.orb_bounds.clear();
  if (N > 1) {
    OrbitHost o = build_orbits(d, N, Z, w, true);
    if (o.ok && o.smax >= 1) {
      HIPCK(c, t.orb_cpk.ensure(o.cpk.size() * 8));
      HIPCK(c, t.orb_rpk.ensure(o.rpk.size() * 8));
      HIPCK(c, hipMemcpy(t.orb_rpk.p, o.rpk.data(), o.rpk.size() * 8, hipMemcpyHostToDevice));
      HIPCK(c, t.orb_mag.ensure(o.mag.size() * 8));
      HIPCK(c, t.orb_w.ensure(o.w.size() * 8));
      HIPCK(c, hipMemcpy(t.orb_cpk.p, o.cpk.data(), o.cpk.size() * 8, hipMemcpyHostToDevice));
      HIPCK(c, hipMemcpy(t.orb_mag.p, o.mag.data(), o.mag.size() * 8, hipMemcpyHostToDevice));
      HIPCK(c, hipMemcpy(t.orb_w.p, o.w.data(), o.w.size() * 8, hipMemcpyHostToDevice));
      HIPCK(c, t.orb_tau2.ensure(o.tau2.size() * 8));
      HIPCK(c, hipMemcpy(t.orb_tau2.p, o.tau2.data(), o.tau2.size() * 8, hipMemcpyHostToDevice));
      std::vector<uint64_t>().swap(o.cpk);
      std::vector<uint64_t>().swap(o.rpk);
      std::vector<double>().swap(o.mag);
      std::vector<double>().swap(o.w);
      t.orb = std::move(o);
    }
  }
  return GVI_OK;
}

// device address of the current publish slot (four doubles per ring entry); bit 0 tags the checked form (publish_to_host)
double* pub_slot(const gvi_ctx* c) {
  return (double*)((unsigned long long)(c->host_slot_dev + 4 * c->pipe.pub_ring) | (c->opt.safe_publish ? 1ull : 0ull));
}

FactorSet* get_set(gvi_ctx* c, int id) {
  if (!c || id < 0 || id >= (int)c->sets.size()) return nullptr;
  return c->sets[id].get();
}

// What every setter that changes what the factors compute owes the resident iteration: the costs of both slots, the
// gradients and the speculative gradients at the trial state were computed under the old setting.  Parked work (gpend,
// solve_deferred, asm_pending), have_trial and the sets' prep_slot are not its business.
void ngd_invalidate(gvi_ctx* c) {
  c->ngd.cost_valid[0] = c->ngd.cost_valid[1] = false;
  c->ngd.grad_valid = false;
  c->ngd.spec_ready = false;
}

static_assert(Options{}.split_flush == SPLIT_FLUSH, "the default of option split_flush is the split kernel's own constant");

}  // namespace
