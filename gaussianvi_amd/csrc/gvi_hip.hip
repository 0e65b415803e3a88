// C-ABI implementation (include/gvi_hip.h): context, factor sets, kernel dispatch, resident NGD state.
#include "../../include/gvi_hip.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "host_linalg.hpp"
#include "kernels_bt.hpp"
#include "chain_launch.hpp"
#include "kernels_factor.hpp"
#include "kernels_orbit.hpp"
#include "kernels_fused.hpp"
#include "kernels_block.hpp"
#include "kernels_orbit_psi.hpp"
#include "kernels_readout.hpp"
#include "kernels_sample.hpp"
#include "kernels_solve.hpp"
#include "kernels_interp.hpp"
#include "kernels_sample_cost.hpp"
#include "options.hpp"
#include "orbits.hpp"
#include "routes.hpp"
#include "spgh.hpp"

using namespace gvi;

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

// ---- the compiled instances of the factor kernels ----
// The lists with_<family>_instance, their tags and the *_supported helpers are in routes.hpp, with the decisions that ask
// them; here the launches instantiate the kernels from the tags.
template <int D, int R>
gvi_status launch_split(gvi_ctx* c, const MomArgs& a, dim3 grid, hipStream_t st) {
  const size_t lds = (size_t)SPLIT_LDS_DOUBLES(D) * 8;
  GVICK(allow_lds(c, (const void*)moments_split_kernel<D, R, true>, (int)lds));
  GVICK(allow_lds(c, (const void*)moments_split_kernel<D, R, false>, (int)lds));
  if (a.full) hipLaunchKernelGGL((moments_split_kernel<D, R, true>), grid, dim3(256), lds, st, a);
  else hipLaunchKernelGGL((moments_split_kernel<D, R, false>), grid, dim3(256), lds, st, a);
  return GVI_OK;
}

template <int D, typename Psi>
void launch_reg(const MomArgs& a, dim3 grid, hipStream_t st) {
  if (a.full) hipLaunchKernelGGL((moments_reg_kernel<D, Psi, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((moments_reg_kernel<D, Psi, false>), grid, dim3(256), 0, st, a);
}

template <int D, int M>
void launch_sreg(const MomArgs& a, dim3 grid, hipStream_t st, bool pipe) {
  if (a.full && pipe) hipLaunchKernelGGL((moments_sreg_kernel<D, M, true, true>), grid, dim3(256), 0, st, a);
  else if (a.full) hipLaunchKernelGGL((moments_sreg_kernel<D, M, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((moments_sreg_kernel<D, M, false>), grid, dim3(256), 0, st, a);
}

// ---- what the decisions of routes.hpp read of a set, its table and the context ----
RouteFacts route_facts(const FactorSet& s, bool psi_ext) {
  const Table& t = *s.table;
  RouteFacts f;
  f.kind = s.kind; f.d = s.d; f.m = s.m; f.K = s.K;
  f.closed_form = s.closed_form; f.all_pos = s.all_pos; f.psi_ext = psi_ext;
  f.readout_order = s.readout_order;
  f.has_arm = s.arm.p != nullptr; f.has_sdf = s.sdf_rows != 0;
  f.arm_ndof = s.arm_ndof; f.seg_J = s.seg_J; f.opsi_rows = psi_kind_lead(s.kind);
  f.Np = t.Np; f.Nmp = t.Nmp; f.p = t.p; f.coded = t.coded; f.has_Zq = t.Zq.p != nullptr;
  f.orb_ok = t.orb.ok; f.orb_smax = t.orb.smax; f.orb_tiles = (int64_t)t.orb.tile_s.size();
  return f;
}
RouteRules rules_of(const gvi_ctx* c) { return route_rules(c->opt, c->force); }

// ---- sign-orbit kernel (kernels_orbit.hpp) ----
// the table's sign-orbit form as kernel arguments, for a pass of nchunk chunks
gvi_status orbit_dev(gvi_ctx* c, FactorSet& s, int nchunk, OrbitDev* out) {
  Table& t = *s.table;
  auto it = t.orb_bounds.find(nchunk);
  if (it == t.orb_bounds.end()) {
    const std::vector<int32_t> b = orbit_chunk_bounds(t.orb, nchunk);
    auto mem = std::make_unique<DevMem>();
    HIPCK(c, mem->ensure(b.size() * 4));
    HIPCK(c, hipMemcpy(mem->p, b.data(), b.size() * 4, hipMemcpyHostToDevice));
    it = t.orb_bounds.emplace(nchunk, std::move(mem)).first;
  }
  OrbitDev& ob = *out;
  ob.cpk = (const uint64_t*)t.orb_cpk.p; ob.rpk = (const uint64_t*)t.orb_rpk.p; ob.mag = t.orb_mag.d(); ob.w = t.orb_w.d();
  ob.tau2 = t.orb_tau2.d();
  ob.bounds = it->second->i();
  ob.norb_p = t.orb.norb_p; ob.w0 = t.orb.w0;
  // the tile list as kernel arguments: class ends and, for up to four chunks, the chunk bounds
  int32_t cum = 0;
  for (int sz = 7; sz >= 0; --sz) {
    if (sz >= 1 && sz <= t.orb.smax) cum += t.orb.cstride[sz] / 64;           // tiles of the class
    ob.cend[sz] = sz > t.orb.smax ? 0 : cum;
  }
  for (int sz = 0; sz < 8; ++sz) {
    const bool in = sz >= 1 && sz <= t.orb.smax;
    ob.cbase[sz] = in ? t.orb.cbase[sz] : 0;
    ob.cgrp[sz] = in ? t.orb.cgrp[sz] : 1;
    ob.cstride[sz] = in ? t.orb.cstride[sz] : 0;
  }
  ob.nb = 0;
  for (int i = 0; i < 5; ++i) ob.bnd[i] = 0;
  if (nchunk <= 4) {
    const std::vector<int32_t> b = orbit_chunk_bounds(t.orb, nchunk);
    ob.nb = nchunk;
    for (int i = 0; i <= nchunk; ++i) ob.bnd[i] = b[(size_t)i];
  }
  return GVI_OK;
}

// arguments of moments_orbit_kernel for a set that orbit_supported accepts, in a pass of nchunk chunks
gvi_status orbit_args(gvi_ctx* c, FactorSet& s, int nchunk, OrbitArgs* out) {
  OrbitArgs a;
  a.H = s.H.d(); a.u0 = s.u0.d(); a.sgn = s.sgn.d(); a.partial = s.partial.d();
  a.K = s.K; a.d = s.d; a.nchunk = nchunk;
  a.pred = c->pipe.pred; a.pred_val = c->pipe.pred_val;
  // private accumulator copies: as many as the occupancy of the set's own instance leaves LDS for (160 KB per CU, 64 KB per
  // block), capped by orbit_copies
  int waves = 0;
  with_orbit_instance(s.m, s.table->orb.smax, [&](auto inst) { waves = inst.waves; });
  if (!waves) return fail(c, GVI_ERR_STATE, "orbit_args: no sign-orbit instance for this set");
  const size_t lds_cap = std::min<size_t>(64 * 1024, 160 * 1024 / waves);
  a.copies = 1;
  while (a.copies * 2 <= c->opt.orbit_copies && (size_t)4 * orbit_lds_doubles(s.d, s.m, a.copies * 2) * 8 <= lds_cap) a.copies *= 2;
  GVICK(orbit_dev(c, s, nchunk, &a.ob));
  *out = a;
  return GVI_OK;
}

template <int M, int SMAX, int WAVES>
void launch_orbit_t(const OrbitArgs& a, bool full, bool all_pos, dim3 grid, size_t lds, hipStream_t st) {
  if (full && all_pos) hipLaunchKernelGGL((moments_orbit_kernel<M, SMAX, true, false, WAVES>), grid, dim3(256), lds, st, a);
  else if (full) hipLaunchKernelGGL((moments_orbit_kernel<M, SMAX, true, true, WAVES>), grid, dim3(256), lds, st, a);
  else if (all_pos) hipLaunchKernelGGL((moments_orbit_kernel<M, SMAX, false, false, WAVES>), grid, dim3(256), lds, st, a);
  else hipLaunchKernelGGL((moments_orbit_kernel<M, SMAX, false, true, WAVES>), grid, dim3(256), lds, st, a);
}

// two sets with the same m and sgn = +1 in one launch.  e0 / e1 non-null: the launch itself carries the start / stop events
// (hipExtLaunchKernel: the kernel's own begin / end timestamps, what rocprofv3 reports -- a hipEventRecord pair around a
// 28 us launch reads ~3 us more than the kernel runs)
template <int M, int SMAX, int WAVES>
void launch_orbit_pair_t(const OrbitArgs& a0, const OrbitArgs& a1, bool full, size_t lds, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const int nbx0 = (a0.K + 3) / 4, nbx1 = (a1.K + 3) / 4;
  const int nb0 = nbx0 * a0.nchunk, nb1 = nbx1 * a1.nchunk;
  const int grid = std::max(nb0, nb1);      // block b takes item b of both sets
  if (full)
    hipExtLaunchKernelGGL((moments_orbit_pair_kernel<M, SMAX, true, false, WAVES>), dim3(grid), dim3(256), (uint32_t)lds, st, e0, e1, 0,
                          a0, a1, nbx0, nb0, nbx1);
  else
    hipExtLaunchKernelGGL((moments_orbit_pair_kernel<M, SMAX, false, false, WAVES>), dim3(grid), dim3(256), (uint32_t)lds, st, e0, e1, 0,
                          a0, a1, nbx0, nb0, nbx1);
}

// m and smax as orbit_pair_supported accepted them
void launch_orbit_pair(const OrbitArgs& a0, const OrbitArgs& a1, int m, int smax, bool full, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const size_t lds = (size_t)4 * std::max(orbit_lds_doubles(a0.d, m, a0.copies), orbit_lds_doubles(a1.d, m, a1.copies)) * 8;
  with_orbit_instance(m, smax, [&]<int M, int SMAX, int WAVES, bool PAIR>(OrbitInst<M, SMAX, WAVES, PAIR>) {
    if constexpr (PAIR) launch_orbit_pair_t<M, SMAX, WAVES>(a0, a1, full, lds, st, e0, e1);
  });
}

// Launches of factor_fused_kernel in this process, per instantiation: [0] <6,4,4,12,6>, [1] <6,6,2,12,6>, [2] <2,4,4,4,2>.
// Read-only bookkeeping for the tests (gvi_debug_fused_launches); no kernel sees it.
inline std::atomic<long long>* fused_launches() { static std::atomic<long long> c[3]; return c; }

// Launches of factor_block3_kernel in this process.  Read-only bookkeeping for the tests (gvi_debug_block3_launches); no
// kernel sees it.
inline std::atomic<long long>& block3_launches() { static std::atomic<long long> c; return c; }

// blocks of 256 threads of `kernel` with `lds` bytes of dynamic LDS that the context's device holds at once (one residency
// round): blocks per CU by the occupancy API times the CUs; asked once per (kernel, lds) and context
gvi_status fused_round_blocks(gvi_ctx* c, const void* kernel, size_t lds, int* out) {
  const auto key = std::make_pair(kernel, lds);
  auto it = c->fused_round.find(key);
  if (it == c->fused_round.end()) {
    int per_cu = 0, cus = 0;
    HIPCK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds));
    HIPCK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    it = c->fused_round.emplace(key, per_cu * cus).first;
  }
  *out = it->second;
  return GVI_OK;
}

// the full pass of the resident iteration as one launch (kernels_fused.hpp)
template <int M, int SMAX, int WAVES, int D0, int D1>
gvi_status launch_fused_t(gvi_ctx* c, FusedArgs& A, unsigned grid, size_t lds, int dmax, int copies, int items, hipEvent_t e0, hipEvent_t e1) {
  const void* const kernel = (const void*)factor_fused_kernel<M, SMAX, WAVES, D0, D1>;
  if (lds > 64 * 1024) GVICK(allow_lds(c, kernel, (int)lds));
  // the walk's priority bands only where the item blocks are all resident at once: on a longer grid the blocks of a CU are
  // of different ages anyway, and the staggered finish is what hands the next block its slot
  if (A.walk_prio) {
    int round = 0;
    GVICK(fused_round_blocks(c, kernel, lds, &round));
    if (A.nblk > round) A.walk_prio = 0;
  }
#ifdef GVI_FUSED_TIMING
  const int dbg = getenv("GVI_FUSED_DBG") ? atoi(getenv("GVI_FUSED_DBG")) : 0;
  static unsigned long long* stamps = nullptr;
  static int nprint = 0;
  constexpr size_t nstamps = 1120 + 5 * FUSED_BLOCK_STAMPS;
  if ((dbg & 8) && !stamps) {
    if (hipMalloc(&stamps, nstamps * 8) != hipSuccess) stamps = nullptr; else (void)hipMemset(stamps, 0, nstamps * 8);
    const int exp = (dbg >> 4) & 7;                           // bit 0: phase-1 priority, bits 1-2: band cuts (kernels_fused.hpp)
    (void)hipMemcpyToSymbol(HIP_SYMBOL(gvi_fused_exp), &exp, sizeof(exp));
  }
#else
  const int dbg = 0;
  unsigned long long* stamps = nullptr;
#endif
  hipExtLaunchKernelGGL((factor_fused_kernel<M, SMAX, WAVES, D0, D1>), dim3(grid), dim3(256), (uint32_t)lds, c->stream, e0, e1, 0, A, dmax, copies, items,
                        (dbg & 8) ? stamps : (unsigned long long*)nullptr);
  ++fused_launches()[M == 2 ? 2 : (SMAX <= 4 ? 0 : 1)];
#ifdef GVI_FUSED_TIMING
  if ((dbg & 8) && stamps && ++nprint > 200 && nprint <= 202) {          // a few warm launches, 100 MHz ticks
    unsigned long long h[1120];
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(h, stamps, sizeof(h), hipMemcpyDeviceToHost);
    for (int blk = 0; blk < 8; ++blk)
      for (int w = 0; w < 4; ++w)
        for (int it = 0; it < 2; ++it) {
          const unsigned long long* ws = h + 352 + ((blk * 4 + w) * 2 + it) * 12;
          fprintf(stderr, "[walk stamps] block %4d wave %d item %d: shader cycles prologue %llu | s=1 %llu (%llu tiles) | s=2 %llu (%llu) | s=3 %llu (%llu) | s=4 %llu (%llu) | reduction %llu\n",
                  blk * 146, w, it, ws[0], ws[1], ws[7], ws[2], ws[8], ws[3], ws[9], ws[4], ws[10], ws[5]);
        }
    for (int w = 0; w < 4; ++w) {
      fprintf(stderr, "[prep stamps] block 0 wave %d, us after the wave's start: prologue [arguments warm | first scalars | barrier] %.2f %.2f %.2f; gather [entry | loads back | stores issued] %.2f %.2f %.2f; products [Sigma row loaded | Cholesky | L^-1 | LDS | Lam + stores | H, u0]:",
              w, (double)(long long)(h[256 + 16 * w + 11] - h[8 * w]) * 0.01, (double)(long long)(h[256 + 16 * w + 12] - h[8 * w]) * 0.01,
              (double)(long long)(h[256 + 16 * w + 13] - h[8 * w]) * 0.01, (double)(long long)(h[256 + 16 * w + 8] - h[8 * w]) * 0.01, (double)(long long)(h[256 + 16 * w + 9] - h[8 * w]) * 0.01, (double)(long long)(h[256 + 16 * w + 10] - h[8 * w]) * 0.01);
      for (int i = 0; i < 6; ++i) fprintf(stderr, " %.2f", (double)(long long)(h[256 + 16 * w + i] - h[8 * w]) * 0.01);
      fprintf(stderr, "\n");
    }
    unsigned long long t0 = ~0ull;
    for (int blk = 0; blk < 8; ++blk) if (h[blk * 32] && h[blk * 32] < t0) t0 = h[blk * 32];
    for (int blk = 0; blk < 8; ++blk)
      for (int w = 0; w < 4; ++w) {
        const unsigned hw = (unsigned)h[320 + blk * 4 + w], xcc = (unsigned)(h[320 + blk * 4 + w] >> 32);
        fprintf(stderr, "[fused stamps] block %4d wave %d (xcc %u se %u cu %2u simd %u slot %2u; absolute, us after the first start):", blk * 146, w,
                xcc & 15, (hw >> 13) & 7, (hw >> 8) & 15, (hw >> 4) & 3, hw & 15);
        for (int i = 0; i < 8; ++i) fprintf(stderr, " %.2f", h[blk * 32 + w * 8 + i] ? (double)(long long)(h[blk * 32 + w * 8 + i] - t0) * 0.01 : -1.0);
        fprintf(stderr, "\n");
      }
    // every item block, grouped by CU: the residency slots of one CU against each other
    std::vector<unsigned long long> hb(5 * (size_t)FUSED_BLOCK_STAMPS);
    (void)hipMemcpy(hb.data(), stamps + 1120, hb.size() * 8, hipMemcpyDeviceToHost);
    struct Blk { int b; double start, p2, bar, end; unsigned slot; };
    std::map<unsigned, std::vector<Blk>> cus;                 // (xcc, se, cu) -> its blocks
    unsigned long long tb0 = ~0ull;
    for (int b = 0; b < A.nblk && b < FUSED_BLOCK_STAMPS; ++b) if (hb[(size_t)b * 5] && hb[(size_t)b * 5] < tb0) tb0 = hb[(size_t)b * 5];
    for (int b = 0; b < A.nblk && b < FUSED_BLOCK_STAMPS; ++b) {
      const unsigned long long* q = hb.data() + (size_t)b * 5;
      if (!q[0] || !q[2]) continue;
      const unsigned hw = (unsigned)q[3], xcc = (unsigned)(q[3] >> 32) & 15;
      auto us = [&](unsigned long long t) { return (double)(long long)(t - tb0) * 0.01; };
      cus[(xcc << 8) | ((hw >> 8) & 255)].push_back({b, us(q[0]), us(q[1]), us(q[2]), us(q[4]), hw & 15});   // (HW_ID bits 15:8: se_id, sh_id, cu_id)
    }
    std::vector<double> spread_bar, spread_end, first_bar, last_bar, walk_first, walk_last;
    int shown = 0;
    for (auto& [id, v] : cus) {
      std::sort(v.begin(), v.end(), [](const Blk& a, const Blk& b) { return a.bar < b.bar; });
      double e0 = 1e300, e1 = -1e300;
      for (const Blk& x : v) { e0 = std::min(e0, x.end); e1 = std::max(e1, x.end); }
      if (v.size() == 4) {
        spread_bar.push_back(v.back().bar - v.front().bar); spread_end.push_back(e1 - e0);
        first_bar.push_back(v.front().bar); last_bar.push_back(v.back().bar);
        walk_first.push_back(v.front().bar - v.front().start); walk_last.push_back(v.back().bar - v.back().start);
      }
      if (shown++ < 6)
        for (const Blk& x : v)
          fprintf(stderr, "[cu stamps] xcc %u se %u cu %2u: block %4d slot %2u, us after the first walk start: walk start %.2f, wave 0 ends phase 2 %.2f, "
                  "behind the barrier %.2f, last exit %.2f\n", id >> 8, (id >> 5) & 7, id & 31, x.b, x.slot, x.start, x.p2, x.bar, x.end);
    }
    auto stat = [](std::vector<double> v, double* med, double* mx) {
      std::sort(v.begin(), v.end());
      *med = v.empty() ? 0.0 : v[v.size() / 2]; *mx = v.empty() ? 0.0 : v.back();
    };
    double m[6], x[6];
    stat(spread_bar, &m[0], &x[0]); stat(spread_end, &m[1], &x[1]); stat(first_bar, &m[2], &x[2]); stat(last_bar, &m[3], &x[3]);
    stat(walk_first, &m[4], &x[4]); stat(walk_last, &m[5], &x[5]);
    fprintf(stderr, "[cu summary] walk_prio %d, %zu CUs with four stamped blocks (of %zu): end of phase 2 (behind the barrier), first-to-last block of a CU: "
            "median %.2f max %.2f us; first block at median %.2f, last at median %.2f max %.2f us; walk (start to barrier) of the first block median %.2f, "
            "of the last median %.2f max %.2f us; last exit, first-to-last: median %.2f max %.2f us\n", A.walk_prio, spread_bar.size(), cus.size(),
            m[0], x[0], m[2], m[3], x[3], m[4], m[5], x[5], m[1], x[1]);
  }
#endif
  return GVI_OK;
}

// prep_kernel for the f.K factors of f at (mu, Sigma) device pointers: the instance of the dimension and its LDS
gvi_status launch_prep(gvi_ctx* c, const FactorDev& f, const double* mu, const double* Sigma, hipStream_t st) {
  const int d = f.d;
  const size_t lds = prep_lds_bytes(d);
  if (d <= 8) hipLaunchKernelGGL(prep_kernel<1>, dim3(f.K), dim3(64), lds, st, f, mu, Sigma);
  else if (d <= 16) hipLaunchKernelGGL(prep_kernel<4>, dim3(f.K), dim3(64), lds, st, f, mu, Sigma);
  else if (d <= 32) hipLaunchKernelGGL(prep_kernel<16>, dim3(f.K), dim3(64), lds, st, f, mu, Sigma);
  else return fail(c, GVI_ERR_UNSUPPORTED, "factor dimension > 32");
  return GVI_OK;
}

// prep (sqrt / inverse / psi operands) for one set at (mu, Sigma) device pointers
gvi_status run_prep(gvi_ctx* c, FactorSet& s, const double* mu, const double* Sigma, int slot = -1,
                    hipStream_t st = nullptr) {
  if (!st) st = c->stream;
  if (slot >= 0 && s.prep_slot == slot) return GVI_OK;     // products of this slot are still resident
  s.prep_slot = slot;
  if (s.K == 0) return GVI_OK;
  GVICK(launch_prep(c, s.dev(c->opt), mu, Sigma, st));
  HIPCK(c, hipGetLastError());
  return GVI_OK;
}

// ---- sign-orbit kernel for the non-polynomial psi kinds (kernels_orbit_psi.hpp; selected by gvi_set_variant(7) only) ----
template <int KIND>
gvi_status launch_orbit_psi_t(gvi_ctx* c, const OrbitPsiArgs& a, bool full, dim3 grid, size_t lds, hipStream_t st) {
  if (full) {
    if (lds > 64 * 1024) GVICK(allow_lds(c, (const void*)moments_orbit_psi_kernel<KIND, true>, (int)lds));
    hipLaunchKernelGGL((moments_orbit_psi_kernel<KIND, true>), grid, dim3(256), lds, st, a);
  } else {
    hipLaunchKernelGGL((moments_orbit_psi_kernel<KIND, false>), grid, dim3(256), lds, st, a);
  }
  return GVI_OK;
}

// ---- the moments (full = 1) or cost (full = 0) pass of one set: plan, then launch ----
// A plan is a value: the route, the chunking and the kernel arguments of the launch the set would issue on its own.  The
// resident iteration plans every set once, then either fuses the launches of two or three plans or issues each one.
struct MomPlan {
  Route route = Route::Empty;
  int full = 0;
  int nchunk = 1;            // chunks per factor: what the epilogue of this pass reduces
  int64_t chunk = 0;
  MomArgs a;                 // every route but the two sign-orbit ones
  dim3 grid;                 // of the set's own launch
  OrbitArgs oa;              // Orbit
  int smax = 0;              // Orbit: the table's largest support (instance key beside m)
  OrbitPsiArgs pa;           // OrbitPsi
  size_t lds = 0;            // Orbit, OrbitPsi, Generic, Closed (HINGE_BOX, HINGE_HALFSPACE): dynamic LDS
  bool pipe = false;         // Sreg: the hand-pipelined body
  int block = 64;            // Closed (HINGE_HALFSPACE), Readout: lanes per block, 64 or 256
  const double* ro_rule = nullptr;   // Readout: the set's 1-D rule on the device and its order
  int ro_order = 0;
};
// a pass of the resident iteration over all sets: what was read, what was decided, what was bound
struct PassPlan {
  RouteFacts F[MAX_SETS];
  RouteDecision D[MAX_SETS];
  MomPlan P[MAX_SETS];
};

// grid, block and LDS of a closed-form launch, and the launch itself, per kernel of with_closed_instance (p.grid = K blocks on entry)
gvi_status plan_closed(gvi_ctx*, const FactorSet&, MomPlan&, ClosedSumsq) { return GVI_OK; }
gvi_status plan_closed(gvi_ctx* c, const FactorSet& s, MomPlan& p, ClosedBox) {
  p.lds = box_closed_lds_doubles(s.d) * 8;
  if (p.lds > BOX_CLOSED_LDS_LIMIT) return fail(c, GVI_ERR_UNSUPPORTED, "closed-form HINGE_BOX kernel LDS budget (d <= 89)");
  return GVI_OK;
}
gvi_status plan_closed(gvi_ctx*, const FactorSet& s, MomPlan& p, ClosedHalfspace) {
  // (d <= 32: decide_route)  a wave holds G = 64 / Jp factors.  One wave per block while the launch has no more waves than the chip has SIMDs
  // (256 CUs x 4): every wave can start at once wherever its block lands; above that four waves per block, a quarter
  // of the workgroups to dispatch
  const int64_t nwaves = (s.K + 64 / halfspace_group(s.seg_J) - 1) / (64 / halfspace_group(s.seg_J));
  const int wpb = nwaves <= 1024 ? 1 : 4;
  p.block = 64 * wpb;
  p.grid = dim3((unsigned)((nwaves + wpb - 1) / wpb));
  p.lds = (size_t)wpb * halfspace_closed_lds_doubles(s.d) * 8;
  return GVI_OK;
}
gvi_status launch_closed(gvi_ctx*, const MomPlan& p, hipStream_t st, ClosedSumsq) {
  hipLaunchKernelGGL(moments_closed_kernel, p.grid, dim3(64), 0, st, p.a);
  return GVI_OK;
}
gvi_status launch_closed(gvi_ctx*, const MomPlan& p, hipStream_t st, ClosedBox) {
  hipLaunchKernelGGL(moments_box_closed_kernel, p.grid, dim3(64), p.lds, st, p.a);
  return GVI_OK;
}
gvi_status launch_closed(gvi_ctx* c, const MomPlan& p, hipStream_t st, ClosedHalfspace) {
  if (p.lds > 64 * 1024) GVICK(allow_lds(c, (const void*)moments_halfspace_closed_kernel, (int)p.lds));
  hipLaunchKernelGGL(moments_halfspace_closed_kernel, p.grid, dim3(p.block), p.lds, st, p.a);
  return GVI_OK;
}

// ---- the read-out-space rule (kernels_readout.hpp; gvi_factors_set_readout_rule) ----
// One wave per factor.  As for the closed-form HINGE_HALFSPACE kernel: one wave per block while the launch has no more waves
// than the chip has SIMDs (256 CUs x 4), above that four waves per block, a quarter of the workgroups to dispatch.
constexpr int READOUT_WPB_SWITCH = 1024;
template <int P, int CLS>
gvi_status plan_readout(gvi_ctx* c, const FactorSet& s, MomPlan& p, ReadoutInst<P, CLS>) {
  const int wpb = s.K <= READOUT_WPB_SWITCH ? 1 : 4;
  p.block = 64 * wpb;
  p.grid = dim3((unsigned)((s.K + wpb - 1) / wpb));
  p.lds = (size_t)wpb * readout_lds_doubles(P, s.d, readout_check_points(CLS, s.seg_J)) * 8;
  p.ro_rule = s.readout_rule.d(); p.ro_order = s.readout_order;
  if (p.lds > 64 * 1024) return fail(c, GVI_ERR_UNSUPPORTED, "read-out rule kernel LDS budget");
  return GVI_OK;
}
template <int P, int CLS>
void launch_readout(const MomPlan& p, hipStream_t st, ReadoutInst<P, CLS>) {
  ReadoutArgs ra;
  ra.a = p.a; ra.rule = p.ro_rule; ra.order = p.ro_order;
  hipLaunchKernelGGL((moments_readout_kernel<P, CLS>), p.grid, dim3(p.block), p.lds, st, ra);
}

// Binds a decision: the partial buffer, the kernel arguments, and the sizes and refusals that take the size functions of the
// kernel headers.  Beyond its buffers it writes nothing into the set.  prep must have run for (mu, Sigma) before the plan is
// launched.
gvi_status bind_plan(gvi_ctx* c, FactorSet& s, const RouteDecision& r, const double* mu, const double* psi_ext, int full, MomPlan* out) {
  MomPlan& p = *out;
  p.route = r.route; p.full = full; p.nchunk = r.nchunk; p.chunk = r.chunk; p.pipe = r.pipe;
  if (r.route == Route::Empty) return GVI_OK;
  HIPCK(c, s.partial.ensure((size_t)s.K * r.nchunk * npairs(s.d) * 8));
  MomArgs& a = p.a;
  a.f = s.dev(c->opt); a.mu = mu; a.psi_ext = psi_ext; a.partial = s.partial.d();
  a.chunk = r.chunk; a.nchunk = r.nchunk; a.full = full; a.flush = c->opt.split_flush;
  a.mchunk = r.mchunk;
  a.pred = c->pipe.pred; a.pred_val = c->pipe.pred_val;
  p.grid = dim3(r.gx, r.gy);
  if (r.route == Route::Closed) {
    gvi_status rc = GVI_OK;
    with_closed_instance(s.kind, [&](auto inst) { rc = plan_closed(c, s, p, inst); });
    GVICK(rc);
  } else if (r.route == Route::Readout) {
    gvi_status rc = GVI_OK;
    with_readout_instance(s.kind, [&](auto inst) { rc = plan_readout(c, s, p, inst); });
    GVICK(rc);
  } else if (r.route == Route::Orbit) {
    GVICK(orbit_args(c, s, r.nchunk, &p.oa));
    p.smax = s.table->orb.smax;
    p.lds = (size_t)4 * orbit_lds_doubles(s.d, s.m, p.oa.copies) * 8;
  } else if (r.route == Route::OrbitPsi) {
    OrbitPsiArgs& pa = p.pa;
    pa.f = a.f; pa.mu = mu; pa.partial = s.partial.d(); pa.nchunk = r.nchunk;
    pa.pred = c->pipe.pred; pa.pred_val = c->pipe.pred_val;
    GVICK(orbit_dev(c, s, r.nchunk, &pa.ob));               // table pointers, class layout, chunk bounds
    const int NR = orbit_psi_rows(s.kind);
    pa.copies = 1;
    while (pa.copies * 2 <= c->opt.orbit_copies && (size_t)4 * orbit_psi_lds_doubles(s.d, NR, pa.copies * 2, true) * 8 <= 64 * 1024) pa.copies *= 2;
    p.lds = (size_t)4 * orbit_psi_lds_doubles(s.d, NR, pa.copies, full != 0) * 8;
  } else if (r.route == Route::Generic) {
    p.lds = generic_lds_bytes(s.d, s.m);
    if (p.lds > GENERIC_LDS_LIMIT) return fail(c, GVI_ERR_UNSUPPORTED, "generic kernel LDS budget");
  }
  return GVI_OK;
}

// plan = decide (a refusal becomes the context's error) + bind
gvi_status plan_moments(gvi_ctx* c, FactorSet& s, const double* mu, const double* psi_ext, int full, MomPlan* out) {
  const RouteDecision r = decide_route(route_facts(s, psi_ext != nullptr), rules_of(c), full);
  if (r.status != GVI_OK) return fail(c, r.status, r.why);
  return bind_plan(c, s, r, mu, psi_ext, full, out);
}

// the launch a plan describes, on its own
gvi_status launch_plan(gvi_ctx* c, FactorSet& s, const MomPlan& p, hipStream_t st) {
  const MomArgs& a = p.a;
  const bool full = p.full != 0;
  bool hit = true;
  gvi_status rc = GVI_OK;
  switch (p.route) {
    case Route::Empty:
      return GVI_OK;
    case Route::Closed:
      hit = with_closed_instance(s.kind, [&](auto inst) { rc = launch_closed(c, p, st, inst); });
      break;
    case Route::Orbit:
      hit = with_orbit_instance(s.m, p.smax, [&]<int M, int SMAX, int WAVES, bool PAIR>(OrbitInst<M, SMAX, WAVES, PAIR>) {
        launch_orbit_t<M, SMAX, WAVES>(p.oa, full, s.all_pos, p.grid, p.lds, st);
      });
      break;
    case Route::OrbitPsi:
      hit = with_orbit_psi_instance(s.kind, [&]<int KIND>(OrbitPsiInst<KIND>) { rc = launch_orbit_psi_t<KIND>(c, p.pa, full, p.grid, p.lds, st); });
      break;
    case Route::Split:
      hit = with_split_instance(s.d, s.m, [&]<int D, int R>(SplitInst<D, R>) { rc = launch_split<D, R>(c, a, p.grid, st); });
      break;
    case Route::Sreg:
      hit = with_sreg_instance(s.kind, s.d, s.m, [&]<int D, int M, bool PIPE>(SregInst<D, M, PIPE>) { launch_sreg<D, M>(a, p.grid, st, p.pipe); });
      break;
    case Route::Scost:
      hit = with_scost_instance(s.kind, s.d, s.m, [&]<int D, int M>(ScostInst<D, M>) {
        hipLaunchKernelGGL((moments_scost_kernel<D, M, 2>), p.grid, dim3(256), 0, st, a);
      });
      break;
    case Route::Reg:
      hit = with_reg_instance(s.kind, s.d, s.m, [&]<int D, typename Psi>(RegInst<D, Psi>) { launch_reg<D, Psi>(a, p.grid, st); });
      break;
    case Route::Generic:
      GVICK(allow_lds(c, (const void*)moments_generic_kernel, (int)GENERIC_LDS_LIMIT));
      hipLaunchKernelGGL(moments_generic_kernel, p.grid, dim3(GEN_BS), p.lds, st, a);
      break;
    case Route::Readout:
      hit = with_readout_instance(s.kind, [&](auto inst) { launch_readout(p, st, inst); });
      break;
  }
  if (!hit) return fail(c, GVI_ERR_UNSUPPORTED, "planned route without a kernel instance");
  GVICK(rc);
  HIPCK(c, hipGetLastError());
  return GVI_OK;
}

// ---- shared pieces of the resident factor stage (prep_all / epilogue_all / fused / block3 launches) ----
// warm-started Jacobi of the symmetric-root products: the set's last eigenvectors go to the launch; a cold start every 32nd
// prep bounds the drift
gvi_status warm_start_of(gvi_ctx* ctx, FactorSet& s, FactorDev& f) {
  if (!ctx->opt.warm_start) return GVI_OK;
  if (s.Vws.bytes == 0) { HIPCK(ctx, s.Vws.ensure((size_t)s.K * s.d * s.d * 8)); s.warm_count = 0; }
  f.Vws = s.Vws.d();
  f.warm = (s.warm_count % 32) != 0;
  s.warm_count++;
  return GVI_OK;
}

// The pending gather of NGD slot i goes into the launch that preps the slot (Args: PrepList / FusedArgs / Block3Args, whose
// gather fields agree).  Returns the workgroups of `block` lanes the launch needs behind its own for the trial mean.
template <class Args>
unsigned take_gather(gvi_ctx* ctx, int i, Args& A, int block) {
  NgdState& g = ctx->ngd;
  NgdState::GatherPending& gp = g.gpend[i];
  if (!gp.on) return 0;
  const size_t T = ctx->T, nn = nn_(ctx);
  A.gather = 1; A.n = ctx->n;
  A.gmu = gp.dmu ? gp.mu_from : g.mu[i].d();
  A.gdmu = gp.dmu; A.gstep = gp.step;
  A.SigD = g.Sig[i].d(); A.SigU = g.Sig[i].d() + T * nn;
  A.mu_out = g.mu[i].d(); A.nmu = (int64_t)T * ctx->n;
  gp.on = false;
  return A.gdmu ? (unsigned)((A.nmu + block - 1) / block) : 0u;
}

// The tail of a launch that ends the factor stage.  publish_slot >= 0: the launch also sums the costs of its `nitems`
// factors and publishes the cost of NGD slot `publish_slot` under the next sequence number.
gvi_status fill_epi_tail(gvi_ctx* ctx, int nitems, int publish_slot, EpiTail* out) {
  EpiTail& tail = *out;
  tail.on = 0; tail.acc = nullptr; tail.half_logdet = nullptr; tail.host_out = nullptr; tail.seq = 0.0; tail.counter = nullptr;
  tail.pred = ctx->pipe.pred; tail.pred_val = ctx->pipe.pred_val;
  tail.accept = nullptr; tail.cost_dev = nullptr; tail.slot_cur = tail.slot_trial = 0; tail.c0_use_imm = 1; tail.c0_imm = 0.0;
  tail.safe = ctx->opt.safe_publish ? 1 : 0;
  if (publish_slot < 0) return GVI_OK;
  const size_t need = (size_t)128 * (2 + (size_t)nitems / EPI_GROUP);
  if (ctx->epi_counter.bytes < need) {
    HIPCK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCK(ctx, ctx->epi_counter.ensure(need));
    HIPCK(ctx, hipMemsetAsync(ctx->epi_counter.p, 0, need, ctx->stream));
  }
  ctx->seq += 1.0;
  tail.on = 1; tail.acc = ctx->ngd.exch1.d(); tail.half_logdet = ctx->ngd.hld[publish_slot].d();
  tail.host_out = pub_slot(ctx); tail.seq = ctx->seq; tail.counter = (unsigned*)ctx->epi_counter.p;
  if (ctx->pipe.tail) {
    tail.accept = ctx->pipe_dev.d() + ctx->pipe.pub_ring; tail.cost_dev = ctx->pipe_dev.d() + 2;   // accept word of THIS ring slot
    tail.slot_cur = 1 - publish_slot; tail.slot_trial = publish_slot;
    tail.c0_use_imm = ctx->pipe.c0_imm ? 1 : 0; tail.c0_imm = ctx->pipe.c0;
  }
  return GVI_OK;
}

// ---- profile bracket of a factor launch (gvi_profile_enable / gvi_profile_last) ----
// The events live on the set the launch is booked on: s.ev[0 = moments | 1 = cost][start | stop].  Sampling: with
// profile_all every eligible launch, else every profile_every-th eligible one (profile_count).  around: the pair is recorded
// round the launch; else the launch carries e0 / e1 itself (hipExtLaunchKernelGGL).
struct ProfBracket {
  FactorSet* s = nullptr;      // null: this launch is not sampled
  int which = 0;
  bool around = true;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};
gvi_status prof_open(gvi_ctx* c, FactorSet& s, int which, bool eligible, bool around, hipStream_t st, ProfBracket* b) {
  *b = ProfBracket();
  if (!c->profile || !eligible) return GVI_OK;
  if (!c->profile_all && (c->ngd.profile_count++ % c->profile_every) != 0) return GVI_OK;
  for (int e = 0; e < 2; ++e)
    if (!s.ev[which][e]) HIPCK(c, hipEventCreate(&s.ev[which][e]));
  b->s = &s; b->which = which; b->around = around; b->st = st;
  b->e0 = s.ev[which][0]; b->e1 = s.ev[which][1];
  if (around) HIPCK(c, hipEventRecord(b->e0, st));
  return GVI_OK;
}
gvi_status prof_close(gvi_ctx* c, const ProfBracket& b) {
  if (!b.s) return GVI_OK;
  if (b.around) HIPCK(c, hipEventRecord(b.e1, b.st));
  b.s->ev_set[b.which] = true;
  return GVI_OK;
}

// what a launch owes gvi_profile_geometry: the plan it sent out for the set, and whether the other set went with it
void record_plan(FactorSet& s, const MomPlan& p, bool fused_pair) { record_pass(s.last, p.route, fused_pair, p.nchunk, p.chunk); }

// a plan's launch on its own, bracketed: every launch under profile_all, else the full pass of set 0
gvi_status launch_single(gvi_ctx* c, FactorSet& s, const MomPlan& p, hipStream_t st) {
  record_plan(s, p, false);
  if (p.route == Route::Empty) return GVI_OK;
  ProfBracket b;
  GVICK(prof_open(c, s, p.full ? 0 : 1, c->profile_all || (p.full && &s == c->sets[0].get()), true, st, &b));
  GVICK(launch_plan(c, s, p, st));
  return prof_close(c, b);
}

// moments (full=1) or cost (full=0) pass for one set; prep must have run for (mu, Sigma).  *nchunk: what run_epilogue reduces
gvi_status run_moments(gvi_ctx* c, FactorSet& s, const double* mu, const double* psi_ext, int full, int* nchunk) {
  MomPlan p;
  GVICK(plan_moments(c, s, mu, psi_ext, full, &p));
  *nchunk = p.nchunk;
  return launch_single(c, s, p, c->stream);
}

gvi_status run_epilogue(gvi_ctx* c, FactorSet& s, int full, int nchunk, double* Ephi, double* cost, double* Vdmu,
                        double* Vddmu, double* Ex, double* Exx, hipStream_t st = nullptr) {
  if (!st) st = c->stream;
  if (s.K == 0) return GVI_OK;
  EpiArgs e;
  e.f = s.dev(c->opt); e.partial = s.partial.d(); e.nchunk = nchunk; e.full = full;
  e.Ephi = Ephi; e.cost = cost; e.Vdmu = Vdmu; e.Vddmu = Vddmu; e.E_xmuphi = Ex; e.E_xxphi = Exx;
  const size_t lds = epilogue_lds_doubles(s.d) * 8;
  hipLaunchKernelGGL(epilogue_kernel, dim3(s.K), dim3(64), lds, st, e);
  HIPCK(c, hipGetLastError());
  return GVI_OK;
}

gvi_status ensure_set_buffers(gvi_ctx* c, FactorSet& s) {
  const size_t K = s.K, d = s.d;
  for (int i = 0; i < 2; ++i) {
    HIPCK(c, s.mu_k[i].ensure(K * d * 8));
    HIPCK(c, s.Sigma_k[i].ensure(K * d * d * 8));
  }
  HIPCK(c, s.Ephi.ensure(K * 8));
  HIPCK(c, s.cost.ensure(K * 8));
  HIPCK(c, s.Vdmu.ensure(K * d * 8));
  HIPCK(c, s.Vddmu.ensure(K * d * d * 8));
  return GVI_OK;
}

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

// =============================================================================================
extern "C" {

const char* gvi_version(void) { return "gvi_hip 0.1 (gfx950, fp64)"; }

const char* gvi_last_error(const gvi_ctx* ctx) { return ctx ? ctx->err.c_str() : g_noctx_err.c_str(); }

gvi_status gvi_ctx_create(int device, int dtype, gvi_ctx** out) {
  if (!out) return fail(nullptr, GVI_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (dtype == GVI_F32) return fail(nullptr, GVI_ERR_UNSUPPORTED, "GVI_F32 (config 5) is not implemented yet");
  if (dtype != GVI_F64) return fail(nullptr, GVI_ERR_ARG, "unknown dtype");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, GVI_ERR_HIP, "no HIP device: this library has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(nullptr, GVI_ERR_ARG, "device index out of range");
  if (hipSetDevice(device) != hipSuccess) return fail(nullptr, GVI_ERR_HIP, "hipSetDevice failed");
  std::unique_ptr<gvi_ctx> c(new gvi_ctx);
  c->device = device; c->dtype = dtype;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
    return fail(nullptr, GVI_ERR_HIP, "hipStreamCreate failed");
  options_from_env(c->opt, getenv);
  if (hipHostMalloc((void**)&c->host_slot, 128, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer((void**)&c->host_slot_dev, c->host_slot, 0) != hipSuccess)
    return fail(nullptr, GVI_ERR_HIP, "host-mapped slot allocation failed");
  for (int q = 0; q < 16; ++q) c->host_slot[q] = 0.0;
  *out = c.release();
  return GVI_OK;
}

gvi_status gvi_ctx_destroy(gvi_ctx* ctx) {
  if (!ctx) return GVI_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  ctx->sets.clear();
  if (ctx->dist.comm && ctx->dist.ncclCommDestroy) (void)ctx->dist.ncclCommDestroy(ctx->dist.comm);
  for (auto& r : ctx->stage_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  for (auto& e : ctx->stage_pool) (void)hipEventDestroy(e);
  if (ctx->dbg_mask) {                                          // the device-wide log pointer must not outlive its buffer
    double* lg = nullptr;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(gvi_dbg_log), &lg, sizeof(double*));
  }
  if (ctx->host_slot) (void)hipHostFree(ctx->host_slot);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return GVI_OK;
}

gvi_status gvi_ctx_set_stream(gvi_ctx* ctx, void* hip_stream) {
  if (!ctx) return GVI_ERR_ARG;
  HIPCK(ctx, hipStreamSynchronize(ctx->stream));
  if (hip_stream) {
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
  } else if (!ctx->own_stream) {
    HIPCK(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->own_stream = true;
  }
  return GVI_OK;
}

gvi_status gvi_ctx_sync(gvi_ctx* ctx) { return ctx ? sync(ctx) : GVI_ERR_ARG; }

gvi_status gvi_spgh_count(int d, int p, int64_t* N) {
  if (!N) return fail(nullptr, GVI_ERR_ARG, "N is NULL");
  const int64_t n = spgh_count(d, p);
  if (n < 0) return fail(nullptr, GVI_ERR_NOTABLE, "(d, p) outside the tabulated rules (1 <= p <= 25, d <= 64)");
  *N = n;
  return GVI_OK;
}

gvi_status gvi_spgh_nodes(int d, int p, int64_t N, double* Z, double* w, int8_t* idx) {
  SparseGrid g;
  if (spgh_generate(d, p, g)) return fail(nullptr, GVI_ERR_NOTABLE, "(d, p) outside the tabulated rules");
  if (N != g.N) return fail(nullptr, GVI_ERR_ARG, "N does not match gvi_spgh_count(d, p)");
  if (Z) memcpy(Z, g.Z.data(), g.Z.size() * 8);
  if (w) memcpy(w, g.w.data(), g.w.size() * 8);
  if (idx) memcpy(idx, g.idx.data(), g.idx.size());
  return GVI_OK;
}

gvi_status gvi_table_file_list(const char* path, int64_t cap, int64_t* count, double* dims, double* degs, int64_t* rows) {
  if (!path || !count) return GVI_ERR_ARG;
  return table_file_list(path, cap, count, dims, degs, rows) ? fail(nullptr, GVI_ERR_ARG, "cannot read table file") : GVI_OK;
}

gvi_status gvi_table_file_read(const char* path, int d, int p, int64_t* N, double* Z, double* w) {
  if (!path || !N) return GVI_ERR_ARG;
  int64_t found = 0;
  const int rc = table_file_read(path, d, p, *N, Z, w, &found);
  if (rc == 2) return fail(nullptr, GVI_ERR_NOTABLE, "key (d, p) not in the table file");
  if (rc == 3) { *N = found; return fail(nullptr, GVI_ERR_ARG, "N does not match the entry"); }
  if (rc) return fail(nullptr, GVI_ERR_ARG, "cannot read table file");
  *N = found;
  return GVI_OK;
}

gvi_status gvi_table_file_write(const char* path, int n_entries, const int32_t* dims, const int32_t* degs) {
  if (!path || n_entries < 0 || (n_entries && (!dims || !degs))) return GVI_ERR_ARG;
  const int rc = table_file_write(path, n_entries, dims, degs);
  if (rc == 2) return fail(nullptr, GVI_ERR_NOTABLE, "(d, p) outside the tabulated rules");
  return rc ? fail(nullptr, GVI_ERR_ARG, "cannot write table file") : GVI_OK;
}

gvi_status gvi_chain_set(gvi_ctx* ctx, int T, int n) {
  if (!ctx) return GVI_ERR_ARG;
  if (T < 1 || n < 1) return fail(ctx, GVI_ERR_ARG, "T and n must be >= 1");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  ctx->T = T; ctx->n = n;
  ctx->sets.clear();
  ctx->post.clear_interp();
  ctx->ngd.ready = false;
  ctx->ngd.have_trial = false;
  ctx->dist.ranges_valid = false;
  return GVI_OK;
}

// gvi_factors_add / gvi_factors_add_table: tabZ != NULL takes the caller's table (private to the set) instead of the
// generated (d, p) one
static gvi_status factors_add_impl(gvi_ctx* ctx, int K, int d, int p, const int32_t* start, int psi_kind,
                                   const double* psi_params, int64_t params_per_factor, const double* temperature,
                                   int64_t tabN, const double* tabZ, const double* tabw, int* set_id) {
  if (!ctx) return GVI_ERR_ARG;
  if (ctx->T < 1) return fail(ctx, GVI_ERR_STATE, "call gvi_chain_set first");
  // K == 0 is a valid EMPTY set: the shard of a rank that received none of a small set's factors (set ids stay
  // aligned across ranks); every launch skips it
  if (K < 0 || (K > 0 && !start)) return fail(ctx, GVI_ERR_ARG, "K < 0 or start is NULL");
  const int n = ctx->n;
  if (d != n && d != 2 * n) return fail(ctx, GVI_ERR_ARG, "factor dimension must be n or 2n");
  for (int k = 0; k < K; ++k)
    if (start[k] < 0 || (int64_t)start[k] * n + d > (int64_t)ctx->T * n)
      return fail(ctx, GVI_ERR_ARG, "start index out of range");
  int m = 0, seg_J = 0;
  int64_t need = 0;
  const char* why = nullptr;
  if (gvi_status rc = psi_kind_layout(psi_kind, d, params_per_factor, &m, &seg_J, &need, &why)) return fail(ctx, rc, why);
  if (gvi_status rc = psi_kind_check_params(psi_kind, d, seg_J, params_per_factor, K, psi_params, &why)) return fail(ctx, rc, why);
  HIPCK(ctx, hipSetDevice(ctx->device));

  std::unique_ptr<FactorSet> s(new FactorSet);
  s->unit_temperature = ctx->update_rule == GVI_RULE_PROX_JKO;    // the rule belongs to the context: a set takes it when it is added
  s->K = K; s->d = d; s->p = p; s->m = m; s->kind = psi_kind; s->seg_J = seg_J;
  s->closed_form = psi_kind_is<PSI_CLOSED_DEFAULT>(psi_kind);      // gvi_factors_set_closed_form(.., 0) for the quadrature
  if (K > 0) s->start.assign(start, start + K);
  // quadrature table: shared between sets with the same (d, p)
  if (tabZ) {
    auto t = std::make_shared<Table>();
    GVICK(upload_table(ctx, *t, d, ctx->opt.trust_table_degree ? p : -1, tabN, tabZ, tabw));
    s->table = t;
  }
  for (auto& t : ctx->tables) if (!s->table && t->d == d && t->p == p) s->table = t;
  if (!s->table) {
    SparseGrid g;
    if (spgh_generate(d, p, g)) return fail(ctx, GVI_ERR_NOTABLE, "(d, p) outside the tabulated rules");
    auto t = std::make_shared<Table>();
    GVICK(upload_table(ctx, *t, d, p, g.N, g.Z.data(), g.w.data()));
    ctx->tables.push_back(t);
    s->table = t;
  }
  // psi operands
  std::vector<double> A((size_t)K * m * d, 0.0), b((size_t)K * m, 0.0), sg((size_t)K * m, 1.0);
  if (psi_kind_is<PSI_SUMSQ>(psi_kind)) {
    const bool quad = PSI_KINDS[psi_kind].rows == M_HALF_D;      // r = Phi x1 - x2 on [Phi | Qinv], else r = x - mu0 on [mu0 | Qinv]
    std::vector<double> Q, lam, W;
    for (int k = 0; k < K; ++k) {
      const double* P = psi_params + (size_t)k * params_per_factor;
      const double* Qin = quad ? P + (size_t)m * m : P + d;
      Q.assign((size_t)m * m, 0.0);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) Q[(size_t)i * m + j] = 0.5 * (Qin[i * m + j] + Qin[j * m + i]);
      jacobi_eigh(m, Q, lam, W);
      // psi = c * r^T Qinv r = sum_r sign(e_r) (sqrt(c |e_r|) w_r^T r)^2 ,  c = 1/2 (QUAD) or 1 (FIXED)
      const double cfac = quad ? 0.5 : 1.0;
      for (int r = 0; r < m; ++r) {
        const double sc = std::sqrt(cfac * std::fabs(lam[r]));
        sg[(size_t)k * m + r] = lam[r] < 0 ? -1.0 : 1.0;
        double* Arow = &A[((size_t)k * m + r) * d];
        if (quad) {                                // r = Phi x1 - x2 = [Phi, -I] x
          for (int a = 0; a < m; ++a) {
            double acc = 0.0;
            for (int j = 0; j < m; ++j) acc += W[(size_t)j * m + r] * P[j * m + a];
            Arow[a] = sc * acc;
            Arow[m + a] = -sc * W[(size_t)a * m + r];
          }
        } else {                                   // r = x - mu0
          double off = 0.0;
          for (int a = 0; a < d; ++a) { Arow[a] = sc * W[(size_t)a * m + r]; off += Arow[a] * P[a]; }
          b[(size_t)k * m + r] = -off;
        }
      }
    }
  }
  auto up = [&](DevMem& dm, const void* src, size_t bytes) -> gvi_status {
    HIPCK(ctx, dm.ensure(bytes ? bytes : 8));
    if (bytes) HIPCK(ctx, hipMemcpy(dm.p, src, bytes, hipMemcpyHostToDevice));
    return GVI_OK;
  };
  GVICK(up(s->A, A.data(), A.size() * 8));
  GVICK(up(s->b, b.data(), b.size() * 8));
  GVICK(up(s->sgn, sg.data(), sg.size() * 8));
  s->all_pos = std::all_of(sg.begin(), sg.end(), [](double v) { return v == 1.0; });
  if (psi_kind_is<PSI_RAW>(psi_kind)) {                       // raw_stride = the kind's own block (_SEG kinds: 3 + J P (d + 1), HINGE_BOX: 4 d, HINGE_HALFSPACE: J (d + 3))
    const int np = (int)need;
    std::vector<double> raw((size_t)K * np);
    for (int k = 0; k < K; ++k) memcpy(&raw[(size_t)k * np], psi_params + (size_t)k * params_per_factor, (size_t)np * 8);
    s->raw_stride = np;
    GVICK(up(s->raw, raw.data(), raw.size() * 8));
  } else {
    GVICK(up(s->raw, nullptr, 0));
  }
  std::vector<double> temp(K, 1.0);
  if (temperature) temp.assign(temperature, temperature + K);
  GVICK(up(s->temperature, temp.data(), temp.size() * 8));
  {
    std::vector<double> one((size_t)K, 1.0);
    GVICK(up(s->ones, one.data(), one.size() * 8));
  }
  // CSR over states for the ordered assemble
  std::vector<int32_t> ptr(ctx->T + 1, 0), idx(K);
  for (int k = 0; k < K; ++k) ptr[start[k] + 1]++;
  for (int t = 0; t < ctx->T; ++t) ptr[t + 1] += ptr[t];
  {
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (int k = 0; k < K; ++k) idx[fill[start[k]]++] = k;
  }
  s->chain_structured = (d == ctx->n && K <= ctx->T) || (d == 2 * ctx->n && K <= ctx->T - 1);
  for (int k = 0; k < K && s->chain_structured; ++k) s->chain_structured = s->start[k] == k;
  GVICK(up(s->dstart, s->start.data(), (size_t)K * 4));
  GVICK(up(s->dptr, ptr.data(), ptr.size() * 4));
  GVICK(up(s->didx, idx.data(), idx.size() * 4));
  HIPCK(ctx, s->S.ensure((size_t)K * d * d * 8));
  HIPCK(ctx, s->Sinv.ensure((size_t)K * d * d * 8));
  HIPCK(ctx, s->Lam.ensure((size_t)K * d * d * 8));
  HIPCK(ctx, s->H.ensure((size_t)K * std::max(m, 1) * d * 8));
  if (split_supported(psi_kind, d, m, s->table->coded)) {           // per-wave row blocks of H for the split kernel (rows >= m stay 0)
    const size_t bytes = (size_t)K * 4 * d * ((m + 3) / 4) * 8;
    HIPCK(ctx, s->Hq.ensure(bytes));
    HIPCK(ctx, hipMemset(s->Hq.p, 0, bytes));
  }
  HIPCK(ctx, s->u0.ensure((size_t)K * std::max(m, 1) * 8));
  GVICK(ensure_set_buffers(ctx, *s));
  HIPCK(ctx, hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
  HIPCK(ctx, hipEventCreateWithFlags(&s->done, hipEventDisableTiming));
  ctx->sets.push_back(std::move(s));
  ctx->dist.ranges_valid = false;
  ctx->ngd.ready = false;
  if (set_id) *set_id = (int)ctx->sets.size() - 1;
  return GVI_OK;
}

gvi_status gvi_factors_add(gvi_ctx* ctx, int K, int d, int p, const int32_t* start, int psi_kind,
                           const double* psi_params, int64_t params_per_factor, const double* temperature,
                           int* set_id) {
  return factors_add_impl(ctx, K, d, p, start, psi_kind, psi_params, params_per_factor, temperature, 0, nullptr, nullptr, set_id);
}

gvi_status gvi_factors_add_table(gvi_ctx* ctx, int K, int d, int p, const int32_t* start, int psi_kind,
                                 const double* psi_params, int64_t params_per_factor, const double* temperature,
                                 int64_t N, const double* Z, const double* w, int* set_id) {
  if (!ctx) return GVI_ERR_ARG;
  if (N < 1 || !Z || !w) return fail(ctx, GVI_ERR_ARG, "bad table");
  return factors_add_impl(ctx, K, d, p, start, psi_kind, psi_params, params_per_factor, temperature, N, Z, w, set_id);
}

gvi_status gvi_factors_set_table(gvi_ctx* ctx, int set_id, int64_t N, const double* Z, const double* w) {
  FactorSet* s = get_set(ctx, set_id);
  if (!s) return fail(ctx, GVI_ERR_ARG, "bad set id");
  if (N < 1 || !Z || !w) return fail(ctx, GVI_ERR_ARG, "bad table");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  auto t = std::make_shared<Table>();
  GVICK(upload_table(ctx, *t, s->d, -1, N, Z, w));
  s->table = t;
  s->prep_slot = -1;
  ngd_invalidate(ctx);                // cost / gradients of the old table are stale
  return GVI_OK;
}

gvi_status gvi_factors_set_sdf2d(gvi_ctx* ctx, int set_id, double origin_x, double origin_y, double cell_size, int rows,
                                 int cols, const double* data) {
  FactorSet* s = get_set(ctx, set_id);
  if (!s) return fail(ctx, GVI_ERR_ARG, "bad set id");
  if (!psi_kind_is<PSI_SDF_2D>(s->kind))
    return fail(ctx, GVI_ERR_ARG, "set is not GVI_PSI_HINGE_SDF_2D / _2D_BODY / _2D_SEG");
  if (rows < 2 || cols < 2 || !(cell_size > 0) || !data) return fail(ctx, GVI_ERR_ARG, "bad grid");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  HIPCK(ctx, s->sdf.ensure((size_t)rows * cols * 8));
  HIPCK(ctx, hipMemcpy(s->sdf.p, data, (size_t)rows * cols * 8, hipMemcpyHostToDevice));
  s->sdf_rows = rows; s->sdf_cols = cols; s->sdf_ox = origin_x; s->sdf_oy = origin_y; s->sdf_cell = cell_size;
  ngd_invalidate(ctx);
  return GVI_OK;
}

gvi_status gvi_factors_set_sdf3d(gvi_ctx* ctx, int set_id, const double* origin, double cell_size, int rows, int cols,
                                 int nz, const double* data) {
  FactorSet* s = get_set(ctx, set_id);
  if (!s) return fail(ctx, GVI_ERR_ARG, "bad set id");
  if (!psi_kind_is<PSI_SDF_3D>(s->kind))
    return fail(ctx, GVI_ERR_ARG, "set is not GVI_PSI_HINGE_SDF_3D / _3D_ARM / _3D_SEG");
  if (rows < 2 || cols < 2 || nz < 2 || !(cell_size > 0) || !data || !origin) return fail(ctx, GVI_ERR_ARG, "bad grid");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  const size_t bytes = (size_t)rows * cols * nz * 8;
  HIPCK(ctx, s->sdf.ensure(bytes));
  HIPCK(ctx, hipMemcpy(s->sdf.p, data, bytes, hipMemcpyHostToDevice));
  s->sdf_rows = rows; s->sdf_cols = cols; s->sdf_nz = nz;
  s->sdf_ox = origin[0]; s->sdf_oy = origin[1]; s->sdf_oz = origin[2]; s->sdf_cell = cell_size;
  ngd_invalidate(ctx);
  return GVI_OK;
}

gvi_status gvi_factors_set_arm(gvi_ctx* ctx, int set_id, int ndof, const double* a, const double* alpha, const double* d,
                               const double* theta_bias, int nspheres, const int32_t* frames, const double* centers,
                               const double* radii) {
  FactorSet* s = get_set(ctx, set_id);
  if (!s) return fail(ctx, GVI_ERR_ARG, "bad set id");
  if (!psi_kind_is<PSI_ARM>(s->kind)) return fail(ctx, GVI_ERR_ARG, "set is not GVI_PSI_HINGE_SDF_3D_ARM");
  if (ndof < 1 || ndof > s->d || nspheres < s->d || !a || !alpha || !d || !theta_bias || !frames || !centers || !radii)
    return fail(ctx, GVI_ERR_ARG, "bad arm model (need 1 <= ndof <= factor dimension <= nspheres: n_balls = factor dimension)");
  for (int q = 0; q < nspheres; ++q)
    if (frames[q] < 0 || frames[q] >= ndof || (q && frames[q] < frames[q - 1]))
      return fail(ctx, GVI_ERR_ARG, "sphere frames must be non-decreasing and < ndof");
  std::vector<double> pk;
  s->arm_ndof = ndof;
  pk.push_back(ndof); pk.push_back(nspheres);
  pk.insert(pk.end(), a, a + ndof); pk.insert(pk.end(), alpha, alpha + ndof);
  pk.insert(pk.end(), d, d + ndof); pk.insert(pk.end(), theta_bias, theta_bias + ndof);
  for (int q = 0; q < nspheres; ++q) pk.push_back(frames[q]);
  pk.insert(pk.end(), centers, centers + 3 * (size_t)nspheres);
  pk.insert(pk.end(), radii, radii + nspheres);
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  HIPCK(ctx, s->arm.ensure(pk.size() * 8));
  HIPCK(ctx, hipMemcpy(s->arm.p, pk.data(), pk.size() * 8, hipMemcpyHostToDevice));
  ngd_invalidate(ctx);
  return GVI_OK;
}

gvi_status gvi_factors_set_closed_form(gvi_ctx* ctx, int set_id, int on) {
  FactorSet* s = get_set(ctx, set_id);
  if (!s) return fail(ctx, GVI_ERR_ARG, "bad set id");
  if (on && !psi_kind_is<PSI_CLOSED>(s->kind))
    return fail(ctx, GVI_ERR_ARG, "closed form exists for QUAD_PRIOR / FIXED_PRIOR / HINGE_BOX / HINGE_HALFSPACE sets only");
  GVICK(sync(ctx));
  s->closed_form = on != 0;
  ngd_invalidate(ctx);
  return GVI_OK;
}

gvi_status gvi_factors_set_temperature(gvi_ctx* ctx, int set_id, const double* temperature) {
  FactorSet* s = get_set(ctx, set_id);
  if (!s || !temperature) return fail(ctx, GVI_ERR_ARG, "bad set id / NULL temperature");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  HIPCK(ctx, hipMemcpy(s->temperature.p, temperature, (size_t)s->K * 8, hipMemcpyHostToDevice));
  ngd_invalidate(ctx);
  return GVI_OK;
}

// The PSI_RAW kinds keep their blocks as gvi_factors_add uploaded them and nothing derived from the VALUES is cached (seg_J and
// raw_stride are layout), so new blocks are one copy; the sum-of-squares kinds build (A, b, sgn) from theirs at gvi_factors_add.
gvi_status gvi_factors_set_params(gvi_ctx* ctx, int set_id, const double* psi_params, int64_t params_per_factor) {
  FactorSet* s = get_set(ctx, set_id);
  if (!s) return fail(ctx, GVI_ERR_ARG, "bad set id");
  if (!psi_kind_is<PSI_RAW>(s->kind)) return fail(ctx, GVI_ERR_ARG, "gvi_factors_set_params: only the kinds that keep their parameter block");
  int m = 0, J = 0;
  int64_t need = 0;
  const char* why = nullptr;
  // a block size the kind itself refuses is another layout too; the values' own refusals keep their texts below
  if (psi_kind_layout(s->kind, s->d, params_per_factor, &m, &J, &need, &why) != GVI_OK || J != s->seg_J || need != s->raw_stride)
    return fail(ctx, GVI_ERR_ARG, "gvi_factors_set_params: the layout of a set is fixed at gvi_factors_add");
  if (gvi_status rc = psi_kind_check_params(s->kind, s->d, J, params_per_factor, s->K, psi_params, &why)) return fail(ctx, rc, why);
  if (s->K == 0) return GVI_OK;
  const int np = s->raw_stride;
  std::vector<double> raw((size_t)s->K * np);
  for (int k = 0; k < s->K; ++k) memcpy(&raw[(size_t)k * np], psi_params + (size_t)k * params_per_factor, (size_t)np * 8);
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  HIPCK(ctx, hipMemcpy(s->raw.p, raw.data(), raw.size() * 8, hipMemcpyHostToDevice));
  ngd_invalidate(ctx);
  return GVI_OK;
}

// The rule is a property of the set beside its table: nothing derived from the blocks' VALUES is kept (the drop rule of a
// read-out is decided on the device per pass), so gvi_factors_set_params and gvi_set_variant leave it alone.
gvi_status gvi_factors_set_readout_rule(gvi_ctx* ctx, int set_id, int order) {
  FactorSet* s = get_set(ctx, set_id);
  if (!s) return fail(ctx, GVI_ERR_ARG, "bad set id");
  const int P = psi_kind_readout_P(s->kind);
  if (P == 0)
    return fail(ctx, GVI_ERR_ARG, "gvi_factors_set_readout_rule: only the kinds on linear read-outs (HINGE_SDF_2D / _3D, HINGE_SDF_*_SEG, HINGE_BALLS_*)");
  if (order != 0 && !readout_order_ok(order, P))
    return fail(ctx, GVI_ERR_ARG, "gvi_factors_set_readout_rule: order is 0 (off) or 2 <= order <= 16 with order^P <= 1024 (P = 3: order <= 10)");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  if (order > 0) {
    SparseGrid g;
    if (spgh_generate(1, order, g) || g.N != order) return fail(ctx, GVI_ERR_NOTABLE, "gvi_factors_set_readout_rule: no 1-D rule of this order");
    std::vector<double> rule(2 * (size_t)order);
    for (int a = 0; a < order; ++a) { rule[a] = g.Z[a]; rule[order + a] = g.w[a]; }
    HIPCK(ctx, s->readout_rule.ensure(2 * (size_t)READOUT_MAX_ORDER * 8));
    HIPCK(ctx, hipMemcpy(s->readout_rule.p, rule.data(), rule.size() * 8, hipMemcpyHostToDevice));
  }
  s->readout_order = order;
  ngd_invalidate(ctx);
  return GVI_OK;
}

gvi_status gvi_factors_readout_info(const gvi_ctx* ctx, int set_id, int* order, int* P, int* J, int64_t* points_per_check_point) {
  FactorSet* s = get_set(const_cast<gvi_ctx*>(ctx), set_id);
  if (!s) return GVI_ERR_ARG;
  const int rp = psi_kind_readout_P(s->kind);
  if (order) *order = s->readout_order;
  if (P) *P = rp;
  if (J) *J = rp == 0 ? 0 : (s->seg_J > 0 ? s->seg_J : 1);
  if (points_per_check_point) *points_per_check_point = s->readout_order > 0 ? readout_points(s->readout_order, rp) : 0;
  return GVI_OK;
}

gvi_status gvi_factors_info(const gvi_ctx* ctx, int set_id, int* K, int* d, int* p, int64_t* N) {
  FactorSet* s = get_set(const_cast<gvi_ctx*>(ctx), set_id);
  if (!s) return GVI_ERR_ARG;
  if (K) *K = s->K;
  if (d) *d = s->d;
  if (p) *p = s->p;
  if (N) *N = s->table->N;
  return GVI_OK;
}

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
  if (dmax > 32) return fail(ctx, GVI_ERR_UNSUPPORTED, "factor dimension > 32");
  if (ctx->opt.chol_rowb) {
    if (dmax <= 8) hipLaunchKernelGGL((prep_all_kernel<1, true>), grid, dim3(64), lds, ctx->stream, L);
    else if (dmax <= 16) hipLaunchKernelGGL((prep_all_kernel<4, true>), grid, dim3(64), lds, ctx->stream, L);
    else hipLaunchKernelGGL((prep_all_kernel<16, true>), grid, dim3(64), lds, ctx->stream, L);
  } else {
    if (dmax <= 8) hipLaunchKernelGGL((prep_all_kernel<1, false>), grid, dim3(64), lds, ctx->stream, L);
    else if (dmax <= 16) hipLaunchKernelGGL((prep_all_kernel<4, false>), grid, dim3(64), lds, ctx->stream, L);
    else hipLaunchKernelGGL((prep_all_kernel<16, false>), grid, dim3(64), lds, ctx->stream, L);
  }
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
  // window between two 8-byte loads
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

// ---- sharded factors: the two exchange steps (no-ops in a single process) ----
static bool dist_on(const gvi_ctx* ctx) { return ctx->dist.world > 1 || ctx->dist.fn || ctx->dist.comm; }

static gvi_status dist_allgather(gvi_ctx* ctx, const void* send, void* recv, int64_t count) {
  gvi_ctx::Dist& d = ctx->dist;
  if (d.fn) {
    if (d.fn(d.user, send, recv, count, (void*)ctx->stream) != 0) return fail(ctx, GVI_ERR_HIP, "all-gather callback failed");
    return GVI_OK;
  }
  if (!d.comm) return fail(ctx, GVI_ERR_STATE, "sharded context without a transport: call gvi_dist_init_rccl / _callback");
  const int rc = d.ncclAllGather(send, recv, (size_t)count, 8 /* ncclFloat64 */, d.comm, ctx->stream);
  if (rc != 0) return fail(ctx, GVI_ERR_HIP, "ncclAllGather failed with code " + std::to_string(rc));
  return GVI_OK;
}

// state range [lo, hi] this rank's factors touch; gathered once per problem definition over all ranks
static gvi_status dist_ranges(gvi_ctx* ctx) {
  gvi_ctx::Dist& d = ctx->dist;
  if (d.ranges_valid) return GVI_OK;
  int lo = ctx->T, hi = -1;
  for (auto& s : ctx->sets)
    for (int k = 0; k < s->K; ++k) {
      lo = std::min(lo, (int)s->start[k]);
      hi = std::max(hi, (int)s->start[k] + (s->d == 2 * ctx->n ? 1 : 0));
    }
  if (hi < lo) { lo = 0; hi = -1; }                         // a rank without factors sends nothing
  const int W = d.world;
  HIPCK(ctx, d.ranges.ensure((size_t)(3 * W + 4) * 8));     // [int range table | own range | cost parts]
  double mine[2] = {(double)lo, (double)hi};
  double* dsend = d.ranges.d() + 2 * W;
  HIPCK(ctx, hipMemcpyAsync(dsend, mine, 16, hipMemcpyHostToDevice, ctx->stream));
  HIPCK(ctx, hipStreamSynchronize(ctx->stream));            // `mine` is a stack buffer
  HIPCK(ctx, d.recv.ensure((size_t)2 * W * 8));
  GVICK(dist_allgather(ctx, dsend, d.recv.p, 2));
  std::vector<double> all(2 * W);
  HIPCK(ctx, hipMemcpyAsync(all.data(), d.recv.p, (size_t)2 * W * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCK(ctx, hipStreamSynchronize(ctx->stream));
  d.lo.resize(W); d.hi.resize(W);
  std::vector<int32_t> packed(2 * W);
  d.maxlen = 1;
  for (int r = 0; r < W; ++r) {
    d.lo[r] = (int32_t)all[2 * r]; d.hi[r] = (int32_t)all[2 * r + 1];
    packed[2 * r] = d.lo[r]; packed[2 * r + 1] = d.hi[r];
    d.maxlen = std::max(d.maxlen, d.hi[r] - d.lo[r] + 1);
  }
  HIPCK(ctx, hipMemcpyAsync(d.ranges.p, packed.data(), packed.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t per = (size_t)ctx->n + 2 * nn_(ctx);
  HIPCK(ctx, d.send.ensure((size_t)(d.maxlen + 1) * per * 8));                     // + the cost record of the fused trial
  HIPCK(ctx, d.recv.ensure(std::max<size_t>((size_t)W * (d.maxlen + 1) * per * 8, (size_t)2 * W * 8)));
  HIPCK(ctx, hipMemsetAsync(d.send.p, 0, (size_t)(d.maxlen + 1) * per * 8, ctx->stream));   // padding records stay zero
  d.rec_fresh = false;
  d.ranges_valid = true;
  return GVI_OK;
}

// exchange 0 on gradient buffer gb: pack own records -> all-gather -> fold in rank order back into exch0[gb]
static gvi_status dist_exchange0(gvi_ctx* ctx, int gb, bool with_cost = false, int publish_slot = -1) {
  if (!dist_on(ctx)) return GVI_OK;
  GVICK(dist_ranges(ctx));
  gvi_ctx::Dist& d = ctx->dist;
  const size_t T = ctx->T, n = ctx->n, nn = n * n, per = n + 2 * nn;
  double* eg = ctx->ngd.exch0[gb].d();
  double* eD = eg + T * n;
  double* eU = eD + T * nn;
  const int lo = d.lo[d.rank], len = d.hi[d.rank] - d.lo[d.rank] + 1;
  // with_cost: the rank's partial cost sum (exch1[0]) rides as one more record and comes back as the ordered total in
  // exch1[0] -- one all-gather for the fused trial instead of exchange 0 + exchange 1; publish_slot >= 0: the fold launch
  // also publishes {total + 1/2 log det of that NGD slot, sequence} to the host
  const int stride = d.maxlen + (with_cost ? 1 : 0);
  const int64_t np = (int64_t)stride * per;
  if (!d.rec_fresh) {                                        // else: written by the assemble (and cost_sum_all_kernel)
    hipLaunchKernelGGL(dist_pack_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, ctx->T, ctx->n, lo, len, d.maxlen,
                       eg, eD, eU, d.send.d(), with_cost ? (const double*)ctx->ngd.exch1.d() : (const double*)nullptr);
    HIPCK(ctx, hipGetLastError());
  }
  d.rec_fresh = false;
  GVICK(dist_allgather(ctx, d.send.p, d.recv.p, np));
  const bool pub = with_cost && publish_slot >= 0;
  if (pub) ctx->seq += 1.0;
  const int64_t nf = (int64_t)T * per + 1;
  hipLaunchKernelGGL(dist_fold_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, ctx->stream, ctx->T, ctx->n, d.world, d.maxlen, stride,
                     (const int32_t*)d.ranges.p, d.recv.d(), eg, eD, eU, with_cost ? ctx->ngd.exch1.d() : (double*)nullptr,
                     pub ? (const double*)ctx->ngd.hld[publish_slot].d() : (const double*)nullptr,
                     pub ? pub_slot(ctx) : (double*)nullptr, ctx->seq);
  HIPCK(ctx, hipGetLastError());
  return GVI_OK;
}

// exchange 1: the ranks' partial cost sums (exch1[0]) -> their ordered total (exch1[0]); recv is reused after exchange 0
static gvi_status dist_exchange1(gvi_ctx* ctx) {
  if (!dist_on(ctx)) return GVI_OK;
  GVICK(dist_ranges(ctx));
  gvi_ctx::Dist& d = ctx->dist;
  double* parts = d.ranges.d() + 2 * d.world + 2;           // [world] behind the range table
  GVICK(dist_allgather(ctx, ctx->ngd.exch1.p, parts, 1));
  hipLaunchKernelGGL(dist_cost_fold_kernel, dim3(1), dim3(64), 0, ctx->stream, d.world, parts, ctx->ngd.exch1.d());
  HIPCK(ctx, hipGetLastError());
  return GVI_OK;
}

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
  NgdState& g = ctx->ngd;
  const size_t T = ctx->T, n = ctx->n, nn = n * n;
  double* eg = g.exch0[gb].d();
  double* eD = eg + T * n;
  double* eU = eD + T * nn;
  const int64_t total = (int64_t)T * (n + 2 * nn);
  StageScope scope(ctx, STAGE_ASSEMBLE);
  double* rec = nullptr;                                     // sharded: the assemble writes this rank's exchange records too
  int rlo = 0, rlen = 0;
  if (dist_on(ctx)) {
    GVICK(dist_ranges(ctx));
    rec = ctx->dist.send.d(); rlo = ctx->dist.lo[ctx->dist.rank]; rlen = ctx->dist.hi[ctx->dist.rank] - rlo + 1;
  }
  hipLaunchKernelGGL(bt_scatter_all_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                     make_set_list(ctx, slot), ctx->T, ctx->n, eg, eD, eU, ctx->pipe.pred, ctx->pipe.pred_val, rec, rlo, rlen);
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
  const size_t T = ctx->T, n = ctx->n, nn = n * n;
  double* eg = g.exch0[gb].d();
  double* eD = eg + T * n;
  double* eU = eD + T * nn;
  if (dual_solve(ctx)) {
    g.solve_deferred[gb] = true;                        // goes out with the next trial factorisation (ngd_trial_state)
    return GVI_OK;
  }
  GVICK(ngd_flush_assemble(ctx, gb));
  return run_bt_solve(ctx, eD, eU, eg, -1.0, g.dmu2[gb].d());
}

// a reader of dmu / [g | V_D | V_U] of gradient buffer gb other than the next trial: a parked solve that nobody fused with a
// factorisation runs now, in stream order, on the second workspace; a pending assemble goes with it, or alone
static gvi_status ngd_join_solve(gvi_ctx* ctx, int gb) {
  NgdState& g = ctx->ngd;
  if (!g.solve_deferred[gb]) return ngd_flush_assemble(ctx, gb);
  g.solve_deferred[gb] = false;
  const size_t T = ctx->T, n = ctx->n, nn = n * n;
  double* eg = g.exch0[gb].d();
  if (!g.asm_pending[gb]) return run_bt_solve(ctx, eg + T * n, eg + T * n + T * nn, eg, -1.0, g.dmu2[gb].d(), 1);
  g.asm_pending[gb] = false;
  ChainWs w;
  GVICK(ensure_chain_ws(ctx, 1, w));
  ChainArgs a1 = make_chain_args(ctx, w, eg + T * n, eg + T * n + T * nn, eg, -1.0, false, nullptr, nullptr, g.dmu2[gb].d(), nullptr);
  a1.asm_on = 1; a1.asmG = eg; a1.asmD = eg + T * n; a1.asmU = eg + T * n + T * nn;
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
  g.cost_valid[t] = false;
  g.spec_ready = false;
  if (g.solve_deferred[g.gcur]) {
    // Lam_trial formed and factorised (log-det + marginals) and the parked gradient solve, side by side in three launches.
    // Lam_trial = Lam + step (V - Lam) is formed by the first pass of the factorisation while it loads the chain (and written
    // to Lam[t] there): "Lam[c] mixed with V" is factorised, no trial_kernel goes first.
    const size_t T = ctx->T, Tnn = T * nn_(ctx);
    double* eg = g.exch0[g.gcur].d();
    const double* V = eg + Tn;
    const TrialMix mix{V, g.Lam[t].d(), step};
    ChainWs w0, w1;
    GVICK(ensure_chain_ws(ctx, 0, w0));
    GVICK(ensure_chain_ws(ctx, 1, w1));
    double* sD = g.Sig[t].d();
    ChainArgs a0 = make_chain_args(ctx, w0, g.Lam[c].d(), g.Lam[c].d() + Tnn, nullptr, 1.0, true, sD, sD + Tnn, nullptr, g.hld[t].d(), &mix);
    ChainArgs a1 = make_chain_args(ctx, w1, V, V + Tnn, eg, -1.0, false, nullptr, nullptr, g.dmu2[g.gcur].d(), nullptr);
    if (g.asm_pending[g.gcur]) {
      // the assemble of this gradient buffer was left to these launches: both operations form V from the per-factor
      // results while they load, the solve leaves [g | V_D | V_U] in the buffer (later trials of this iteration read it)
      g.asm_pending[g.gcur] = false;
      a0.asm_on = a1.asm_on = 1;
      a1.asmG = eg; a1.asmD = eg + Tn; a1.asmU = eg + Tn + Tnn;
      const AsmList AL = make_asm_list(ctx);
      GVICK(run_chain(ctx, a0, a1, true, true, &AL));
    } else GVICK(run_chain(ctx, a0, a1, true, true));
    g.solve_deferred[g.gcur] = false;
    // mu_trial and the gather ride in the prep launch of the cost pass
    GVICK(ngd_gather_with_prep(ctx, t, g.mu[c].d(), g.dmu2[g.gcur].d(), step));
  } else {
    hipLaunchKernelGGL(trial_kernel, dim3((unsigned)((Tn + bt + 255) / 256)), dim3(256), 0, ctx->stream, (int64_t)Tn,
                       (int64_t)bt, step, g.mu[c].d(), g.dmu2[g.gcur].d(), g.Lam[c].d(), g.exch0[g.gcur].d() + Tn,
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
  const double* ex = g.exch0[g.gcur].d();
  hipLaunchKernelGGL(trial_kernel, dim3((unsigned)((Tn + bt + 255) / 256)), dim3(256), 0, ctx->stream, (int64_t)Tn, (int64_t)bt,
                     step, g.mu[c].d(), ex, g.Lam[c].d(), ex + Tn, g.mu[t].d(), g.Lam[t].d(), 1);
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

// ---- transports of the exchange ----
namespace {
struct RcclApi {
  struct Id128 { char b[128]; };       // ncclUniqueId: 128 opaque bytes, passed BY VALUE to ncclCommInitRank
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, Id128, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
};
bool load_rccl(RcclApi& r, std::string& err) {
  // GVI_RCCL_PATH, when set, names the ONLY candidate (an explicit choice is not second-guessed); else the usual names
  const char* forced = getenv("GVI_RCCL_PATH");
  const bool only = forced && *forced;
  const char* names[] = {forced, only ? nullptr : "librccl.so.1", only ? nullptr : "librccl.so", only ? nullptr : "/opt/rocm/lib/librccl.so.1"};
  std::string why;                                   // dlerror() clears the message it returns: read it ONCE per failed dlopen
  for (const char* nm : names) {
    if (!nm || !*nm) continue;
    r.lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    if (r.lib) break;
    const char* e = dlerror();
    why = e ? e : "?";
  }
  if (!r.lib) { err = "cannot load librccl: " + (why.empty() ? std::string("no candidate name") : why); return false; }
  r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.lib, "ncclGetUniqueId");
  r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.lib, "ncclCommInitRank");
  r.AllGather = (decltype(r.AllGather))dlsym(r.lib, "ncclAllGather");
  r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
  if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.CommDestroy) { err = "librccl lacks an expected symbol"; return false; }
  return true;
}
}  // namespace

gvi_status gvi_dist_unique_id(void* id128) {
  if (!id128) return fail(nullptr, GVI_ERR_ARG, "id128 is NULL");
  RcclApi r;
  std::string err;
  if (!load_rccl(r, err)) return fail(nullptr, GVI_ERR_HIP, err);
  const int rc = r.GetUniqueId(id128);
  return rc == 0 ? GVI_OK : fail(nullptr, GVI_ERR_HIP, "ncclGetUniqueId failed with code " + std::to_string(rc));
}

gvi_status gvi_dist_init_rccl(gvi_ctx* ctx, int rank, int world, const void* id128) {
  if (!ctx || !id128 || world < 1 || rank < 0 || rank >= world) return fail(ctx, GVI_ERR_ARG, "bad rank / world / id");
  HIPCK(ctx, hipSetDevice(ctx->device));
  GVICK(sync(ctx));
  RcclApi r;
  std::string err;
  if (!load_rccl(r, err)) return fail(ctx, GVI_ERR_HIP, err);
  RcclApi::Id128 id;
  memcpy(id.b, id128, 128);
  void* comm = nullptr;
  const int rc = r.CommInitRank(&comm, world, id, rank);
  if (rc != 0 || !comm) return fail(ctx, GVI_ERR_HIP, "ncclCommInitRank failed with code " + std::to_string(rc));
  gvi_ctx::Dist& d = ctx->dist;
  if (d.comm && d.ncclCommDestroy) d.ncclCommDestroy(d.comm);
  d.rank = rank; d.world = world; d.fn = nullptr; d.user = nullptr;
  d.rccl_lib = r.lib; d.comm = comm; d.ncclAllGather = r.AllGather; d.ncclCommDestroy = r.CommDestroy;
  d.ranges_valid = false;
  ngd_invalidate(ctx);
  return GVI_OK;
}

gvi_status gvi_dist_init_callback(gvi_ctx* ctx, int rank, int world, gvi_allgather_fn fn, void* user) {
  if (!ctx || !fn || world < 1 || rank < 0 || rank >= world) return fail(ctx, GVI_ERR_ARG, "bad rank / world / callback");
  GVICK(sync(ctx));
  gvi_ctx::Dist& d = ctx->dist;
  if (d.comm && d.ncclCommDestroy) { d.ncclCommDestroy(d.comm); d.comm = nullptr; }
  d.rank = rank; d.world = world; d.fn = fn; d.user = user;
  d.ranges_valid = false;
  ngd_invalidate(ctx);
  return GVI_OK;
}

gvi_status gvi_dist_info(const gvi_ctx* ctx, int* rank, int* world, int* records_per_rank) {
  if (!ctx) return GVI_ERR_ARG;
  if (rank) *rank = ctx->dist.rank;
  if (world) *world = ctx->dist.world;
  if (records_per_rank) *records_per_rank = ctx->dist.ranges_valid ? ctx->dist.maxlen : 0;
  return GVI_OK;
}

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
  if (which == 0) { *dev_ptr = ctx->ngd.exch0[ctx->ngd.gcur].p; *count = (int64_t)((size_t)ctx->T * ctx->n + bt_count(ctx)); }
  else if (which == 1) { *dev_ptr = ctx->ngd.exch1.p; *count = 1; }
  else if (which == 2) { *dev_ptr = ctx->ngd.exch0[1 - ctx->ngd.gcur].p; *count = (int64_t)((size_t)ctx->T * ctx->n + bt_count(ctx)); }
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
  if (gq) GVICK(d2h(ctx, gq, g.exch0[g.gcur].p, T * n * 8));
  std::vector<double> V, L;
  if (dD || dU || VD || VU) {
    V.resize(bt);
    GVICK(d2h(ctx, V.data(), g.exch0[g.gcur].d() + T * n, bt * 8));
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

}  // extern "C"

// posterior queries: samples and log-density, many right-hand sides, dense-time posterior, costs of sampled trajectories
// (textually part of this translation unit: the kernel headers define __global__ functions and cannot be included twice)
#include "posterior_host.inc"
