// Binding and launching of the factor stage: a decision of routes.hpp becomes buffers, kernel arguments and a launch.  A
// fragment of the library's one translation unit (gvi_hip.hip); not a stand-alone header.
//
//   holds      the kernel-instance launchers (launch_split / _reg / _sreg / _orbit_t / _orbit_pair / _orbit_psi_t / _closed /
//              _readout); route_facts and rules_of; the orbit arguments (orbit_dev, orbit_args); the launch counters; the fused
//              launch (fused_round_blocks, launch_fused_t); prep (launch_prep, run_prep); MomPlan / PassPlan; plan_closed /
//              plan_readout, bind_plan, plan_moments, launch_plan; warm_start_of, take_gather, fill_epi_tail; ProfBracket with
//              prof_open / prof_close; record_plan, launch_single; run_moments, run_epilogue, ensure_set_buffers
//   relies on  host_ctx.inc (gvi_ctx, FactorSet, Table, DevMem, fail / HIPCK / GVICK, allow_lds, pub_slot, nn_)
//   defines    no entry point

namespace {

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

#ifdef GVI_FUSED_TIMING
#include "fused_timing.inc"
#endif

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
  if ((dbg & 8) && stamps && ++nprint > 200 && nprint <= 202) fused_timing_dump(c, A, stamps);   // a few warm launches (fused_timing.inc)
#endif
  return GVI_OK;
}

// prep_kernel for the f.K factors of f at (mu, Sigma) device pointers: the instance of the dimension and its LDS
gvi_status launch_prep(gvi_ctx* c, const FactorDev& f, const double* mu, const double* Sigma, hipStream_t st) {
  const size_t lds = prep_lds_bytes(f.d);
  if (!with_prep_instance(f.d, [&]<int EPLP>(PrepInst<EPLP>) { hipLaunchKernelGGL(prep_kernel<EPLP>, dim3(f.K), dim3(64), lds, st, f, mu, Sigma); }))
    return fail(c, GVI_ERR_UNSUPPORTED, "factor dimension > 32");
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

}  // namespace
