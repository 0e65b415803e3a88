// Entry points that set a problem up: the context, the quadrature tables, the chain shape and the factor sets.  A fragment of
// the library's one translation unit, included by gvi_hip.hip inside its extern "C" bracket; not a stand-alone header.
//
//   holds      factors_add_impl beside the entry points
//   relies on  host_ctx.inc (gvi_ctx, FactorSet, Table, upload_table, sync, get_set, ngd_invalidate, fail / HIPCK / GVICK);
//              launch_factor.inc (ensure_set_buffers); spgh.hpp, host_linalg.hpp, psi_kinds.hpp
//   defines    gvi_version, gvi_last_error; gvi_ctx_create / _destroy / _set_stream / _sync; gvi_spgh_count / _nodes;
//              gvi_table_file_list / _read / _write; gvi_chain_set; gvi_factors_add / _add_table; gvi_factors_set_table /
//              _set_sdf2d / _set_sdf3d / _set_arm / _set_closed_form / _set_temperature / _set_params / _set_readout_rule;
//              gvi_factors_readout_info, gvi_factors_info

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
