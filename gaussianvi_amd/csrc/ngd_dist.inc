// Sharded factors (one process per GPU): the two exchange steps of the resident iteration, no-ops in a single process.  A
// fragment of the library's one translation unit, included by gvi_hip.hip inside its extern "C" bracket; not a stand-alone
// header.  The transports themselves are set up in dist_transport.inc.
//
//   holds      dist_on; dist_allgather; dist_ranges; dist_exchange0 (gradient records, optionally with the cost), dist_exchange1
//              (cost sums)
//   relies on  host_ctx.inc (gvi_ctx and gvi_ctx::Dist, grad_buf, pub_slot, nn_)
//   defines    no entry point

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
  const GradBuf e = grad_buf(ctx, gb);
  const int lo = d.lo[d.rank], len = d.hi[d.rank] - d.lo[d.rank] + 1;
  // with_cost: the rank's partial cost sum (exch1[0]) rides as one more record and comes back as the ordered total in
  // exch1[0] -- one all-gather for the fused trial instead of exchange 0 + exchange 1; publish_slot >= 0: the fold launch
  // also publishes {total + 1/2 log det of that NGD slot, sequence} to the host
  const int stride = d.maxlen + (with_cost ? 1 : 0);
  const int64_t np = (int64_t)stride * per;
  if (!d.rec_fresh) {                                        // else: written by the assemble (and cost_sum_all_kernel)
    hipLaunchKernelGGL(dist_pack_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, ctx->T, ctx->n, lo, len, d.maxlen,
                       e.g, e.D, e.U, d.send.d(), with_cost ? (const double*)ctx->ngd.exch1.d() : (const double*)nullptr);
    HIPCK(ctx, hipGetLastError());
  }
  d.rec_fresh = false;
  GVICK(dist_allgather(ctx, d.send.p, d.recv.p, np));
  const bool pub = with_cost && publish_slot >= 0;
  if (pub) ctx->seq += 1.0;
  const int64_t nf = (int64_t)T * per + 1;
  hipLaunchKernelGGL(dist_fold_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, ctx->stream, ctx->T, ctx->n, d.world, d.maxlen, stride,
                     (const int32_t*)d.ranges.p, d.recv.d(), e.g, e.D, e.U, with_cost ? ctx->ngd.exch1.d() : (double*)nullptr,
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
