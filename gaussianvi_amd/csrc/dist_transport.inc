// Transports of the sharded exchange: the RCCL loader and the entry points that give a context its rank, world and
// all-gather.  A fragment of the library's one translation unit, included by gvi_hip.hip inside its extern "C" bracket; not a
// stand-alone header.  The exchange steps that use the transport are in ngd_dist.inc.
//
//   holds      RcclApi, load_rccl
//   relies on  host_ctx.inc (gvi_ctx::Dist, sync, ngd_invalidate)
//   defines    gvi_dist_unique_id, gvi_dist_init_rccl, gvi_dist_init_callback, gvi_dist_info

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
