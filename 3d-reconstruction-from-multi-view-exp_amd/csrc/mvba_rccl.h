// The RCCL binding of libmvba.so: the table of entry points (g_rccl) and rccl_load(), which fills it once per process.
//
// Included by mvba.hip before anything that talks to a communicator (mvba_engine.h's global_cost, mvba_step.h's allreduce_Ab, the
// comm entry points): uses <dlfcn.h>, <rccl/rccl.h> and fail() of mvba_common.h.
//
// libmvba.so is NOT linked against librccl: a process may already hold one (PyTorch maps its own
// bundled librccl.so the moment torch.distributed creates a group), and two copies -- or headers of
// one release bound to the code of another by accident of load order -- is the version skew a
// collective library does not forgive.  The policy is explicit instead: use the librccl the
// process has ALREADY loaded if there is one (RTLD_NOLOAD), else load ROCm's; bind the seven entry
// points by name (all part of the NCCL 2.x C API: plain pointers, enums whose values have not
// changed since 2.0, the 128-byte id), and refuse a library whose major version differs from the
// headers this file was compiled against.  mvba_get_info reports both versions.
namespace {
struct Rccl {
  void *lib = nullptr;
  int version = 0;
  std::string origin;
  ncclResult_t (*GetVersion)(int *) = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;

int rccl_load() {
  if (g_rccl.lib) return MVBA_OK;
  const char *names[] = {"librccl.so.1", "librccl.so"};
  void *lib = nullptr;
  std::string origin;
  for (const char *n : names)
    if (!lib && (lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) origin = std::string(n) + " (already mapped by the process)";
  if (const char *ev = getenv("MVBA_RCCL_LIBRARY"))
    if (!lib && (lib = dlopen(ev, RTLD_NOW | RTLD_GLOBAL))) origin = ev;
  for (const char *n : {"/opt/rocm/lib/librccl.so.1", "librccl.so.1"})
    if (!lib && (lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) origin = n;
  if (!lib) return fail(MVBA_ERR_RCCL, std::string("librccl not found: ") + dlerror());
  Rccl r;
  r.lib = lib;
  r.origin = origin;
#define BIND(field, sym)                                                                       \
  if (!(r.field = reinterpret_cast<decltype(r.field)>(dlsym(lib, sym))))                       \
    return fail(MVBA_ERR_RCCL, std::string("librccl (") + origin + ") lacks " + sym)
  BIND(GetVersion, "ncclGetVersion");
  BIND(GetUniqueId, "ncclGetUniqueId");
  BIND(CommInitRank, "ncclCommInitRank");
  BIND(CommDestroy, "ncclCommDestroy");
  BIND(AllReduce, "ncclAllReduce");
  BIND(AllGather, "ncclAllGather");
  BIND(GetErrorString, "ncclGetErrorString");
#undef BIND
  if (r.GetVersion(&r.version) != ncclSuccess) return fail(MVBA_ERR_RCCL, "ncclGetVersion failed");
  // version code: major * 10000 + minor * 100 + patch since 2.9 (major * 1000 + ... before)
  const int major = r.version >= 10000 ? r.version / 10000 : r.version / 1000;
  if (major != NCCL_MAJOR)
    return fail(MVBA_ERR_RCCL, "librccl (" + origin + ") is NCCL " + std::to_string(r.version) + ", this library was built against " +
                                   std::to_string(NCCL_VERSION_CODE));
  g_rccl = r;
  return MVBA_OK;
}
}  // namespace
