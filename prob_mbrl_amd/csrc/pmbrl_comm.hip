// Gradient all-reduce: RCCL through dlopen (no link-time dependency), the communicators, and the plan's transports.
// Host code only.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <string.h>

#include <string>

#include "pmbrl_host.h"

namespace {
struct RcclId { char internal[PMBRL_COMM_ID_BYTES]; };          // = ncclUniqueId (rccl.h:43)
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(RcclId*) = nullptr;
  int (*CommInitRank)(void**, int, RcclId, int) = nullptr;      // ncclCommInitRank(comm*, nranks, id BY VALUE, rank)
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;                       // ncclCommCount(comm, int* count)
  const char* (*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;
int rccl_load() {
  if (g_rccl.lib) return 0;
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);      // the copy torch.distributed already loaded
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
  if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) return fail(-4, std::string("librccl not found: ") + dlerror());
  RcclApi a;
  a.lib = h;
  a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
  a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
  a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(h, "ncclAllReduce"));
  a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
  a.CommCount = reinterpret_cast<decltype(a.CommCount)>(dlsym(h, "ncclCommCount"));
  a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
  if (!a.GetUniqueId || !a.CommInitRank || !a.AllReduce || !a.CommDestroy)
    return fail(-4, "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy");
  g_rccl = a;
  return 0;
}
int rccl_fail(const char* what, int rc) {
  return fail(-200 - rc, std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error"));
}
}  // namespace
struct pmbrl_comm {
  void* comm;
  int rank, nranks, device;
};
extern "C" int pmbrl_comm_unique_id(void* id_out) {
  if (!id_out) return fail(-1, "null argument");
  if (int rc = rccl_load()) return rc;
  RcclId id;
  if (int rc = g_rccl.GetUniqueId(&id)) return rccl_fail("ncclGetUniqueId", rc);
  memcpy(id_out, &id, sizeof(id));
  return 0;
}
extern "C" int pmbrl_comm_init(const void* id_in, int32_t rank, int32_t nranks, int32_t device, pmbrl_comm** out) {
  if (!id_in || !out || nranks < 1 || rank < 0 || rank >= nranks) return fail(-1, "bad argument");
  if (int rc = rccl_load()) return rc;
  HIPCHK(hipSetDevice(device));
  RcclId id;
  memcpy(&id, id_in, sizeof(id));
  void* c = nullptr;
  if (int rc = g_rccl.CommInitRank(&c, nranks, id, rank)) return rccl_fail("ncclCommInitRank", rc);
  *out = new pmbrl_comm{c, rank, nranks, device};
  return 0;
}
extern "C" int pmbrl_allreduce_sum(pmbrl_comm* comm, void* stream, float* buf_d, int64_t n) {
  if (!comm || !buf_d || n < 0) return fail(-1, "bad argument");
  // ncclFloat32 = 7, ncclSum = 0 (rccl.h: ncclDataType_t, ncclRedOp_t)
  if (int rc = g_rccl.AllReduce(buf_d, buf_d, (size_t)n, 7, 0, comm->comm, (hipStream_t)stream))
    return rccl_fail("ncclAllReduce", rc);
  return 0;
}
extern "C" int pmbrl_comm_count(pmbrl_comm* comm, int32_t* nranks_out) {
  if (!comm || !nranks_out) return fail(-1, "null argument");
  if (!g_rccl.CommCount) return fail(-4, "librccl lacks ncclCommCount");
  int n = 0;
  if (int rc = g_rccl.CommCount(comm->comm, &n)) return rccl_fail("ncclCommCount", rc);
  *nranks_out = n;
  return 0;
}
extern "C" void pmbrl_comm_destroy(pmbrl_comm* comm) {
  if (!comm) return;
  if (g_rccl.CommDestroy) (void)g_rccl.CommDestroy(comm->comm);
  delete comm;
}

static int pm_coll_rccl(void* ctx, void* stream, double* buf_d, int64_t n) {
  pmbrl_comm* comm = static_cast<pmbrl_comm*>(ctx);
  return g_rccl.AllReduce(buf_d, buf_d, (size_t)n, 8 /* ncclDouble */, 0 /* ncclSum */, comm->comm, (hipStream_t)stream);
}
extern "C" int pmbrl_plan_set_comm(pmbrl_plan* plan, pmbrl_comm* comm) {
  if (!plan || !comm) return fail(-1, "null argument");
  plan->coll = pm_coll_rccl;
  plan->coll_ctx = comm;
  return 0;
}
extern "C" int pmbrl_plan_set_collective(pmbrl_plan* plan, pmbrl_collective_fn fn, void* ctx) {
  if (!plan) return fail(-1, "null argument");
  plan->coll = fn;
  plan->coll_ctx = ctx;
  return 0;
}

extern "C" int pmbrl_plan_set_grad_comm(pmbrl_plan* plan, pmbrl_comm* comm, pmbrl_p2p* p2p) {
  if (!plan) return fail(-1, "null argument");
  if (comm && p2p) return fail(-1, "pmbrl_plan_set_grad_comm: at most one of the two transports");
  HIPCHK(hipSetDevice(plan->device));
  // whatever follows, the plan first lets go of the transport it had (a refusal leaves it without one)
  for (int k = 0; k < 2; ++k) replay_drop(plan, k);     // (a recording holds the transport it was made with)
  if (plan->tail_buf_d) {
    HIPCHK(hipDeviceSynchronize());                       // (calls still queued may read it)
    HIPCHK(hipFree(plan->tail_buf_d));
    plan->tail_buf_d = nullptr;
  }
  plan->grad_comm = nullptr;
  plan->grad_p2p = nullptr;
  plan->tail_err_d = nullptr;
  // (a plan of LOCAL groups that runs the span form with one rank -- plan_layout: groups beyond the CU count -- is fine)
  if ((comm || p2p) && plan->span && plan->cfg.mm_span_ranks > 1)
    return fail(-3, "pmbrl_plan_set_grad_comm: not offered with moment-matching groups spread over ranks (mm_span_rows)");
  int rank = 0, world = 1;
  int* err_d = nullptr;
  const size_t n = plan->pol.n_params;
  if (comm) { rank = comm->rank; world = comm->nranks; }
  if (p2p) {
    size_t cap = 0;
    pm_p2p_describe(p2p, &rank, &world, &cap, &err_d);
    if ((n + 2) * sizeof(float) > cap)
      return fail(-2, "pmbrl_plan_set_grad_comm: the flat gradient is larger than the peer-to-peer slots (max_bytes of pmbrl_p2p_create)");
  }
  if (!comm && !p2p) return 0;
  const size_t nx = (n + 2 + 3) / 4 * 4 + (size_t)world;
  HIPCHK(hipMalloc(&plan->tail_buf_d, nx * sizeof(float)));
  HIPCHK(hipMemset(plan->tail_buf_d, 0, nx * sizeof(float)));
  plan->grad_comm = comm;
  plan->grad_p2p = p2p;
  plan->tail_rank = rank;
  plan->tail_world = world;
  plan->tail_err_d = err_d;
  return 0;
}
