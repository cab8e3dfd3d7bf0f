// rsf_comm.hip — the posterior-pool communicator: RCCL bound at run time, rsf_comm_*, rsf_pool_allgather[_all] and
// rsf_pool_allreduce_sum[_all].  It needs the HIP runtime API and the ctx but no kernel: it is compiled for the host alone.
#include <rccl/rccl.h>  // types and prototypes only: the library is bound with dlopen (see struct Rccl)
#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <vector>

#include "rsf_host.h"

using namespace rsfh;

namespace {

// RCCL, bound at run time: a process that already holds a copy (PyTorch links its own) must not get a second one,
// and a caller that never pools across GPUs needs none at all.
struct Rccl {
  void *h = nullptr;
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclCommInitAll) comm_init_all = nullptr;
  decltype(&ncclGroupStart) group_start = nullptr;
  decltype(&ncclGroupEnd) group_end = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclAllReduce) all_reduce = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
};

void bind_rccl(Rccl &r) {
  const char *env = std::getenv("RSF_RCCL_LIB");
  const char *names[] = {"librccl.so", "librccl.so.1"};
  if (env && *env) r.h = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
  for (const char *n : names) if (!r.h) r.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);  // the copy already in the process
  if (!r.h) {  // a copy PyTorch loaded by path is found through one of its symbols
    Dl_info info;
    void *sym = dlsym(RTLD_DEFAULT, "ncclGetUniqueId");
    if (sym && dladdr(sym, &info) && info.dli_fname) r.h = dlopen(info.dli_fname, RTLD_NOW | RTLD_NOLOAD);
  }
  for (const char *n : names) if (!r.h) r.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
  if (!r.h) r.h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!r.h) return;
  r.get_unique_id = (decltype(r.get_unique_id))dlsym(r.h, "ncclGetUniqueId");
  r.comm_init_rank = (decltype(r.comm_init_rank))dlsym(r.h, "ncclCommInitRank");
  r.comm_init_all = (decltype(r.comm_init_all))dlsym(r.h, "ncclCommInitAll");
  r.group_start = (decltype(r.group_start))dlsym(r.h, "ncclGroupStart");
  r.group_end = (decltype(r.group_end))dlsym(r.h, "ncclGroupEnd");
  r.comm_destroy = (decltype(r.comm_destroy))dlsym(r.h, "ncclCommDestroy");
  r.all_gather = (decltype(r.all_gather))dlsym(r.h, "ncclAllGather");
  r.all_reduce = (decltype(r.all_reduce))dlsym(r.h, "ncclAllReduce");
  r.error_string = (decltype(r.error_string))dlsym(r.h, "ncclGetErrorString");
  if (!r.get_unique_id || !r.comm_init_rank || !r.comm_init_all || !r.group_start || !r.group_end || !r.comm_destroy || !r.all_gather ||
      !r.all_reduce || !r.error_string)
    r.h = nullptr;
}

const Rccl *rccl() {  // bound once, whichever thread asks first
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, bind_rccl, std::ref(r));
  return r.h ? &r : nullptr;
}

#define RCCL_TRY(R, expr)                                                                          \
  do {                                                                                             \
    ncclResult_t e_ = (expr);                                                                      \
    if (e_ != ncclSuccess) return fail(RSF_ERR_DEVICE, "%s -> %s", #expr, (R)->error_string(e_));  \
  } while (0)

}  // namespace

void rsfh::release_comm(rsf_ctx *c) {
  if (c->comm) { const Rccl *R = rccl(); if (R) (void)R->comm_destroy(c->comm); }
}

extern "C" {

int rsf_comm_unique_id(uint8_t id[RSF_COMM_ID_BYTES]) {
  if (!id) return fail(RSF_ERR_INVALID, "rsf_comm_unique_id: NULL argument");
  static_assert(sizeof(ncclUniqueId) == RSF_COMM_ID_BYTES, "RCCL unique id size");
  const Rccl *R = rccl();
  if (!R) return fail(RSF_ERR_UNSUPPORTED, "rsf_comm_unique_id: RCCL (librccl.so) could not be loaded: %s", dlerror());
  ncclUniqueId u;
  RCCL_TRY(R, R->get_unique_id(&u));
  std::memcpy(id, u.internal, RSF_COMM_ID_BYTES);
  return RSF_OK;
}

int rsf_comm_init(rsf_ctx *c, int32_t world, int32_t rank, const uint8_t id[RSF_COMM_ID_BYTES]) {
  if (!c || world < 1 || rank < 0 || rank >= world) return fail(RSF_ERR_INVALID, "rsf_comm_init: bad argument");
  if (c->world) return fail(RSF_ERR_STATE, "rsf_comm_init: this ctx already has a communicator (rsf_comm_destroy first)");
  if (world > 1 && !id) return fail(RSF_ERR_INVALID, "rsf_comm_init: world > 1 needs the id from rsf_comm_unique_id on rank 0");
  if (id) {  // (world = 1 with an id makes a real one-rank communicator: the single-GPU test of the RCCL binding)
    const Rccl *R = rccl();
    if (!R) return fail(RSF_ERR_UNSUPPORTED, "rsf_comm_init: RCCL (librccl.so) could not be loaded");
    RSF_ENTER(c, NEED_NOTHING);
    ncclUniqueId u;
    std::memcpy(u.internal, id, RSF_COMM_ID_BYTES);
    RCCL_TRY(R, R->comm_init_rank(&c->comm, world, u, rank));
  }
  c->world = world;
  c->rank = rank;
  return RSF_OK;
}

int rsf_comm_destroy(rsf_ctx *c) {
  if (!c) return fail(RSF_ERR_INVALID, "rsf_comm_destroy: NULL ctx");
  ncclComm_t comm = c->comm;
  c->comm = nullptr;  // the ctx is out of its group whatever RCCL says about the teardown
  c->world = 0;
  c->rank = 0;
  if (comm) {
    DeviceGuard guard(c->device);
    (void)hipStreamSynchronize(c->stream);
    const Rccl *R = rccl();
    if (R) RCCL_TRY(R, R->comm_destroy(comm));
  }
  return RSF_OK;
}

int rsf_pool_allgather(rsf_ctx *c, const double *send, int64_t count, double *recv) {
  RSF_ENTER(c, NEED_COMM, send && recv && count >= 1, "bad argument");
  int rc;
  const size_t bytes = (size_t)count * sizeof(double);
  const double *ds;
  double *dr;
  if ((rc = stage_in(c, SLOT_SEND, send, bytes, &ds))) return rc;
  if ((rc = stage_out(c, SLOT_RECV, recv, bytes * (size_t)c->world, &dr))) return rc;
  if (!c->comm) {
    if (dr != ds) HIP_TRY(hipMemcpyAsync(dr, ds, bytes, hipMemcpyDeviceToDevice, c->stream));
  } else {
    const Rccl *R = rccl();
    RCCL_TRY(R, R->all_gather(ds, dr, (size_t)count, ncclFloat64, c->comm, c->stream));
  }
  if ((rc = copy_back(c, SLOT_RECV, recv, bytes * (size_t)c->world))) return rc;
  return finish(c);
}

int rsf_pool_allreduce_sum(rsf_ctx *c, double *buf, int64_t count) {
  RSF_ENTER(c, NEED_COMM, buf && count >= 1, "bad argument");
  if (!c->comm) return RSF_OK;
  int rc;
  const size_t bytes = (size_t)count * sizeof(double);
  const double *ds;
  if ((rc = stage_in(c, SLOT_SEND, buf, bytes, &ds))) return rc;
  const Rccl *R = rccl();
  RCCL_TRY(R, R->all_reduce(ds, (void *)ds, (size_t)count, ncclFloat64, ncclSum, c->comm, c->stream));
  if (host_mem(c)) HIP_TRY(hipMemcpyAsync(buf, ds, bytes, hipMemcpyDeviceToHost, c->stream));
  return finish(c);
}

// ---- single-process form: one ctx per device, one host thread drives them all (ncclCommInitAll + grouped calls) ----
namespace {

int check_group(rsf_ctx *const *ctxs, int32_t n, const char *who, bool need_comm) {
  if (!ctxs || n < 1) return fail(RSF_ERR_INVALID, "%s: bad argument", who);
  for (int32_t i = 0; i < n; ++i) {
    if (!ctxs[i]) return fail(RSF_ERR_INVALID, "%s: ctxs[%d] is NULL", who, i);
    for (int32_t j = 0; j < i; ++j)
      if (ctxs[j] == ctxs[i]) return fail(RSF_ERR_INVALID, "%s: ctxs[%d] and ctxs[%d] are the same ctx", who, j, i);
    if (need_comm && (ctxs[i]->world != n || ctxs[i]->rank != i || !ctxs[i]->comm))
      return fail(RSF_ERR_STATE, "%s: ctxs[%d] is not rank %d of a %d-rank group made by rsf_comm_init_all", who, i, i, n);
  }
  return RSF_OK;
}

}  // namespace

int rsf_comm_init_all(rsf_ctx *const *ctxs, int32_t n) {
  int rc = check_group(ctxs, n, "rsf_comm_init_all", false);
  if (rc) return rc;
  for (int32_t i = 0; i < n; ++i)
    if (ctxs[i]->world) return fail(RSF_ERR_STATE, "rsf_comm_init_all: ctxs[%d] already has a communicator (rsf_comm_destroy first)", i);
  const Rccl *R = rccl();
  if (!R) return fail(RSF_ERR_UNSUPPORTED, "rsf_comm_init_all: RCCL (librccl.so) could not be loaded");
  std::vector<int> devs(n);
  std::vector<ncclComm_t> comms(n, nullptr);
  for (int32_t i = 0; i < n; ++i) devs[i] = ctxs[i]->device;
  RCCL_TRY(R, R->comm_init_all(comms.data(), n, devs.data()));
  for (int32_t i = 0; i < n; ++i) { ctxs[i]->comm = comms[i]; ctxs[i]->world = n; ctxs[i]->rank = i; }
  return RSF_OK;
}

int rsf_pool_allgather_all(rsf_ctx *const *ctxs, int32_t n, const double *const *send, int64_t count, double *const *recv) {
  int rc = check_group(ctxs, n, "rsf_pool_allgather_all", true);
  if (rc) return rc;
  if (!send || !recv || count < 1) return fail(RSF_ERR_INVALID, "rsf_pool_allgather_all: bad argument");
  for (int32_t i = 0; i < n; ++i)
    if (!send[i] || !recv[i]) return fail(RSF_ERR_INVALID, "rsf_pool_allgather_all: send[%d] / recv[%d] is NULL", i, i);
  const Rccl *R = rccl();
  const size_t bytes = (size_t)count * sizeof(double);
  std::vector<const double *> ds(n);
  std::vector<double *> dr(n);
  for (int32_t i = 0; i < n; ++i) {
    RSF_ENTER(ctxs[i], NEED_NOTHING);
    if ((rc = stage_in(ctxs[i], SLOT_SEND, send[i], bytes, &ds[i]))) return rc;
    if ((rc = stage_out(ctxs[i], SLOT_RECV, recv[i], bytes * (size_t)n, &dr[i]))) return rc;
  }
  RCCL_TRY(R, R->group_start());
  for (int32_t i = 0; i < n; ++i) {
    DeviceGuard guard(ctxs[i]->device);
    const ncclResult_t e = R->all_gather(ds[i], dr[i], (size_t)count, ncclFloat64, ctxs[i]->comm, ctxs[i]->stream);
    if (e != ncclSuccess) { (void)R->group_end(); return fail(RSF_ERR_DEVICE, "ncclAllGather (rank %d) -> %s", i, R->error_string(e)); }
  }
  RCCL_TRY(R, R->group_end());
  for (int32_t i = 0; i < n; ++i) {
    DeviceGuard guard(ctxs[i]->device);
    if ((rc = copy_back(ctxs[i], SLOT_RECV, recv[i], bytes * (size_t)n))) return rc;
    if ((rc = finish(ctxs[i]))) return rc;
  }
  return RSF_OK;
}

int rsf_pool_allreduce_sum_all(rsf_ctx *const *ctxs, int32_t n, double *const *bufs, int64_t count) {
  int rc = check_group(ctxs, n, "rsf_pool_allreduce_sum_all", true);
  if (rc) return rc;
  if (!bufs || count < 1) return fail(RSF_ERR_INVALID, "rsf_pool_allreduce_sum_all: bad argument");
  for (int32_t i = 0; i < n; ++i)
    if (!bufs[i]) return fail(RSF_ERR_INVALID, "rsf_pool_allreduce_sum_all: bufs[%d] is NULL", i);
  const Rccl *R = rccl();
  const size_t bytes = (size_t)count * sizeof(double);
  std::vector<const double *> ds(n);
  for (int32_t i = 0; i < n; ++i) {
    RSF_ENTER(ctxs[i], NEED_NOTHING);
    if ((rc = stage_in(ctxs[i], SLOT_SEND, bufs[i], bytes, &ds[i]))) return rc;
  }
  RCCL_TRY(R, R->group_start());
  for (int32_t i = 0; i < n; ++i) {
    DeviceGuard guard(ctxs[i]->device);
    const ncclResult_t e = R->all_reduce(ds[i], (void *)ds[i], (size_t)count, ncclFloat64, ncclSum, ctxs[i]->comm, ctxs[i]->stream);
    if (e != ncclSuccess) { (void)R->group_end(); return fail(RSF_ERR_DEVICE, "ncclAllReduce (rank %d) -> %s", i, R->error_string(e)); }
  }
  RCCL_TRY(R, R->group_end());
  for (int32_t i = 0; i < n; ++i) {
    DeviceGuard guard(ctxs[i]->device);
    if (host_mem(ctxs[i])) HIP_TRY(hipMemcpyAsync(bufs[i], ds[i], bytes, hipMemcpyDeviceToHost, ctxs[i]->stream));
    if ((rc = finish(ctxs[i]))) return rc;
  }
  return RSF_OK;
}

}  // extern "C"
