// rsf_hip.hip — gfx950 (MI355X / CDNA4) implementation of include/rsf_abi.h: the host side of the C ABI.
// The kernels are in rsf_kernels.h (device building blocks: rsf_device*.h, rsf_math.h).
//
// There is no host fallback in this file: every entry point either runs on the GPU or fails.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only: the library is bound with dlopen (see struct Rccl)
#include <dlfcn.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <functional>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/rsf_abi.h"
#include "../../include/rsf_diag.h"
#include "../../include/rsf_predict.h"
#include "rsf_kernels.h"
#include "rsf_diag.h"
#include "rsf_diag_rank.h"
#include "rsf_predict.h"
#include "rsf_psis.h"

using rsf::Consts;
using namespace rsfk;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(RSF_ERR_DEVICE, "%s -> %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
};

struct DeviceGuard {  // run on the ctx device, restore the caller's current device afterwards
  int prev = -1;
  DeviceGuard() = default;
  explicit DeviceGuard(int dev) { (void)select(dev); }  // unchecked: rsf_destroy, rsf_comm_destroy (free what can be freed), later loops of *_all
  bool select(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) return false;
    return prev == dev || hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Staging slots of RSF_MEM_HOST callers (rsf_ctx::stage), named by what each holds in the call that uses it.  The rule that
// makes sharing them safe: within one ABI call every array the call stages has a slot of its own (the names of one line
// below are distinct slots); a slot is reused only ACROSS calls, and every RSF_MEM_HOST call ends in finish()'s synchronise,
// so no copy of an earlier call is in flight when the next one writes the slot.
enum Slot : int {
  // rsf_mcmc_run / _replay / _replay_ssq: supplied variates and sums of squares in, trace rows out
  SLOT_Z, SLOT_U, SLOT_G, SLOT_TQ, SLOT_TS, SLOT_TA, SLOT_SSQ_NEW, SLOT_COUNT,
  // the drained run's second trace set lies in the replay inputs' slots: a drained run stages none (run_mcmc_drained checks it)
  SLOT_TQ_B = SLOT_Z, SLOT_TS_B = SLOT_U, SLOT_TA_B = SLOT_G,
  // rsf_mcmc_propose: z in SLOT_Z
  SLOT_Q_NEW = SLOT_TQ, SLOT_IN_BOUNDS = SLOT_TA,
  // rsf_forward_batch
  SLOT_DC = SLOT_Z, SLOT_A = SLOT_U, SLOT_B = SLOT_G, SLOT_DATA = SLOT_TQ, SLOT_SSQ_OUT = SLOT_TS, SLOT_ACC_OUT = SLOT_TA,
  // rsf_mcmc_init (q0 in SLOT_Q), rsf_mcmc_get_state / _set_state / _init_state
  SLOT_Q = SLOT_Z, SLOT_V = SLOT_U,
  // rsf_pool_summary / _kde / _histogram, rsf_diag_partials, rsf_diag_rank_prepare: the samples or the trace in SLOT_X
  SLOT_X = SLOT_Z, SLOT_GRID = SLOT_U, SLOT_POOL_OUT = SLOT_G,
  // rsf_predict_partials (std2 in SLOT_U), rsf_predict_quantiles (the series in SLOT_X)
  // rsf_predict_psis_loo: the series in SLOT_SERIES, std2 in SLOT_STD2, the observation in SLOT_OBS
  SLOT_STD2 = SLOT_U, SLOT_OBS = SLOT_G, SLOT_SERIES = SLOT_TQ,
  // rsf_pool_allgather[_all] / _allreduce_sum[_all] (the reduction is in place in SLOT_SEND)
  SLOT_SEND = SLOT_Z, SLOT_RECV = SLOT_U,
};

}  // namespace

struct rsf_ctx {
  rsf_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  int block = kMaxBlock;
  // model
  bool have_model = false;
  rsf_model m{};
  int32_t nout = 0;
  double delta_t = 0, h = 0;
  int32_t kc = 0, nchunks = 0;
  int32_t kc32 = 0, nchunks32 = 0;  // the float32 SAMPLER's own chunking: its tables are floats, twice as many fit the budget
  size_t lds_bytes = 0;
  DevBuf vl;
  // chains
  bool have_chains = false;
  bool external_chains = false;  // made by rsf_mcmc_init_state: no observation, advanced by rsf_mcmc_replay_ssq only
  rsf_mcmc_config mc{};
  DevBuf data, q, ssq, std2, V, wref, wsum, wsq, wn, wbuf, stats;
  int64_t group_chains = 0;  // chains per observation group (0: one series)
  int64_t iters_done = 0;
  // staging for RSF_MEM_HOST callers
  DevBuf stage[SLOT_COUNT];
  // drain pipeline of rsf_mcmc_run for RSF_MEM_HOST callers: the trace of launch k is copied out on its own stream
  // while launch k+1 computes
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_done[2] = {nullptr, nullptr};
  // one-proposal replay as a captured graph (the drop-in single-chain MCMC.sample() is launch-bound)
  struct ReplayGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipGraphNode_t kernel = nullptr;
    void *host = nullptr;   // pinned: [z C*d][u C][g C] | [tq C*d][ts C][ta C bytes]
    void *dev = nullptr;
    int64_t C = 0;
    int d = 0;
    const void *fn = nullptr;
    size_t lds = 0;
    int block = 0;
  } rg;
  // posterior-pool communicator (one process per GPU)
  int32_t world = 0, rank = 0;  // world 0: rsf_comm_init not called
  ncclComm_t comm = nullptr;
  DevBuf pool;    // workspace of the posterior post-processing kernels: the moments' partials
  DevBuf poolws;  // ... and the KDE's per-workgroup densities or the histogram's integer counts
  DevBuf diag;  // workspace of the convergence diagnostics (rsf_diag_partials)
  DevBuf rankws;  // rank workspace (rsf_diag_rank_prepare): the four derived series, then the sort buffers
  int64_t rank_n = 0, rank_C = 0;  // shape of the prepared trace; rank_d 0 = nothing prepared
  int32_t rank_d = 0;
  DevBuf predict;  // workspace of the posterior predictive checks (rsf_predict_*): per-wave partials and their sums; quantiles
};

namespace {

int ensure(DevBuf &b, size_t bytes) {
  if (bytes <= b.cap && b.p) return RSF_OK;
  if (b.p) { HIP_TRY(hipFree(b.p)); b.p = nullptr; b.cap = 0; }
  if (bytes == 0) bytes = 8;
  HIP_TRY(hipMalloc(&b.p, bytes));
  b.cap = bytes;
  return RSF_OK;
}

void release(DevBuf &b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

bool host_mem(const rsf_ctx *c) { return c->cfg.mem_space == RSF_MEM_HOST; }

// input array: device pointer the kernels may read (staged copy for host callers)
template <class T> int stage_in(rsf_ctx *c, Slot slot, const T *src, size_t bytes, const T **dev) {
  if (!src) { *dev = nullptr; return RSF_OK; }
  if (!host_mem(c)) { *dev = src; return RSF_OK; }
  int rc = ensure(c->stage[slot], bytes);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->stage[slot].p, src, bytes, hipMemcpyHostToDevice, c->stream));
  *dev = (const T *)c->stage[slot].p;
  return RSF_OK;
}

// output array: device pointer the kernels may write
template <class T> int stage_out(rsf_ctx *c, Slot slot, T *dst, size_t bytes, T **dev) {
  if (!dst) { *dev = nullptr; return RSF_OK; }
  if (!host_mem(c)) { *dev = dst; return RSF_OK; }
  int rc = ensure(c->stage[slot], bytes);
  if (rc) return rc;
  *dev = (T *)c->stage[slot].p;
  return RSF_OK;
}

int copy_back(rsf_ctx *c, Slot slot, void *dst, size_t bytes) {
  if (!dst || !host_mem(c)) return RSF_OK;
  HIP_TRY(hipMemcpyAsync(dst, c->stage[slot].p, bytes, hipMemcpyDeviceToHost, c->stream));
  return RSF_OK;
}

int finish(rsf_ctx *c) {  // host callers get synchronous semantics
  HIP_TRY(hipGetLastError());
  if (host_mem(c)) HIP_TRY(hipStreamSynchronize(c->stream));
  return RSF_OK;
}

// What an entry point that touches the device begins with: its arguments (a NULL ctx, and whatever else the caller folds
// into args_ok and names in `what`), the state it needs, and the ctx's device selected for as long as the caller's guard
// lives.  fn: the entry point the messages name.
enum Need { NEED_NOTHING, NEED_MODEL, NEED_CHAINS, NEED_COMM };

int enter(DeviceGuard &guard, rsf_ctx *c, const char *fn, Need need, bool args_ok = true, const char *what = "NULL ctx") {
  static const char *const first[] = {nullptr, "rsf_set_model", "rsf_mcmc_init", "rsf_comm_init"};
  if (!c || !args_ok) return fail(RSF_ERR_INVALID, "%s: %s", fn, what);
  const bool have[] = {true, c->have_model, c->have_chains, c->world != 0};
  if (!have[need]) return fail(RSF_ERR_STATE, "%s: call %s first", fn, first[need]);
  if (!guard.select(c->device)) return fail(RSF_ERR_DEVICE, "%s: cannot select device %d", fn, c->device);
  return RSF_OK;
}

// ... as the first statement of the entry point itself, which it names; `guard` lives to the end of the enclosing block
#define RSF_ENTER(c, ...)                                            \
  DeviceGuard guard;                                                 \
  if (int rc_ = enter(guard, c, __func__, __VA_ARGS__)) return rc_

Consts make_consts(const rsf_ctx *c, const double *data, int64_t group_chains = 0) {
  Consts K{};
  K.mu_ref = c->m.mu_ref; K.V_ref = c->m.V_ref; K.k1 = c->m.k1; K.mu0 = c->m.mu_t_zero;
  K.a_def = c->m.a; K.b_def = c->m.b;
  K.h = c->h; K.hh = 0.5 * c->h; K.h6 = c->h / 6.0;
  K.inv_dt = 1.0 / c->delta_t;
  K.cacc = K.h6 * K.inv_dt;
  K.inv_vref = 1.0 / c->m.V_ref;
  K.t0 = c->m.t_start;
  K.dt = c->delta_t;
  K.vl = (const double *)c->vl.p;
  K.data = data;
  K.nout = c->nout; K.S = c->m.substeps; K.kc = c->kc; K.nchunks = c->nchunks;
  K.group_chains = group_chains;
  return K;
}

unsigned grid_for(const rsf_ctx *c, int64_t n) { return (unsigned)((n + c->block - 1) / c->block); }

int mode_of(const rsf_ctx *c) {
  return (c->m.flags & RSF_FLAG_DOP853) ? DOP853 : ((c->m.flags & RSF_FLAG_FP32_SOLVE) ? RK4_F32 : RK4_F64);
}

// radiation damping in a kernel of integrator `mode`.  The float64 RK4 kernels carry W = kvk v / V_ref = k1 v / a in place of
// v / V_ref with damping on (rsf_device.h, Lane::vrw), which needs k1 != 0; with k1 = 0 the damping pass is an exact identity
// and they run without it.
bool damped(const rsf_ctx *c, int mode) {
  return (c->m.flags & RSF_FLAG_RADIATION_DAMPING) && (mode != RK4_F64 || c->m.k1 != 0.0);
}

// chains a lane of the sampler kernel carries: two in the float32 mode (mcmc_f32x2_kernel), else one
int chains_per_lane(const rsf_ctx *c) { return mode_of(c) == RK4_F32 ? 2 : 1; }

// the table chunk as the sampler kernel stages it: doubles, or floats in the float32 sampler — with a chunk length of its own
// (kc32, rsf_set_model): nsteps 4000 is ONE chunk of 48 KB there, resident for the whole launch, where the shared length kc
// (sized for doubles) made it two, staged — with two workgroup barriers each — for every proposal
size_t mcmc_table_bytes(const rsf_ctx *c) {
  if (mode_of(c) != RK4_F32) return c->lds_bytes;
  const size_t floats = 2 * (size_t)c->m.substeps * (size_t)c->kc32 + 1 + (size_t)c->kc32 + 1;
  return (floats * sizeof(float) + 15) & ~(size_t)15;
}

// the sampler's kernel constants: the chains' observations and groups, and the chunking the sampler kernel of this mode uses
Consts make_sampler_consts(const rsf_ctx *c) {
  Consts K = make_consts(c, (const double *)c->data.p, c->group_chains);
  if (mode_of(c) == RK4_F32) { K.kc = c->kc32; K.nchunks = c->nchunks32; }
  return K;
}

// ---- kernel selection -----------------------------------------------------------------------------------------------
// A runtime selector becomes a template argument: with<V0, V1, ...>(v, f) hands f the one of the listed values that equals
// v (the last if none does) as a std::integral_constant.  Every *_fn below returns the TYPED pointer of one instantiation
// (the same address on every call: the replay graph compares it), and asks damped() itself with the integrator its kernel
// runs.  Only combinations that are launched are named: naming one instantiates it.
template <auto V0, auto... Vs, class F> auto with(int v, F f) {
  if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<decltype(V0), V0>{});
  else return v == (int)V0 ? f(std::integral_constant<decltype(V0), V0>{}) : with<Vs...>(v, f);
}

using ForwardFn = void (*)(Consts, int64_t, const double *, const double *, const double *, double *, double *);
using SamplerFn = void (*)(Consts, McmcArgs);

ForwardFn forward_fn(const rsf_ctx *c, bool want_ssq, bool want_acc) {  // NULL: nothing requested, nothing to launch
  return with<RK4_F32, DOP853, RK4_F64>(mode_of(c), [&](auto MODE) {
    return with<true, false>(damped(c, MODE), [&](auto DAMP) -> ForwardFn {
      if (want_ssq && want_acc) return forward_kernel<DAMP, true, true, MODE>;
      if (want_ssq) return forward_kernel<DAMP, true, false, MODE>;
      return want_acc ? forward_kernel<DAMP, false, true, MODE> : nullptr;
    });
  });
}

// rsf_mcmc_init's solve with its sensitivities, void (*)(Consts, InitArgs): DOP853, or the float64 RK4 — in the float32 mode as well
auto init_fn(const rsf_ctx *c, int d) {
  const bool dop = mode_of(c) == DOP853;
  return with<1, 3>(d, [&](auto D) {
    return with<true, false>(damped(c, dop ? DOP853 : RK4_F64), [&](auto DAMP) { return dop ? init_dp_kernel<D, DAMP> : init_kernel<D, DAMP>; });
  });
}

auto ssq32_fn(const rsf_ctx *c, int d) {  // void (*)(Consts, int64_t C, const double *q, double *ssq)
  return with<1, 3>(d, [&](auto D) { return with<true, false>(damped(c, RK4_F32), [&](auto DAMP) { return ssq32_kernel<D, DAMP>; }); });
}

// INJECT (rsf_mcmc_replay_ssq, any mode): the chain logic alone, which has no solve to damp
SamplerFn sampler_fn(const rsf_ctx *c, bool replay, bool inject) {
  return with<1, 3>(c->mc.n_params, [&](auto D) -> SamplerFn {
    if (inject) return mcmc_kernel<D, false, true, RK4_F64, true>;
    return with<RK4_F32, DOP853, RK4_F64>(mode_of(c), [&](auto MODE) {
      return with<true, false>(damped(c, MODE), [&](auto DAMP) {
        return with<true, false>(replay, [&](auto REPLAY) -> SamplerFn {
          if constexpr (MODE == RK4_F32) return mcmc_f32x2_kernel<D, DAMP, REPLAY>;
          else return mcmc_kernel<D, DAMP, REPLAY, MODE>;
        });
      });
    });
  });
}

// rsf_predict_partials' solve, void (*)(Consts, PredictArgs): the float64 RK4 tiers, in the float32 mode as well (like init_kernel)
auto predict_fn(const rsf_ctx *c, int d, bool want_series) {
  return with<1, 3>(d, [&](auto D) {
    return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) {
      return with<true, false>(want_series, [&](auto SERIES) { return predict_kernel<D, DAMP, SERIES>; });
    });
  });
}

auto propose_fn(int d) { return with<1, 3>(d, [](auto D) { return propose_kernel<D>; }); }        // void (*)(ProposeArgs)
auto diag_chain_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return diag_chain_kernel<D>; }); }  // 1 <= d <= RSF_MAX_PARAMS

// One launch on the ctx stream.  The parameter types come from the kernel's pointer alone, and the call's arguments are
// converted to them before their addresses are taken: a wrong count, order or type does not compile.
template <class T> struct as_declared { using type = T; };

template <class... P>
int launch(rsf_ctx *c, void (*fn)(P...), unsigned grid, unsigned block, size_t lds, typename as_declared<P>::type... a) {
  void *args[] = {(void *)&a...};
  HIP_TRY(hipLaunchKernel((const void *)fn, dim3(grid), dim3(block), args, lds, c->stream));
  return RSF_OK;
}

// The sampler kernel of a launch, and its grid and LDS: the table chunk (mcmc_table_bytes), and behind it per-lane slots
// (rsf_kernels.h: the float64 RK4 sampler parks the chain state there; the others keep only a three-parameter chain's
// Cholesky factor, one per chain of the lane).  INJECT (rsf_mcmc_replay_ssq, any mode): the chain logic alone on supplied
// sums of squares — no tables, one chain per lane, its slots at the base of LDS.
struct SamplerLaunch {
  SamplerFn fn;
  unsigned grid;
  size_t lds;
  int32_t lc_off;  // McmcArgs::lc_off: the slots' offset in doubles
};

SamplerLaunch sampler_launch(const rsf_ctx *c, bool replay, bool inject) {
  const int d = c->mc.n_params, mode = inject ? RK4_F64 : mode_of(c), nc = inject ? 1 : chains_per_lane(c);
  const size_t table = inject ? 0 : mcmc_table_bytes(c);
  const size_t slots = mode == RK4_F64 ? park_slots(d) : factor_slots(d) * nc;
  const int64_t per = (int64_t)c->block * nc;
  return {sampler_fn(c, replay, inject), (unsigned)((c->mc.n_chains + per - 1) / per), table + slots * sizeof(double) * (size_t)c->block,
          (int32_t)(table / sizeof(double))};
}

// [n][d] (the C ABI's layout) <-> [d][n] (the kernels' structure of arrays); both device pointers, on the ctx stream
int transpose(rsf_ctx *c, int64_t n, int d, const double *src, double *dst, bool to_soa) {
  if (d == 1) {
    if (src != dst) HIP_TRY(hipMemcpyAsync(dst, src, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return RSF_OK;
  }
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((n + kMaxBlock - 1) / kMaxBlock)), dim3(kMaxBlock), 0, c->stream, n, d, src, dst, to_soa);
  return RSF_OK;
}

// the caller's q [C][d] and V [C][d*d] into the chain state; a NULL one stays as it is
int put_q_V(rsf_ctx *c, int64_t C, int d, const double *q, const double *V) {
  const size_t cb = (size_t)C * sizeof(double);
  const double *dq, *dV;
  int rc;
  if ((rc = stage_in(c, SLOT_Q, q, cb * d, &dq))) return rc;
  if ((rc = stage_in(c, SLOT_V, V, cb * d * d, &dV))) return rc;
  if (q && (rc = transpose(c, C, d, dq, (double *)c->q.p, true))) return rc;
  if (V && (rc = transpose(c, C, d * d, dV, (double *)c->V.p, true))) return rc;
  return RSF_OK;
}

// RSF_MEM_HOST callers with a long run: launches of `per` iterations write their trace rows into one of two device
// staging sets; while launch k+1 computes, the rows of launch k go to the caller's arrays on a second stream.  The
// chain is the same as with one launch (the kernel continues from iter_base; tests: continuation == single launch).
// trace bytes per launch (cfg1: ~30 iterations, ~5 ms of compute); RSF_DRAIN_BYTES overrides it (tests use a tiny value)
size_t drain_bytes() {
  const char *e = std::getenv("RSF_DRAIN_BYTES");
  const long long v = e ? std::atoll(e) : 0;
  return v > 0 ? (size_t)v : (size_t)32 << 20;
}

int run_mcmc_drained(rsf_ctx *c, const SamplerLaunch &L, const Consts &K, McmcArgs A, int64_t per, double *tq, double *ts, uint8_t *ta) {
  const int d = c->mc.n_params;
  const size_t C = (size_t)A.C;
  const int64_t n_iters = A.n_iters;
  if (!c->copy_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (auto &e : c->ev_done) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  if (A.z || A.u || A.g || A.ssq_new)  // set 1 lies in their slots (Slot)
    return fail(RSF_ERR_STATE, "rsf_mcmc_run: a drained run cannot take supplied variates or sums of squares");
  const Slot slot_q[2] = {SLOT_TQ, SLOT_TQ_B}, slot_s[2] = {SLOT_TS, SLOT_TS_B}, slot_a[2] = {SLOT_TA, SLOT_TA_B};
  double *dq[2], *ds[2];
  uint8_t *da[2];
  int rc;
  for (int b = 0; b < 2; ++b) {
    if ((rc = stage_out(c, slot_q[b], tq, (size_t)per * C * d * sizeof(double), &dq[b]))) return rc;
    if ((rc = stage_out(c, slot_s[b], ts, (size_t)per * C * sizeof(double), &ds[b]))) return rc;
    if ((rc = stage_out(c, slot_a[b], ta, (size_t)per * C, &da[b]))) return rc;
  }
  auto drain = [&](int b, int64_t first, int64_t n) -> int {
    const size_t r0 = (size_t)first * C, rn = (size_t)n * C;
    HIP_TRY(hipStreamWaitEvent(c->copy_stream, c->ev_done[b], 0));
    if (tq) HIP_TRY(hipMemcpyAsync(tq + r0 * d, dq[b], rn * d * sizeof(double), hipMemcpyDeviceToHost, c->copy_stream));
    if (ts) HIP_TRY(hipMemcpyAsync(ts + r0, ds[b], rn * sizeof(double), hipMemcpyDeviceToHost, c->copy_stream));
    if (ta) HIP_TRY(hipMemcpyAsync(ta + r0, da[b], rn, hipMemcpyDeviceToHost, c->copy_stream));
    HIP_TRY(hipStreamSynchronize(c->copy_stream));  // the staging set is free again, the rows are in the caller's arrays
    return RSF_OK;
  };
  const int64_t base = A.iter_base;
  int64_t done = 0, prev_first = 0, prev_n = 0;
  int b = 0;
  while (done < n_iters) {
    const int64_t n = std::min(per, n_iters - done);
    A.n_iters = n; A.iter_base = base + done;
    A.tq = dq[b]; A.ts = ds[b]; A.ta = da[b];
    if ((rc = launch(c, L.fn, L.grid, c->block, L.lds, K, A))) return rc;
    HIP_TRY(hipEventRecord(c->ev_done[b], c->stream));
    if (prev_n && (rc = drain(b ^ 1, prev_first, prev_n))) return rc;
    prev_first = done; prev_n = n;
    done += n;
    b ^= 1;
  }
  if ((rc = drain(b ^ 1, prev_first, prev_n))) return rc;
  c->iters_done += n_iters;
  return finish(c);
}

constexpr int64_t kReplayGraphMaxChains = 4096;  // beyond this the copies dominate and the plain path is as good

void release_replay_graph(rsf_ctx *c) {
  auto &g = c->rg;
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  if (g.host) (void)hipHostFree(g.host);
  if (g.dev) (void)hipFree(g.dev);
  g = rsf_ctx::ReplayGraph{};
}

// ONE replayed proposal per call from host memory — what the drop-in MCMC.sample() does a thousand times, each call
// otherwise being three small H2D copies, a 0.1 ms kernel, three D2H copies and a synchronise.  The sequence is a
// three-node hipGraph (H2D of one pinned input block, the kernel, D2H of one pinned output block) instantiated once per
// (chains, parameters, kernel) and relaunched with fresh kernel arguments: one runtime call per proposal instead of seven.
int run_replay_graph(rsf_ctx *c, const SamplerLaunch &L, const Consts &K, McmcArgs A, const double *z, const double *u, const double *g, double *tq,
                     double *ts, uint8_t *ta) {
  auto &G = c->rg;
  const int d = c->mc.n_params;
  const size_t C = (size_t)A.C;
  const size_t in_bytes = (C * d + 2 * C) * sizeof(double), out_bytes = (C * d + C) * sizeof(double) + C;
  const size_t out_off = (in_bytes + 255) & ~(size_t)255, total = out_off + ((out_bytes + 255) & ~(size_t)255);
  char *hb = (char *)G.host, *db = (char *)G.dev;
  const bool rebuild = !G.exec || G.C != A.C || G.d != d || G.fn != (const void *)L.fn || G.lds != L.lds || G.block != c->block;
  if (rebuild) {
    release_replay_graph(c);
    HIP_TRY(hipHostMalloc(&G.host, total, hipHostMallocDefault));
    HIP_TRY(hipMalloc(&G.dev, total));
    hb = (char *)G.host; db = (char *)G.dev;
  }
  A.z = (const double *)db; A.u = A.z + C * d; A.g = A.u + C;
  A.tq = tq ? (double *)(db + out_off) : nullptr;
  A.ts = ts ? (double *)(db + out_off) + C * d : nullptr;
  A.ta = ta ? (uint8_t *)((double *)(db + out_off) + C * d + C) : nullptr;
  Consts Kc = K;
  void *params[2] = {&Kc, &A};
  hipKernelNodeParams kp{};
  kp.func = (void *)L.fn;
  kp.gridDim = dim3(L.grid); kp.blockDim = dim3(c->block);
  kp.sharedMemBytes = (unsigned)L.lds;
  kp.kernelParams = params;
  kp.extra = nullptr;
  if (rebuild) {
    hipGraphNode_t h2d, d2h;
    HIP_TRY(hipGraphCreate(&G.graph, 0));
    HIP_TRY(hipGraphAddMemcpyNode1D(&h2d, G.graph, nullptr, 0, db, hb, in_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipGraphAddKernelNode(&G.kernel, G.graph, &h2d, 1, &kp));
    HIP_TRY(hipGraphAddMemcpyNode1D(&d2h, G.graph, &G.kernel, 1, hb + out_off, db + out_off, out_bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipGraphInstantiate(&G.exec, G.graph, nullptr, nullptr, 0));
    G.C = A.C; G.d = d; G.fn = (const void *)L.fn; G.lds = L.lds; G.block = c->block;
  } else {
    HIP_TRY(hipGraphExecKernelNodeSetParams(G.exec, G.kernel, &kp));
  }
  double *hz = (double *)hb;
  std::memcpy(hz, z, C * d * sizeof(double));
  std::memcpy(hz + C * d, u, C * sizeof(double));
  std::memcpy(hz + C * d + C, g, C * sizeof(double));
  HIP_TRY(hipGraphLaunch(G.exec, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const double *ho = (const double *)(hb + out_off);
  if (tq) std::memcpy(tq, ho, C * d * sizeof(double));
  if (ts) std::memcpy(ts, ho + C * d, C * sizeof(double));
  if (ta) std::memcpy(ta, (const uint8_t *)(ho + C * d + C), C);
  c->iters_done += 1;
  return RSF_OK;
}

// the sampler's arguments that the ctx alone decides: chain state, limits, adaptation, and the iteration the launch begins at
McmcArgs mcmc_args(const rsf_ctx *c, int64_t n_iters) {
  McmcArgs A{};
  A.C = c->mc.n_chains; A.chain_offset = c->mc.chain_offset; A.n_iters = n_iters; A.iter_base = c->iters_done;
  A.seed = c->mc.seed; A.n0 = c->mc.n0; A.shape = 0.5 * (c->mc.n0 + (double)c->nout);  // MCMC.py:158
  A.gd = A.shape - 1.0 / 3.0; A.gc = 1.0 / std::sqrt(9.0 * A.gd);
  for (int p = 0; p < RSF_MAX_PARAMS; ++p) {
    A.lo[p] = c->mc.lo[p]; A.hi[p] = c->mc.hi[p];
    const double w = 1e-6 * (c->mc.hi[p] - c->mc.lo[p]);
    A.am_eps[p] = w * w;
  }
  A.adapt_mode = c->mc.adapt_mode; A.adapt_interval = c->mc.adapt_interval > 0 ? c->mc.adapt_interval : 1;
  A.dict_scale = 2.38 * 2.38 / (double)(c->mc.prior_len > 0 ? c->mc.prior_len : 2);
  A.q = (double *)c->q.p; A.ssq = (double *)c->ssq.p; A.std2 = (double *)c->std2.p; A.V = (double *)c->V.p;
  A.wref = (double *)c->wref.p; A.wsum = (double *)c->wsum.p; A.wsq = (double *)c->wsq.p; A.wn = (int32_t *)c->wn.p;
  A.wbuf = (double *)c->wbuf.p;
  A.stats = (unsigned long long *)c->stats.p;
  return A;
}

// rsf_mcmc_run, _replay (z, u, g) and _replay_ssq (ssq_new as well): all three report as rsf_mcmc_run
int run_mcmc(rsf_ctx *c, int64_t n_iters, const double *z, const double *u, const double *g, const double *ssq_new, double *tq,
             double *ts, uint8_t *ta, bool replay) {
  DeviceGuard guard;
  int rc;
  if ((rc = enter(guard, c, "rsf_mcmc_run", NEED_CHAINS, n_iters >= 0, "bad argument"))) return rc;
  if (c->external_chains && !ssq_new)
    return fail(RSF_ERR_STATE, "chains made by rsf_mcmc_init_state have no observation: advance them with rsf_mcmc_replay_ssq");
  if (n_iters > INT32_MAX) return fail(RSF_ERR_INVALID, "at most 2^31 - 1 iterations per call (every lane counts its own)");
  if (n_iters == 0) return RSF_OK;
  const int d = c->mc.n_params;
  const int64_t C = c->mc.n_chains;
  const size_t rows = (size_t)n_iters * (size_t)C;
  const SamplerLaunch L = sampler_launch(c, replay, ssq_new != nullptr);
  const Consts K = make_sampler_consts(c);
  McmcArgs A = mcmc_args(c, n_iters);
  A.lc_off = L.lc_off;
  if (replay && !ssq_new && host_mem(c) && n_iters == 1 && C <= kReplayGraphMaxChains) return run_replay_graph(c, L, K, A, z, u, g, tq, ts, ta);
  if ((rc = stage_in(c, SLOT_Z, z, rows * d * sizeof(double), &A.z))) return rc;
  if ((rc = stage_in(c, SLOT_U, u, rows * sizeof(double), &A.u))) return rc;
  if ((rc = stage_in(c, SLOT_G, g, rows * sizeof(double), &A.g))) return rc;
  if ((rc = stage_in(c, SLOT_SSQ_NEW, ssq_new, rows * sizeof(double), &A.ssq_new))) return rc;
  if (host_mem(c) && !replay) {
    const size_t row_bytes = (size_t)C * ((tq ? d * sizeof(double) : 0) + (ts ? sizeof(double) : 0) + (ta ? 1 : 0));
    const int64_t per = row_bytes ? std::max<int64_t>(1, (int64_t)(drain_bytes() / row_bytes)) : n_iters;
    if (per < n_iters) return run_mcmc_drained(c, L, K, A, per, tq, ts, ta);
  }
  if ((rc = stage_out(c, SLOT_TQ, tq, rows * d * sizeof(double), &A.tq))) return rc;
  if ((rc = stage_out(c, SLOT_TS, ts, rows * sizeof(double), &A.ts))) return rc;
  if ((rc = stage_out(c, SLOT_TA, ta, rows, &A.ta))) return rc;
  if ((rc = launch(c, L.fn, L.grid, c->block, L.lds, K, A))) return rc;
  if ((rc = copy_back(c, SLOT_TQ, tq, rows * d * sizeof(double)))) return rc;
  if ((rc = copy_back(c, SLOT_TS, ts, rows * sizeof(double)))) return rc;
  if ((rc = copy_back(c, SLOT_TA, ta, rows))) return rc;
  c->iters_done += n_iters;
  return finish(c);
}

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

void free_chains(rsf_ctx *c) {
  release(c->data); release(c->q); release(c->ssq); release(c->std2); release(c->V);
  release(c->wref); release(c->wsum); release(c->wsq); release(c->wn); release(c->wbuf); release(c->stats);
  c->have_chains = false;
  c->external_chains = false;
}

// RK4 table chunk: the output intervals kc whose (2*S*kc + 1) loading values + kc observations + the observation's sample
// 0 fit `entries`, at most all nout - 1 of them (0: not even one fits).  float32 solve (group8): residuals are summed in
// float32 over groups of eight samples (k = 1..8, 9..16, ...; rsf_device_f32.h, Out32) and its assembly trip covers one
// group: chunks begin on a group boundary.
int64_t rk4_chunk_len(int64_t entries, int S, int32_t nout, bool group8) {
  int64_t kc = std::min<int64_t>((entries - 2) / (2 * (int64_t)S + 1), nout - 1);
  if (group8 && kc < nout - 1 && kc >= 8) kc &= ~(int64_t)7;
  return kc;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int rsf_version(void) { return RSF_ABI_VERSION; }
const char *rsf_backend(void) { return "hip-gfx950"; }
#ifndef RSF_BUILD_ID  // csrc/Makefile passes the SHA-256 prefix of the kernel sources
#define RSF_BUILD_ID "unknown"
#endif
const char *rsf_build_id(void) { return RSF_BUILD_ID; }
const char *rsf_last_error(void) { return g_err; }

int rsf_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { fail(RSF_ERR_DEVICE, "hipGetDeviceCount -> %s", hipGetErrorString(e)); return 0; }
  return n;
}

int rsf_create(const rsf_config *cfg, rsf_ctx **out) {
  if (!cfg || !out) return fail(RSF_ERR_INVALID, "rsf_create: NULL argument");
  if (cfg->size != sizeof(rsf_config) || cfg->version != RSF_ABI_VERSION)
    return fail(RSF_ERR_INVALID, "rsf_create: config size/version mismatch");
  if (cfg->mem_space != RSF_MEM_HOST && cfg->mem_space != RSF_MEM_DEVICE)
    return fail(RSF_ERR_INVALID, "rsf_create: bad mem_space");
  int block = cfg->block_threads ? (int)cfg->block_threads : kMaxBlock;
  if (block % 64 != 0 || block < 64 || block > kMaxBlock)
    return fail(RSF_ERR_INVALID, "rsf_create: block_threads must be a multiple of 64 in [64, %d]", kMaxBlock);
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (n <= 0) return fail(RSF_ERR_DEVICE, "rsf_create: no HIP device visible (this library has no CPU fallback)");
  int dev = cfg->device;
  if (dev < 0) HIP_TRY(hipGetDevice(&dev));
  if (dev >= n) return fail(RSF_ERR_INVALID, "rsf_create: device %d out of range (%d visible)", dev, n);
  rsf_ctx *c = new (std::nothrow) rsf_ctx();
  if (!c) return fail(RSF_ERR_NOMEM, "rsf_create: out of memory");
  c->cfg = *cfg;
  c->device = dev;
  c->stream = (hipStream_t)cfg->stream;  // NULL = the device's default stream
  c->block = block;
  *out = c;
  return RSF_OK;
}

int rsf_destroy(rsf_ctx *c) {
  if (!c) return RSF_OK;
  {
    DeviceGuard guard(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_chains(c);
    release(c->vl);
    for (auto &s : c->stage) release(s);
    release(c->pool);
    release(c->poolws);
    release(c->diag);
    release(c->rankws);
    release(c->predict);
    release_replay_graph(c);
    if (c->comm) { const Rccl *R = rccl(); if (R) (void)R->comm_destroy(c->comm); }
    for (auto &e : c->ev_done) if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  }
  delete c;
  return RSF_OK;
}

int rsf_sync(rsf_ctx *c) {
  RSF_ENTER(c, NEED_NOTHING);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RSF_OK;
}

int rsf_set_model(rsf_ctx *c, const rsf_model *m) {
  RSF_ENTER(c, NEED_NOTHING, m != nullptr, "NULL argument");
  int rc;
  if (m->size != sizeof(rsf_model)) return fail(RSF_ERR_INVALID, "rsf_set_model: struct size mismatch");
  if (m->nsteps < 2 || m->substeps < 1 || !(m->t_final > m->t_start))
    return fail(RSF_ERR_INVALID, "rsf_set_model: need nsteps >= 2, substeps >= 1, t_final > t_start");
  if ((m->flags & RSF_FLAG_DOP853) && (m->flags & RSF_FLAG_FP32_SOLVE))
    return fail(RSF_ERR_INVALID, "rsf_set_model: the dop853 integrator is float64 only");
  const double delta_t = (m->t_final - m->t_start) / m->nsteps;                  // RateStateModel.py:176
  const int32_t nout = (int32_t)std::floor((m->t_final - m->t_start) / delta_t); // RateStateModel.py:358
  if (nout < 2) return fail(RSF_ERR_INVALID, "rsf_set_model: fewer than 2 output samples");
  const int S = m->substeps;
  const double h = delta_t / S, hh = 0.5 * h;
  const bool dop = m->flags & RSF_FLAG_DOP853;
  const size_t words = kLdsBudget / sizeof(double) - 2 * rsf::kLdsPad;
  int64_t kc;
  std::vector<double> vl;
  if (dop) {
    // DOP853 mode: per output interval the 12 loading values of the standard step (first step clipped to the
    // interval).  x is accumulated like scipy's r.t (x <- x + h with h = fl(fl(x + dt) - x)), so the stage times
    // are bit-identical to the ones the kernel — and the reference — use.
    kc = (int64_t)words / (rsf::dp::kTab + 1);
    if (kc > nout - 1) kc = nout - 1;
    vl.resize((size_t)rsf::dp::kTab * (size_t)(nout - 1));
    double x = m->t_start;
    for (int32_t k = 0; k < nout - 1; ++k) {
      const double xend = x + delta_t, hk = xend - x;
      for (int st = 0; st < rsf::dp::kTab; ++st) {
        const double t = st == 0 ? x : (st == 11 ? x + hk : x + RSF_DP_C[st] * hk);
        vl[(size_t)rsf::dp::kTab * k + st] = m->V_ref * (1 + std::exp(-t / 20) * std::sin(10 * t));
      }
      x = x + hk;
    }
  } else {
    kc = rk4_chunk_len((int64_t)words, S, nout, m->flags & RSF_FLAG_FP32_SOLVE);
    if (kc < 1) return fail(RSF_ERR_UNSUPPORTED, "rsf_set_model: substeps=%d does not fit the LDS staging budget", S);
    // chain-independent loading velocity at every RK4 stage time, RateStateModel.py:327-329
    vl.resize(2 * (size_t)S * (size_t)(nout - 1) + 1);
    for (size_t j = 0; j < vl.size(); ++j) {
      const double t = m->t_start + (double)j * hh;
      vl[j] = m->V_ref * (1 + std::exp(-t / 20) * std::sin(10 * t));
    }
  }
  const size_t nvl = vl.size();
  if ((rc = ensure(c->vl, nvl * sizeof(double)))) return rc;
  HIP_TRY(hipMemcpyAsync(c->vl.p, vl.data(), nvl * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // vl (host vector) goes out of scope
  if (c->have_chains) free_chains(c);  // chain state (SSq, sigma^2, covariance) belongs to the previous model
  c->m = *m;
  c->delta_t = delta_t; c->h = h; c->nout = nout;
  c->kc = (int32_t)kc;
  c->nchunks = (int32_t)((nout - 1 + kc - 1) / kc);
  c->kc32 = c->kc; c->nchunks32 = c->nchunks;
  if ((m->flags & RSF_FLAG_FP32_SOLVE) && !dop) {
    // the float32 sampler stages floats: the same budget in bytes holds twice the entries
    const int64_t k32 = rk4_chunk_len((int64_t)(kLdsBudget / sizeof(float)), S, nout, true);
    c->kc32 = (int32_t)k32;
    c->nchunks32 = (int32_t)((nout - 1 + k32 - 1) / k32);
  }
  c->lds_bytes = (size_t)((dop ? rsf::dp::kTab * kc : 2 * S * kc + 1) + kc + 1 + 2 * rsf::kLdsPad) * sizeof(double);
  c->have_model = true;
  return RSF_OK;
}

int rsf_model_nout(rsf_ctx *c, int32_t *nout) {
  if (!c || !nout) return fail(RSF_ERR_INVALID, "rsf_model_nout: NULL argument");
  if (!c->have_model) return fail(RSF_ERR_STATE, "rsf_model_nout: call rsf_set_model first");
  *nout = c->nout;
  return RSF_OK;
}

int rsf_forward_batch(rsf_ctx *c, int64_t n, const double *dc, const double *a, const double *b,
                      const double *data, double *ssq_out, double *acc_out) {
  RSF_ENTER(c, NEED_MODEL, dc && n >= 0, "bad argument");
  int rc;
  if (ssq_out && !data) return fail(RSF_ERR_INVALID, "rsf_forward_batch: ssq_out needs data");
  if (n == 0) return RSF_OK;
  const size_t nb = (size_t)n * sizeof(double);
  const double *ddc, *da, *db, *ddata;
  double *dssq, *dacc;
  if ((rc = stage_in(c, SLOT_DC, dc, nb, &ddc))) return rc;
  if ((rc = stage_in(c, SLOT_A, a, nb, &da))) return rc;
  if ((rc = stage_in(c, SLOT_B, b, nb, &db))) return rc;
  if ((rc = stage_in(c, SLOT_DATA, ssq_out ? data : nullptr, (size_t)c->nout * sizeof(double), &ddata))) return rc;
  if ((rc = stage_out(c, SLOT_SSQ_OUT, ssq_out, nb, &dssq))) return rc;
  if ((rc = stage_out(c, SLOT_ACC_OUT, acc_out, nb * (size_t)c->nout, &dacc))) return rc;
  if (const ForwardFn fn = forward_fn(c, ssq_out != nullptr, acc_out != nullptr))
    if ((rc = launch(c, fn, grid_for(c, n), c->block, c->lds_bytes, make_consts(c, ddata), n, ddc, da, db, dssq, dacc))) return rc;
  if ((rc = copy_back(c, SLOT_SSQ_OUT, ssq_out, nb))) return rc;
  if ((rc = copy_back(c, SLOT_ACC_OUT, acc_out, nb * (size_t)c->nout))) return rc;
  return finish(c);
}

// What rsf_mcmc_init and rsf_mcmc_init_state share: the config checks (fn: the entry point the messages name), the
// chain-state arrays (structure of arrays, rsf_kernels.h) with the adaptation window and counters, and a fresh window about
// the chains' points once q is set.
int check_mcmc_config(const rsf_mcmc_config *cfg, const char *fn) {
  if (cfg->size != sizeof(rsf_mcmc_config)) return fail(RSF_ERR_INVALID, "%s: struct size mismatch", fn);
  if (cfg->n_params != 1 && cfg->n_params != 3) return fail(RSF_ERR_UNSUPPORTED, "%s: n_params must be 1 or 3", fn);
  if (cfg->n_chains < 1) return fail(RSF_ERR_INVALID, "%s: n_chains < 1", fn);
  if (cfg->adapt_mode == RSF_ADAPT_REFERENCE_DICT && cfg->n_params != 1)
    return fail(RSF_ERR_UNSUPPORTED, "%s: reference_dict adaptation is defined for 1 parameter only", fn);
  if (cfg->adapt_mode < 0 || cfg->adapt_mode > RSF_ADAPT_AM || (cfg->adapt_mode && cfg->adapt_interval < 2))
    return fail(RSF_ERR_INVALID, "%s: bad adapt_mode / adapt_interval", fn);
  return RSF_OK;
}

int alloc_chains(rsf_ctx *c, const rsf_mcmc_config *cfg) {
  const int d = cfg->n_params;
  const int64_t C = cfg->n_chains;
  const size_t cb = (size_t)C * sizeof(double);
  int rc;
  if ((rc = ensure(c->q, cb * d))) return rc;
  if ((rc = ensure(c->ssq, cb))) return rc;
  if ((rc = ensure(c->std2, cb))) return rc;
  if ((rc = ensure(c->V, cb * d * d))) return rc;
  if ((rc = ensure(c->wref, cb * d))) return rc;
  if ((rc = ensure(c->wsum, cb * d))) return rc;
  if ((rc = ensure(c->wsq, cb * d * d))) return rc;
  if ((rc = ensure(c->wn, (size_t)C * sizeof(int32_t)))) return rc;
  if (cfg->adapt_mode == RSF_ADAPT_REFERENCE_DICT) {  // the window's samples themselves: np.cov's own arithmetic needs them
    if (cfg->adapt_interval > RSF_DICT_MAX_INTERVAL)
      return fail(RSF_ERR_UNSUPPORTED, "reference_dict adaptation keeps at most %d samples per window", RSF_DICT_MAX_INTERVAL);
    if ((rc = ensure(c->wbuf, cb * (size_t)cfg->adapt_interval))) return rc;
    HIP_TRY(hipMemsetAsync(c->wbuf.p, 0, cb * (size_t)cfg->adapt_interval, c->stream));
  }
  if ((rc = ensure(c->stats, RSF_CNT_COUNT * sizeof(unsigned long long)))) return rc;
  return RSF_OK;
}

int reset_window(rsf_ctx *c, const rsf_mcmc_config *cfg) {
  const int d = cfg->n_params;
  const int64_t C = cfg->n_chains;
  const size_t cb = (size_t)C * sizeof(double);
  HIP_TRY(hipMemcpyAsync(c->wref.p, c->q.p, cb * d, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->wsum.p, 0, cb * d, c->stream));
  HIP_TRY(hipMemsetAsync(c->wsq.p, 0, cb * d * d, c->stream));
  HIP_TRY(hipMemsetAsync(c->wn.p, 0, (size_t)C * sizeof(int32_t), c->stream));
  HIP_TRY(hipMemsetAsync(c->stats.p, 0, RSF_CNT_COUNT * sizeof(unsigned long long), c->stream));
  return RSF_OK;
}

int rsf_mcmc_init(rsf_ctx *c, const rsf_mcmc_config *cfg, const double *q0, const double *data) {
  RSF_ENTER(c, NEED_MODEL, cfg && q0 && data, "NULL argument");
  int rc;
  if ((rc = check_mcmc_config(cfg, "rsf_mcmc_init"))) return rc;
  const int G = cfg->n_groups > 1 ? cfg->n_groups : 1;
  // a workgroup's chains share one observation series: a group must be whole workgroups' worth of chains
  const int wg_chains = c->block * chains_per_lane(c);
  if (cfg->n_groups < 0 || cfg->n_chains % G || (G > 1 && (cfg->n_chains / G) % wg_chains))
    return fail(RSF_ERR_INVALID, "rsf_mcmc_init: n_chains/n_groups must be a whole multiple of a workgroup's chains (%d%s)", wg_chains,
                chains_per_lane(c) == 2 ? ": the float32 sampler carries two chains per lane" : "");
  const int d = cfg->n_params;
  const int64_t C = cfg->n_chains;
  const size_t cb = (size_t)C * sizeof(double);
  const size_t data_bytes = (size_t)G * (size_t)c->nout * sizeof(double);
  if ((rc = ensure(c->data, data_bytes))) return rc;
  if ((rc = alloc_chains(c, cfg))) return rc;
  const hipMemcpyKind kind = host_mem(c) ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  HIP_TRY(hipMemcpyAsync(c->data.p, data, data_bytes, kind, c->stream));
  const double *dq0;
  if ((rc = stage_in(c, SLOT_Q, q0, cb * d, &dq0))) return rc;
  if ((rc = transpose(c, C, d, dq0, (double *)c->q.p, true))) return rc;
  if ((rc = reset_window(c, cfg))) return rc;
  InitArgs A{};
  A.C = C;
  A.fd = cfg->fd_rel_step;
  A.inv_dof = 1.0 / (double)(c->nout - (cfg->prior_len ? cfg->prior_len : d));
  for (int p = 0; p < RSF_MAX_PARAMS; ++p) A.width[p] = cfg->hi[p] - cfg->lo[p];
  A.q0 = (const double *)c->q.p;
  A.ssq = (double *)c->ssq.p; A.std2 = (double *)c->std2.p; A.V = (double *)c->V.p;
  c->group_chains = G > 1 ? C / G : 0;
  // both kernels take the shared chunking (c->kc, c->lds_bytes): only the float32 SAMPLER has its own (rsf_kernels.h, kLdsBudget)
  const Consts K = make_consts(c, (const double *)c->data.p, c->group_chains);
  // the init kernels run one lane per TRAJECTORY: 1 + d adjacent lanes per chain (rsf_kernels.h, InitGroup)
  if ((rc = launch(c, init_fn(c, d), grid_for(c, C * (d + 1)), c->block, c->lds_bytes, K, A))) return rc;
  if (mode_of(c) == RK4_F32 && (rc = launch(c, ssq32_fn(c, d), grid_for(c, C), c->block, c->lds_bytes, K, C, A.q0, A.ssq))) return rc;
  c->mc = *cfg;
  c->iters_done = 0;
  c->have_chains = true;
  c->external_chains = false;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));  // q0/data may be host buffers the caller reuses
  return RSF_OK;
}

int rsf_mcmc_get_state(rsf_ctx *c, double *q, double *ssq, double *std2, double *V) {
  RSF_ENTER(c, NEED_CHAINS);
  int rc;
  const int d = c->mc.n_params;
  const size_t cb = (size_t)c->mc.n_chains * sizeof(double);
  const hipMemcpyKind kind = host_mem(c) ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  const int64_t C = c->mc.n_chains;
  double *dq, *dV;
  if ((rc = stage_out(c, SLOT_Q, q, cb * d, &dq))) return rc;
  if ((rc = stage_out(c, SLOT_V, V, cb * d * d, &dV))) return rc;
  if (q && (rc = transpose(c, C, d, (const double *)c->q.p, dq, false))) return rc;
  if (V && (rc = transpose(c, C, d * d, (const double *)c->V.p, dV, false))) return rc;
  if ((rc = copy_back(c, SLOT_Q, q, cb * d))) return rc;
  if ((rc = copy_back(c, SLOT_V, V, cb * d * d))) return rc;
  if (ssq) HIP_TRY(hipMemcpyAsync(ssq, c->ssq.p, cb, kind, c->stream));
  if (std2) HIP_TRY(hipMemcpyAsync(std2, c->std2.p, cb, kind, c->stream));
  return finish(c);
}

int rsf_mcmc_set_state(rsf_ctx *c, const double *q, const double *ssq, const double *std2, const double *V) {
  RSF_ENTER(c, NEED_CHAINS);
  int rc;
  const size_t cb = (size_t)c->mc.n_chains * sizeof(double);
  const hipMemcpyKind kind = host_mem(c) ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if ((rc = put_q_V(c, c->mc.n_chains, c->mc.n_params, q, V))) return rc;
  if (ssq) HIP_TRY(hipMemcpyAsync(c->ssq.p, ssq, cb, kind, c->stream));
  if (std2) HIP_TRY(hipMemcpyAsync(c->std2.p, std2, cb, kind, c->stream));
  return finish(c);
}

int rsf_mcmc_run(rsf_ctx *c, int64_t n_iters, double *tq, double *ts, uint8_t *ta) {
  return run_mcmc(c, n_iters, nullptr, nullptr, nullptr, nullptr, tq, ts, ta, false);
}

int rsf_mcmc_replay(rsf_ctx *c, int64_t n_iters, const double *z, const double *u, const double *g,
                    double *tq, double *ts, uint8_t *ta) {
  if (!z || !u || !g) return fail(RSF_ERR_INVALID, "rsf_mcmc_replay: z, u and g are required");
  return run_mcmc(c, n_iters, z, u, g, nullptr, tq, ts, ta, true);
}

int rsf_mcmc_replay_ssq(rsf_ctx *c, int64_t n_iters, const double *z, const double *u, const double *g, const double *ssq_new,
                        double *tq, double *ts, uint8_t *ta) {
  if (!z || !u || !g || !ssq_new) return fail(RSF_ERR_INVALID, "rsf_mcmc_replay_ssq: z, u, g and ssq_new are required");
  return run_mcmc(c, n_iters, z, u, g, ssq_new, tq, ts, ta, true);
}

int rsf_mcmc_init_state(rsf_ctx *c, const rsf_mcmc_config *cfg, const double *q, const double *ssq, const double *std2, const double *V) {
  RSF_ENTER(c, NEED_NOTHING, cfg && q && ssq && std2 && V, "NULL argument");
  int rc;
  if ((rc = check_mcmc_config(cfg, "rsf_mcmc_init_state"))) return rc;
  const size_t cb = (size_t)cfg->n_chains * sizeof(double);
  if ((rc = alloc_chains(c, cfg))) return rc;
  const hipMemcpyKind kind = host_mem(c) ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if ((rc = put_q_V(c, cfg->n_chains, cfg->n_params, q, V))) return rc;
  HIP_TRY(hipMemcpyAsync(c->ssq.p, ssq, cb, kind, c->stream));
  HIP_TRY(hipMemcpyAsync(c->std2.p, std2, cb, kind, c->stream));
  if ((rc = reset_window(c, cfg))) return rc;
  c->mc = *cfg;
  c->group_chains = 0;
  c->iters_done = 0;
  c->have_chains = true;
  c->external_chains = true;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));  // the arguments may be host buffers the caller reuses
  return RSF_OK;
}

int rsf_mcmc_propose(rsf_ctx *c, const double *z, double *q_new, uint8_t *in_bounds) {
  if (!c || !z || !q_new || !in_bounds) return fail(RSF_ERR_INVALID, "rsf_mcmc_propose: NULL argument");
  if (!c->have_chains) return fail(RSF_ERR_STATE, "rsf_mcmc_propose: call rsf_mcmc_init or rsf_mcmc_init_state first");
  RSF_ENTER(c, NEED_NOTHING);
  int rc;
  const int d = c->mc.n_params;
  const int64_t C = c->mc.n_chains;
  ProposeArgs A{};
  A.C = C; A.q = (const double *)c->q.p; A.V = (const double *)c->V.p;
  for (int p = 0; p < RSF_MAX_PARAMS; ++p) { A.lo[p] = c->mc.lo[p]; A.hi[p] = c->mc.hi[p]; }
  if ((rc = stage_in(c, SLOT_Z, z, (size_t)C * d * sizeof(double), &A.z))) return rc;
  if ((rc = stage_out(c, SLOT_Q_NEW, q_new, (size_t)C * d * sizeof(double), &A.qn))) return rc;
  if ((rc = stage_out(c, SLOT_IN_BOUNDS, in_bounds, (size_t)C, &A.inb))) return rc;
  if ((rc = launch(c, propose_fn(d), (unsigned)((C + kMaxBlock - 1) / kMaxBlock), kMaxBlock, 0, A))) return rc;
  if ((rc = copy_back(c, SLOT_Q_NEW, q_new, (size_t)C * d * sizeof(double)))) return rc;
  if ((rc = copy_back(c, SLOT_IN_BOUNDS, in_bounds, (size_t)C))) return rc;
  return finish(c);
}

int rsf_mcmc_stats(rsf_ctx *c, int64_t *n_acc, int64_t *n_eval, int64_t *n_nonfinite, int64_t *n_done) {
  RSF_ENTER(c, NEED_CHAINS);
  unsigned long long s[3];
  HIP_TRY(hipMemcpyAsync(s, c->stats.p, sizeof s, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n_acc) *n_acc = (int64_t)s[RSF_CNT_ACCEPTED];
  if (n_eval) *n_eval = (int64_t)s[RSF_CNT_EVALUATED];
  if (n_nonfinite) *n_nonfinite = (int64_t)s[RSF_CNT_NONFINITE];
  if (n_done) *n_done = c->iters_done;
  return RSF_OK;
}

int rsf_mcmc_counters(rsf_ctx *c, int64_t *out, int32_t n) {
  RSF_ENTER(c, NEED_CHAINS, out && n >= 0, "bad argument");
  unsigned long long s[RSF_CNT_COUNT];
  HIP_TRY(hipMemcpyAsync(s, c->stats.p, sizeof s, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int32_t k = 0; k < n && k < RSF_CNT_COUNT; ++k) out[k] = (int64_t)s[k];
  return RSF_OK;
}

namespace {

// moments of x[i*stride] with x already a device pointer; result on the host
int pool_moments(rsf_ctx *c, int64_t n, const double *dx, int64_t stride, double out[5]) {
  int rc = ensure(c->pool, sizeof(PoolPartial) * kPoolBlocks);
  if (rc) return rc;
  double shift = 0.0;
  HIP_TRY(hipMemcpyAsync(&shift, dx, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int blocks = (int)std::min<int64_t>(kPoolBlocks, (n + kMaxBlock - 1) / kMaxBlock);
  hipLaunchKernelGGL(pool_moments_kernel, dim3(blocks), dim3(kMaxBlock), 0, c->stream, n, dx, stride, shift, (PoolPartial *)c->pool.p);
  std::vector<PoolPartial> h(blocks);
  HIP_TRY(hipMemcpyAsync(h.data(), c->pool.p, sizeof(PoolPartial) * blocks, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  double cnt = 0, sum = 0, sumsq = 0, mn = INFINITY, mx = -INFINITY;
  for (const auto &p : h) { cnt += p.cnt; sum += p.sum; sumsq += p.sumsq; mn = std::fmin(mn, p.mn); mx = std::fmax(mx, p.mx); }
  const double mean_s = sum / cnt;
  out[0] = cnt; out[1] = shift + mean_s;
  out[2] = cnt > 1 ? (sumsq - cnt * mean_s * mean_s) / (cnt - 1) : 0.0;
  out[3] = mn; out[4] = mx;
  return RSF_OK;
}

}  // namespace

int rsf_pool_summary(rsf_ctx *c, int64_t n, const double *x, int64_t stride, double *out) {
  RSF_ENTER(c, NEED_NOTHING, x && out && n >= 1 && stride >= 1, "bad argument");
  int rc;
  const double *dx;
  if ((rc = stage_in(c, SLOT_X, x, (size_t)((n - 1) * stride + 1) * sizeof(double), &dx))) return rc;
  return pool_moments(c, n, dx, stride, out);
}

int rsf_pool_kde(rsf_ctx *c, int64_t n, const double *x, int64_t stride, int32_t m, const double *grid, double bw_factor,
                 double *density) {
  RSF_ENTER(c, NEED_NOTHING, x && grid && density && n >= 2 && m >= 1 && stride >= 1, "bad argument");
  int rc;
  const double *dx, *dg;
  double *dd;
  if ((rc = stage_in(c, SLOT_X, x, (size_t)((n - 1) * stride + 1) * sizeof(double), &dx))) return rc;
  if ((rc = stage_in(c, SLOT_GRID, grid, (size_t)m * sizeof(double), &dg))) return rc;
  if ((rc = stage_out(c, SLOT_POOL_OUT, density, (size_t)m * sizeof(double), &dd))) return rc;
  double s[5];
  if ((rc = pool_moments(c, n, dx, stride, s))) return rc;
  const double factor = bw_factor > 0.0 ? bw_factor : std::pow((double)n, -1.0 / 5.0);  // scipy scotts_factor, d = 1
  const double cov = s[2] * factor * factor;
  if (!(cov > 0.0)) return fail(RSF_ERR_INVALID, "rsf_pool_kde: the samples have zero variance (singular KDE)");
  const int blocks = (int)std::min<int64_t>(kPoolBlocks, (n + kKdeTile - 1) / kKdeTile);
  DevBuf &ws = c->poolws;
  if ((rc = ensure(ws, (size_t)blocks * (size_t)m * sizeof(double)))) return rc;
  hipLaunchKernelGGL(pool_kde_kernel, dim3(blocks), dim3(kMaxBlock), 0, c->stream, n, dx, stride, (int)m, dg, 0.5 / cov,
                     (double *)ws.p);
  hipLaunchKernelGGL(pool_kde_reduce_kernel, dim3((m + kMaxBlock - 1) / kMaxBlock), dim3(kMaxBlock), 0, c->stream, blocks, (int)m,
                     (const double *)ws.p, 1.0 / ((double)n * std::sqrt(2.0 * 3.14159265358979323846 * cov)), dd);
  if ((rc = copy_back(c, SLOT_POOL_OUT, density, (size_t)m * sizeof(double)))) return rc;
  return finish(c);
}

int rsf_pool_histogram(rsf_ctx *c, int64_t n, const double *x, int64_t stride, int32_t nbins, double lo, double hi, double *counts) {
  if (!c || !x || !counts || n < 1 || stride < 1 || nbins < 1 || nbins > kHistMaxBins || !(hi > lo) || !std::isfinite(hi - lo))
    return fail(RSF_ERR_INVALID, "rsf_pool_histogram: bad argument (1 <= nbins <= %d, finite lo < hi)", kHistMaxBins);
  RSF_ENTER(c, NEED_NOTHING);
  int rc;
  const double *dx;
  double *dout;
  const int nb = nbins + 2;
  if ((rc = stage_in(c, SLOT_X, x, (size_t)((n - 1) * stride + 1) * sizeof(double), &dx))) return rc;
  if ((rc = stage_out(c, SLOT_POOL_OUT, counts, (size_t)nb * sizeof(double), &dout))) return rc;
  DevBuf &ws = c->poolws;
  if ((rc = ensure(ws, (size_t)nb * sizeof(unsigned long long)))) return rc;
  HIP_TRY(hipMemsetAsync(ws.p, 0, (size_t)nb * sizeof(unsigned long long), c->stream));
  const int blocks = (int)std::min<int64_t>(kPoolBlocks, (n + kMaxBlock - 1) / kMaxBlock);
  hipLaunchKernelGGL(pool_hist_kernel, dim3(blocks), dim3(kMaxBlock), (size_t)nb * sizeof(unsigned int), c->stream, n, dx, stride,
                     (int)nbins, lo, hi, (double)nbins / (hi - lo), (hi - lo) / (double)nbins, (unsigned long long *)ws.p);
  hipLaunchKernelGGL(pool_hist_finish_kernel, dim3((nb + kMaxBlock - 1) / kMaxBlock), dim3(kMaxBlock), 0, c->stream, nb,
                     (const unsigned long long *)ws.p, dout);
  if ((rc = copy_back(c, SLOT_POOL_OUT, counts, (size_t)nb * sizeof(double)))) return rc;
  return finish(c);
}

// ---- convergence diagnostics (include/rsf_diag.h) ----------------------------------------------
namespace {
// The lags [lag_begin, lag_end) of a partials call on n draws of C chains and d parameters, and the grid they make: L lags in
// ntiles tiles for each of nbc blocks of chains.  fn: the entry point the messages name.
struct LagGrid { int64_t lag_begin, lag_end, L, nbc, ntiles; };

int check_lags(const char *fn, int64_t n, int64_t C, int32_t d, int64_t lag_begin, int64_t lag_end, LagGrid *g) {
  const int64_t N = n / 2;
  if (lag_begin < 0 || lag_end <= lag_begin || lag_end > N)
    return fail(RSF_ERR_INVALID, "%s: lags [%lld, %lld) are not a non-empty range within [0, %lld)", fn, (long long)lag_begin,
                (long long)lag_end, (long long)N);
  const int64_t L = lag_end - lag_begin;
  *g = {lag_begin, lag_end, L, (C + kDiagBlock - 1) / kDiagBlock, (L + kLagTile - 1) / kLagTile};
  if (g->nbc * d * g->ntiles > INT32_MAX) return fail(RSF_ERR_INVALID, "%s: too many lags for one call; ask for fewer", fn);
  return RSF_OK;
}

// rsf_diag_partials after its checks, on a trace x already in device memory
int diag_partials_dev(rsf_ctx *c, int64_t n, int64_t C, int32_t d, const double *x, int64_t S, const rsfk::DiagCenter &cen,
                      const LagGrid &lg, double *partials) {
  const int64_t N = n / 2, L = lg.L, nbc = lg.nbc;
  const int64_t K = S ? C / S : 0, nbs = S ? std::min<int64_t>(kDiagSuperBlocks, (K + kDiagBlock / 64 - 1) / (kDiagBlock / 64)) : 0;
  // workspace, doubles: mh[2][d][C] | fm[d][C] | fv[d][C] | chain partials[nbc][d][3] | superchain partials[nbs][d][4] |
  // lag partials[nbc][d][L] | sums[d*3 + d*4 + d*L]
  const int64_t nf1 = d * kDiagChainFields, nf2 = d * kDiagSuperFields, nf3 = d * L;
  const int64_t o_fm = 2 * d * C, o_fv = o_fm + d * C, o_p1 = o_fv + d * C, o_p2 = o_p1 + nbc * nf1, o_p3 = o_p2 + nbs * nf2,
                o_sum = o_p3 + nbc * nf3, total = o_sum + nf1 + nf2 + nf3;
  int rc;
  if ((rc = ensure(c->diag, (size_t)total * sizeof(double)))) return rc;
  double *w = (double *)c->diag.p;
  const rsfk::DiagShape sh{n, C, d, N, n - N};
  if ((rc = launch(c, diag_chain_fn(d), (unsigned)nbc, kDiagBlock, 0, sh, x, cen, w, w + o_fm, w + o_fv, w + o_p1))) return rc;
  if (S) hipLaunchKernelGGL(diag_super_kernel, dim3((unsigned)nbs), dim3(kDiagBlock), 0, c->stream, C, (int)d, S, cen, (const double *)(w + o_fm),
                            (const double *)(w + o_fv), w + o_p2);
  hipLaunchKernelGGL(diag_lag_kernel, dim3((unsigned)(nbc * d * lg.ntiles)), dim3(kDiagBlock), 0, c->stream, sh, x, (const double *)w,
                     lg.lag_begin, lg.lag_end, w + o_p3);
  const int64_t sum_blocks = (std::max<int64_t>(nf1, std::max(nf2, nf3)) + kDiagBlock - 1) / kDiagBlock;
  hipLaunchKernelGGL(diag_sum_kernel, dim3((unsigned)sum_blocks), dim3(kDiagBlock), 0, c->stream, nbc, nf1, (const double *)(w + o_p1), w + o_sum);
  if (S) hipLaunchKernelGGL(diag_sum_kernel, dim3((unsigned)sum_blocks), dim3(kDiagBlock), 0, c->stream, nbs, nf2, (const double *)(w + o_p2),
                            w + o_sum + nf1);
  hipLaunchKernelGGL(diag_sum_kernel, dim3((unsigned)sum_blocks), dim3(kDiagBlock), 0, c->stream, nbc, nf3, (const double *)(w + o_p3),
                     w + o_sum + nf1 + nf2);
  HIP_TRY(hipGetLastError());
  std::vector<double> h((size_t)(nf1 + nf2 + nf3), 0.0);
  HIP_TRY(hipMemcpyAsync(h.data(), w + o_sum, sizeof(double) * (size_t)(nf1 + (S ? nf2 : 0)), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(h.data() + nf1 + nf2, w + o_sum + nf1 + nf2, sizeof(double) * (size_t)nf3, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int p = 0; p < d; ++p) {
    double *o = partials + (int64_t)p * (RSF_DIAG_HEAD + L);
    const double *h1 = h.data() + p * kDiagChainFields, *h2 = h.data() + nf1 + p * kDiagSuperFields, *h3 = h.data() + nf1 + nf2 + p * L;
    o[0] = 2.0 * (double)C;
    o[1] = h1[0]; o[2] = h1[1]; o[3] = h1[2];
    o[4] = (double)K;
    for (int f = 0; f < kDiagSuperFields; ++f) o[5 + f] = S ? h2[f] : 0.0;
    for (int64_t j = 0; j < L; ++j) o[RSF_DIAG_HEAD + j] = h3[j];
  }
  return RSF_OK;
}
}  // namespace

int rsf_diag_partials(rsf_ctx *c, int64_t n, int64_t C, int32_t d, const double *trace, int64_t S, const double *center,
                      int64_t lag_begin, int64_t lag_end, double *partials) {
  if (!c || !trace || !center || !partials) return fail(RSF_ERR_INVALID, "rsf_diag_partials: NULL argument");
  if (n < 4 || C < 1 || d < 1 || d > RSF_MAX_PARAMS)
    return fail(RSF_ERR_INVALID, "rsf_diag_partials: need n_iters >= 4, n_chains >= 1, 1 <= n_params <= %d", RSF_MAX_PARAMS);
  if (S < 0 || (S > 0 && C % S)) return fail(RSF_ERR_INVALID, "rsf_diag_partials: chains_per_superchain %lld does not divide %lld chains",
                                             (long long)S, (long long)C);
  if (n > INT64_MAX / 8 / C / d) return fail(RSF_ERR_INVALID, "rsf_diag_partials: trace too large");
  LagGrid lg;
  int rc;
  if ((rc = check_lags("rsf_diag_partials", n, C, d, lag_begin, lag_end, &lg))) return rc;
  rsfk::DiagCenter cen{{0.0, 0.0, 0.0}};
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(center[p])) return fail(RSF_ERR_INVALID, "rsf_diag_partials: center[%d] is not finite", p);
    cen.v[p] = center[p];
  }
  RSF_ENTER(c, NEED_NOTHING);
  const double *dx;
  if ((rc = stage_in(c, SLOT_X, trace, (size_t)(n * C * d) * sizeof(double), &dx))) return rc;
  return diag_partials_dev(c, n, C, d, dx, S, cen, lg, partials);
}

int rsf_diag_finish(int64_t n, int32_t d, int64_t S, const double *center, const double *partials, int64_t n_lags, double *out) {
  if (!center || !partials || !out) return fail(RSF_ERR_INVALID, "rsf_diag_finish: NULL argument");
  if (n < 4 || d < 1 || d > RSF_MAX_PARAMS || S < 0)
    return fail(RSF_ERR_INVALID, "rsf_diag_finish: need n_iters >= 4, 1 <= n_params <= %d, chains_per_superchain >= 0", RSF_MAX_PARAMS);
  const int64_t N = n / 2;
  if (n_lags < 2 || n_lags > N) return fail(RSF_ERR_INVALID, "rsf_diag_finish: n_lags %lld outside [2, %lld]", (long long)n_lags, (long long)N);
  const double Nd = (double)N;
  std::vector<double> r((size_t)n_lags);
  for (int p = 0; p < d; ++p) {
    const double *q = partials + (int64_t)p * (RSF_DIAG_HEAD + n_lags);
    double *o = out + (int64_t)p * RSF_DIAG_OUT;
    for (int f = 0; f < RSF_DIAG_OUT; ++f) o[f] = NAN;
    o[RSF_DIAG_K] = q[4];
    o[RSF_DIAG_LAGS_COMPLETE] = 1.0;
    bool finite = std::isfinite(center[p]);
    for (int64_t f = 0; f < RSF_DIAG_HEAD + n_lags; ++f) finite = finite && std::isfinite(q[f]);
    if (!finite) continue;  // a non-finite draw: every statistic of this parameter is NaN
    const double Mp = q[0], ybar = q[1] / Mp, W = q[3] / Mp;
    const double BN = (q[2] - q[1] * ybar) / (Mp - 1.0);
    const double var_plus = (Nd - 1.0) / Nd * W + BN;
    o[RSF_DIAG_MEAN] = center[p] + ybar;
    o[RSF_DIAG_VAR_PLUS] = var_plus;
    o[RSF_DIAG_W] = W;
    o[RSF_DIAG_B_OVER_N] = BN;
    const double K = q[4];
    if (S > 0 && K > 1.0) {
      const double B_nu = (q[6] - q[5] * q[5] / K) / (K - 1.0), W_nu = (q[7] + q[8]) / K;
      if (W_nu > 0.0) o[RSF_DIAG_NESTED_RHAT] = std::sqrt(1.0 + B_nu / W_nu);
    }
    if (!(W > 0.0)) continue;  // every split chain constant
    o[RSF_DIAG_SPLIT_RHAT] = std::sqrt(var_plus / W);
    // ArviZ's _ess on the split chains, step by step (tests/diagnostics_reference.py), with the sequence cut at n_lags
    auto rho = [&](int64_t t) { return 1.0 - (W - q[RSF_DIAG_HEAD + t] / Mp) / var_plus; };
    std::fill(r.begin(), r.end(), 0.0);
    double ev = 1.0, od = rho(1);
    r[0] = ev; r[1] = od;
    int64_t t = 1;
    const int64_t lim = std::min(N - 3, n_lags - 2);  // the pair (t+1, t+2) needs lag t+2 < n_lags
    while (t < lim && ev + od > 0.0) {  // Geyer's initial positive sequence
      ev = rho(t + 1);
      od = rho(t + 2);
      if (ev + od >= 0.0) { r[t + 1] = ev; r[t + 2] = od; }
      t += 2;
    }
    o[RSF_DIAG_LAGS_COMPLETE] = (ev + od > 0.0 && t < N - 3) ? 0.0 : 1.0;
    const int64_t max_t = t - 2;
    if (ev > 0.0) r[max_t + 1] = ev;
    for (int64_t u = 1; u <= max_t - 2; u += 2)  // Geyer's initial monotone sequence
      if (r[u + 1] + r[u + 2] > r[u - 1] + r[u]) { r[u + 1] = 0.5 * (r[u - 1] + r[u]); r[u + 2] = r[u + 1]; }
    double tau = 0.0;
    for (int64_t u = 0; u <= max_t; ++u) tau += r[u];
    tau = -1.0 + 2.0 * tau + r[max_t + 1];
    const double MN = Mp * Nd;
    tau = std::max(tau, 1.0 / std::log10(MN));
    o[RSF_DIAG_TAU] = tau;
    o[RSF_DIAG_ESS] = MN / tau;
    o[RSF_DIAG_MCSE_MEAN] = std::sqrt(var_plus / o[RSF_DIAG_ESS]);
  }
  return RSF_OK;
}

// ---- rank-normalised diagnostics and order statistics (include/rsf_diag.h, rsf_diag_rank_*) ------------------
namespace {
constexpr int64_t kRankMaxDraws = INT64_C(1) << 32;  // 32-bit sort indices

// the rank workspace, carved from c->rank (byte offsets rounded to 256)
struct RankWs {
  double *series;            // [4][A][d]
  uint64_t *keys[2];         // [A]
  uint32_t *idx[2];          // [A + 1] (the spare one holds P during the ranks)
  uint32_t *th;              // [256][ntiles]: tile histograms, then offsets
  uint32_t *tm, *tlast, *tfirst;  // [ntiles]
  uint32_t *hist;            // [8][256] + the non-finite count
  uint32_t *hpart;           // [kRankKeyBlocks][kRankHist]: per-workgroup histograms of rank_key_kernel
  void *part;                // [kRankReduceBlocks] RankArg or 2 doubles
  double *probs, *stats;     // [n_probs], [d][RSF_DIAG_RANK_STATS + n_probs]
};

size_t rank_ws_layout(int64_t A, int d, int np, char *base, RankWs *w) {
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) / 256 * 256; return base ? base + at : nullptr; };  // base NULL: size only
  const int64_t ntiles = (A + kRankTile - 1) / kRankTile;
  w->series = (double *)take((size_t)(4 * A * d) * sizeof(double));
  for (int b = 0; b < 2; ++b) w->keys[b] = (uint64_t *)take((size_t)A * sizeof(uint64_t));
  for (int b = 0; b < 2; ++b) w->idx[b] = (uint32_t *)take((size_t)(A + 1) * sizeof(uint32_t));
  w->th = (uint32_t *)take((size_t)(256 * ntiles) * sizeof(uint32_t));
  w->tm = (uint32_t *)take((size_t)ntiles * sizeof(uint32_t));
  w->tlast = (uint32_t *)take((size_t)ntiles * sizeof(uint32_t));
  w->tfirst = (uint32_t *)take((size_t)ntiles * sizeof(uint32_t));
  w->hist = (uint32_t *)take(kRankHist * sizeof(uint32_t));
  w->hpart = (uint32_t *)take((size_t)kRankKeyBlocks * kRankHist * sizeof(uint32_t));
  w->part = take(kRankReduceBlocks * sizeof(RankArg));
  w->probs = (double *)take((size_t)(np > 0 ? np : 1) * sizeof(double));
  w->stats = (double *)take((size_t)(d * (RSF_DIAG_RANK_STATS + np)) * sizeof(double));
  return o;
}

// Sorts parameter p's keys (of x, or of |x - median| when folded) into keys[*cur] / idx[*cur]; *bad = a non-finite draw
int rank_sort(rsf_ctx *c, RankWs &w, int64_t A, int d, int p, const double *x, bool folded, const double *st, int *cur, bool *bad) {
  const int64_t ntiles = (A + kRankTile - 1) / kRankTile;
  const int nkb = (int)std::min<int64_t>(kRankKeyBlocks, ntiles);
  hipLaunchKernelGGL(rank_key_kernel, dim3((unsigned)nkb), dim3(kRankThreads), 0, c->stream, A, d, p, x, folded, st, w.keys[0], w.idx[0], w.hpart);
  hipLaunchKernelGGL(rank_hist_kernel, dim3((kRankHist + kRankThreads - 1) / kRankThreads), dim3(kRankThreads), 0, c->stream, nkb,
                     (const uint32_t *)w.hpart, w.hist);
  HIP_TRY(hipGetLastError());
  std::vector<uint32_t> h(kRankHist);
  HIP_TRY(hipMemcpyAsync(h.data(), w.hist, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *bad = h[kRankDigits * 256] != 0;
  *cur = 0;
  if (*bad) return RSF_OK;
  for (int g = 0; g < kRankDigits; ++g) {
    bool one = false;  // one bucket holds every key: the pass would not move anything
    for (int b = 0; b < 256; ++b) one = one || (int64_t)h[g * 256 + b] == A;
    if (one) continue;
    const int s = *cur;
    hipLaunchKernelGGL(rank_upsweep_kernel, dim3((unsigned)ntiles), dim3(kRankThreads), 0, c->stream, A, 8 * g, (const uint64_t *)w.keys[s],
                       w.th, ntiles);
    hipLaunchKernelGGL(rank_offsets_kernel, dim3(256), dim3(kRankThreads), 0, c->stream, (const uint32_t *)(w.hist + g * 256), w.th, ntiles);
    hipLaunchKernelGGL(rank_scatter_kernel, dim3((unsigned)ntiles), dim3(kRankThreads), 0, c->stream, A, 8 * g, (const uint64_t *)w.keys[s],
                       (const uint32_t *)w.idx[s], w.keys[1 - s], w.idx[1 - s], (const uint32_t *)w.th, ntiles);
    *cur = 1 - s;
  }
  HIP_TRY(hipGetLastError());
  return RSF_OK;
}

// the normal scores of the sorted pairs keys[s] / idx[s] into out (+ p, stride d); idx[1 - s] holds P
int rank_scores(rsf_ctx *c, RankWs &w, const RankShape &rs, int s, double *out) {
  const int64_t ntiles = (rs.A + kRankTile - 1) / kRankTile;
  const uint64_t *k = w.keys[s];
  const uint32_t *ix = w.idx[s];
  uint32_t *P = w.idx[1 - s];
  hipLaunchKernelGGL(rank_tile_kernel, dim3((unsigned)ntiles), dim3(kRankThreads), 0, c->stream, rs, k, ix, w.tm, w.tlast, w.tfirst);
  hipLaunchKernelGGL(rank_carry_kernel, dim3(1), dim3(kRankThreads), 0, c->stream, ntiles, (uint32_t)rs.A, w.tm, w.tlast, w.tfirst);
  hipLaunchKernelGGL(rank_prefix_kernel, dim3((unsigned)ntiles), dim3(kRankThreads), 0, c->stream, rs, k, ix, (const uint32_t *)w.tm, P);
  hipLaunchKernelGGL(rank_z_kernel, dim3((unsigned)ntiles), dim3(kRankThreads), 0, c->stream, rs, k, ix, (const uint32_t *)w.tlast,
                     (const uint32_t *)w.tfirst, (const uint32_t *)P, out);
  HIP_TRY(hipGetLastError());
  return RSF_OK;
}

int rank_grid(int64_t work, int64_t cap) { return (int)std::max<int64_t>(1, std::min<int64_t>(cap, (work + kRankThreads - 1) / kRankThreads)); }
}  // namespace

namespace {
// the first probability outside [0, 1] (NaN included), or -1
int first_bad_prob(int n, const double *probs) {
  for (int i = 0; i < n; ++i)
    if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) return i;
  return -1;
}
// a materialised series [nout][n] as the select kernels index it
int check_series_shape(const char *fn, int64_t n, int64_t nout) {
  if (n < 1 || n >= (INT64_C(1) << 31) || nout < 1 || nout > INT32_MAX || n > INT64_MAX / 8 / nout)
    return fail(RSF_ERR_INVALID, "%s: need 1 <= n < 2^31 draws and 1 <= nout rows", fn);
  return RSF_OK;
}
// the series is the largest allocation of its call: a failure to stage it is reported as RSF_ERR_NOMEM with its size
int series_nomem(const char *fn, int64_t n, int64_t nout, const char *advice = "") {
  (void)hipGetLastError();
  return fail(RSF_ERR_NOMEM, "%s: cannot allocate the series' device copy (%lld x %lld doubles)%s", fn, (long long)nout, (long long)n, advice);
}
int stage_series(rsf_ctx *c, const char *fn, Slot slot, const double *series, int64_t n, int64_t nout, const double **dev) {
  return stage_in(c, slot, series, (size_t)n * (size_t)nout * sizeof(double), dev) ? series_nomem(fn, n, nout) : RSF_OK;
}
}  // namespace

int rsf_diag_rank_prepare(rsf_ctx *c, int64_t n, int64_t C, int32_t d, const double *trace, int32_t n_probs, const double *probs,
                          double hdi_prob, double *stats, double *series) {
  if (!c || !trace || !stats || (n_probs > 0 && !probs)) return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: NULL argument");
  if (n < 4 || C < 1 || d < 1 || d > RSF_MAX_PARAMS || n_probs < 0)
    return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: need n_iters >= 4, n_chains >= 1, 1 <= n_params <= %d, n_probs >= 0", RSF_MAX_PARAMS);
  if (n >= kRankMaxDraws || C >= kRankMaxDraws || n * C >= kRankMaxDraws)
    return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: n_iters * n_chains must be below 2^32");
  if (const int i = first_bad_prob(n_probs, probs); i >= 0) return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: probs[%d] outside [0, 1]", i);
  const int64_t A = n * C;
  if (!(hdi_prob > 0.0 && hdi_prob < 1.0)) return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: hdi_prob outside (0, 1)");
  const double kd = std::floor(hdi_prob * (double)A);  // ArviZ: int(floor(hdi_prob * n))
  if (kd < 1.0 || kd >= (double)A)
    return fail(RSF_ERR_INVALID, "rsf_diag_rank_prepare: the HDI of %g of %lld draws spans %g of them; need 1 <= k < n*C", hdi_prob,
                (long long)A, kd);
  const int64_t khdi = (int64_t)kd;
  RSF_ENTER(c, NEED_NOTHING);
  int rc;
  c->rank_d = 0;
  const double *x;
  if ((rc = stage_in(c, SLOT_X, trace, (size_t)(A * d) * sizeof(double), &x))) return rc;
  RankWs w;
  const size_t bytes = rank_ws_layout(A, d, n_probs, nullptr, &w);
  if ((rc = ensure(c->rankws, bytes))) return rc;
  rank_ws_layout(A, d, n_probs, (char *)c->rankws.p, &w);
  const int ns = RSF_DIAG_RANK_STATS + n_probs;
  HIP_TRY(hipMemsetAsync(w.stats, 0, (size_t)(d * ns) * sizeof(double), c->stream));
  if (n_probs) HIP_TRY(hipMemcpyAsync(w.probs, probs, (size_t)n_probs * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const int64_t N = n / 2, stride = A * d;
  std::vector<char> bad((size_t)d, 0);
  for (int p = 0; p < d; ++p) {
    const RankShape rs{A, (n % 2) ? N * C : 0, (n % 2) ? N * C + C : 0, d, p, 2.0 * (double)C * (double)N};
    double *st = w.stats + (int64_t)p * ns;
    int cur;
    bool nonfinite;
    if ((rc = rank_sort(c, w, A, d, p, x, false, st, &cur, &nonfinite))) return rc;
    if (nonfinite) {  // every output of this parameter is NaN
      bad[(size_t)p] = 1;
      hipLaunchKernelGGL(rank_fill_kernel, dim3((unsigned)rank_grid(A, 4096)), dim3(kRankThreads), 0, c->stream, rs, w.series, stride, (double)NAN);
      HIP_TRY(hipGetLastError());
      continue;
    }
    const uint64_t *sorted = w.keys[cur];
    hipLaunchKernelGGL(rank_order_kernel, dim3(1), dim3(kRankThreads), 0, c->stream, sorted, A, (int)n_probs, (const double *)w.probs, st);
    const int nh = rank_grid(A - khdi, kRankReduceBlocks);
    hipLaunchKernelGGL(rank_hdi_kernel, dim3((unsigned)nh), dim3(kRankThreads), 0, c->stream, sorted, A, khdi, (RankArg *)w.part);
    hipLaunchKernelGGL(rank_hdi_final_kernel, dim3(1), dim3(kRankThreads), 0, c->stream, sorted, A, khdi, nh, (const RankArg *)w.part, st);
    if ((rc = rank_scores(c, w, rs, cur, w.series))) return rc;                        // bulk: z(x)
    if ((rc = rank_sort(c, w, A, d, p, x, true, st, &cur, &nonfinite))) return rc;    // folded: z(|x - median|)
    if ((rc = rank_scores(c, w, rs, cur, w.series + stride))) return rc;
    hipLaunchKernelGGL(rank_indicator_kernel, dim3((unsigned)rank_grid(A, 4096)), dim3(kRankThreads), 0, c->stream, rs, x, (const double *)st,
                       w.series + 2 * stride, w.series + 3 * stride);
    const int nr = rank_grid(A, kRankReduceBlocks);
    for (int q = 0; q < RSF_DIAG_RANK_SERIES; ++q) {
      hipLaunchKernelGGL(rank_range_kernel, dim3((unsigned)nr), dim3(kRankThreads), 0, c->stream, rs, (const double *)(w.series + q * stride),
                         (double *)w.part);
      hipLaunchKernelGGL(rank_range_final_kernel, dim3(1), dim3(64), 0, c->stream, nr, (const double *)w.part, st + kStConst + q);
    }
    HIP_TRY(hipGetLastError());
  }
  std::vector<double> h((size_t)(d * ns));
  HIP_TRY(hipMemcpyAsync(h.data(), w.stats, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (series)
    HIP_TRY(hipMemcpyAsync(series, w.series, (size_t)(4 * stride) * sizeof(double), host_mem(c) ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int p = 0; p < d; ++p) {
    double *o = stats + (int64_t)p * ns;
    for (int f = 0; f < ns; ++f) o[f] = bad[(size_t)p] ? NAN : h[(size_t)(p * ns + f)];
    o[kStNonFinite] = bad[(size_t)p] ? 1.0 : 0.0;
    if (bad[(size_t)p])
      for (int q = 0; q < RSF_DIAG_RANK_SERIES; ++q) o[kStConst + q] = 0.0;
  }
  c->rank_n = n; c->rank_C = C; c->rank_d = d;
  return RSF_OK;
}

int rsf_diag_rank_partials(rsf_ctx *c, int64_t lag_begin, int64_t lag_end, double *partials) {
  if (!c || !partials) return fail(RSF_ERR_INVALID, "rsf_diag_rank_partials: NULL argument");
  if (!c->rank_d || !c->rankws.p) return fail(RSF_ERR_INVALID, "rsf_diag_rank_partials: no prepared trace (call rsf_diag_rank_prepare first)");
  const int64_t n = c->rank_n, C = c->rank_C;
  const int32_t d = c->rank_d;
  LagGrid lg;
  int rc;
  if ((rc = check_lags("rsf_diag_rank_partials", n, C, d, lag_begin, lag_end, &lg))) return rc;
  RSF_ENTER(c, NEED_NOTHING);
  const rsfk::DiagCenter zero{{0.0, 0.0, 0.0}};
  const double *series = (const double *)c->rankws.p;  // the workspace starts with the series
  for (int q = 0; q < RSF_DIAG_RANK_SERIES; ++q) {
    if ((rc = diag_partials_dev(c, n, C, d, series + q * n * C * d, 0, zero, lg, partials + (int64_t)q * d * (RSF_DIAG_HEAD + lg.L)))) return rc;
  }
  return RSF_OK;
}

int rsf_diag_rank_finish(int64_t n, int32_t d, const double *stats, int32_t n_probs, const double *partials, int64_t n_lags, double *out) {
  if (!stats || !partials || !out) return fail(RSF_ERR_INVALID, "rsf_diag_rank_finish: NULL argument");
  if (n < 4 || d < 1 || d > RSF_MAX_PARAMS || n_probs < 0)
    return fail(RSF_ERR_INVALID, "rsf_diag_rank_finish: need n_iters >= 4, 1 <= n_params <= %d, n_probs >= 0", RSF_MAX_PARAMS);
  const int64_t N = n / 2;
  if (n_lags < 2 || n_lags > N) return fail(RSF_ERR_INVALID, "rsf_diag_rank_finish: n_lags %lld outside [2, %lld]", (long long)n_lags, (long long)N);
  const double zero[RSF_MAX_PARAMS] = {0.0, 0.0, 0.0};
  std::vector<double> o((size_t)(RSF_DIAG_RANK_SERIES * d * RSF_DIAG_OUT));
  for (int q = 0; q < RSF_DIAG_RANK_SERIES; ++q) {
    const int rc = rsf_diag_finish(n, d, 0, zero, partials + (int64_t)q * d * (RSF_DIAG_HEAD + n_lags), n_lags, o.data() + q * d * RSF_DIAG_OUT);
    if (rc) return rc;
  }
  const int ns = RSF_DIAG_RANK_STATS + n_probs;
  for (int p = 0; p < d; ++p) {
    const double *st = stats + (int64_t)p * ns;
    double *r = out + (int64_t)p * RSF_DIAG_RANK_OUT;
    double ess[RSF_DIAG_RANK_SERIES], rh[RSF_DIAG_RANK_SERIES];
    bool complete = true;
    for (int q = 0; q < RSF_DIAG_RANK_SERIES; ++q) {
      const double *f = o.data() + (q * d + p) * RSF_DIAG_OUT;
      const double T = partials[((int64_t)q * d + p) * (RSF_DIAG_HEAD + n_lags)] * (double)N;  // M' N
      ess[q] = st[kStConst + q] != 0.0 ? T : f[RSF_DIAG_ESS];  // ArviZ _ess: a constant series has ess = M'N (tau = 1)
      rh[q] = f[RSF_DIAG_SPLIT_RHAT];
      complete = complete && f[RSF_DIAG_LAGS_COMPLETE] != 0.0;
    }
    for (int f = 0; f < RSF_DIAG_RANK_OUT; ++f) r[f] = NAN;
    r[RSF_DIAG_RANK_LAGS_COMPLETE] = complete ? 1.0 : 0.0;
    if (st[kStNonFinite] != 0.0) continue;
    auto nanmax = [](double a, double b) { return std::isnan(a) || std::isnan(b) ? NAN : std::max(a, b); };
    auto nanmin = [](double a, double b) { return std::isnan(a) || std::isnan(b) ? NAN : std::min(a, b); };
    r[RSF_DIAG_RANK_RHAT_BULK] = rh[0];
    r[RSF_DIAG_RANK_RHAT_TAIL] = rh[1];
    r[RSF_DIAG_RANK_RHAT] = nanmax(rh[0], rh[1]);
    r[RSF_DIAG_RANK_ESS_BULK] = ess[0];
    r[RSF_DIAG_RANK_ESS_Q05] = ess[2];
    r[RSF_DIAG_RANK_ESS_Q95] = ess[3];
    r[RSF_DIAG_RANK_ESS_TAIL] = nanmin(ess[2], ess[3]);
  }
  return RSF_OK;
}

int rsf_diag_rank_release(rsf_ctx *c) {
  RSF_ENTER(c, NEED_NOTHING, true, "NULL argument");
  if (c->rankws.p) HIP_TRY(hipStreamSynchronize(c->stream));
  release(c->rankws);
  c->rank_d = 0;
  return RSF_OK;
}

// ---- posterior predictive checks (include/rsf_predict.h) -----------------------------------------
int rsf_predict_partials(rsf_ctx *c, int64_t n, int32_t d, const double *q, const double *std2, const double *data,
                         const double *center_y, const double *center_l, double *partials, double *series_out) {
  RSF_ENTER(c, NEED_MODEL, q && std2 && data && center_y && center_l && partials, "NULL argument");
  if (n < 1 || (d != 1 && d != 3)) return fail(RSF_ERR_INVALID, "rsf_predict_partials: need n >= 1 and d = 1 or 3");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_predict_partials: a model flagged RSF_FLAG_DOP853 is not supported (the predictive solve is the float64 RK4)");
  const int64_t nout = c->nout;
  const int S = c->m.substeps, wpb = c->block / 64;
  const int64_t grid = (n + c->block - 1) / c->block, nwaves = grid * wpb, nslabs = (nwaves + kPredSlab - 1) / kPredSlab;
  const int64_t nf = nout * kPredFields;
  if (nslabs > 65535 || n > INT64_MAX / 64 / nout) return fail(RSF_ERR_INVALID, "rsf_predict_partials: too many draws for one call; split the pool into shards");
  // the kernel's own chunking of the loading table: its waves' tiles share LDS with the chunk (rsf_predict.h, kPredTableBudget)
  const int64_t kc = std::min<int64_t>(((int64_t)(kPredTableBudget / sizeof(double)) - 1) / (2 * (int64_t)S), nout - 1);
  if (kc < 1) return fail(RSF_ERR_UNSUPPORTED, "rsf_predict_partials: substeps=%d does not fit the LDS staging budget", S);
  int rc;
  const size_t nb = (size_t)n * sizeof(double), rowb = (size_t)nout * sizeof(double);
  const double *dq, *dstd2, *ddata;
  double *dser = nullptr;
  // (the largest allocation first: it fails before anything is copied)
  if (series_out && stage_out(c, SLOT_SERIES, series_out, nb * (size_t)nout, &dser)) return series_nomem(__func__, n, nout, "; pass fewer draws per call");
  if ((rc = stage_in(c, SLOT_Q, q, nb * d, &dq))) return rc;
  if ((rc = stage_in(c, SLOT_STD2, std2, nb, &dstd2))) return rc;
  if ((rc = stage_in(c, SLOT_OBS, data, rowb, &ddata))) return rc;
  // workspace, doubles: per-wave partials[nwaves][nf] | slab sums[nslabs][nf] | sums[nf] | center_y[nout] | center_l[nout]
  const int64_t o_slab = nwaves * nf, o_sum = o_slab + nslabs * nf, o_cy = o_sum + nf, o_cl = o_cy + nout, total = o_cl + nout;
  if ((rc = ensure(c->predict, (size_t)total * sizeof(double)))) return rc;
  double *w = (double *)c->predict.p;
  HIP_TRY(hipMemcpyAsync(w + o_cy, center_y, rowb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(w + o_cl, center_l, rowb, hipMemcpyHostToDevice, c->stream));
  Consts K = make_consts(c, nullptr);
  K.kc = (int32_t)kc;
  K.nchunks = (int32_t)((nout - 1 + kc - 1) / kc);
  PredictArgs A{};
  A.n = n; A.q = dq; A.std2 = dstd2; A.data = ddata; A.cy = w + o_cy; A.cl = w + o_cl; A.part = w; A.series = dser;
  A.tab_doubles = (int32_t)((2 * S * kc + 1 + 1) & ~(int64_t)1);
  const size_t lds = ((size_t)A.tab_doubles + (size_t)wpb * kPredWaveDoubles) * sizeof(double);
  if ((rc = launch(c, predict_fn(c, d, dser != nullptr), (unsigned)grid, c->block, lds, K, A))) return rc;
  const unsigned fb = (unsigned)((nf + 255) / 256);
  hipLaunchKernelGGL(predict_sum_kernel, dim3(fb, (unsigned)nslabs), dim3(256), 0, c->stream, nwaves, (int64_t)kPredSlab, nf, (const double *)w, w + o_slab);
  hipLaunchKernelGGL(predict_sum_kernel, dim3(fb, 1), dim3(256), 0, c->stream, nslabs, nslabs, nf, (const double *)(w + o_slab), w + o_sum);
  HIP_TRY(hipGetLastError());
  std::vector<double> h((size_t)nf);
  HIP_TRY(hipMemcpyAsync(h.data(), w + o_sum, (size_t)nf * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if ((rc = copy_back(c, SLOT_SERIES, series_out, nb * (size_t)nout))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  partials[0] = (double)n;
  partials[1] = h[kPredFields - 1];  // sum of sigma^2: the same in every row, taken from row 0
  for (int64_t k = 0; k < nout; ++k)
    for (int f = 0; f < RSF_PREDICT_FIELDS; ++f) partials[RSF_PREDICT_HEAD + k * RSF_PREDICT_FIELDS + f] = h[(size_t)(k * kPredFields + f)];
  return RSF_OK;
}

int rsf_predict_finish(int64_t n_rows, const double *partials, const double *center_y, const double *center_l, double *out_rows,
                       double *out_totals) {
  if (!partials || !center_y || !center_l || !out_rows || !out_totals) return fail(RSF_ERR_INVALID, "rsf_predict_finish: NULL argument");
  if (n_rows < 1) return fail(RSF_ERR_INVALID, "rsf_predict_finish: n_rows < 1");
  const double n = partials[0];
  double elpd = 0.0, pw = 0.0;
  for (int64_t k = 0; k < n_rows; ++k) {
    const double *p = partials + RSF_PREDICT_HEAD + k * RSF_PREDICT_FIELDS;
    double *o = out_rows + k * RSF_PREDICT_OUT;
    bool finite = p[RSF_PREDICT_NONFINITE] == 0.0 && std::isfinite(center_y[k]) && std::isfinite(center_l[k]);
    for (int f = 0; f < RSF_PREDICT_NONFINITE; ++f) finite = finite && std::isfinite(p[f]);
    if (!finite) {  // a non-finite draw: every statistic of this output time is NaN
      for (int f = 0; f < RSF_PREDICT_OUT; ++f) o[f] = NAN;
    } else {
      const double my = p[RSF_PREDICT_SUM_Y] / n, ml = p[RSF_PREDICT_SUM_L] / n;
      o[RSF_PREDICT_MEAN] = center_y[k] + my;
      o[RSF_PREDICT_VAR] = (p[RSF_PREDICT_SUM_Y2] - p[RSF_PREDICT_SUM_Y] * my) / (n - 1.0);
      o[RSF_PREDICT_PIT] = p[RSF_PREDICT_SUM_PHI] / n;
      o[RSF_PREDICT_LPD] = center_l[k] + std::log(p[RSF_PREDICT_SUM_EXP] / n);
      o[RSF_PREDICT_P_WAIC] = (p[RSF_PREDICT_SUM_L2] - p[RSF_PREDICT_SUM_L] * ml) / (n - 1.0);
    }
    elpd += o[RSF_PREDICT_LPD] - o[RSF_PREDICT_P_WAIC];
    pw += o[RSF_PREDICT_P_WAIC];
  }
  const double nr = (double)n_rows, me = elpd / nr;
  double ss = 0.0;
  for (int64_t k = 0; k < n_rows; ++k) {
    const double e = out_rows[k * RSF_PREDICT_OUT + RSF_PREDICT_LPD] - out_rows[k * RSF_PREDICT_OUT + RSF_PREDICT_P_WAIC] - me;
    ss += e * e;
  }
  out_totals[RSF_PREDICT_MEAN_STD2] = partials[1] / n;
  out_totals[RSF_PREDICT_ELPD_WAIC] = elpd;
  out_totals[RSF_PREDICT_P_WAIC_TOTAL] = pw;
  out_totals[RSF_PREDICT_ELPD_WAIC_SE] = std::sqrt(nr * (ss / (nr - 1.0)));
  return RSF_OK;
}

int rsf_predict_quantiles(rsf_ctx *c, int64_t n, int64_t nout, const double *series, int32_t n_probs, const double *probs, double *out) {
  RSF_ENTER(c, NEED_NOTHING, series && probs && out, "NULL argument");
  int rc;
  if ((rc = check_series_shape(__func__, n, nout))) return rc;
  if (n_probs < 1 || n_probs > RSF_PREDICT_MAX_PROBS)
    return fail(RSF_ERR_INVALID, "rsf_predict_quantiles: n_probs outside 1..%d", RSF_PREDICT_MAX_PROBS);
  if (const int i = first_bad_prob(n_probs, probs); i >= 0) return fail(RSF_ERR_INVALID, "rsf_predict_quantiles: probs[%d] is outside [0, 1]", i);
  PredictProbs P{};
  std::copy(probs, probs + n_probs, P.p);
  const double *ds;
  if ((rc = stage_series(c, __func__, SLOT_X, series, n, nout, &ds))) return rc;
  const size_t ob = (size_t)n_probs * (size_t)nout * sizeof(double);
  if ((rc = ensure(c->poolws, ob))) return rc;
  hipLaunchKernelGGL(predict_select_kernel, dim3((unsigned)nout), dim3(kPredSelectThreads), 0, c->stream, n, nout, ds, (int)n_probs, P, (double *)c->poolws.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, c->poolws.p, ob, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RSF_OK;
}

int rsf_predict_psis_loo(rsf_ctx *c, int64_t n, int64_t nout, const double *series, const double *std2, const double *data, double r_eff,
                         double *out_rows) {
  RSF_ENTER(c, NEED_NOTHING, series && std2 && data && out_rows, "NULL argument");
  int rc;
  if ((rc = check_series_shape(__func__, n, nout))) return rc;
  if (!(std::isfinite(r_eff) && r_eff > 0.0)) return fail(RSF_ERR_INVALID, "rsf_predict_psis_loo: r_eff must be finite and > 0");
  const double tl = std::ceil(std::min(0.2 * (double)n, 3.0 * std::sqrt((double)n / r_eff)));
  if (tl > (double)RSF_PSIS_MAX_TAIL)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_predict_psis_loo: a tail of %.0f draws exceeds RSF_PSIS_MAX_TAIL = %d (n = %lld, r_eff = %g)", tl,
                RSF_PSIS_MAX_TAIL, (long long)n, r_eff);
  static_assert(kPsisMaxTail == RSF_PSIS_MAX_TAIL && kPsisOut == RSF_PSIS_OUT, "csrc/rsf_psis.h and include/rsf_psis.h agree");
  const size_t nb = (size_t)n * sizeof(double), rowb = (size_t)nout * sizeof(double);
  const double *ds, *dstd2, *ddata;
  // (the largest allocation first: it fails before anything is copied)
  if ((rc = stage_series(c, __func__, SLOT_SERIES, series, n, nout, &ds))) return rc;
  if ((rc = stage_in(c, SLOT_STD2, std2, nb, &dstd2))) return rc;
  if ((rc = stage_in(c, SLOT_OBS, data, rowb, &ddata))) return rc;
  // workspace: the draws' constants [2][n] in c->predict, the rows [nout][RSF_PSIS_OUT] in c->poolws
  const size_t ob = (size_t)nout * RSF_PSIS_OUT * sizeof(double);
  if ((rc = ensure(c->predict, 2 * nb))) return rc;
  if ((rc = ensure(c->poolws, ob))) return rc;
  PsisArgs A{};
  A.n = n; A.nout = nout; A.series = ds; A.par = (const double *)c->predict.p; A.data = ddata; A.out = (double *)c->poolws.p;
  A.tail_len = (int32_t)tl;
  A.cap = 8;
  while (A.cap < A.tail_len) A.cap <<= 1;
  const size_t lds = 2 * (size_t)A.cap * sizeof(double);
  if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)psis_row_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if ((rc = launch(c, psis_params_kernel, (unsigned)((n + 255) / 256), 256, 0, n, dstd2, (double *)c->predict.p))) return rc;
  if ((rc = launch(c, psis_row_kernel, (unsigned)nout, kPsisThreads, lds, A))) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_rows, c->poolws.p, ob, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RSF_OK;
}

int rsf_predict_psis_finish(int64_t nout, int64_t n, const double *psis_rows, const double *lpd_rows, double *out_totals) {
  if (!psis_rows || !lpd_rows || !out_totals) return fail(RSF_ERR_INVALID, "rsf_predict_psis_finish: NULL argument");
  if (nout < 1 || n < 1) return fail(RSF_ERR_INVALID, "rsf_predict_psis_finish: nout < 1 or n < 1");
  const double thr = n > 1 ? std::min(1.0 - 1.0 / std::log10((double)n), 0.7) : -INFINITY;
  double elpd = 0.0, p = 0.0, kmax = -INFINITY, high = 0.0;
  bool ok = true;
  for (int64_t k = 0; k < nout; ++k) {
    const double e = psis_rows[k * RSF_PSIS_OUT + RSF_PSIS_ELPD], pk = psis_rows[k * RSF_PSIS_OUT + RSF_PSIS_PARETO_K];
    ok = ok && std::isfinite(e) && !std::isnan(pk) && std::isfinite(lpd_rows[k]);
    elpd += e;
    p += lpd_rows[k] - e;
    kmax = std::max(kmax, pk);
    high += pk > thr ? 1.0 : 0.0;
  }
  const double nr = (double)nout, me = elpd / nr;
  double ss = 0.0;
  for (int64_t k = 0; k < nout; ++k) {
    const double e = psis_rows[k * RSF_PSIS_OUT + RSF_PSIS_ELPD] - me;
    ss += e * e;
  }
  out_totals[RSF_PSIS_ELPD_LOO] = ok ? elpd : NAN;
  out_totals[RSF_PSIS_P_LOO] = ok ? p : NAN;
  out_totals[RSF_PSIS_ELPD_LOO_SE] = ok ? std::sqrt(nr * (ss / (nr - 1.0))) : NAN;
  out_totals[RSF_PSIS_K_THRESHOLD] = thr;
  out_totals[RSF_PSIS_N_HIGH_K] = ok ? high : NAN;
  out_totals[RSF_PSIS_MAX_PARETO_K] = ok ? kmax : NAN;
  return RSF_OK;
}

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

int rsf_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  if (!ctr || !key || !out) return fail(RSF_ERR_INVALID, "rsf_philox4x32_10: NULL argument");
  uint32_t *d = nullptr;
  HIP_TRY(hipMalloc(&d, 4 * sizeof(uint32_t)));
  hipLaunchKernelGGL(probe_philox_kernel, dim3(1), dim3(64), 0, nullptr, ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], d);
  hipError_t e = hipMemcpy(out, d, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(RSF_ERR_DEVICE, "rsf_philox4x32_10: %s", hipGetErrorString(e));
  return RSF_OK;
}

int rsf_mcmc_draws(uint64_t seed, int64_t chain, int64_t iteration, int32_t d, double shape, double *z, double *u,
                   double *g) {
  if (d < 1 || d > 3) return fail(RSF_ERR_INVALID, "rsf_mcmc_draws: n_params out of range");
  double *dev = nullptr, h[5];
  HIP_TRY(hipMalloc(&dev, sizeof h));
  hipLaunchKernelGGL(probe_draws_kernel, dim3(1), dim3(64), 0, nullptr, seed, (uint64_t)chain, (uint32_t)iteration, d, shape, dev);
  hipError_t e = hipMemcpy(h, dev, sizeof h, hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  if (e != hipSuccess) return fail(RSF_ERR_DEVICE, "rsf_mcmc_draws: %s", hipGetErrorString(e));
  if (z) for (int p = 0; p < d; ++p) z[p] = h[p];
  if (u) *u = h[3];
  if (g) *g = h[4];
  return RSF_OK;
}

int rsf_mcmc_adapt(int32_t d, int32_t n, const double *window, int32_t adapt_mode, int32_t prior_len, double *V_out) {
  if ((d != 1 && d != 3) || n < 1 || !window || !V_out || (adapt_mode != RSF_ADAPT_REFERENCE_DICT && adapt_mode != RSF_ADAPT_AM))
    return fail(RSF_ERR_INVALID, "rsf_mcmc_adapt: bad argument");
  if (adapt_mode == RSF_ADAPT_REFERENCE_DICT && d != 1)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_mcmc_adapt: reference_dict adaptation is defined for 1 parameter only");
  if (adapt_mode == RSF_ADAPT_REFERENCE_DICT && n > RSF_DICT_MAX_INTERVAL)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_mcmc_adapt: reference_dict windows hold at most %d samples", RSF_DICT_MAX_INTERVAL);
  double *dev = nullptr, h[10];
  const size_t wb = (size_t)n * d * sizeof(double);
  HIP_TRY(hipMalloc(&dev, wb + sizeof h));
  hipError_t e = hipMemcpy(dev + 10, window, wb, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(probe_adapt_kernel, dim3(1), dim3(64), 0, nullptr, (int)d, (int)n, (const double *)(dev + 10), (int)adapt_mode,
                       2.38 * 2.38 / (double)(prior_len > 0 ? prior_len : 2), dev);
    e = hipMemcpy(h, dev, sizeof h, hipMemcpyDeviceToHost);
  }
  (void)hipFree(dev);
  if (e != hipSuccess) return fail(RSF_ERR_DEVICE, "rsf_mcmc_adapt: %s", hipGetErrorString(e));
  if (h[d * d] == 0.0) return fail(RSF_ERR_NOT_POSDEF, "rsf_mcmc_adapt: the window's covariance is not positive definite");
  for (int i = 0; i < d * d; ++i) V_out[i] = h[i];
  return RSF_OK;
}

}  // extern "C"
