// rsf_host.h — what the units of librsf_hip.so share on the host side (internal: not installed, not under include/): the error
// buffer, device buffers and the device guard, the ctx, staging of RSF_MEM_HOST callers, the entry check, the kernel constants
// and the kernel dispatch.  Templates are defined here; everything else is declared here and defined once, in rsf_hip.hip
// unless a comment names another unit.  Units call each other through these declarations, never through an included kernel:
// this header includes no header that defines a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstddef>
#include <type_traits>

#include "../../include/rsf_abi.h"
#include "rsf_kernel_common.h"

typedef struct ncclComm *ncclComm_t;  // as <rccl/rccl.h> has it: only rsf_comm.hip includes that header

#pragma GCC visibility push(hidden)  // nothing below is part of the library's dynamic symbol table

namespace rsfh {

using rsf::Consts;

extern thread_local char g_err[512];  // rsf_last_error()
int fail(int code, const char *fmt, ...);  // formats g_err and returns code

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(RSF_ERR_DEVICE, "%s -> %s", #expr, hipGetErrorString(e_)); \
  } while (0)

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
  // rsf_kstiff_observe: rsf_forward_batch's slots, and the stiffness of each point
  SLOT_STIFFNESS = SLOT_SSQ_NEW,
  // rsf_mcmc_init (q0 in SLOT_Q), rsf_mcmc_get_state / _set_state / _init_state
  SLOT_Q = SLOT_Z, SLOT_V = SLOT_U,
  // rsf_pool_summary / _kde / _histogram, rsf_diag_partials, rsf_diag_rank_prepare: the samples or the trace in SLOT_X
  SLOT_X = SLOT_Z, SLOT_GRID = SLOT_U, SLOT_POOL_OUT = SLOT_G,
  // rsf_predict_partials (std2 in SLOT_U), rsf_predict_quantiles (the series in SLOT_X)
  // rsf_predict_psis_loo: the series in SLOT_SERIES, std2 in SLOT_STD2, the observation in SLOT_OBS
  SLOT_STD2 = SLOT_U, SLOT_OBS = SLOT_G, SLOT_SERIES = SLOT_TQ,
  // rsf_evidence_propose (theta, logg, inbox out), rsf_evidence_logg (theta in, logg out), rsf_evidence_logtarget (theta, the
  // observation and logg in, l out), rsf_evidence_partials (l1 in SLOT_EV_L, l2 in SLOT_EV_L2)
  SLOT_EV_THETA = SLOT_Z, SLOT_EV_LOGG = SLOT_U, SLOT_EV_OBS = SLOT_G, SLOT_EV_L = SLOT_TQ, SLOT_EV_L2 = SLOT_TS, SLOT_EV_INBOX = SLOT_TA,
  // rsf_smc_init (q out), rsf_smc_weight_sums (l), rsf_smc_resample (q, l in; cum, anc, q_out, l_out out), rsf_smc_move (q, l in
  // and out, the observation), rsf_smc_move_propose (q in; q_new in SLOT_SMC_Q_OUT, inbox out), rsf_smc_move_accept (q, l in and
  // out; q_new, inbox, ssq_new in), rsf_smc_std2 (l in, std2 in SLOT_SMC_L_OUT)
  SLOT_SMC_Q = SLOT_Z, SLOT_SMC_L = SLOT_U, SLOT_SMC_OBS = SLOT_G, SLOT_SMC_CUM = SLOT_G, SLOT_SMC_ANC = SLOT_TQ, SLOT_SMC_INBOX = SLOT_TQ,
  SLOT_SMC_Q_OUT = SLOT_TS, SLOT_SMC_L_OUT = SLOT_TA, SLOT_SMC_SSQ = SLOT_SSQ_NEW,
  // rsf_grid_logtarget (the observation in; l, ssq out), rsf_grid_columns (l, ssq in; fields, m0, cum0 out), rsf_grid_draw (cum0 in;
  // q, cell out), rsf_grid_cdf (cum0 in).  The axes and the other HOST tables of a grid call lie in the ctx's poolws workspace
  SLOT_GRID_L = SLOT_TQ, SLOT_GRID_SSQ = SLOT_TS, SLOT_GRID_OBS = SLOT_G, SLOT_GRID_FIELDS = SLOT_Z, SLOT_GRID_M0 = SLOT_U, SLOT_GRID_CUM0 = SLOT_TA,
  SLOT_GRID_Q = SLOT_Z, SLOT_GRID_CELL = SLOT_U,
  // rsf_pool_allgather[_all] / _allreduce_sum[_all] (the reduction is in place in SLOT_SEND)
  SLOT_SEND = SLOT_Z, SLOT_RECV = SLOT_U,
};

}  // namespace rsfh

struct rsf_ctx {
  rsf_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  int block = rsfk::kMaxBlock;
  // model
  bool have_model = false;
  rsf_model m{};
  int32_t nout = 0;
  double delta_t = 0, h = 0;
  int32_t kc = 0, nchunks = 0;
  int32_t kc32 = 0, nchunks32 = 0;  // the float32 SAMPLER's own chunking: its tables are floats, twice as many fit the budget
  size_t lds_bytes = 0;
  rsfh::DevBuf vl;
  double vl_lo = 0, vl_hi = 0;  // smallest and largest value of the table in vl (rsfh::set_loading_range): Consts::vl_lo / vl_hi
  // chains
  bool have_chains = false;
  bool external_chains = false;  // made by rsf_mcmc_init_state: no observation, advanced by rsf_mcmc_replay_ssq only
  rsf_mcmc_config mc{};
  rsfh::DevBuf data, q, ssq, std2, V, wref, wsum, wsq, wn, wbuf, stats;
  int64_t group_chains = 0;  // chains per observation group (0: one series)
  int64_t iters_done = 0;
  // staging for RSF_MEM_HOST callers
  rsfh::DevBuf stage[rsfh::SLOT_COUNT];
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
  rsfh::DevBuf pool;    // workspace of the posterior post-processing kernels: the moments' partials
  rsfh::DevBuf poolws;  // ... and the KDE's per-workgroup densities or the histogram's integer counts
  rsfh::DevBuf diag;  // workspace of the convergence diagnostics (rsf_diag_partials)
  rsfh::DevBuf rankws;  // rank workspace (rsf_diag_rank_prepare): the four derived series, then the sort buffers
  int64_t rank_n = 0, rank_C = 0;  // shape of the prepared trace; rank_d 0 = nothing prepared
  int32_t rank_d = 0;
  rsfh::DevBuf predict;  // workspace of the posterior predictive checks (rsf_predict_*): per-wave partials and their sums; quantiles
};

namespace rsfh {

int ensure(DevBuf &b, size_t bytes);
void release(DevBuf &b);
bool host_mem(const rsf_ctx *c);

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

int copy_back(rsf_ctx *c, Slot slot, void *dst, size_t bytes);
int finish(rsf_ctx *c);  // host callers get synchronous semantics

// one thread per element in workgroups of kMaxBlock
inline unsigned blocks_of(int64_t n) { return (unsigned)((n + rsfk::kMaxBlock - 1) / rsfk::kMaxBlock); }

// The arrays of one call for an RSF_MEM_HOST caller of rsf_fit.hip and rsf_mala.hip.  Their calls take more arrays than the ctx
// has named staging slots (Slot above), so they stage all of them in ONE workspace, the ctx's pool buffer: add() every array,
// commit() sizes the workspace and copies the inputs in, dev() is the pointer the kernels take, back() copies the outputs out.  A
// device caller's pointers pass through.
struct Staged {
  struct Item { void *host; size_t bytes, off; bool in, out; };
  rsf_ctx *c;
  Item items[16];
  int count = 0;
  size_t total = 0;
  explicit Staged(rsf_ctx *ctx) : c(ctx) {}
  int add(const void *p, size_t bytes, bool in, bool out) {
    items[count] = {const_cast<void *>(p), bytes, total, in, out};
    total += (bytes + 255) & ~(size_t)255;
    return count++;
  }
  int commit() {
    if (!host_mem(c)) return RSF_OK;
    if (int rc = ensure(c->pool, total)) return rc;
    for (int k = 0; k < count; ++k)
      if (items[k].in) HIP_TRY(hipMemcpyAsync((char *)c->pool.p + items[k].off, items[k].host, items[k].bytes, hipMemcpyHostToDevice, c->stream));
    return RSF_OK;
  }
  template <class T> T *dev(int k) const { return host_mem(c) ? (T *)((char *)c->pool.p + items[k].off) : (T *)items[k].host; }
  int back() {
    if (!host_mem(c)) return RSF_OK;
    for (int k = 0; k < count; ++k)
      if (items[k].out) HIP_TRY(hipMemcpyAsync(items[k].host, (char *)c->pool.p + items[k].off, items[k].bytes, hipMemcpyDeviceToHost, c->stream));
    return RSF_OK;
  }
};

// What an entry point that touches the device begins with: its arguments (a NULL ctx, and whatever else the caller folds
// into args_ok and names in `what`), the state it needs, and the ctx's device selected for as long as the caller's guard
// lives.  fn: the entry point the messages name.
enum Need { NEED_NOTHING, NEED_MODEL, NEED_CHAINS, NEED_COMM };

int enter(DeviceGuard &guard, rsf_ctx *c, const char *fn, Need need, bool args_ok = true, const char *what = "NULL ctx");

// ... as the first statement of the entry point itself, which it names; `guard` lives to the end of the enclosing block
#define RSF_ENTER(c, ...)                                            \
  DeviceGuard guard;                                                 \
  if (int rc_ = enter(guard, c, __func__, __VA_ARGS__)) return rc_

Consts make_consts(const rsf_ctx *c, const double *data, int64_t group_chains = 0);
unsigned grid_for(const rsf_ctx *c, int64_t n);
int mode_of(const rsf_ctx *c);  // rsfk::Mode
// radiation damping in a kernel of integrator `mode`.  The float64 RK4 kernels carry W = kvk v / V_ref = k1 v / a in place of
// v / V_ref with damping on (rsf_device.h, Lane::vrw), which needs k1 != 0; with k1 = 0 the damping pass is an exact identity
// and they run without it.
bool damped(const rsf_ctx *c, int mode);
// chains a lane of the sampler kernel carries: two in the float32 mode (mcmc_f32x2_kernel), else one
int chains_per_lane(const rsf_ctx *c);
// the first probability outside [0, 1] (NaN included), or -1
int first_bad_prob(int n, const double *probs);
// the chains' state goes with the model, or the loading history (rsf_law.hip), they were made under
void free_chains(rsf_ctx *c);
// the built-in loading history V_ref (1 + exp(-t / 20) sin 10 t) at t_start + j hh, j = 0 .. n - 1 (rsf_set_model's RK4 table)
void builtin_loading(const rsf_model &m, double hh, double *vl, size_t n);
// the range of the table about to become c->vl — whoever writes that table calls this with the host copy (rsf_set_model,
// rsf_set_loading): the float64 sampler's a-priori bound on a TIGHT trip's increments rests on it (rsf_device.h, tight_needs_guard)
void set_loading_range(rsf_ctx *c, const double *vl, size_t n);
// what rsf_destroy frees of the other units' state: the replay graph (rsf_sampler.hip), the communicator (rsf_comm.hip)
void release_replay_graph(rsf_ctx *c);
void release_comm(rsf_ctx *c);
// the grid of an rsf_grid_* call (rsf_finish.cpp): d in [dmin, 3], n[p] >= 2, N = prod n[p] < 2^31, the nodes x finite and strictly
// increasing per axis, the weights w (NULL: not checked) finite and > 0 → *N; fn: the entry point the messages name
int grid_check(const char *fn, int d, int dmin, const int32_t *n, const double *x, const double *w, int64_t *N);

// ---- kernel selection -----------------------------------------------------------------------------------------------
// A runtime selector becomes a template argument: with<V0, V1, ...>(v, f) hands f the one of the listed values that equals
// v (the last if none does) as a std::integral_constant.  Every *_fn of the units returns the TYPED pointer of one instantiation
// (the same address on every call: the replay graph compares it), and asks damped() itself with the integrator its kernel
// runs.  Only combinations that are launched are named: naming one instantiates it.
template <auto V0, auto... Vs, class F> auto with(int v, F f) {
  if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<decltype(V0), V0>{});
  else return v == (int)V0 ? f(std::integral_constant<decltype(V0), V0>{}) : with<Vs...>(v, f);
}

// One launch on the ctx stream: EVERY launch of a kernel on it, and its return code is the launch's check.  The parameter types
// come from the kernel's pointer alone, and the call's arguments are converted to them before their addresses are taken: a
// wrong count, order or type does not compile.  grid: a plain count converts to dim3.
template <class T> struct as_declared { using type = T; };

template <class... P>
int launch(rsf_ctx *c, void (*fn)(P...), dim3 grid, unsigned block, size_t lds, typename as_declared<P>::type... a) {
  void *args[] = {(void *)&a...};
  HIP_TRY(hipLaunchKernel((const void *)fn, grid, dim3(block), args, lds, c->stream));
  return RSF_OK;
}

// ---- the last step of a reduction (rsf_pool.hip; kernels: rsf_kernels_pool.h) -----------------------------------------
// The workgroups' partials part[b][nf] of any unit, device pointers, summed on the ctx stream.  Each is named by the order of
// its additions, which is its contract: the results' bits depend on it.
// In index order: out[s][f] = scale * (0.0 + part[s per][f] + part[s per + 1][f] + ...), slab s of `per` partials, the last slab
// up to nblocks; ceil(nblocks / per) slabs.  One thread per field in grid_x workgroups of 256 (0: as many as cover nf).
int sum_in_order(rsf_ctx *c, int64_t nblocks, int64_t per, int64_t nf, const double *part, double scale, double *out, unsigned grid_x = 0);
// Strided, then a tree: out[f] from one workgroup of 256 per field; thread t adds part[t][f], part[t + 256][f], ... in that order
// from 0.0, then the descending shuffle tree of each wave (wave_sum), then the four waves in index order.
int sum_strided_tree(rsf_ctx *c, int nblocks, int nf, const double *part, double *out);

}  // namespace rsfh

#pragma GCC visibility pop
