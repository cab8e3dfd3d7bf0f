// rsf_hip.hip — gfx950 (MI355X / CDNA4) implementation of include/rsf_abi.h, the core unit: the definitions of the host
// plumbing that rsf_host.h declares, the ctx, the model, the forward batch, the chains' state and the probe entry points, with
// their kernels (rsf_kernels_core.h; device building blocks: rsf_device*.h, rsf_math.h).  The other kernel families have units
// of their own: rsf_sampler.hip, rsf_pool.hip, rsf_diag.hip, rsf_predict.hip; rsf_comm.hip and rsf_finish.cpp have no kernel.
//
// There is no host fallback in this library: every entry point either runs on the GPU or fails.

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <vector>

#include "../../include/rsf_abi.h"
#include "rsf_host.h"
#include "rsf_kernels_core.h"

using namespace rsfk;
using namespace rsfh;

namespace rsfh {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------

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

int enter(DeviceGuard &guard, rsf_ctx *c, const char *fn, Need need, bool args_ok, const char *what) {
  static const char *const first[] = {nullptr, "rsf_set_model", "rsf_mcmc_init", "rsf_comm_init"};
  if (!c || !args_ok) return fail(RSF_ERR_INVALID, "%s: %s", fn, what);
  const bool have[] = {true, c->have_model, c->have_chains, c->world != 0};
  if (!have[need]) return fail(RSF_ERR_STATE, "%s: call %s first", fn, first[need]);
  if (!guard.select(c->device)) return fail(RSF_ERR_DEVICE, "%s: cannot select device %d", fn, c->device);
  return RSF_OK;
}

Consts make_consts(const rsf_ctx *c, const double *data, int64_t group_chains) {
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
  K.vl_lo = c->vl_lo; K.vl_hi = c->vl_hi;
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

int first_bad_prob(int n, const double *probs) {
  for (int i = 0; i < n; ++i)
    if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) return i;
  return -1;
}

void free_chains(rsf_ctx *c) {
  release(c->data); release(c->q); release(c->ssq); release(c->std2); release(c->V);
  release(c->wref); release(c->wsum); release(c->wsq); release(c->wn); release(c->wbuf); release(c->stats);
  c->have_chains = false;
  c->external_chains = false;
}

// chain-independent loading velocity at every RK4 stage time, RateStateModel.py:327-329
void builtin_loading(const rsf_model &m, double hh, double *vl, size_t n) {
  for (size_t j = 0; j < n; ++j) {
    const double t = m.t_start + (double)j * hh;
    vl[j] = m.V_ref * (1 + std::exp(-t / 20) * std::sin(10 * t));
  }
}

void set_loading_range(rsf_ctx *c, const double *vl, size_t n) {
  double lo = vl[0], hi = vl[0];
  for (size_t j = 1; j < n; ++j) {
    lo = vl[j] < lo ? vl[j] : lo;
    hi = vl[j] > hi ? vl[j] : hi;
  }
  c->vl_lo = lo;
  c->vl_hi = hi;
}

}  // namespace rsfh

namespace {

using ForwardFn = void (*)(Consts, int64_t, const double *, const double *, const double *, double *, double *);

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

auto propose_fn(int d) { return with<1, 3>(d, [](auto D) { return propose_kernel<D>; }); }  // void (*)(ProposeArgs)
// [n][d] (the C ABI's layout) <-> [d][n] (the kernels' structure of arrays); both device pointers, on the ctx stream
int transpose(rsf_ctx *c, int64_t n, int d, const double *src, double *dst, bool to_soa) {
  if (d == 1) {
    if (src != dst) HIP_TRY(hipMemcpyAsync(dst, src, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return RSF_OK;
  }
  return launch(c, transpose_kernel, (unsigned)((n + kMaxBlock - 1) / kMaxBlock), kMaxBlock, 0, n, d, src, dst, to_soa);
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
    release_comm(c);
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
    vl.resize(2 * (size_t)S * (size_t)(nout - 1) + 1);
    builtin_loading(*m, hh, vl.data(), vl.size());
  }
  const size_t nvl = vl.size();
  if ((rc = ensure(c->vl, nvl * sizeof(double)))) return rc;
  HIP_TRY(hipMemcpyAsync(c->vl.p, vl.data(), nvl * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // vl (host vector) goes out of scope
  set_loading_range(c, vl.data(), nvl);
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
// chain-state arrays (structure of arrays, rsf_kernel_common.h) with the adaptation window and counters, and a fresh window about
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
  // both kernels take the shared chunking (c->kc, c->lds_bytes): only the float32 SAMPLER has its own (rsf_kernel_common.h, kLdsBudget)
  const Consts K = make_consts(c, (const double *)c->data.p, c->group_chains);
  // the init kernels run one lane per TRAJECTORY: 1 + d adjacent lanes per chain (rsf_kernels_core.h, InitGroup)
  if ((rc = launch(c, init_fn(c, d), grid_for(c, C * (d + 1)), c->block, c->lds_bytes, K, A))) return rc;
  if (mode_of(c) == RK4_F32 && (rc = launch(c, ssq32_fn(c, d), grid_for(c, C), c->block, c->lds_bytes, K, C, A.q0, A.ssq))) return rc;
  c->mc = *cfg;
  c->iters_done = 0;
  c->have_chains = true;
  c->external_chains = false;
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

int rsf_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  if (!ctr || !key || !out) return fail(RSF_ERR_INVALID, "rsf_philox4x32_10: NULL argument");
  uint32_t *d = nullptr;
  HIP_TRY(hipMalloc(&d, 4 * sizeof(uint32_t)));
  // no ctx: the null stream, so not rsfh::launch; the copy that follows reports a failure
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
  // no ctx: the null stream, so not rsfh::launch; the copy that follows reports a failure
  hipLaunchKernelGGL(probe_draws_kernel, dim3(1), dim3(64), 0, nullptr, seed, (uint64_t)chain, (uint32_t)iteration, d, shape, dev);
  hipError_t e = hipMemcpy(h, dev, sizeof h, hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  if (e != hipSuccess) return fail(RSF_ERR_DEVICE, "rsf_mcmc_draws: %s", hipGetErrorString(e));
  if (z) for (int p = 0; p < d; ++p) z[p] = h[p];
  if (u) *u = h[3];
  if (g) *g = h[4];
  return RSF_OK;
}

}  // extern "C"
