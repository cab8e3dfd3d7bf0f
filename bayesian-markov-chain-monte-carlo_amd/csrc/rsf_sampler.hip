// rsf_sampler.hip — the sampler's host side: the kernel of a launch with its grid and LDS, the plain, drained and
// graph-replayed runs, rsf_mcmc_run / _replay / _replay_ssq, and rsf_mcmc_adapt (kernels: rsf_kernels_sampler.h).
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <algorithm>

#include "rsf_host.h"
#include "rsf_kernels_sampler.h"

using namespace rsfk;
using namespace rsfh;

namespace {

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

using SamplerFn = void (*)(Consts, McmcArgs);

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

// The sampler kernel of a launch, and its grid and LDS: the table chunk (mcmc_table_bytes), and behind it per-lane slots
// (rsf_kernels_sampler.h: the float64 RK4 sampler parks the chain state there; the others keep only a three-parameter chain's
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

}  // namespace

void rsfh::release_replay_graph(rsf_ctx *c) {
  auto &g = c->rg;
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  if (g.host) (void)hipHostFree(g.host);
  if (g.dev) (void)hipFree(g.dev);
  g = rsf_ctx::ReplayGraph{};
}

namespace {

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

}  // namespace

extern "C" {

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

// The self-test of the sampler's window arithmetic lives with the sampler: probe_adapt_kernel is compiled in the module of
// the kernels whose adaptation it restates (rsf_kernels_sampler.h).
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
    // no ctx: the null stream, so not rsfh::launch; the copy that follows reports a failure
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
