// rsf_smc.hip — tempered sequential Monte Carlo over the box prior (include/rsf_smc.h): rsf_smc_init / _weight_sums / _resample /
// _move / _move_propose / _move_accept / _std2 (kernels: rsf_kernels_smc.h).  rsf_smc_section, rsf_smc_increment and
// rsf_smc_log_evidence, the host arithmetic, are in rsf_finish.cpp.  Behind them the same calls for P independent populations per
// launch (include/rsf_smc_batch.h: rsf_smc_batch_init / _logtarget / _weight_sums / _resample / _move / _std2; kernels:
// rsf_kernels_smc_batch.h, which needs the chain logic of rsf_kernels_smc.h and therefore lives in this unit).
#include <cmath>
#include <cstdio>
#include <algorithm>

#include "rsf_host.h"
#include "rsf_kernels_smc.h"
#include "rsf_kernels_smc_batch.h"

using namespace rsfk;
using namespace rsfh;

namespace {

// the box of a call into A.lo[], A.hi[]; fn: the entry point the message names
int set_box(const char *fn, int d, const double *lo, const double *hi, SmcArgs &A) {
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p])) return fail(RSF_ERR_INVALID, "%s: need finite lo[%d] < hi[%d]", fn, p, p);
    A.lo[p] = lo[p]; A.hi[p] = hi[p];
  }
  return RSF_OK;
}

// chol[d][d]: lower triangular with a positive finite diagonal, into A.L
int set_factor(const char *fn, int d, const double *chol, SmcArgs &A) {
  int e = 0;
  for (int p = 0; p < d; ++p)
    for (int r = 0; r < d; ++r) {
      const double v = chol[p * d + r];
      if (!std::isfinite(v) || (r > p && v != 0.0) || (r == p && !(v > 0.0)))
        return fail(RSF_ERR_INVALID, "%s: chol is not a lower triangular factor with a positive diagonal (entry [%d][%d])", fn, p, r);
      if (r <= p) A.L[e++] = v;
    }
  return RSF_OK;
}

int set_stream(const char *fn, int64_t n, int64_t offset, int64_t iter, int64_t iter_min, uint64_t seed, SmcArgs &A) {
  if (n < 1 || offset < 0 || iter < iter_min || iter > 0xffffffffll - RSF_SMC_MAX_STEPS)
    return fail(RSF_ERR_INVALID, "%s: need n >= 1, offset >= 0 and an iteration in [%lld, 2^32 - %d)", fn, (long long)iter_min, RSF_SMC_MAX_STEPS + 1);
  A.n = n; A.offset = offset; A.seed = seed; A.iter = (uint32_t)iter;
  return RSF_OK;
}

auto init_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return smc_init_kernel<D>; }); }
auto propose_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return smc_propose_kernel<D>; }); }
// the float64 RK4 solve with or without damping, chosen as predict_kernel's dispatcher chooses
auto move_fn(const rsf_ctx *c, int d) {
  return with<1, 3>(d, [&](auto D) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return smc_move_kernel<D, DAMP>; }); });
}

// the accepted counts of `steps` steps: zeroed before the launch, read after it (the pool workspace's first bytes)
int counts_begin(rsf_ctx *c, int steps, unsigned long long **cnt) {
  int rc;
  if ((rc = ensure(c->pool, sizeof(unsigned long long) * RSF_SMC_MAX_STEPS))) return rc;
  *cnt = (unsigned long long *)c->pool.p;
  HIP_TRY(hipMemsetAsync(*cnt, 0, sizeof(unsigned long long) * steps, c->stream));
  return RSF_OK;
}
int counts_end(rsf_ctx *c, int steps, const unsigned long long *cnt, int64_t *accepted) {
  unsigned long long h[RSF_SMC_MAX_STEPS];
  HIP_TRY(hipMemcpyAsync(h, cnt, sizeof(unsigned long long) * steps, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int s = 0; s < steps; ++s) accepted[s] = (int64_t)h[s];
  return RSF_OK;
}

}  // namespace

extern "C" {

int rsf_smc_init(rsf_ctx *c, int64_t n, int32_t d, const double *lo, const double *hi, uint64_t seed, int64_t offset, double *q) {
  RSF_ENTER(c, NEED_NOTHING, lo && hi && q, "NULL argument");
  if (d < 1 || d > RSF_SMC_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_smc_init: need 1 <= d <= %d", RSF_SMC_MAX_PARAMS);
  int rc;
  SmcArgs A{};
  if ((rc = set_stream(__func__, n, offset, 0, 0, seed, A))) return rc;
  if ((rc = set_box(__func__, d, lo, hi, A))) return rc;
  const size_t nb = (size_t)n * d * sizeof(double);
  double *dq;
  if ((rc = stage_out(c, SLOT_SMC_Q, q, nb, &dq))) return rc;
  if ((rc = launch(c, init_fn(d), blocks_of(n), kMaxBlock, 0, A, dq))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_Q, q, nb))) return rc;
  return finish(c);
}

int rsf_smc_weight_sums(rsf_ctx *c, int64_t n, const double *l, int32_t m, const double *deltas, double lmax, double *out) {
  RSF_ENTER(c, NEED_NOTHING, l && deltas && out, "NULL argument");
  if (n < 1 || m < 1 || m > RSF_SMC_MAX_CANDIDATES) return fail(RSF_ERR_INVALID, "rsf_smc_weight_sums: need n >= 1 and 1 <= m <= %d", RSF_SMC_MAX_CANDIDATES);
  if (std::isinf(lmax)) return fail(RSF_ERR_INVALID, "rsf_smc_weight_sums: lmax is finite, or NaN for the largest finite l");
  SmcDeltas dl{};
  for (int k = 0; k < m; ++k) {
    if (!std::isfinite(deltas[k]) || deltas[k] < 0.0) return fail(RSF_ERR_INVALID, "rsf_smc_weight_sums: deltas[%d] is not finite and >= 0", k);
    dl.v[k] = deltas[k];
  }
  int rc;
  const double *dl_l;
  if ((rc = stage_in(c, SLOT_SMC_L, l, (size_t)n * sizeof(double), &dl_l))) return rc;
  // workspace, doubles: sums[kSmcFields] | head[kSmcHead] | the workgroups' partials of the sums | ... of the head
  const int blocks = (int)std::min<int64_t>(kSmcBlocks, (n + kMaxBlock - 1) / kMaxBlock);
  if ((rc = ensure(c->pool, sizeof(double) * (kSmcFields + kSmcHead) * (kSmcBlocks + 1)))) return rc;
  double *ws = (double *)c->pool.p, *head = ws + kSmcFields, *part = head + kSmcHead, *parth = part + (size_t)kSmcFields * kSmcBlocks;
  double h[kSmcHead + kSmcFields];
  if ((rc = launch(c, smc_max_kernel, blocks, kMaxBlock, 0, n, dl_l, parth))) return rc;
  if ((rc = launch(c, smc_max_finish_kernel, 1, kMaxBlock, 0, blocks, parth, head))) return rc;
  HIP_TRY(hipMemcpyAsync(h, head, kSmcHead * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (h[1] + h[2] != (double)n) return fail(RSF_ERR_INVALID, "rsf_smc_weight_sums: %lld of l are NaN or +inf", (long long)((double)n - h[1] - h[2]));
  if (!(h[1] > 0.0)) return fail(RSF_ERR_INVALID, "rsf_smc_weight_sums: every particle has l = -inf (no particle lies in the target's support)");
  if (!std::isnan(lmax)) h[0] = lmax;
  if ((rc = launch(c, smc_weight_sums_kernel, blocks, kMaxBlock, 0, n, dl_l, h[0], dl, part))) return rc;
  if ((rc = sum_strided_tree(c, blocks, kSmcFields, part, ws))) return rc;
  HIP_TRY(hipMemcpyAsync(h + kSmcHead, ws, kSmcFields * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  out[0] = h[0]; out[1] = h[1]; out[2] = h[2];
  for (int k = 0; k < 2 * m; ++k) out[RSF_SMC_HEAD + k] = h[kSmcHead + k];
  return RSF_OK;
}

int rsf_smc_resample(rsf_ctx *c, int64_t n, int32_t d, const double *q, const double *l, double delta, double lmax, double u, double *cum,
                     int64_t *anc, double *q_out, double *l_out) {
  RSF_ENTER(c, NEED_NOTHING, q && l && cum && anc && q_out && l_out, "NULL argument");
  if (n < 1 || d < 1 || d > RSF_SMC_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_smc_resample: need n >= 1, 1 <= d <= %d", RSF_SMC_MAX_PARAMS);
  if (!std::isfinite(delta) || delta < 0.0 || !std::isfinite(lmax) || !(u > 0.0 && u <= 1.0))
    return fail(RSF_ERR_INVALID, "rsf_smc_resample: need finite delta >= 0, finite lmax and u inside (0, 1]");
  int rc;
  const size_t nb = (size_t)n * sizeof(double);
  const double *dq, *dl;
  double *dcum, *dqo, *dlo;
  int64_t *danc;
  if ((rc = stage_in(c, SLOT_SMC_Q, q, nb * d, &dq))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_L, l, nb, &dl))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_CUM, cum, nb, &dcum))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_ANC, anc, (size_t)n * sizeof(int64_t), &danc))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_Q_OUT, q_out, nb * d, &dqo))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_L_OUT, l_out, nb, &dlo))) return rc;
  const int64_t ntiles = (n + kSmcTile - 1) / kSmcTile;
  if ((rc = ensure(c->pool, sizeof(double) * (size_t)ntiles))) return rc;
  double *tsum = (double *)c->pool.p;
  if ((rc = launch(c, smc_scan_tiles_kernel, (unsigned)ntiles, kMaxBlock, 0, n, dl, delta, lmax, tsum))) return rc;
  if ((rc = launch(c, smc_scan_carry_kernel, 1, 64, 0, ntiles, tsum))) return rc;
  if ((rc = launch(c, smc_scan_final_kernel, (unsigned)ntiles, kMaxBlock, 0, n, dl, delta, lmax, tsum, dcum))) return rc;
  if ((rc = launch(c, smc_ancestor_kernel, blocks_of(n), kMaxBlock, 0, n, dcum, u, danc))) return rc;
  if ((rc = launch(c, smc_gather_kernel, blocks_of(n), kMaxBlock, 0, n, d, danc, dq, dl, dqo, dlo))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_CUM, cum, nb))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_ANC, anc, (size_t)n * sizeof(int64_t)))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_Q_OUT, q_out, nb * d))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_L_OUT, l_out, nb))) return rc;
  return finish(c);
}

int rsf_smc_move(rsf_ctx *c, int64_t n, int32_t d, double *q, double *l, const double *data, double shape, const double *lo, const double *hi,
                 const double *chol, double beta, uint64_t seed, int64_t offset, int64_t iter0, int32_t steps, int64_t *accepted) {
  RSF_ENTER(c, NEED_MODEL, q && l && data && lo && hi && chol && accepted, "NULL argument");
  if (d != 1 && d != 3) return fail(RSF_ERR_INVALID, "rsf_smc_move: need d = 1 or 3");
  if (!std::isfinite(shape) || !(shape > 0.0) || !std::isfinite(beta) || !(beta > 0.0))
    return fail(RSF_ERR_INVALID, "rsf_smc_move: shape and beta must be finite and > 0");
  if (steps < 1 || steps > RSF_SMC_MAX_STEPS) return fail(RSF_ERR_INVALID, "rsf_smc_move: need 1 <= steps <= %d", RSF_SMC_MAX_STEPS);
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_smc_move: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  int rc;
  SmcArgs A{};
  if ((rc = set_stream(__func__, n, offset, iter0, 1, seed, A))) return rc;
  if ((rc = set_box(__func__, d, lo, hi, A))) return rc;
  if ((rc = set_factor(__func__, d, chol, A))) return rc;
  A.steps = steps; A.beta = beta; A.shape = shape;
  const size_t nb = (size_t)n * sizeof(double);
  const double *dq, *dl, *ddata;
  unsigned long long *cnt;
  if ((rc = stage_in(c, SLOT_SMC_Q, (const double *)q, nb * d, &dq))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_L, (const double *)l, nb, &dl))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_OBS, data, (size_t)c->nout * sizeof(double), &ddata))) return rc;
  if ((rc = counts_begin(c, steps, &cnt))) return rc;
  // the shared chunking of the float64 tables (c->kc, c->lds_bytes), as rsf_evidence_logtarget's solve
  if ((rc = launch(c, move_fn(c, d), grid_for(c, n), c->block, c->lds_bytes, make_consts(c, ddata), A, (double *)dq, (double *)dl, cnt))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_Q, q, nb * d))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_L, l, nb))) return rc;
  return counts_end(c, steps, cnt, accepted);
}

int rsf_smc_move_propose(rsf_ctx *c, int64_t n, int32_t d, const double *q, const double *lo, const double *hi, const double *chol, uint64_t seed,
                         int64_t offset, int64_t iter, double *q_new, uint8_t *inbox) {
  RSF_ENTER(c, NEED_NOTHING, q && lo && hi && chol && q_new && inbox, "NULL argument");
  if (d < 1 || d > RSF_SMC_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_smc_move_propose: need 1 <= d <= %d", RSF_SMC_MAX_PARAMS);
  int rc;
  SmcArgs A{};
  if ((rc = set_stream(__func__, n, offset, iter, 1, seed, A))) return rc;
  if ((rc = set_box(__func__, d, lo, hi, A))) return rc;
  if ((rc = set_factor(__func__, d, chol, A))) return rc;
  const size_t nb = (size_t)n * d * sizeof(double);
  const double *dq;
  double *dqn;
  uint8_t *dinb;
  if ((rc = stage_in(c, SLOT_SMC_Q, q, nb, &dq))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_Q_OUT, q_new, nb, &dqn))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_INBOX, inbox, (size_t)n, &dinb))) return rc;
  if ((rc = launch(c, propose_fn(d), blocks_of(n), kMaxBlock, 0, A, dq, dqn, dinb))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_Q_OUT, q_new, nb))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_INBOX, inbox, (size_t)n))) return rc;
  return finish(c);
}

int rsf_smc_move_accept(rsf_ctx *c, int64_t n, int32_t d, double *q, double *l, const double *q_new, const uint8_t *inbox, const double *ssq_new,
                        double shape, double beta, uint64_t seed, int64_t offset, int64_t iter, int64_t *accepted) {
  RSF_ENTER(c, NEED_NOTHING, q && l && q_new && inbox && ssq_new && accepted, "NULL argument");
  if (d < 1 || d > RSF_SMC_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_smc_move_accept: need 1 <= d <= %d", RSF_SMC_MAX_PARAMS);
  if (!std::isfinite(shape) || !(shape > 0.0) || !std::isfinite(beta) || !(beta > 0.0))
    return fail(RSF_ERR_INVALID, "rsf_smc_move_accept: shape and beta must be finite and > 0");
  int rc;
  SmcArgs A{};
  if ((rc = set_stream(__func__, n, offset, iter, 1, seed, A))) return rc;
  A.steps = 1; A.beta = beta; A.shape = shape;
  const size_t nb = (size_t)n * sizeof(double);
  const double *dq, *dl, *dqn, *dssq;
  const uint8_t *dinb;
  unsigned long long *cnt;
  if ((rc = stage_in(c, SLOT_SMC_Q, (const double *)q, nb * d, &dq))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_L, (const double *)l, nb, &dl))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_Q_OUT, q_new, nb * d, &dqn))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_INBOX, inbox, (size_t)n, &dinb))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_SSQ, ssq_new, nb, &dssq))) return rc;
  if ((rc = counts_begin(c, 1, &cnt))) return rc;
  if ((rc = launch(c, smc_accept_kernel, blocks_of(n), kMaxBlock, 0, A, d, dqn, dinb, dssq, (double *)dq, (double *)dl, cnt))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_Q, q, nb * d))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_L, l, nb))) return rc;
  return counts_end(c, 1, cnt, accepted);
}

int rsf_smc_std2(rsf_ctx *c, int64_t n, const double *l, double shape, uint64_t seed, int64_t offset, int64_t iter, double *std2) {
  RSF_ENTER(c, NEED_NOTHING, l && std2, "NULL argument");
  if (!std::isfinite(shape) || !(shape >= 1.0)) return fail(RSF_ERR_INVALID, "rsf_smc_std2: shape must be finite and >= 1 (the gamma variate's range)");
  int rc;
  SmcArgs A{};
  if ((rc = set_stream(__func__, n, offset, iter, 0, seed, A))) return rc;
  A.shape = shape;
  const size_t nb = (size_t)n * sizeof(double);
  const double *dl;
  double *ds;
  if ((rc = stage_in(c, SLOT_SMC_L, l, nb, &dl))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_L_OUT, std2, nb, &ds))) return rc;
  const double gd = shape - 1.0 / 3.0;
  if ((rc = launch(c, smc_std2_kernel, blocks_of(n), kMaxBlock, 0, A, gd, 1.0 / std::sqrt(9.0 * gd), dl, ds))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_L_OUT, std2, nb))) return rc;
  return finish(c);
}

}  // extern "C"

// ---- P independent populations per call (include/rsf_smc_batch.h) ------------------------------------------------------------------
namespace {

// "<entry point>: population p", what the single calls' checks name in a message about one population
struct Who {
  char s[96];
  Who(const char *fn, int p) { snprintf(s, sizeof s, "%s: population %d", fn, p); }
};

int check_batch(const char *fn, int32_t P, int64_t n) {
  if (P < 1 || P > RSF_SMC_BATCH_MAX) return fail(RSF_ERR_INVALID, "%s: need 1 <= P <= %d populations", fn, RSF_SMC_BATCH_MAX);
  if (n < 1) return fail(RSF_ERR_INVALID, "%s: need n >= 1", fn);
  return RSF_OK;
}

int set_groups(const char *fn, int32_t P, int32_t G, const int32_t *group, const uint8_t *active, SmcPop *pops) {
  if (G < 1) return fail(RSF_ERR_INVALID, "%s: need G >= 1 observation series", fn);
  for (int p = 0; p < P; ++p) {
    if (active && !active[p]) continue;
    if (group[p] < 0 || group[p] >= G) return fail(RSF_ERR_INVALID, "%s: population %d: group %d is outside 0..%d", fn, p, group[p], G - 1);
    pops[p].group = group[p];
  }
  return RSF_OK;
}

// The populations' parameters on the device (the ctx's second pool workspace).  The source is pageable host memory, which the
// runtime has read when the copy call returns (as rsf_set_model's table): the caller's array may go out of scope.
int put_pops(rsf_ctx *c, int32_t P, const SmcPop *pops, const SmcPop **dev) {
  int rc;
  if ((rc = ensure(c->poolws, sizeof(SmcPop) * RSF_SMC_BATCH_MAX))) return rc;
  HIP_TRY(hipMemcpyAsync(c->poolws.p, pops, sizeof(SmcPop) * P, hipMemcpyHostToDevice, c->stream));
  *dev = (const SmcPop *)c->poolws.p;
  return RSF_OK;
}

// rows [p] of `bytes` each of an output staged in `slot`, back to a host caller for the active populations only
int copy_back_active(rsf_ctx *c, Slot slot, void *dst, size_t bytes, int32_t P, const uint8_t *active) {
  if (!host_mem(c)) return RSF_OK;
  for (int p = 0; p < P; ++p)
    if (active[p])
      HIP_TRY(hipMemcpyAsync((char *)dst + p * bytes, (const char *)c->stage[slot].p + p * bytes, bytes, hipMemcpyDeviceToHost, c->stream));
  return RSF_OK;
}

auto batch_init_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return smc_batch_init_kernel<D>; }); }
auto batch_logtarget_fn(const rsf_ctx *c, int d) {
  return with<1, 3>(d, [&](auto D) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return smc_batch_logtarget_kernel<D, DAMP>; }); });
}
auto batch_move_fn(const rsf_ctx *c, int d) {
  return with<1, 3>(d, [&](auto D) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return smc_batch_move_kernel<D, DAMP>; }); });
}

}  // namespace

extern "C" {

int rsf_smc_batch_init(rsf_ctx *c, int32_t P, int64_t n, int32_t d, const double *lo, const double *hi, const uint64_t *seeds,
                       const int64_t *offsets, double *q) {
  RSF_ENTER(c, NEED_NOTHING, lo && hi && seeds && offsets && q, "NULL argument");
  int rc;
  if ((rc = check_batch(__func__, P, n))) return rc;
  if (d < 1 || d > RSF_SMC_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_smc_batch_init: need 1 <= d <= %d", RSF_SMC_MAX_PARAMS);
  SmcArgs A{}, S{};
  if ((rc = set_box(__func__, d, lo, hi, A))) return rc;
  A.n = n;
  SmcPop pops[RSF_SMC_BATCH_MAX] = {};
  for (int p = 0; p < P; ++p) {
    if ((rc = set_stream(Who(__func__, p).s, n, offsets[p], 0, 0, seeds[p], S))) return rc;
    pops[p].seed = S.seed; pops[p].offset = S.offset; pops[p].iter = S.iter;
  }
  const SmcPop *dp;
  const size_t nb = (size_t)P * n * d * sizeof(double);
  double *dq;
  if ((rc = put_pops(c, P, pops, &dp))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_Q, q, nb, &dq))) return rc;
  if ((rc = launch(c, batch_init_fn(d), dim3(blocks_of(n), P), kMaxBlock, 0, A, dp, dq))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_Q, q, nb))) return rc;
  return finish(c);
}

int rsf_smc_batch_logtarget(rsf_ctx *c, int32_t P, int64_t n, int32_t d, const double *q, const double *data, int32_t G,
                            const int32_t *group, double shape, const double *lo, const double *hi, double *l) {
  RSF_ENTER(c, NEED_MODEL, q && data && group && lo && hi && l, "NULL argument");
  int rc;
  if ((rc = check_batch(__func__, P, n))) return rc;
  if (d != 1 && d != 3) return fail(RSF_ERR_INVALID, "rsf_smc_batch_logtarget: need d = 1 or 3");
  if (!std::isfinite(shape) || !(shape > 0.0)) return fail(RSF_ERR_INVALID, "rsf_smc_batch_logtarget: shape must be finite and > 0");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_smc_batch_logtarget: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  SmcArgs A{};
  if ((rc = set_box(__func__, d, lo, hi, A))) return rc;
  A.n = n; A.shape = shape;
  SmcPop pops[RSF_SMC_BATCH_MAX] = {};
  if ((rc = set_groups(__func__, P, G, group, nullptr, pops))) return rc;
  const SmcPop *dp;
  const size_t nb = (size_t)P * n * sizeof(double);
  const double *dq, *ddata;
  double *dl;
  if ((rc = put_pops(c, P, pops, &dp))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_Q, q, nb * d, &dq))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_OBS, data, (size_t)G * c->nout * sizeof(double), &ddata))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_L, l, nb, &dl))) return rc;
  if ((rc = launch(c, batch_logtarget_fn(c, d), dim3(grid_for(c, n), P), c->block, c->lds_bytes, make_consts(c, ddata), A, dp, dq, dl))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_L, l, nb))) return rc;
  return finish(c);
}

int rsf_smc_batch_weight_sums(rsf_ctx *c, int32_t P, int64_t n, const double *l, int32_t m, const double *deltas, const double *lmax,
                              const uint8_t *active, double *out) {
  RSF_ENTER(c, NEED_NOTHING, l && deltas && lmax && active && out, "NULL argument");
  int rc;
  if ((rc = check_batch(__func__, P, n))) return rc;
  if (m < 1 || m > RSF_SMC_MAX_CANDIDATES) return fail(RSF_ERR_INVALID, "rsf_smc_batch_weight_sums: need 1 <= m <= %d", RSF_SMC_MAX_CANDIDATES);
  SmcPop pops[RSF_SMC_BATCH_MAX] = {};
  for (int p = 0; p < P; ++p) {
    if (!(pops[p].active = active[p] != 0)) continue;
    if (std::isinf(lmax[p])) return fail(RSF_ERR_INVALID, "rsf_smc_batch_weight_sums: population %d: lmax is finite, or NaN for the largest finite l", p);
    pops[p].lmax = lmax[p];
    for (int k = 0; k < m; ++k) {
      const double v = deltas[(size_t)p * m + k];
      if (!std::isfinite(v) || v < 0.0) return fail(RSF_ERR_INVALID, "rsf_smc_batch_weight_sums: population %d: deltas[%d] is not finite and >= 0", p, k);
      pops[p].dl[k] = v;
    }
  }
  const SmcPop *dp;
  const double *dl_l;
  if ((rc = put_pops(c, P, pops, &dp))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_L, l, (size_t)P * n * sizeof(double), &dl_l))) return rc;
  // workspace, doubles: sums[P][kSmcFields] | head[P][kSmcHead] | the workgroups' partials of the sums [P][blocks][..] | ... of the head
  const int blocks = (int)std::min<int64_t>(kSmcBlocks, (n + kMaxBlock - 1) / kMaxBlock);
  if ((rc = ensure(c->pool, sizeof(double) * (kSmcFields + kSmcHead) * (size_t)P * (blocks + 1)))) return rc;
  double *ws = (double *)c->pool.p, *head = ws + (size_t)kSmcFields * P, *part = head + (size_t)kSmcHead * P, *parth = part + (size_t)kSmcFields * P * blocks;
  if ((rc = launch(c, smc_batch_max_kernel, dim3(blocks, P), kMaxBlock, 0, n, dp, dl_l, parth))) return rc;
  if ((rc = launch(c, smc_batch_max_finish_kernel, P, kMaxBlock, 0, blocks, dp, parth, head))) return rc;
  // a population without a finite l has the head -inf: its sums are computed and not used (the check below refuses the call)
  if ((rc = launch(c, smc_batch_weight_sums_kernel, dim3(blocks, P), kMaxBlock, 0, n, dp, dl_l, head, part))) return rc;
  if ((rc = launch(c, smc_batch_tree_kernel, dim3(kSmcFields, P), kMaxBlock, 0, blocks, kSmcFields, dp, part, ws))) return rc;
  double h[RSF_SMC_BATCH_MAX * (kSmcFields + kSmcHead)];
  HIP_TRY(hipMemcpyAsync(h, ws, sizeof(double) * (kSmcFields + kSmcHead) * P, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const double *hs = h, *hh = h + (size_t)kSmcFields * P;
  for (int p = 0; p < P; ++p) {
    if (!active[p]) continue;
    const double *e = hh + p * kSmcHead;
    if (e[1] + e[2] != (double)n)
      return fail(RSF_ERR_INVALID, "rsf_smc_batch_weight_sums: population %d: %lld of l are NaN or +inf", p, (long long)((double)n - e[1] - e[2]));
    if (!(e[1] > 0.0))
      return fail(RSF_ERR_INVALID, "rsf_smc_batch_weight_sums: population %d: every particle has l = -inf (no particle lies in the target's support)", p);
  }
  for (int p = 0; p < P; ++p) {
    if (!active[p]) continue;
    double *o = out + (size_t)p * (RSF_SMC_HEAD + 2 * m);
    const double *e = hh + p * kSmcHead;
    o[0] = std::isnan(lmax[p]) ? e[0] : lmax[p]; o[1] = e[1]; o[2] = e[2];
    for (int k = 0; k < 2 * m; ++k) o[RSF_SMC_HEAD + k] = hs[p * kSmcFields + k];
  }
  return RSF_OK;
}

int rsf_smc_batch_resample(rsf_ctx *c, int32_t P, int64_t n, int32_t d, const double *q, const double *l, const double *delta,
                           const double *lmax, const double *u, const uint8_t *active, double *cum, int64_t *anc, double *q_out,
                           double *l_out) {
  RSF_ENTER(c, NEED_NOTHING, q && l && delta && lmax && u && active && cum && anc && q_out && l_out, "NULL argument");
  int rc;
  if ((rc = check_batch(__func__, P, n))) return rc;
  if (d < 1 || d > RSF_SMC_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_smc_batch_resample: need 1 <= d <= %d", RSF_SMC_MAX_PARAMS);
  SmcPop pops[RSF_SMC_BATCH_MAX] = {};
  for (int p = 0; p < P; ++p) {
    if (!(pops[p].active = active[p] != 0)) continue;
    if (!std::isfinite(delta[p]) || delta[p] < 0.0 || !std::isfinite(lmax[p]) || !(u[p] > 0.0 && u[p] <= 1.0))
      return fail(RSF_ERR_INVALID, "rsf_smc_batch_resample: population %d: need finite delta >= 0, finite lmax and u inside (0, 1]", p);
    pops[p].delta = delta[p]; pops[p].lmax = lmax[p]; pops[p].u = u[p];
  }
  const SmcPop *dp;
  const size_t nb = (size_t)n * sizeof(double);
  const double *dq, *dl;
  double *dcum, *dqo, *dlo;
  int64_t *danc;
  if ((rc = put_pops(c, P, pops, &dp))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_Q, q, nb * d * P, &dq))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_L, l, nb * P, &dl))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_CUM, cum, nb * P, &dcum))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_ANC, anc, (size_t)n * sizeof(int64_t) * P, &danc))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_Q_OUT, q_out, nb * d * P, &dqo))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_L_OUT, l_out, nb * P, &dlo))) return rc;
  const int64_t ntiles = (n + kSmcTile - 1) / kSmcTile;
  if ((rc = ensure(c->pool, sizeof(double) * (size_t)ntiles * P))) return rc;
  double *tsum = (double *)c->pool.p;
  if ((rc = launch(c, smc_batch_scan_tiles_kernel, dim3((unsigned)ntiles, P), kMaxBlock, 0, n, dp, dl, tsum))) return rc;
  if ((rc = launch(c, smc_batch_scan_carry_kernel, P, 64, 0, ntiles, dp, tsum))) return rc;
  if ((rc = launch(c, smc_batch_scan_final_kernel, dim3((unsigned)ntiles, P), kMaxBlock, 0, n, dp, dl, tsum, dcum))) return rc;
  if ((rc = launch(c, smc_batch_ancestor_kernel, dim3(blocks_of(n), P), kMaxBlock, 0, n, dp, dcum, danc))) return rc;
  if ((rc = launch(c, smc_batch_gather_kernel, dim3(blocks_of(n), P), kMaxBlock, 0, n, d, dp, danc, dq, dl, dqo, dlo))) return rc;
  if ((rc = copy_back_active(c, SLOT_SMC_CUM, cum, nb, P, active))) return rc;
  if ((rc = copy_back_active(c, SLOT_SMC_ANC, anc, (size_t)n * sizeof(int64_t), P, active))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_Q_OUT, q_out, nb * d * P))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_L_OUT, l_out, nb * P))) return rc;
  return finish(c);
}

int rsf_smc_batch_move(rsf_ctx *c, int32_t P, int64_t n, int32_t d, double *q, double *l, const double *data, int32_t G,
                       const int32_t *group, double shape, const double *lo, const double *hi, const double *chol, const double *beta,
                       const uint64_t *seeds, const int64_t *offsets, const int64_t *iter0, int32_t steps, const uint8_t *active,
                       int64_t *accepted) {
  RSF_ENTER(c, NEED_MODEL, q && l && data && group && lo && hi && chol && beta && seeds && offsets && iter0 && active && accepted, "NULL argument");
  int rc;
  if ((rc = check_batch(__func__, P, n))) return rc;
  if (d != 1 && d != 3) return fail(RSF_ERR_INVALID, "rsf_smc_batch_move: need d = 1 or 3");
  if (!std::isfinite(shape) || !(shape > 0.0)) return fail(RSF_ERR_INVALID, "rsf_smc_batch_move: shape must be finite and > 0");
  if (steps < 1 || steps > RSF_SMC_MAX_STEPS) return fail(RSF_ERR_INVALID, "rsf_smc_batch_move: need 1 <= steps <= %d", RSF_SMC_MAX_STEPS);
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_smc_batch_move: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  SmcArgs A{}, S{};
  if ((rc = set_box(__func__, d, lo, hi, A))) return rc;
  A.n = n; A.steps = steps; A.shape = shape;
  SmcPop pops[RSF_SMC_BATCH_MAX] = {};
  if ((rc = set_groups(__func__, P, G, group, active, pops))) return rc;
  for (int p = 0; p < P; ++p) {
    if (!(pops[p].active = active[p] != 0)) continue;
    const Who who(__func__, p);
    if (!std::isfinite(beta[p]) || !(beta[p] > 0.0)) return fail(RSF_ERR_INVALID, "%s: beta must be finite and > 0", who.s);
    if ((rc = set_stream(who.s, n, offsets[p], iter0[p], 1, seeds[p], S))) return rc;
    if ((rc = set_factor(who.s, d, chol + (size_t)p * d * d, S))) return rc;
    pops[p].seed = S.seed; pops[p].offset = S.offset; pops[p].iter = S.iter; pops[p].beta = beta[p];
    for (int k = 0; k < d * (d + 1) / 2; ++k) pops[p].L[k] = S.L[k];
  }
  const SmcPop *dp;
  const size_t nb = (size_t)P * n * sizeof(double);
  const double *dq, *dl, *ddata;
  if ((rc = put_pops(c, P, pops, &dp))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_Q, (const double *)q, nb * d, &dq))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_L, (const double *)l, nb, &dl))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_OBS, data, (size_t)G * c->nout * sizeof(double), &ddata))) return rc;
  // the accepted counts cnt[P][steps]: zeroed before the launch, read after it (the pool workspace's first bytes)
  const size_t cb = sizeof(unsigned long long) * (size_t)P * steps;
  if ((rc = ensure(c->pool, sizeof(unsigned long long) * RSF_SMC_BATCH_MAX * RSF_SMC_MAX_STEPS))) return rc;
  unsigned long long *cnt = (unsigned long long *)c->pool.p;
  HIP_TRY(hipMemsetAsync(cnt, 0, cb, c->stream));
  if ((rc = launch(c, batch_move_fn(c, d), dim3(grid_for(c, n), P), c->block, c->lds_bytes, make_consts(c, ddata), A, dp, (double *)dq, (double *)dl, cnt)))
    return rc;
  if ((rc = copy_back(c, SLOT_SMC_Q, q, nb * d))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_L, l, nb))) return rc;
  static thread_local unsigned long long h[RSF_SMC_BATCH_MAX * RSF_SMC_MAX_STEPS];
  HIP_TRY(hipMemcpyAsync(h, cnt, cb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int p = 0; p < P; ++p)
    for (int s = 0; active[p] && s < steps; ++s) accepted[(size_t)p * steps + s] = (int64_t)h[(size_t)p * steps + s];
  return RSF_OK;
}

int rsf_smc_batch_std2(rsf_ctx *c, int32_t P, int64_t n, const double *l, double shape, const uint64_t *seeds, const int64_t *offsets,
                       const int64_t *iter, double *std2) {
  RSF_ENTER(c, NEED_NOTHING, l && seeds && offsets && iter && std2, "NULL argument");
  int rc;
  if ((rc = check_batch(__func__, P, n))) return rc;
  if (!std::isfinite(shape) || !(shape >= 1.0)) return fail(RSF_ERR_INVALID, "rsf_smc_batch_std2: shape must be finite and >= 1 (the gamma variate's range)");
  SmcArgs A{}, S{};
  A.n = n; A.shape = shape;
  SmcPop pops[RSF_SMC_BATCH_MAX] = {};
  for (int p = 0; p < P; ++p) {
    if ((rc = set_stream(Who(__func__, p).s, n, offsets[p], iter[p], 0, seeds[p], S))) return rc;
    pops[p].seed = S.seed; pops[p].offset = S.offset; pops[p].iter = S.iter;
  }
  const SmcPop *dp;
  const size_t nb = (size_t)P * n * sizeof(double);
  const double *dl;
  double *ds;
  if ((rc = put_pops(c, P, pops, &dp))) return rc;
  if ((rc = stage_in(c, SLOT_SMC_L, l, nb, &dl))) return rc;
  if ((rc = stage_out(c, SLOT_SMC_L_OUT, std2, nb, &ds))) return rc;
  const double gd = shape - 1.0 / 3.0;
  if ((rc = launch(c, smc_batch_std2_kernel, dim3(blocks_of(n), P), kMaxBlock, 0, A, dp, gd, 1.0 / std::sqrt(9.0 * gd), dl, ds))) return rc;
  if ((rc = copy_back(c, SLOT_SMC_L_OUT, std2, nb))) return rc;
  return finish(c);
}

}  // extern "C"
