// rsf_predict.hip — posterior predictive checks, PSIS-LOO and the predictive band with noise on the device
// (include/rsf_predict.h, include/rsf_psis.h, include/rsf_predict_noise.h): rsf_predict_partials / _quantiles / _psis_loo /
// _noise_quantiles (kernels: rsf_predict.h, rsf_psis.h, rsf_predict_noise.h).  The host arithmetic that finishes their results
// is rsf_finish.cpp.
#include <climits>
#include <cmath>
#include <algorithm>
#include <vector>

#include "../../include/rsf_predict.h"
#include "rsf_host.h"
#include "rsf_predict.h"
#include "rsf_psis.h"
#include "rsf_predict_noise.h"

using namespace rsfk;
using namespace rsfh;

namespace {
// rsf_predict_partials' solve, void (*)(Consts, PredictArgs): the float64 RK4 tiers, in the float32 mode as well (like init_kernel)
auto predict_fn(const rsf_ctx *c, int d, bool want_series) {
  return with<1, 3>(d, [&](auto D) {
    return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) {
      return with<true, false>(want_series, [&](auto SERIES) { return predict_kernel<D, DAMP, SERIES>; });
    });
  });
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

extern "C" {

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
  if ((rc = sum_in_order(c, nwaves, kPredSlab, nf, w, 1.0, w + o_slab))) return rc;
  if ((rc = sum_in_order(c, nslabs, nslabs, nf, w + o_slab, 1.0, w + o_sum))) return rc;
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
  if ((rc = launch(c, predict_select_kernel, (unsigned)nout, kPredSelectThreads, 0, n, nout, ds, n_probs, P, (double *)c->poolws.p))) return rc;
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
  HIP_TRY(hipMemcpyAsync(out_rows, c->poolws.p, ob, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RSF_OK;
}

int rsf_predict_noise_quantiles(rsf_ctx *c, int64_t n, int64_t nout, const double *series, const double *std2, int32_t n_probs,
                                const double *probs, double *out, int32_t *passes_out) {
  RSF_ENTER(c, NEED_NOTHING, series && std2 && probs && out, "NULL argument");
  int rc;
  if ((rc = check_series_shape(__func__, n, nout))) return rc;
  if (n_probs < 1 || n_probs > RSF_PREDICT_MAX_PROBS)
    return fail(RSF_ERR_INVALID, "rsf_predict_noise_quantiles: n_probs outside 1..%d", RSF_PREDICT_MAX_PROBS);
  static_assert(kNoiseMaxProbs == RSF_PREDICT_MAX_PROBS && kNoiseMaxPasses == RSF_PREDICT_NOISE_MAX_PASSES,
                "csrc/rsf_predict_noise.h and include/rsf_predict_noise.h agree");
  for (int i = 0; i < n_probs; ++i)
    if (!(probs[i] > 0.0 && probs[i] < 1.0))
      return fail(RSF_ERR_INVALID, "rsf_predict_noise_quantiles: probs[%d] is not strictly inside (0, 1)", i);
  const size_t nb = (size_t)n * sizeof(double);
  const double *ds, *dstd2;
  // (the largest allocation first: it fails before anything is copied)
  if ((rc = stage_series(c, __func__, SLOT_SERIES, series, n, nout, &ds))) return rc;
  if ((rc = stage_in(c, SLOT_STD2, std2, nb, &dstd2))) return rc;
  // workspace: the draws' constants [2][n] and the std2 flag in c->predict; out [n_probs][nout], then the passes [nout], in c->poolws
  const size_t ob = (size_t)n_probs * (size_t)nout * sizeof(double), pb = (size_t)nout * sizeof(int32_t);
  if ((rc = ensure(c->predict, 2 * nb + sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c->poolws, ob + pb))) return rc;
  NoiseArgs A{};
  A.n = n; A.nout = nout; A.series = ds; A.par = (const double *)c->predict.p; A.bad = (const uint32_t *)((const char *)c->predict.p + 2 * nb);
  A.out = (double *)c->poolws.p; A.passes = (int32_t *)((char *)c->poolws.p + ob); A.nprobs = n_probs;
  std::copy(probs, probs + n_probs, A.p);
  HIP_TRY(hipMemsetAsync((void *)A.bad, 0, sizeof(uint32_t), c->stream));
  if ((rc = launch(c, noise_params_kernel, (unsigned)((n + 255) / 256), 256, 0, n, dstd2, (double *)c->predict.p, (uint32_t *)A.bad))) return rc;
  // the row kernel unrolls its loops over the targets: few probabilities take the short one (a target's arithmetic is the same in both)
  if ((rc = launch(c, n_probs <= 4 ? noise_quantile_row_kernel<4> : noise_quantile_row_kernel<kNoiseMaxProbs>, (unsigned)nout, kNoiseThreads, 0, A))) return rc;
  HIP_TRY(hipMemcpyAsync(out, A.out, ob, hipMemcpyDeviceToHost, c->stream));
  if (passes_out) HIP_TRY(hipMemcpyAsync(passes_out, A.passes, pb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RSF_OK;
}

}  // extern "C"
