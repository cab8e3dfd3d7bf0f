// rsf_law_predict.hip — the posterior predictive checks under either state law and any observable, and the partials of a series
// that already exists (include/rsf_law_predict.h): rsf_law_predict_partials / rsf_predict_series_partials (kernels:
// rsf_kernels_law_predict.h).  The workspace, the two levels of the partials' sum and the partials' layout are
// rsf_predict_partials' (rsf_predict.hip); rsf_predict_finish (rsf_finish.cpp) finishes them.
#include <climits>
#include <algorithm>
#include <vector>

#include "rsf_host.h"
#include "rsf_kernels_law_predict.h"

using namespace rsfk;
using namespace rsfh;

namespace {

auto law_predict_fn(const rsf_ctx *c, int d, int law, bool want_series) {  // void (*)(Consts, PredictArgs, int32_t)
  return with<1, 3>(d, [&](auto D) {
    return with<RSF_LAW_SLIP, RSF_LAW_AGEING>(law, [&](auto LAW) {
      return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) {
        return with<true, false>(want_series, [&](auto SERIES) { return law_predict_kernel<D, LAW, DAMP, SERIES>; });
      });
    });
  });
}

// The per-wave fields in c->predict summed and copied out.  Workspace, doubles: per-wave partials[nwaves][nf] | slab sums[nslabs][nf] |
// sums[nf] | center_y[nout] | center_l[nout] — rsf_predict_partials' layout, its two levels (kPredSlab waves, then the slabs) and
// its head.
struct Workspace {
  int64_t nout, grid, nwaves, nslabs, nf, o_slab, o_sum, o_cy, o_cl, total;
  double *w = nullptr;
  Workspace(const rsf_ctx *c, int64_t n, int64_t nout_) : nout(nout_) {
    const int wpb = c->block / 64;
    grid = (n + c->block - 1) / c->block;
    nwaves = grid * wpb;
    nslabs = (nwaves + kPredSlab - 1) / kPredSlab;
    nf = nout * kPredFields;
    o_slab = nwaves * nf; o_sum = o_slab + nslabs * nf; o_cy = o_sum + nf; o_cl = o_cy + nout; total = o_cl + nout;
  }
  int centres(rsf_ctx *c, const double *center_y, const double *center_l) {
    if (int rc = ensure(c->predict, (size_t)total * sizeof(double))) return rc;
    w = (double *)c->predict.p;
    HIP_TRY(hipMemcpyAsync(w + o_cy, center_y, (size_t)nout * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(w + o_cl, center_l, (size_t)nout * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return RSF_OK;
  }
  // (the series of an RSF_MEM_HOST caller is copied back between the sums and the synchronise: series_out NULL = none)
  int finish(rsf_ctx *c, int64_t n, double *partials, double *series_out) {
    int rc;
    if ((rc = sum_in_order(c, nwaves, kPredSlab, nf, w, 1.0, w + o_slab))) return rc;
    if ((rc = sum_in_order(c, nslabs, nslabs, nf, w + o_slab, 1.0, w + o_sum))) return rc;
    std::vector<double> h((size_t)nf);
    HIP_TRY(hipMemcpyAsync(h.data(), w + o_sum, (size_t)nf * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if ((rc = copy_back(c, SLOT_SERIES, series_out, (size_t)n * sizeof(double) * (size_t)nout))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    partials[0] = (double)n;
    partials[1] = h[kPredFields - 1];  // sum of sigma^2: the same in every row, taken from row 0
    for (int64_t k = 0; k < nout; ++k)
      for (int f = 0; f < RSF_PREDICT_FIELDS; ++f) partials[RSF_PREDICT_HEAD + k * RSF_PREDICT_FIELDS + f] = h[(size_t)(k * kPredFields + f)];
    return RSF_OK;
  }
};

}  // namespace

extern "C" {

int rsf_law_predict_partials(rsf_ctx *c, int32_t law, int32_t observable, int64_t n, int32_t d, const double *q, const double *std2,
                             const double *data, const double *center_y, const double *center_l, double *partials, double *series_out) {
  RSF_ENTER(c, NEED_MODEL, q && std2 && data && center_y && center_l && partials, "NULL argument");
  if (law != RSF_LAW_AGEING && law != RSF_LAW_SLIP)
    return fail(RSF_ERR_INVALID, "rsf_law_predict_partials: law is RSF_LAW_AGEING (0) or RSF_LAW_SLIP (1), not %d", law);
  if (observable != RSF_OBS_ACC && observable != RSF_OBS_MU && observable != RSF_OBS_THETA && observable != RSF_OBS_VELOCITY)
    return fail(RSF_ERR_INVALID, "rsf_law_predict_partials: observable is RSF_OBS_ACC (0), RSF_OBS_MU (1), RSF_OBS_THETA (2) or RSF_OBS_VELOCITY (3), not %d",
                observable);
  if (n < 1 || (d != 1 && d != 3)) return fail(RSF_ERR_INVALID, "rsf_law_predict_partials: need n >= 1 and d = 1 or 3");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_law_predict_partials: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  const int64_t nout = c->nout;
  const int S = c->m.substeps, wpb = c->block / 64;
  Workspace W(c, n, nout);
  if (W.nslabs > 65535 || n > INT64_MAX / 64 / nout) return fail(RSF_ERR_INVALID, "rsf_law_predict_partials: too many draws for one call; split the pool into shards");
  // the kernel's own chunking of the loading table, rsf_predict_partials': its waves' tiles share LDS with the chunk (kPredTableBudget)
  const int64_t kc = std::min<int64_t>(((int64_t)(kPredTableBudget / sizeof(double)) - 1) / (2 * (int64_t)S), nout - 1);
  if (kc < 1) return fail(RSF_ERR_UNSUPPORTED, "rsf_law_predict_partials: substeps=%d does not fit the LDS staging budget", S);
  int rc;
  const size_t nb = (size_t)n * sizeof(double), rowb = (size_t)nout * sizeof(double);
  const double *dq, *dstd2, *ddata;
  double *dser = nullptr;
  // (the largest allocation first: it fails before anything is copied)
  if (series_out && stage_out(c, SLOT_SERIES, series_out, nb * (size_t)nout, &dser)) {
    (void)hipGetLastError();
    return fail(RSF_ERR_NOMEM, "rsf_law_predict_partials: cannot allocate the series' device copy (%lld x %lld doubles); pass fewer draws per call",
                (long long)nout, (long long)n);
  }
  if ((rc = stage_in(c, SLOT_Q, q, nb * d, &dq))) return rc;
  if ((rc = stage_in(c, SLOT_STD2, std2, nb, &dstd2))) return rc;
  if ((rc = stage_in(c, SLOT_OBS, data, rowb, &ddata))) return rc;
  if ((rc = W.centres(c, center_y, center_l))) return rc;
  Consts K = make_consts(c, nullptr);
  K.kc = (int32_t)kc;
  K.nchunks = (int32_t)((nout - 1 + kc - 1) / kc);
  PredictArgs A{};
  A.n = n; A.q = dq; A.std2 = dstd2; A.data = ddata; A.cy = W.w + W.o_cy; A.cl = W.w + W.o_cl; A.part = W.w; A.series = dser;
  A.tab_doubles = (int32_t)((2 * S * kc + 1 + 1) & ~(int64_t)1);
  const size_t lds = ((size_t)A.tab_doubles + (size_t)wpb * kPredWaveDoubles) * sizeof(double);
  if ((rc = launch(c, law_predict_fn(c, d, law, dser != nullptr), (unsigned)W.grid, c->block, lds, K, A, observable))) return rc;
  return W.finish(c, n, partials, series_out);
}

int rsf_predict_series_partials(rsf_ctx *c, int64_t n, int64_t nout, const double *series, const double *std2, const double *data,
                                const double *center_y, const double *center_l, double *partials) {
  RSF_ENTER(c, NEED_NOTHING, series && std2 && data && center_y && center_l && partials, "NULL argument");
  if (n < 1 || n >= (INT64_C(1) << 31) || nout < 1 || nout > INT32_MAX / kPredFields || n > INT64_MAX / 64 / nout)
    return fail(RSF_ERR_INVALID, "rsf_predict_series_partials: need 1 <= n < 2^31 draws and 1 <= nout rows");
  Workspace W(c, n, nout);
  if (W.nslabs > 65535) return fail(RSF_ERR_INVALID, "rsf_predict_series_partials: too many draws for one call; split the pool into shards");
  int rc;
  const size_t nb = (size_t)n * sizeof(double), rowb = (size_t)nout * sizeof(double);
  const double *ds, *dstd2, *ddata;
  // (the largest allocation first: it fails before anything is copied)
  if (stage_in(c, SLOT_SERIES, series, nb * (size_t)nout, &ds)) {
    (void)hipGetLastError();
    return fail(RSF_ERR_NOMEM, "rsf_predict_series_partials: cannot allocate the series' device copy (%lld x %lld doubles)", (long long)nout, (long long)n);
  }
  if ((rc = stage_in(c, SLOT_STD2, std2, nb, &dstd2))) return rc;
  if ((rc = stage_in(c, SLOT_OBS, data, rowb, &ddata))) return rc;
  if ((rc = W.centres(c, center_y, center_l))) return rc;
  PredictArgs A{};
  A.n = n; A.std2 = dstd2; A.data = ddata; A.cy = W.w + W.o_cy; A.cl = W.w + W.o_cl; A.part = W.w; A.series = const_cast<double *>(ds);
  A.tab_doubles = 0;
  const size_t lds = (size_t)(c->block / 64) * kPredWaveDoubles * sizeof(double);
  if ((rc = launch(c, series_partials_kernel, (unsigned)W.grid, c->block, lds, A, (int32_t)nout))) return rc;
  return W.finish(c, n, partials, nullptr);
}

}  // extern "C"
