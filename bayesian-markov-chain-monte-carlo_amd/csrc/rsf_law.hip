// rsf_law.hip — the caller's loading history and the state law (include/rsf_law.h): rsf_set_loading / rsf_get_loading /
// rsf_loading_size and rsf_law_forward (kernel: rsf_kernels_law.h).
#include <cmath>
#include <vector>

#include "rsf_host.h"
#include "rsf_kernels_law.h"

using namespace rsfk;
using namespace rsfh;

namespace {

// the RK4 table's length: V_l at t_start + j (h / 2), j = 0 .. 2 S (nout - 1)
int64_t table_len(const rsf_ctx *c) { return 2 * (int64_t)c->m.substeps * (c->nout - 1) + 1; }

auto forward_fn(const rsf_ctx *c, int law) {  // void (*)(Consts, int64_t, const double *, const double *, const double *, double *, double *)
  return with<RSF_LAW_SLIP, RSF_LAW_AGEING>(law, [&](auto LAW) {
    return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return law_forward_kernel<LAW, DAMP>; });
  });
}

}  // namespace

extern "C" {

int rsf_loading_size(rsf_ctx *c, int64_t *n) {
  if (!c || !n) return fail(RSF_ERR_INVALID, "rsf_loading_size: NULL argument");
  if (!c->have_model) return fail(RSF_ERR_STATE, "rsf_loading_size: call rsf_set_model first");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_loading_size: a model flagged RSF_FLAG_DOP853 has no table of RK4 stage times");
  *n = table_len(c);
  return RSF_OK;
}

int rsf_set_loading(rsf_ctx *c, const double *vl, int64_t n) {
  RSF_ENTER(c, NEED_MODEL);
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_set_loading: a model flagged RSF_FLAG_DOP853 evaluates the built-in history off the table");
  if (c->m.flags & RSF_FLAG_FP32_SOLVE)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_set_loading: a model flagged RSF_FLAG_FP32_SOLVE runs the built-in history only");
  const int64_t len = table_len(c);
  std::vector<double> builtin;
  if (!vl) {
    builtin.resize((size_t)len);
    builtin_loading(c->m, 0.5 * c->h, builtin.data(), builtin.size());
    vl = builtin.data();
  } else {
    if (n != len) return fail(RSF_ERR_INVALID, "rsf_set_loading: the table has %lld values (2 substeps (nout - 1) + 1), not %lld", (long long)len, (long long)n);
    for (int64_t j = 0; j < len; ++j)
      if (!std::isfinite(vl[j])) return fail(RSF_ERR_INVALID, "rsf_set_loading: vl[%lld] is not finite", (long long)j);
  }
  // the table keeps its size (rsf_set_model allocated it): the copy is ordered on the ctx stream behind every earlier launch
  HIP_TRY(hipMemcpyAsync(c->vl.p, vl, (size_t)len * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's array, or `builtin`, may go away
  set_loading_range(c, vl, (size_t)len);
  if (c->have_chains) free_chains(c);        // chain state (SSq, sigma^2, covariance) belongs to the previous history
  return RSF_OK;
}

int rsf_get_loading(rsf_ctx *c, double *vl, int64_t n) {
  RSF_ENTER(c, NEED_MODEL, vl != nullptr, "NULL argument");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_get_loading: a model flagged RSF_FLAG_DOP853 has no table of RK4 stage times");
  if (n != table_len(c)) return fail(RSF_ERR_INVALID, "rsf_get_loading: the table has %lld values, not %lld", (long long)table_len(c), (long long)n);
  HIP_TRY(hipMemcpyAsync(vl, c->vl.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RSF_OK;
}

int rsf_law_forward(rsf_ctx *c, int32_t law, int64_t n, const double *dc, const double *a, const double *b, const double *data,
                    double *ssq_out, double *acc_out) {
  RSF_ENTER(c, NEED_MODEL, dc && n >= 0, "bad argument");
  int rc;
  if (law != RSF_LAW_AGEING && law != RSF_LAW_SLIP) return fail(RSF_ERR_INVALID, "rsf_law_forward: law is RSF_LAW_AGEING (0) or RSF_LAW_SLIP (1), not %d", law);
  if (ssq_out && !data) return fail(RSF_ERR_INVALID, "rsf_law_forward: ssq_out needs data");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_law_forward: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  if (n == 0 || (!ssq_out && !acc_out)) return RSF_OK;
  const size_t nb = (size_t)n * sizeof(double);
  const double *ddc, *da, *db, *ddata;
  double *dssq, *dacc;
  if ((rc = stage_in(c, SLOT_DC, dc, nb, &ddc))) return rc;
  if ((rc = stage_in(c, SLOT_A, a, nb, &da))) return rc;
  if ((rc = stage_in(c, SLOT_B, b, nb, &db))) return rc;
  if ((rc = stage_in(c, SLOT_DATA, ssq_out ? data : nullptr, (size_t)c->nout * sizeof(double), &ddata))) return rc;
  if ((rc = stage_out(c, SLOT_SSQ_OUT, ssq_out, nb, &dssq))) return rc;
  if ((rc = stage_out(c, SLOT_ACC_OUT, acc_out, nb * (size_t)c->nout, &dacc))) return rc;
  // the shared chunking of the float64 tables (c->kc, c->lds_bytes), as rsf_dr_run's solve
  if ((rc = launch(c, forward_fn(c, law), grid_for(c, n), c->block, c->lds_bytes, make_consts(c, ddata), n, ddc, da, db, dssq, dacc))) return rc;
  if ((rc = copy_back(c, SLOT_SSQ_OUT, ssq_out, nb))) return rc;
  if ((rc = copy_back(c, SLOT_ACC_OUT, acc_out, nb * (size_t)c->nout))) return rc;
  return finish(c);
}

}  // extern "C"
