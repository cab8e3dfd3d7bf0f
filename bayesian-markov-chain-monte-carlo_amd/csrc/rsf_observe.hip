// rsf_observe.hip — the observables of the state-law solve (include/rsf_observe.h): rsf_law_observe (kernel:
// rsf_kernels_observe.h).
#include "rsf_host.h"
#include "rsf_kernels_observe.h"

using namespace rsfk;
using namespace rsfh;

namespace {

auto observe_fn(const rsf_ctx *c, int law) {  // void (*)(Consts, int32_t, int64_t, const double *, const double *, const double *, double *, double *)
  return with<RSF_LAW_SLIP, RSF_LAW_AGEING>(law, [&](auto LAW) {
    return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return law_observe_kernel<LAW, DAMP>; });
  });
}

}  // namespace

extern "C" {

int rsf_law_observe(rsf_ctx *c, int32_t law, int32_t observable, int64_t n, const double *dc, const double *a, const double *b,
                    const double *data, double *ssq_out, double *series_out) {
  RSF_ENTER(c, NEED_MODEL, dc && n >= 0, "bad argument");
  int rc;
  if (law != RSF_LAW_AGEING && law != RSF_LAW_SLIP) return fail(RSF_ERR_INVALID, "rsf_law_observe: law is RSF_LAW_AGEING (0) or RSF_LAW_SLIP (1), not %d", law);
  if (observable != RSF_OBS_ACC && observable != RSF_OBS_MU && observable != RSF_OBS_THETA && observable != RSF_OBS_VELOCITY)
    return fail(RSF_ERR_INVALID, "rsf_law_observe: observable is RSF_OBS_ACC (0), RSF_OBS_MU (1), RSF_OBS_THETA (2) or RSF_OBS_VELOCITY (3), not %d", observable);
  if (ssq_out && !data) return fail(RSF_ERR_INVALID, "rsf_law_observe: ssq_out needs data");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_law_observe: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  if (n == 0 || (!ssq_out && !series_out)) return RSF_OK;
  const size_t nb = (size_t)n * sizeof(double);
  const double *ddc, *da, *db, *ddata;
  double *dssq, *dser;
  if ((rc = stage_in(c, SLOT_DC, dc, nb, &ddc))) return rc;
  if ((rc = stage_in(c, SLOT_A, a, nb, &da))) return rc;
  if ((rc = stage_in(c, SLOT_B, b, nb, &db))) return rc;
  if ((rc = stage_in(c, SLOT_DATA, ssq_out ? data : nullptr, (size_t)c->nout * sizeof(double), &ddata))) return rc;
  if ((rc = stage_out(c, SLOT_SSQ_OUT, ssq_out, nb, &dssq))) return rc;
  if ((rc = stage_out(c, SLOT_ACC_OUT, series_out, nb * (size_t)c->nout, &dser))) return rc;
  // the shared chunking of the float64 tables (c->kc, c->lds_bytes), as rsf_law_forward
  if ((rc = launch(c, observe_fn(c, law), grid_for(c, n), c->block, c->lds_bytes, make_consts(c, ddata), observable, n, ddc, da, db, dssq, dser))) return rc;
  if ((rc = copy_back(c, SLOT_SSQ_OUT, ssq_out, nb))) return rc;
  if ((rc = copy_back(c, SLOT_ACC_OUT, series_out, nb * (size_t)c->nout))) return rc;
  return finish(c);
}

}  // extern "C"
