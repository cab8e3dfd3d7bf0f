// rsf_law_fit.hip — multi-start Levenberg-Marquardt least squares under either state law and any observable
// (include/rsf_law_fit.h): rsf_law_fit_normal / rsf_law_fit_run (kernels: rsf_kernels_law_fit.h; the argument checks are
// rsf_fit.hip's: rsf_fit_host.h).
#include <cmath>

#include "rsf_fit_host.h"
#include "rsf_kernels_law_fit.h"

using namespace rsfk;
using namespace rsfh;

namespace {

template <class F> auto law_fit_fn(const rsf_ctx *c, int d, int law, F pick) {
  return with<1, 3>(d, [&](auto D) {
    return with<RSF_LAW_SLIP, RSF_LAW_AGEING>(law, [&](auto LAW) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return pick(D, LAW, DAMP); }); });
  });
}
auto normal_fn(const rsf_ctx *c, int d, int law) {
  return law_fit_fn(c, d, law, [](auto D, auto LAW, auto DAMP) { return law_fit_normal_kernel<D, LAW, DAMP>; });
}
auto run_fn(const rsf_ctx *c, int d, int law) {
  return law_fit_fn(c, d, law, [](auto D, auto LAW, auto DAMP) { return law_fit_kernel<D, LAW, DAMP>; });
}

// the law and the observable of a call: rsf_law_observe's checks and messages under the caller's name
int check_law(const char *fn, int32_t law, int32_t observable) {
  if (law != RSF_LAW_AGEING && law != RSF_LAW_SLIP) return fail(RSF_ERR_INVALID, "%s: law is RSF_LAW_AGEING (0) or RSF_LAW_SLIP (1), not %d", fn, law);
  if (observable != RSF_OBS_ACC && observable != RSF_OBS_MU && observable != RSF_OBS_THETA && observable != RSF_OBS_VELOCITY)
    return fail(RSF_ERR_INVALID, "%s: observable is RSF_OBS_ACC (0), RSF_OBS_MU (1), RSF_OBS_THETA (2) or RSF_OBS_VELOCITY (3), not %d", fn, observable);
  return RSF_OK;
}

}  // namespace

extern "C" {

int rsf_law_fit_normal(rsf_ctx *c, int32_t law, int32_t observable, int64_t n, int32_t d, const double *q, const double *data, int32_t n_groups,
                       double fd, double *ssq, double *grad, double *jtj) {
  RSF_ENTER(c, NEED_MODEL, q && data && ssq && grad && jtj, "NULL argument");
  int rc;
  if ((rc = check_law(__func__, law, observable))) return rc;
  FitArgs A{};
  if ((rc = set_solve(__func__, c, n, d, n_groups, fd, A))) return rc;
  const size_t nb = (size_t)n * sizeof(double);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, false), idata = s.add(data, (size_t)n_groups * c->nout * sizeof(double), true, false);
  const int issq = s.add(ssq, nb, false, true), ig = s.add(grad, nb * d, false, true), ih = s.add(jtj, nb * d * d, false, true);
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.ssq = s.dev<double>(issq); A.grad = s.dev<double>(ig); A.jtj = s.dev<double>(ih);
  // one lane per TRAJECTORY: 1 + d adjacent lanes per start, the shared chunking of the float64 tables (c->kc, c->lds_bytes)
  if ((rc = launch(c, normal_fn(c, d, law), grid_for(c, n * (d + 1)), c->block, c->lds_bytes, make_consts(c, s.dev<const double>(idata)), A, observable)))
    return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_law_fit_run(rsf_ctx *c, int32_t law, int32_t observable, int64_t n, int32_t d, double *q, const double *data, int32_t n_groups,
                    const double *lo, const double *hi, double fd, double ftol, int32_t n_iter, double *ssq, double *grad, double *jtj, double *lam,
                    int32_t *status, int32_t *iters) {
  RSF_ENTER(c, NEED_MODEL, q && data && lo && hi && ssq && grad && jtj && lam && status && iters, "NULL argument");
  int rc;
  if ((rc = check_law(__func__, law, observable))) return rc;
  FitArgs A{};
  if ((rc = set_solve(__func__, c, n, d, n_groups, fd, A))) return rc;
  if ((rc = set_run(__func__, n_iter, ftol, A))) return rc;
  if ((rc = set_box(__func__, d, lo, hi, A))) return rc;
  const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int32_t);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, true), idata = s.add(data, (size_t)n_groups * c->nout * sizeof(double), true, false);
  const int issq = s.add(ssq, nb, true, true), ig = s.add(grad, nb * d, true, true), ih = s.add(jtj, nb * d * d, true, true);
  const int il = s.add(lam, nb, true, true), ist = s.add(status, ni, true, true), iit = s.add(iters, ni, true, true);
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.ssq = s.dev<double>(issq); A.grad = s.dev<double>(ig); A.jtj = s.dev<double>(ih); A.lam = s.dev<double>(il);
  A.status = s.dev<int32_t>(ist); A.iters = s.dev<int32_t>(iit);
  if ((rc = launch(c, run_fn(c, d, law), grid_for(c, n * (d + 1)), c->block, c->lds_bytes, make_consts(c, s.dev<const double>(idata)), A, observable)))
    return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

}  // extern "C"
