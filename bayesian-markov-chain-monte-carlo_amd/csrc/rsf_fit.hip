// rsf_fit.hip — multi-start Levenberg-Marquardt least squares (include/rsf_fit.h): rsf_fit_normal / _run / _trial / _decide
// (kernels: rsf_kernels_fit.h; the argument checks shared with rsf_law_fit.hip: rsf_fit_host.h).  rsf_fit_laplace, the host arithmetic, is in rsf_finish.cpp.
#include <cmath>

#include "rsf_fit_host.h"

using namespace rsfk;
using namespace rsfh;

namespace {

auto normal_fn(const rsf_ctx *c, int d) {
  return with<1, 3>(d, [&](auto D) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return fit_normal_kernel<D, DAMP>; }); });
}
auto run_fn(const rsf_ctx *c, int d) {
  return with<1, 3>(d, [&](auto D) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return fit_kernel<D, DAMP>; }); });
}
auto trial_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return fit_trial_kernel<D>; }); }
auto decide_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return fit_decide_kernel<D>; }); }

}  // namespace

extern "C" {

int rsf_fit_normal(rsf_ctx *c, int64_t n, int32_t d, const double *q, const double *data, int32_t n_groups, double fd, double *ssq,
                   double *grad, double *jtj) {
  RSF_ENTER(c, NEED_MODEL, q && data && ssq && grad && jtj, "NULL argument");
  int rc;
  FitArgs A{};
  if ((rc = set_solve(__func__, c, n, d, n_groups, fd, A))) return rc;
  const size_t nb = (size_t)n * sizeof(double);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, false), idata = s.add(data, (size_t)n_groups * c->nout * sizeof(double), true, false);
  const int issq = s.add(ssq, nb, false, true), ig = s.add(grad, nb * d, false, true), ih = s.add(jtj, nb * d * d, false, true);
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.ssq = s.dev<double>(issq); A.grad = s.dev<double>(ig); A.jtj = s.dev<double>(ih);
  // one lane per TRAJECTORY: 1 + d adjacent lanes per start, the shared chunking of the float64 tables (c->kc, c->lds_bytes)
  if ((rc = launch(c, normal_fn(c, d), grid_for(c, n * (d + 1)), c->block, c->lds_bytes, make_consts(c, s.dev<const double>(idata)), A))) return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_fit_run(rsf_ctx *c, int64_t n, int32_t d, double *q, const double *data, int32_t n_groups, const double *lo, const double *hi,
                double fd, double ftol, int32_t n_iter, double *ssq, double *grad, double *jtj, double *lam, int32_t *status,
                int32_t *iters) {
  RSF_ENTER(c, NEED_MODEL, q && data && lo && hi && ssq && grad && jtj && lam && status && iters, "NULL argument");
  int rc;
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
  if ((rc = launch(c, run_fn(c, d), grid_for(c, n * (d + 1)), c->block, c->lds_bytes, make_consts(c, s.dev<const double>(idata)), A))) return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_fit_trial(rsf_ctx *c, int64_t n, int32_t d, const double *q, const double *grad, const double *jtj, const double *lam,
                  const double *lo, const double *hi, const int32_t *status, double *q_trial, uint8_t *ok) {
  RSF_ENTER(c, NEED_NOTHING, q && grad && jtj && lam && lo && hi && status && q_trial && ok, "NULL argument");
  if (n < 1 || d < 1 || d > RSF_FIT_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_fit_trial: need n >= 1 and 1 <= d <= %d", RSF_FIT_MAX_PARAMS);
  int rc;
  FitArgs A{};
  if ((rc = set_box(__func__, d, lo, hi, A))) return rc;
  A.n = n;
  const size_t nb = (size_t)n * sizeof(double);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, false), ig = s.add(grad, nb * d, true, false), ih = s.add(jtj, nb * d * d, true, false);
  const int il = s.add(lam, nb, true, false), ist = s.add(status, (size_t)n * sizeof(int32_t), true, false);
  const int iqt = s.add(q_trial, nb * d, false, true), iok = s.add(ok, (size_t)n, false, true);
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.grad = s.dev<double>(ig); A.jtj = s.dev<double>(ih); A.lam = s.dev<double>(il); A.status = s.dev<int32_t>(ist);
  if ((rc = launch(c, trial_fn(d), blocks_of(n), kMaxBlock, 0, A, s.dev<double>(iqt), s.dev<uint8_t>(iok)))) return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_fit_decide(rsf_ctx *c, int64_t n, int32_t d, double *q, double *ssq, double *grad, double *jtj, double *lam, int32_t *status,
                   int32_t *iters, const double *q_trial, const uint8_t *ok, const double *ssq_new, const double *grad_new,
                   const double *jtj_new, double ftol) {
  RSF_ENTER(c, NEED_NOTHING, q && ssq && grad && jtj && lam && status && iters && q_trial && ok && ssq_new && grad_new && jtj_new, "NULL argument");
  if (n < 1 || d < 1 || d > RSF_FIT_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_fit_decide: need n >= 1 and 1 <= d <= %d", RSF_FIT_MAX_PARAMS);
  if (!std::isfinite(ftol) || ftol < 0.0) return fail(RSF_ERR_INVALID, "rsf_fit_decide: ftol must be finite and >= 0");
  int rc;
  FitArgs A{};
  A.n = n; A.ftol = ftol;
  const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int32_t);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, true), issq = s.add(ssq, nb, true, true), ig = s.add(grad, nb * d, true, true);
  const int ih = s.add(jtj, nb * d * d, true, true), il = s.add(lam, nb, true, true), ist = s.add(status, ni, true, true);
  const int iit = s.add(iters, ni, true, true), iqt = s.add(q_trial, nb * d, true, false), iok = s.add(ok, (size_t)n, true, false);
  const int isn = s.add(ssq_new, nb, true, false), ign = s.add(grad_new, nb * d, true, false), ihn = s.add(jtj_new, nb * d * d, true, false);
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.ssq = s.dev<double>(issq); A.grad = s.dev<double>(ig); A.jtj = s.dev<double>(ih); A.lam = s.dev<double>(il);
  A.status = s.dev<int32_t>(ist); A.iters = s.dev<int32_t>(iit);
  if ((rc = launch(c, decide_fn(d), blocks_of(n), kMaxBlock, 0, A, s.dev<const double>(iqt), s.dev<const uint8_t>(iok), s.dev<const double>(isn),
                   s.dev<const double>(ign), s.dev<const double>(ihn))))
    return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

}  // extern "C"
