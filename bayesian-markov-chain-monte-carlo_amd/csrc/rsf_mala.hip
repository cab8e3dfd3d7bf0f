// rsf_mala.hip — Gauss-Newton manifold MALA (include/rsf_mala.h): rsf_mala_run / _propose / _accept (kernels: rsf_kernels_mala.h).
#include <cmath>

#include "rsf_host.h"
#include "rsf_kernels_mala.h"

using namespace rsfk;
using namespace rsfh;

namespace {

// what the three calls share: the shape, the box, the sampler's constants and the Philox stream; iterations first .. first + count - 1
int set_chain(const char *fn, int64_t n, int32_t d, bool solve, const double *lo, const double *hi, double eps, double lam, double shape,
              uint64_t seed, int64_t offset, int64_t first, int64_t count, MalaArgs &A) {
  if (n < 1 || (solve ? (d != 1 && d != 3) : (d < 1 || d > RSF_MALA_MAX_PARAMS)))
    return fail(RSF_ERR_INVALID, "%s: need n >= 1 and %s", fn, solve ? "d = 1 or 3" : "1 <= d <= 3");
  if (!std::isfinite(eps) || !(eps > 0.0) || !std::isfinite(shape) || !(shape > 0.0)) return fail(RSF_ERR_INVALID, "%s: eps and shape must be finite and > 0", fn);
  if (!std::isfinite(lam) || lam < 0.0) return fail(RSF_ERR_INVALID, "%s: lam must be finite and >= 0", fn);
  if (offset < 0) return fail(RSF_ERR_INVALID, "%s: offset must be >= 0", fn);
  if (first < 1 || first + count > ((int64_t)1 << 32)) return fail(RSF_ERR_INVALID, "%s: the Philox iterations must lie in 1 .. 2^32 - 1", fn);
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p])) return fail(RSF_ERR_INVALID, "%s: need finite lo[%d] < hi[%d]", fn, p, p);
    A.lo[p] = lo[p]; A.hi[p] = hi[p];
  }
  A.n = n; A.offset = offset; A.seed = seed; A.iter = (uint32_t)first;
  A.eps = eps; A.lam = lam; A.shape = shape;
  return RSF_OK;
}

auto run_fn(const rsf_ctx *c, int d) {
  return with<1, 3>(d, [&](auto D) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return mala_kernel<D, DAMP>; }); });
}
auto propose_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return mala_propose_kernel<D>; }); }
auto accept_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return mala_accept_kernel<D>; }); }

}  // namespace

extern "C" {

int rsf_mala_run(rsf_ctx *c, int64_t n, int32_t d, double *q, double *ssq, double *grad, double *jtj, const double *data, int32_t n_groups,
                 const double *lo, const double *hi, double fd, double eps, double lam, double shape, uint64_t seed, int64_t offset,
                 int64_t iter0, int32_t n_iter, int32_t *accepted, int32_t *outbox, int32_t *stuck, double *trace_q, double *trace_ssq) {
  RSF_ENTER(c, NEED_MODEL, q && ssq && grad && jtj && data && lo && hi && accepted && outbox && stuck, "NULL argument");
  if (n_iter < 1 || n_iter > RSF_MALA_MAX_ITER) return fail(RSF_ERR_INVALID, "rsf_mala_run: need 1 <= n_iter <= %d", RSF_MALA_MAX_ITER);
  if (!trace_q != !trace_ssq) return fail(RSF_ERR_INVALID, "rsf_mala_run: trace_q and trace_ssq are both NULL or both given");
  int rc;
  MalaArgs A{};
  if ((rc = set_chain(__func__, n, d, true, lo, hi, eps, lam, shape, seed, offset, iter0, n_iter, A))) return rc;
  if (!std::isfinite(fd) || !(fd > 0.0)) return fail(RSF_ERR_INVALID, "rsf_mala_run: fd must be finite and > 0");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_mala_run: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  // a workgroup's chains share one observation series: rsf_fit_normal's rule
  if (n_groups < 1 || n % n_groups || (n_groups > 1 && (n / n_groups) % c->block))
    return fail(RSF_ERR_INVALID, "rsf_mala_run: need n_groups >= 1 and, with more than one, n/n_groups a whole multiple of a workgroup's threads (%d)", c->block);
  A.fd = fd; A.n_iter = n_iter;
  A.group_chains = n_groups > 1 ? n / n_groups : 0;
  const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int32_t);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, true), issq = s.add(ssq, nb, true, true), ig = s.add(grad, nb * d, true, true);
  const int ih = s.add(jtj, nb * d * d, true, true), idata = s.add(data, (size_t)n_groups * c->nout * sizeof(double), true, false);
  const int ia = s.add(accepted, ni, true, true), io = s.add(outbox, ni, true, true), ist = s.add(stuck, ni, true, true);
  const int itq = trace_q ? s.add(trace_q, nb * d * n_iter, false, true) : -1, its = trace_q ? s.add(trace_ssq, nb * n_iter, false, true) : -1;
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.ssq = s.dev<double>(issq); A.grad = s.dev<double>(ig); A.jtj = s.dev<double>(ih);
  A.accepted = s.dev<int32_t>(ia); A.outbox = s.dev<int32_t>(io); A.stuck = s.dev<int32_t>(ist);
  if (trace_q) { A.tq = s.dev<double>(itq); A.ts = s.dev<double>(its); }
  // one lane per TRAJECTORY, as rsf_fit_run: 1 + d adjacent lanes per chain
  if ((rc = launch(c, run_fn(c, d), grid_for(c, n * (d + 1)), c->block, c->lds_bytes, make_consts(c, s.dev<const double>(idata)), A))) return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_mala_propose(rsf_ctx *c, int64_t n, int32_t d, const double *q, const double *ssq, const double *grad, const double *jtj, const double *lo,
                     const double *hi, double eps, double lam, double shape, uint64_t seed, int64_t offset, int64_t iter, double *q_new,
                     uint8_t *inbox, uint8_t *stuck) {
  RSF_ENTER(c, NEED_NOTHING, q && ssq && grad && jtj && lo && hi && q_new && inbox && stuck, "NULL argument");
  int rc;
  MalaArgs A{};
  if ((rc = set_chain(__func__, n, d, false, lo, hi, eps, lam, shape, seed, offset, iter, 1, A))) return rc;
  const size_t nb = (size_t)n * sizeof(double);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, false), issq = s.add(ssq, nb, true, false), ig = s.add(grad, nb * d, true, false);
  const int ih = s.add(jtj, nb * d * d, true, false), iqn = s.add(q_new, nb * d, false, true), iin = s.add(inbox, (size_t)n, false, true);
  const int ist = s.add(stuck, (size_t)n, false, true);
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.ssq = s.dev<double>(issq); A.grad = s.dev<double>(ig); A.jtj = s.dev<double>(ih);
  if ((rc = launch(c, propose_fn(d), blocks_of(n), kMaxBlock, 0, A, s.dev<double>(iqn), s.dev<uint8_t>(iin), s.dev<uint8_t>(ist)))) return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_mala_accept(rsf_ctx *c, int64_t n, int32_t d, double *q, double *ssq, double *grad, double *jtj, const double *lo, const double *hi,
                    double eps, double lam, double shape, uint64_t seed, int64_t offset, int64_t iter, const double *q_new, const uint8_t *inbox,
                    const double *ssq_new, const double *grad_new, const double *jtj_new, int32_t *accepted, int32_t *outbox, int32_t *stuck) {
  RSF_ENTER(c, NEED_NOTHING, q && ssq && grad && jtj && lo && hi && q_new && inbox && ssq_new && grad_new && jtj_new && accepted && outbox && stuck,
            "NULL argument");
  int rc;
  MalaArgs A{};
  if ((rc = set_chain(__func__, n, d, false, lo, hi, eps, lam, shape, seed, offset, iter, 1, A))) return rc;
  const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int32_t);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, true), issq = s.add(ssq, nb, true, true), ig = s.add(grad, nb * d, true, true);
  const int ih = s.add(jtj, nb * d * d, true, true), iqn = s.add(q_new, nb * d, true, false), iin = s.add(inbox, (size_t)n, true, false);
  const int isn = s.add(ssq_new, nb, true, false), ign = s.add(grad_new, nb * d, true, false), ihn = s.add(jtj_new, nb * d * d, true, false);
  const int ia = s.add(accepted, ni, true, true), io = s.add(outbox, ni, true, true), ist = s.add(stuck, ni, true, true);
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.ssq = s.dev<double>(issq); A.grad = s.dev<double>(ig); A.jtj = s.dev<double>(ih);
  A.accepted = s.dev<int32_t>(ia); A.outbox = s.dev<int32_t>(io); A.stuck = s.dev<int32_t>(ist);
  if ((rc = launch(c, accept_fn(d), blocks_of(n), kMaxBlock, 0, A, s.dev<const double>(iqn), s.dev<const uint8_t>(iin), s.dev<const double>(isn),
                   s.dev<const double>(ign), s.dev<const double>(ihn))))
    return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

}  // extern "C"
