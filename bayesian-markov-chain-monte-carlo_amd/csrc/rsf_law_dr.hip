// rsf_law_dr.hip — the delayed-rejection sampler under either state law and any observable (include/rsf_law_dr.h):
// rsf_law_dr_run / rsf_law_dr_ssq (kernels: rsf_kernels_law_dr.h; the argument checks are rsf_dr.hip's: rsf_dr_host.h).
#include <cmath>

#include "rsf_dr_host.h"
#include "rsf_kernels_law_dr.h"

using namespace rsfk;
using namespace rsfh;

namespace {

template <class F> auto law_dr_fn(const rsf_ctx *c, int d, int law, F pick) {
  return with<1, 3>(d, [&](auto D) {
    return with<RSF_LAW_SLIP, RSF_LAW_AGEING>(law, [&](auto LAW) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return pick(D, LAW, DAMP); }); });
  });
}
auto run_fn(const rsf_ctx *c, int d, int law) {
  return law_dr_fn(c, d, law, [](auto D, auto LAW, auto DAMP) { return law_dr_kernel<D, LAW, DAMP>; });
}
auto ssq_fn(const rsf_ctx *c, int d, int law) {
  return law_dr_fn(c, d, law, [](auto D, auto LAW, auto DAMP) { return law_dr_ssq_kernel<D, LAW, DAMP>; });
}

}  // namespace

extern "C" {

int rsf_law_dr_run(rsf_ctx *c, int32_t law, int32_t observable, int64_t n, int32_t d, double *q, double *l, const double *data, int32_t n_groups,
                   const double *lo, const double *hi, const double *chol, double gamma, int32_t stages, double shape, uint64_t seed, int64_t offset,
                   int64_t iter0, int32_t n_iter, int32_t *accepted1, int32_t *accepted2, int32_t *outbox1, int32_t *outbox2, int32_t *stuck,
                   double *trace_q, double *trace_l) {
  RSF_ENTER(c, NEED_MODEL, q && l && data && lo && hi && chol && accepted1 && accepted2 && outbox1 && outbox2 && stuck, "NULL argument");
  int rc;
  if ((rc = check_law(__func__, law, observable))) return rc;
  if (n_iter < 1 || n_iter > RSF_DR_MAX_ITER) return fail(RSF_ERR_INVALID, "rsf_law_dr_run: need 1 <= n_iter <= %d", RSF_DR_MAX_ITER);
  if (!trace_q != !trace_l) return fail(RSF_ERR_INVALID, "rsf_law_dr_run: trace_q and trace_l are both NULL or both given");
  if (stages != 1 && stages != 2) return fail(RSF_ERR_INVALID, "rsf_law_dr_run: stages is 1 or 2");
  if (!good_gamma(gamma) || !std::isfinite(shape) || !(shape > 0.0))
    return fail(RSF_ERR_INVALID, "rsf_law_dr_run: gamma must lie in (0, 1], shape be finite and > 0");
  DrArgs A{};
  if ((rc = set_chains(__func__, c, n, d, true, n_groups, lo, hi, seed, offset, iter0, n_iter, A))) return rc;
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_law_dr_run: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  if ((rc = set_factors(__func__, c, d, n_groups, chol, A))) return rc;
  A.gamma = gamma; A.shape = shape; A.stages = stages; A.n_iter = n_iter;
  const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int32_t);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, true), il = s.add(l, nb, true, true);
  const int idata = s.add(data, (size_t)n_groups * c->nout * sizeof(double), true, false);
  const int ia1 = s.add(accepted1, ni, true, true), ia2 = s.add(accepted2, ni, true, true), io1 = s.add(outbox1, ni, true, true);
  const int io2 = s.add(outbox2, ni, true, true), ist = s.add(stuck, ni, true, true);
  const int itq = trace_q ? s.add(trace_q, nb * d * n_iter, false, true) : -1, itl = trace_q ? s.add(trace_l, nb * n_iter, false, true) : -1;
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.l = s.dev<double>(il);
  A.accepted1 = s.dev<int32_t>(ia1); A.accepted2 = s.dev<int32_t>(ia2); A.outbox1 = s.dev<int32_t>(io1); A.outbox2 = s.dev<int32_t>(io2);
  A.stuck = s.dev<int32_t>(ist);
  if (trace_q) { A.tq = s.dev<double>(itq); A.tl = s.dev<double>(itl); }
  // the shared chunking of the float64 tables (c->kc, c->lds_bytes), as rsf_law_observe
  if ((rc = launch(c, run_fn(c, d, law), grid_for(c, n), c->block, c->lds_bytes, make_consts(c, s.dev<const double>(idata)), A, observable))) return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_law_dr_ssq(rsf_ctx *c, int32_t law, int32_t observable, int64_t n, int32_t d, const double *y, const uint8_t *mask, const double *data,
                   int32_t n_groups, double *ssq) {
  RSF_ENTER(c, NEED_MODEL, y && mask && data && ssq, "NULL argument");
  const double box[2][RSF_DR_MAX_PARAMS] = {{0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}};  // the solve takes no box
  int rc;
  if ((rc = check_law(__func__, law, observable))) return rc;
  DrArgs A{};
  if ((rc = set_chains(__func__, c, n, d, true, n_groups, box[0], box[1], 0, 0, 1, 1, A))) return rc;
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_law_dr_ssq: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  const size_t nb = (size_t)n * sizeof(double);
  Staged s(c);
  const int iy = s.add(y, nb * d, true, false), im = s.add(mask, (size_t)n, true, false);
  const int idata = s.add(data, (size_t)n_groups * c->nout * sizeof(double), true, false), is = s.add(ssq, nb, true, true);
  if ((rc = s.commit())) return rc;
  if ((rc = launch(c, ssq_fn(c, d, law), grid_for(c, n), c->block, c->lds_bytes, make_consts(c, s.dev<const double>(idata)), A, observable,
                   s.dev<const double>(iy), s.dev<const uint8_t>(im), s.dev<double>(is))))
    return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

}  // extern "C"
