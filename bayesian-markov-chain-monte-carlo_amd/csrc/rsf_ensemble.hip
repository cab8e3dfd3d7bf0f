// rsf_ensemble.hip — the affine-invariant stretch move in island ensembles (include/rsf_ensemble.h): rsf_ensemble_run / _propose /
// _accept / _ssq (kernels: rsf_kernels_ensemble.h).
#include <cmath>

#include "rsf_host.h"
#include "rsf_kernels_ensemble.h"

using namespace rsfk;
using namespace rsfh;

namespace {

// what the three calls share: the islands, the box, the coordinates and the Philox stream; iterations first .. first + count - 1
int set_walkers(const char *fn, const rsf_ctx *c, int64_t n, int32_t d, bool solve, const double *lo, const double *hi, uint32_t logmask,
                uint64_t seed, int64_t offset, int64_t first, int64_t count, EnsArgs &A) {
  if (solve ? (d != 1 && d != 3) : (d < 1 || d > RSF_ENSEMBLE_MAX_PARAMS)) return fail(RSF_ERR_INVALID, "%s: need %s", fn, solve ? "d = 1 or 3" : "1 <= d <= 3");
  if (n < 1 || n % (2 * (int64_t)c->block))
    return fail(RSF_ERR_INVALID, "%s: n must be a whole number of islands of 2 x %d walkers (twice the workgroup's threads)", fn, c->block);
  if (offset < 0) return fail(RSF_ERR_INVALID, "%s: offset must be >= 0", fn);
  if (first < 1 || first + count > ((int64_t)1 << 32)) return fail(RSF_ERR_INVALID, "%s: the Philox iterations must lie in 1 .. 2^32 - 1", fn);
  if (logmask >> d) return fail(RSF_ERR_INVALID, "%s: logmask has a bit at or beyond d = %d", fn, d);
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p])) return fail(RSF_ERR_INVALID, "%s: need finite lo[%d] < hi[%d]", fn, p, p);
    if (((logmask >> p) & 1u) && lo[p] < 0.0) return fail(RSF_ERR_INVALID, "%s: parameter %d moves in log coordinates and needs lo[%d] >= 0", fn, p, p);
    A.lo[p] = lo[p]; A.hi[p] = hi[p];
  }
  A.n = n; A.offset = offset; A.seed = seed; A.iter = (uint32_t)first; A.B = c->block; A.logmask = logmask;
  return RSF_OK;
}

auto run_fn(const rsf_ctx *c, int d) {
  return with<1, 3>(d, [&](auto D) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return ensemble_move_kernel<D, DAMP>; }); });
}
auto ssq_fn(const rsf_ctx *c, int d) {
  return with<1, 3>(d, [&](auto D) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return ensemble_ssq_kernel<D, DAMP>; }); });
}
auto propose_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return ensemble_propose_kernel<D>; }); }
auto accept_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return ensemble_accept_kernel<D>; }); }

}  // namespace

extern "C" {

int rsf_ensemble_run(rsf_ctx *c, int64_t n, int32_t d, double *q, double *l, const double *data, int32_t n_groups, const double *lo, const double *hi,
                     double a, uint32_t logmask, double shape, uint64_t seed, int64_t offset, int64_t iter0, int32_t n_iter, int32_t *accepted,
                     int32_t *outbox, int32_t *stuck, double *trace_q, double *trace_l) {
  RSF_ENTER(c, NEED_MODEL, q && l && data && lo && hi && accepted && outbox && stuck, "NULL argument");
  if (n_iter < 1 || n_iter > RSF_ENSEMBLE_MAX_ITER) return fail(RSF_ERR_INVALID, "rsf_ensemble_run: need 1 <= n_iter <= %d", RSF_ENSEMBLE_MAX_ITER);
  if (!trace_q != !trace_l) return fail(RSF_ERR_INVALID, "rsf_ensemble_run: trace_q and trace_l are both NULL or both given");
  int rc;
  EnsArgs A{};
  if ((rc = set_walkers(__func__, c, n, d, true, lo, hi, logmask, seed, offset, iter0, n_iter, A))) return rc;
  if (!std::isfinite(a) || !(a > 1.0) || !std::isfinite(shape) || !(shape > 0.0))
    return fail(RSF_ERR_INVALID, "rsf_ensemble_run: a must be finite and > 1, shape finite and > 0");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_ensemble_run: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  // an island's walkers share one observation series
  if (n_groups < 1 || n % n_groups || (n / n_groups) % (2 * (int64_t)c->block))
    return fail(RSF_ERR_INVALID, "rsf_ensemble_run: need n_groups >= 1 and n/n_groups a whole number of islands of 2 x %d walkers", c->block);
  A.a = a; A.shape = shape; A.n_iter = n_iter;
  A.group_walkers = n_groups > 1 ? n / n_groups : 0;
  const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int32_t);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, true), il = s.add(l, nb, true, true);
  const int idata = s.add(data, (size_t)n_groups * c->nout * sizeof(double), true, false);
  const int ia = s.add(accepted, ni, true, true), io = s.add(outbox, ni, true, true), ist = s.add(stuck, ni, true, true);
  const int itq = trace_q ? s.add(trace_q, nb * d * n_iter, false, true) : -1, itl = trace_q ? s.add(trace_l, nb * n_iter, false, true) : -1;
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.l = s.dev<double>(il);
  A.accepted = s.dev<int32_t>(ia); A.outbox = s.dev<int32_t>(io); A.stuck = s.dev<int32_t>(ist);
  if (trace_q) { A.tq = s.dev<double>(itq); A.tl = s.dev<double>(itl); }
  // one workgroup per island; behind the shared chunking of the float64 tables (c->kc, c->lds_bytes) the resting half's positions
  const size_t lds = c->lds_bytes + (size_t)c->block * d * sizeof(double);
  if ((rc = launch(c, run_fn(c, d), (unsigned)(n / (2 * (int64_t)c->block)), c->block, lds, make_consts(c, s.dev<const double>(idata)), A))) return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_ensemble_propose(rsf_ctx *c, int64_t n, int32_t d, const double *q, const double *l, const double *lo, const double *hi, double a,
                         uint32_t logmask, uint64_t seed, int64_t offset, int64_t iter, int32_t half, double *q_new, uint8_t *inbox, double *logz_jac) {
  RSF_ENTER(c, NEED_NOTHING, q && l && lo && hi && q_new && inbox && logz_jac, "NULL argument");
  int rc;
  EnsArgs A{};
  if ((rc = set_walkers(__func__, c, n, d, false, lo, hi, logmask, seed, offset, iter, 1, A))) return rc;
  if (!std::isfinite(a) || !(a > 1.0)) return fail(RSF_ERR_INVALID, "rsf_ensemble_propose: a must be finite and > 1");
  if (half != 0 && half != 1) return fail(RSF_ERR_INVALID, "rsf_ensemble_propose: half is 0 or 1");
  A.a = a; A.half = half;
  const size_t nb = (size_t)n * sizeof(double);
  Staged s(c);
  // the outputs' rows of the resting half stay as they are: a host caller's arrays travel both ways
  const int iq = s.add(q, nb * d, true, false), il = s.add(l, nb, true, false), iqn = s.add(q_new, nb * d, true, true);
  const int iin = s.add(inbox, (size_t)n, true, true), ij = s.add(logz_jac, nb, true, true);
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.l = s.dev<double>(il);
  if ((rc = launch(c, propose_fn(d), blocks_of(n / 2), kMaxBlock, 0, A, s.dev<double>(iqn), s.dev<uint8_t>(iin), s.dev<double>(ij)))) return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_ensemble_accept(rsf_ctx *c, int64_t n, int32_t d, double *q, double *l, const double *lo, const double *hi, double shape, uint64_t seed,
                        int64_t offset, int64_t iter, int32_t half, const double *q_new, const uint8_t *inbox, const double *logz_jac,
                        const double *ssq_new, int32_t *accepted, int32_t *outbox, int32_t *stuck) {
  RSF_ENTER(c, NEED_NOTHING, q && l && lo && hi && q_new && inbox && logz_jac && ssq_new && accepted && outbox && stuck, "NULL argument");
  int rc;
  EnsArgs A{};
  if ((rc = set_walkers(__func__, c, n, d, false, lo, hi, 0u, seed, offset, iter, 1, A))) return rc;
  if (!std::isfinite(shape) || !(shape > 0.0)) return fail(RSF_ERR_INVALID, "rsf_ensemble_accept: shape must be finite and > 0");
  if (half != 0 && half != 1) return fail(RSF_ERR_INVALID, "rsf_ensemble_accept: half is 0 or 1");
  A.shape = shape; A.half = half;
  const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int32_t);
  Staged s(c);
  const int iq = s.add(q, nb * d, true, true), il = s.add(l, nb, true, true), iqn = s.add(q_new, nb * d, true, false);
  const int iin = s.add(inbox, (size_t)n, true, false), ij = s.add(logz_jac, nb, true, false), isn = s.add(ssq_new, nb, true, false);
  const int ia = s.add(accepted, ni, true, true), io = s.add(outbox, ni, true, true), ist = s.add(stuck, ni, true, true);
  if ((rc = s.commit())) return rc;
  A.q = s.dev<double>(iq); A.l = s.dev<double>(il);
  A.accepted = s.dev<int32_t>(ia); A.outbox = s.dev<int32_t>(io); A.stuck = s.dev<int32_t>(ist);
  if ((rc = launch(c, accept_fn(d), blocks_of(n / 2), kMaxBlock, 0, A, s.dev<const double>(iqn), s.dev<const uint8_t>(iin), s.dev<const double>(ij),
                   s.dev<const double>(isn))))
    return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

int rsf_ensemble_ssq(rsf_ctx *c, int64_t n, int32_t d, const double *q_new, const uint8_t *inbox, const double *data, int32_t n_groups, int32_t half,
                     double *ssq_new) {
  RSF_ENTER(c, NEED_MODEL, q_new && inbox && data && ssq_new, "NULL argument");
  if (d != 1 && d != 3) return fail(RSF_ERR_INVALID, "rsf_ensemble_ssq: need d = 1 or 3");
  if (n < 1 || n % (2 * (int64_t)c->block))
    return fail(RSF_ERR_INVALID, "rsf_ensemble_ssq: n must be a whole number of islands of 2 x %d walkers (twice the workgroup's threads)", c->block);
  if (half != 0 && half != 1) return fail(RSF_ERR_INVALID, "rsf_ensemble_ssq: half is 0 or 1");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_ensemble_ssq: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  if (n_groups < 1 || n % n_groups || (n / n_groups) % (2 * (int64_t)c->block))
    return fail(RSF_ERR_INVALID, "rsf_ensemble_ssq: need n_groups >= 1 and n/n_groups a whole number of islands of 2 x %d walkers", c->block);
  int rc;
  EnsArgs A{};
  A.n = n; A.B = c->block; A.half = half;
  A.group_walkers = n_groups > 1 ? n / n_groups : 0;
  const size_t nb = (size_t)n * sizeof(double);
  Staged s(c);
  const int iqn = s.add(q_new, nb * d, true, false), iin = s.add(inbox, (size_t)n, true, false);
  const int idata = s.add(data, (size_t)n_groups * c->nout * sizeof(double), true, false), isn = s.add(ssq_new, nb, true, true);
  if ((rc = s.commit())) return rc;
  if ((rc = launch(c, ssq_fn(c, d), (unsigned)(n / (2 * (int64_t)c->block)), c->block, c->lds_bytes, make_consts(c, s.dev<const double>(idata)), A,
                   s.dev<const double>(iqn), s.dev<const uint8_t>(iin), s.dev<double>(isn))))
    return rc;
  if ((rc = s.back())) return rc;
  return finish(c);
}

}  // extern "C"
