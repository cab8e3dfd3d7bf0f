// rsf_evidence.hip — the marginal likelihood of the pooled draws by bridge sampling (include/rsf_evidence.h):
// rsf_evidence_propose / _logg / _logtarget / _partials (kernels: rsf_kernels_evidence.h).  rsf_evidence_finish, the host
// arithmetic, is in rsf_finish.cpp.
#include <cmath>
#include <algorithm>

#include "rsf_host.h"
#include "rsf_kernels_evidence.h"

using namespace rsfk;
using namespace rsfh;

namespace {

// the box and the transform flags of a call into lo[], hi[], tr[] of a kernel argument; fn: the entry point the message names
template <class ARGS>
int set_box(const char *fn, int d, const double *lo, const double *hi, const int32_t *transform, ARGS &A) {
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p])) return fail(RSF_ERR_INVALID, "%s: need finite lo[%d] < hi[%d]", fn, p, p);
    if (transform[p] != 0 && transform[p] != 1) return fail(RSF_ERR_INVALID, "%s: transform[%d] is neither 0 (identity) nor 1 (log)", fn, p);
    if (transform[p] == 1 && !(lo[p] > 0.0)) return fail(RSF_ERR_INVALID, "%s: the log transform of parameter %d needs lo > 0", fn, p);
    A.lo[p] = lo[p]; A.hi[p] = hi[p]; A.tr[p] = transform[p];
  }
  return RSF_OK;
}

// the proposal N(mean, L L^T): mean finite, chol[d][d] lower triangular with a positive finite diagonal
int set_gauss(const char *fn, int d, const double *mean, const double *chol, const int32_t *transform, EvGauss &G) {
  double logdet = 0.0;
  int e = 0;
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(mean[p])) return fail(RSF_ERR_INVALID, "%s: mean[%d] is not finite", fn, p);
    if (transform[p] != 0 && transform[p] != 1) return fail(RSF_ERR_INVALID, "%s: transform[%d] is neither 0 (identity) nor 1 (log)", fn, p);
    G.m[p] = mean[p];
    G.tr[p] = transform[p];
    for (int r = 0; r < d; ++r) {
      const double v = chol[p * d + r];
      if (!std::isfinite(v) || (r > p && v != 0.0) || (r == p && !(v > 0.0)))
        return fail(RSF_ERR_INVALID, "%s: chol is not a lower triangular factor with a positive diagonal (entry [%d][%d])", fn, p, r);
      if (r <= p) G.L[e++] = v;
    }
    logdet += std::log(chol[p * d + p]);
  }
  G.logc = -logdet - 0.5 * (double)d * std::log(2.0 * 3.14159265358979323846);
  return RSF_OK;
}

auto propose_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return evidence_propose_kernel<D>; }); }
auto logg_fn(int d) { return with<1, 2, 3>(d, [](auto D) { return evidence_logg_kernel<D>; }); }
// the float64 RK4 solve with or without damping, chosen as predict_kernel's dispatcher chooses
auto logtarget_fn(const rsf_ctx *c, int d) {
  return with<1, 3>(d, [&](auto D) { return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) { return evidence_logtarget_kernel<D, DAMP>; }); });
}

// the four sums of one set (a device pointer) into h[kEvFields]; n = 0: zeros, nothing is launched
template <bool NUM>
int terms(rsf_ctx *c, int64_t n, const double *dl, double lstar, double s1, double s2r, double *ws, double h[kEvFields]) {
  std::fill(h, h + kEvFields, 0.0);
  if (n == 0) return RSF_OK;
  int rc;
  const int blocks = (int)std::min<int64_t>(kEvBlocks, (n + kMaxBlock - 1) / kMaxBlock);
  if ((rc = launch(c, evidence_terms_kernel<NUM>, blocks, kMaxBlock, 0, n, dl, lstar, s1, s2r, ws + kEvFields))) return rc;
  if ((rc = sum_strided_tree(c, blocks, kEvFields, ws + kEvFields, ws))) return rc;
  HIP_TRY(hipMemcpyAsync(h, ws, kEvFields * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RSF_OK;
}

}  // namespace

extern "C" {

int rsf_evidence_propose(rsf_ctx *c, int64_t n2, int32_t d, const double *mean, const double *chol, const int32_t *transform,
                         const double *lo, const double *hi, uint64_t seed, int64_t offset, double *theta, double *logg, uint8_t *inbox) {
  RSF_ENTER(c, NEED_NOTHING, mean && chol && transform && lo && hi && theta && logg && inbox, "NULL argument");
  if (n2 < 1 || d < 1 || d > RSF_EVIDENCE_MAX_PARAMS || offset < 0)
    return fail(RSF_ERR_INVALID, "rsf_evidence_propose: need n2 >= 1, 1 <= d <= %d, offset >= 0", RSF_EVIDENCE_MAX_PARAMS);
  int rc;
  EvGauss G{};
  if ((rc = set_gauss(__func__, d, mean, chol, transform, G))) return rc;
  if ((rc = set_box(__func__, d, lo, hi, transform, G))) return rc;
  EvProposeArgs A{};
  A.n = n2; A.offset = offset; A.seed = seed;
  const size_t nb = (size_t)n2 * sizeof(double);
  if ((rc = stage_out(c, SLOT_EV_THETA, theta, nb * d, &A.theta))) return rc;
  if ((rc = stage_out(c, SLOT_EV_LOGG, logg, nb, &A.logg))) return rc;
  if ((rc = stage_out(c, SLOT_EV_INBOX, inbox, (size_t)n2, &A.inbox))) return rc;
  if ((rc = launch(c, propose_fn(d), (unsigned)((n2 + kMaxBlock - 1) / kMaxBlock), kMaxBlock, 0, G, A))) return rc;
  if ((rc = copy_back(c, SLOT_EV_THETA, theta, nb * d))) return rc;
  if ((rc = copy_back(c, SLOT_EV_LOGG, logg, nb))) return rc;
  if ((rc = copy_back(c, SLOT_EV_INBOX, inbox, (size_t)n2))) return rc;
  return finish(c);
}

int rsf_evidence_logg(rsf_ctx *c, int64_t n, int32_t d, const double *theta, const double *mean, const double *chol,
                      const int32_t *transform, double *logg) {
  RSF_ENTER(c, NEED_NOTHING, theta && mean && chol && transform && logg, "NULL argument");
  if (n < 1 || d < 1 || d > RSF_EVIDENCE_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_evidence_logg: need n >= 1, 1 <= d <= %d", RSF_EVIDENCE_MAX_PARAMS);
  int rc;
  EvGauss G{};
  if ((rc = set_gauss(__func__, d, mean, chol, transform, G))) return rc;
  const size_t nb = (size_t)n * sizeof(double);
  const double *dth;
  double *dg;
  if ((rc = stage_in(c, SLOT_EV_THETA, theta, nb * d, &dth))) return rc;
  if ((rc = stage_out(c, SLOT_EV_LOGG, logg, nb, &dg))) return rc;
  if ((rc = launch(c, logg_fn(d), (unsigned)((n + kMaxBlock - 1) / kMaxBlock), kMaxBlock, 0, G, n, dth, dg))) return rc;
  if ((rc = copy_back(c, SLOT_EV_LOGG, logg, nb))) return rc;
  return finish(c);
}

int rsf_evidence_logtarget(rsf_ctx *c, int64_t n, int32_t d, const double *theta, const double *data, double shape, const double *lo,
                           const double *hi, const int32_t *transform, const double *logg, double *l) {
  RSF_ENTER(c, NEED_MODEL, theta && data && lo && hi && transform && logg && l, "NULL argument");
  if (n < 1 || (d != 1 && d != 3)) return fail(RSF_ERR_INVALID, "rsf_evidence_logtarget: need n >= 1 and d = 1 or 3");
  if (!std::isfinite(shape) || !(shape > 0.0)) return fail(RSF_ERR_INVALID, "rsf_evidence_logtarget: shape must be finite and > 0");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_evidence_logtarget: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  int rc;
  EvTargetArgs A{};
  if ((rc = set_box(__func__, d, lo, hi, transform, A))) return rc;
  A.n = n; A.shape = shape;
  const size_t nb = (size_t)n * sizeof(double);
  const double *ddata;
  if ((rc = stage_in(c, SLOT_EV_THETA, theta, nb * d, &A.theta))) return rc;
  if ((rc = stage_in(c, SLOT_EV_LOGG, logg, nb, &A.logg))) return rc;
  if ((rc = stage_in(c, SLOT_EV_OBS, data, (size_t)c->nout * sizeof(double), &ddata))) return rc;
  if ((rc = stage_out(c, SLOT_EV_L, l, nb, &A.l))) return rc;
  // the shared chunking of the float64 tables (c->kc, c->lds_bytes), as rsf_mcmc_init's solve
  if ((rc = launch(c, logtarget_fn(c, d), grid_for(c, n), c->block, c->lds_bytes, make_consts(c, ddata), A))) return rc;
  if ((rc = copy_back(c, SLOT_EV_L, l, nb))) return rc;
  return finish(c);
}

int rsf_evidence_partials(rsf_ctx *c, int64_t n1, const double *l1, int64_t n2, const double *l2, double lstar, double r, double s1,
                          double s2, double *partials) {
  RSF_ENTER(c, NEED_NOTHING, partials && (l1 || n1 == 0) && (l2 || n2 == 0), "NULL argument");
  if (n1 < 0 || n2 < 0 || !std::isfinite(lstar) || !std::isfinite(r) || !(r > 0.0) || !(s1 > 0.0 && s1 < 1.0) || !(s2 > 0.0 && s2 < 1.0))
    return fail(RSF_ERR_INVALID, "rsf_evidence_partials: need n1, n2 >= 0, finite lstar, finite r > 0, s1 and s2 inside (0, 1)");
  int rc;
  const double *d1 = nullptr, *d2 = nullptr;
  if (n1 && (rc = stage_in(c, SLOT_EV_L, l1, (size_t)n1 * sizeof(double), &d1))) return rc;
  if (n2 && (rc = stage_in(c, SLOT_EV_L2, l2, (size_t)n2 * sizeof(double), &d2))) return rc;
  // workspace, doubles: sums[kEvFields] | the workgroups' partials[kEvBlocks][kEvFields]
  if ((rc = ensure(c->pool, sizeof(double) * kEvFields * (kEvBlocks + 1)))) return rc;
  double *ws = (double *)c->pool.p, h1[kEvFields], h2[kEvFields];
  if ((rc = terms<false>(c, n1, d1, lstar, s1, s2 * r, ws, h1))) return rc;
  if ((rc = terms<true>(c, n2, d2, lstar, s1, s2 * r, ws, h2))) return rc;
  if (h1[0] != (double)n1)
    return fail(RSF_ERR_INVALID, "rsf_evidence_partials: %lld of the posterior draws' l1 are not finite (no posterior draw lies outside the support)",
                (long long)((double)n1 - h1[0]));
  if (h2[0] + h2[1] != (double)n2) return fail(RSF_ERR_INVALID, "rsf_evidence_partials: %lld of l2 are NaN or +inf", (long long)((double)n2 - h2[0] - h2[1]));
  partials[0] = (double)n1; partials[1] = (double)n2; partials[2] = h2[0];
  partials[3] = h2[2]; partials[4] = h1[2];
  partials[5] = h2[2]; partials[6] = h2[3];        // f1 = t2
  partials[7] = r * h1[2]; partials[8] = (r * r) * h1[3];  // f2 = r t1
  return RSF_OK;
}

}  // extern "C"
