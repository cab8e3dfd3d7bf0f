// rsf_law_grid.hip — the exact posterior of a state-law model on a tensor grid in the coordinates of a fit
// (include/rsf_law_grid.h): rsf_law_logtarget, rsf_law_grid_moments (kernels: rsf_kernels_law_grid.h).
#include <cmath>
#include <vector>

#include "rsf_host.h"
#include "rsf_kernels_law_grid.h"

using namespace rsfk;
using namespace rsfh;

namespace {

// the axes' nodes and weights on the device, in the ctx's poolws workspace (an axis the grid lacks: one node 0 of weight 1), as
// rsf_grid.hip uploads its own.  One copy; the stream is synchronised before the host buffer goes away.
int upload_axes(rsf_ctx *c, int d, const int32_t *n, const double *z, const double *w, LawGridAxes &G) {
  size_t total = 0;
  for (int p = 0; p < d; ++p) total += (size_t)n[p];
  std::vector<double> h;
  h.reserve(2 * total + 2);
  h.insert(h.end(), z, z + total);
  if (w) h.insert(h.end(), w, w + total); else h.insert(h.end(), total, 1.0);
  h.push_back(0.0);
  h.push_back(1.0);
  if (int rc = ensure(c->poolws, h.size() * sizeof(double))) return rc;
  HIP_TRY(hipMemcpyAsync(c->poolws.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const double *dev = (const double *)c->poolws.p;
  size_t off = 0;
  for (int p = 0; p < RSF_LAW_GRID_MAX_PARAMS; ++p) {
    G.n[p] = p < d ? n[p] : 1;
    G.z[p] = p < d ? dev + off : dev + 2 * total;
    G.w[p] = p < d ? dev + total + off : dev + 2 * total + 1;
    if (p < d) off += (size_t)n[p];
  }
  return RSF_OK;
}

// tr and perm (always), m and L (with_factor) → M; fn: the entry point the messages name
int check_map(const char *fn, int d, const double *m, const double *L, const int32_t *tr, const int32_t *perm, bool with_factor, LawGridMap &M) {
  bool seen[RSF_LAW_GRID_MAX_PARAMS] = {false, false, false};
  for (int p = 0; p < d; ++p) {
    if (perm[p] < 0 || perm[p] >= d || seen[perm[p]]) return fail(RSF_ERR_INVALID, "%s: perm is not a permutation of 0 .. %d", fn, d - 1);
    seen[perm[p]] = true;
    M.perm[p] = perm[p];
    M.tr[p] = tr[p] != 0;
  }
  for (int p = d; p < RSF_LAW_GRID_MAX_PARAMS; ++p) { M.perm[p] = p; M.tr[p] = 0; }
  if (!with_factor) return RSF_OK;
  for (int p = 0, e = 0; p < d; ++p) {
    if (!std::isfinite(m[p])) return fail(RSF_ERR_INVALID, "%s: m[%d] is not finite", fn, p);
    M.m[p] = m[p];
    for (int r = 0; r <= p; ++r, ++e) {
      if (!std::isfinite(L[e])) return fail(RSF_ERR_INVALID, "%s: L holds a value that is not finite", fn);
      M.L[e] = L[e];
    }
    if (!(L[e - 1] > 0.0)) return fail(RSF_ERR_INVALID, "%s: the diagonal entry %d of L is not > 0", fn, p);
  }
  return RSF_OK;
}

auto logtarget_fn(const rsf_ctx *c, int d, int law) {  // void (*)(Consts, int32_t, LawTargetArgs)
  return with<RSF_LAW_SLIP, RSF_LAW_AGEING>(law, [&](auto LAW) {
    return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) {
      return with<1, 3>(d, [&](auto D) { return law_logtarget_kernel<D, LAW, DAMP>; });
    });
  });
}

}  // namespace

extern "C" {

int rsf_law_logtarget(rsf_ctx *c, int32_t law, int32_t observable, int32_t d, const int32_t *n, const double *z, const double *m,
                      const double *L, const int32_t *tr, const int32_t *perm, int64_t npoints, const double *theta, const double *logg,
                      const double *data, double shape, const double *lo, const double *hi, double *l, double *ssq, double *q_out) {
  RSF_ENTER(c, NEED_MODEL, tr && perm && data && lo && hi && l && ssq && (theta || (n && z && m && L)), "NULL argument");
  int rc;
  if (law != RSF_LAW_AGEING && law != RSF_LAW_SLIP) return fail(RSF_ERR_INVALID, "rsf_law_logtarget: law is RSF_LAW_AGEING (0) or RSF_LAW_SLIP (1), not %d", law);
  if (observable != RSF_OBS_ACC && observable != RSF_OBS_MU && observable != RSF_OBS_THETA && observable != RSF_OBS_VELOCITY)
    return fail(RSF_ERR_INVALID, "rsf_law_logtarget: observable is RSF_OBS_ACC (0), RSF_OBS_MU (1), RSF_OBS_THETA (2) or RSF_OBS_VELOCITY (3), not %d", observable);
  if (d != 1 && d != 3) return fail(RSF_ERR_INVALID, "rsf_law_logtarget: need d = 1 or 3");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_law_logtarget: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  if (!std::isfinite(shape) || !(shape > 0.0)) return fail(RSF_ERR_INVALID, "rsf_law_logtarget: shape must be finite and > 0");
  LawTargetArgs A{};
  if ((rc = check_map(__func__, d, m, L, tr, perm, theta == nullptr, A.M))) return rc;
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p])) return fail(RSF_ERR_INVALID, "rsf_law_logtarget: need finite lo[%d] < hi[%d]", p, p);
    A.lo[p] = lo[p]; A.hi[p] = hi[p];
  }
  for (int p = 0; p < d; ++p)
    if (A.M.tr[p] && !(lo[A.M.perm[p]] > 0.0)) return fail(RSF_ERR_INVALID, "rsf_law_logtarget: the logged parameter %d needs lo > 0", A.M.perm[p]);
  int64_t N = npoints;
  if (theta) {
    if (npoints < 1) return fail(RSF_ERR_INVALID, "rsf_law_logtarget: need npoints >= 1 with theta");
    for (int p = 0; p < RSF_LAW_GRID_MAX_PARAMS; ++p) A.G.n[p] = 1;
  } else {
    if ((rc = grid_check(__func__, d, 1, n, z, nullptr, &N))) return rc;
    if ((rc = upload_axes(c, d, n, z, nullptr, A.G))) return rc;
  }
  A.N = N; A.shape = shape;
  const size_t nb = (size_t)N * sizeof(double);
  Staged S(c);
  const int kdata = S.add(data, (size_t)c->nout * sizeof(double), true, false);
  const int kth = theta ? S.add(theta, nb * d, true, false) : -1, kg = logg ? S.add(logg, nb, true, false) : -1;
  const int kl = S.add(l, nb, false, true), ks = S.add(ssq, nb, false, true), kq = q_out ? S.add(q_out, nb * d, false, true) : -1;
  if ((rc = S.commit())) return rc;
  A.theta = kth < 0 ? nullptr : S.dev<const double>(kth);
  A.logg = kg < 0 ? nullptr : S.dev<const double>(kg);
  A.l = S.dev<double>(kl); A.ssq = S.dev<double>(ks);
  A.q_out = kq < 0 ? nullptr : S.dev<double>(kq);
  // the shared chunking of the float64 tables (c->kc, c->lds_bytes), as rsf_law_observe
  if ((rc = launch(c, logtarget_fn(c, d, law), grid_for(c, N), c->block, c->lds_bytes, make_consts(c, S.dev<const double>(kdata)), observable, A))) return rc;
  if ((rc = S.back())) return rc;
  return finish(c);
}

int rsf_law_grid_moments(rsf_ctx *c, int32_t d, const int32_t *n, const double *z, const double *w, const double *m, const double *L,
                         const int32_t *tr, const int32_t *perm, const double *l, const double *ssq, double lmax, const double *center,
                         double *fields, double *total) {
  RSF_ENTER(c, NEED_NOTHING, n && z && w && m && L && tr && perm && l && ssq && center && total, "NULL argument");
  int rc;
  if (d != 1 && d != 3) return fail(RSF_ERR_INVALID, "rsf_law_grid_moments: need d = 1 or 3");
  int64_t N;
  if ((rc = grid_check(__func__, d, 1, n, z, w, &N))) return rc;
  LawMomentArgs A{};
  if ((rc = check_map(__func__, d, m, L, tr, perm, true, A.M))) return rc;
  if (std::isnan(lmax) || lmax == INFINITY) return fail(RSF_ERR_INVALID, "rsf_law_grid_moments: lmax is NaN or +inf");
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(center[p])) return fail(RSF_ERR_INVALID, "rsf_law_grid_moments: center[%d] is not finite", p);
    A.center[p] = center[p];
  }
  if ((rc = upload_axes(c, d, n, z, w, A.G))) return rc;
  A.lmax = lmax;
  const int64_t ncol = N / n[0];
  const size_t nb = (size_t)N * sizeof(double), fb = (size_t)ncol * RSF_LAW_GRID_FIELDS * sizeof(double);
  Staged S(c);
  const int kl = S.add(l, nb, true, false), ks = S.add(ssq, nb, true, false);
  const int kf = fields ? S.add(fields, fb, false, true) : -1;
  if ((rc = S.commit())) return rc;
  A.l = S.dev<const double>(kl); A.ssq = S.dev<const double>(ks);
  double *dfields;
  if (kf >= 0) dfields = S.dev<double>(kf);
  else {  // a workspace of its own: the diag buffer, which no grid call uses
    if ((rc = ensure(c->diag, fb))) return rc;
    dfields = (double *)c->diag.p;
  }
  auto fn = with<1, 3>(d, [](auto D) { return law_grid_moments_kernel<D>; });
  if ((rc = launch(c, fn, (unsigned)ncol, kMaxBlock, 0, A, dfields))) return rc;
  std::vector<double> h((size_t)ncol * RSF_LAW_GRID_FIELDS);
  HIP_TRY(hipMemcpyAsync(h.data(), dfields, fb, hipMemcpyDeviceToHost, c->stream));
  if ((rc = S.back())) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int f = 0; f < RSF_LAW_GRID_FIELDS; ++f) {  // the columns in index order
    double s = 0.0;
    for (int64_t col = 0; col < ncol; ++col) s += h[(size_t)col * RSF_LAW_GRID_FIELDS + f];
    total[f] = s;
  }
  return RSF_OK;
}

}  // extern "C"
