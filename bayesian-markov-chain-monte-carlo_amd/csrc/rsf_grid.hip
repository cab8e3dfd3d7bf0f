// rsf_grid.hip — the exact posterior on a tensor quadrature grid (include/rsf_grid.h): rsf_grid_logtarget / _columns / _draw / _cdf
// (kernels: rsf_kernels_grid.h).  rsf_grid_finish, the host arithmetic, is in rsf_finish.cpp.
#include <cmath>
#include <algorithm>
#include <vector>

#include "rsf_host.h"
#include "rsf_kernels_grid.h"

using namespace rsfk;
using namespace rsfh;

namespace {

// The HOST tables of a call on the device, in the ctx's poolws workspace: the axes' nodes and weights (an axis the grid lacks: one
// node 0 of weight 1) and up to two further tables.  One copy; the stream is synchronised before the host buffer goes away.
struct Upload {
  GridAxes G{};
  const double *extra[2] = {nullptr, nullptr};
};

int upload(rsf_ctx *c, int d, const int32_t *n, const double *x, const double *w, const double *e0, size_t n0, const double *e1, size_t n1, Upload &U) {
  size_t total = 0;
  for (int p = 0; p < d; ++p) total += (size_t)n[p];
  std::vector<double> h;
  h.reserve(2 * total + 2 + n0 + n1);
  h.insert(h.end(), x, x + total);
  if (w) h.insert(h.end(), w, w + total); else h.insert(h.end(), total, 1.0);
  h.push_back(0.0);
  h.push_back(1.0);
  if (e0) h.insert(h.end(), e0, e0 + n0);
  if (e1) h.insert(h.end(), e1, e1 + n1);
  if (int rc = ensure(c->poolws, h.size() * sizeof(double))) return rc;
  HIP_TRY(hipMemcpyAsync(c->poolws.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const double *dev = (const double *)c->poolws.p;
  size_t off = 0;
  for (int p = 0; p < RSF_GRID_MAX_PARAMS; ++p) {
    U.G.n[p] = p < d ? n[p] : 1;
    U.G.x[p] = p < d ? dev + off : dev + 2 * total;
    U.G.w[p] = p < d ? dev + total + off : dev + 2 * total + 1;
    if (p < d) off += (size_t)n[p];
  }
  if (e0) U.extra[0] = dev + 2 * total + 2;
  if (e1) U.extra[1] = dev + 2 * total + 2 + (e0 ? n0 : 0);
  return RSF_OK;
}

int check_coords(const char *fn, int d, int32_t coords) {
  if (coords != RSF_GRID_PLAIN && coords != RSF_GRID_PRODUCT) return fail(RSF_ERR_INVALID, "%s: coords is neither RSF_GRID_PLAIN nor RSF_GRID_PRODUCT", fn);
  if (coords == RSF_GRID_PRODUCT && d != 3) return fail(RSF_ERR_INVALID, "%s: RSF_GRID_PRODUCT needs d = 3", fn);
  return RSF_OK;
}

// the float64 RK4 solve with or without damping, chosen as rsf_evidence_logtarget's dispatcher chooses; PRODUCT exists for d = 3 alone
auto logtarget_fn(const rsf_ctx *c, int d, int coords) {
  return with<true, false>(damped(c, RK4_F64), [&](auto DAMP) {
    if (d == 1) return grid_logtarget_kernel<1, DAMP, RSF_GRID_PLAIN>;
    return with<RSF_GRID_PLAIN, RSF_GRID_PRODUCT>(coords, [&](auto COORD) { return grid_logtarget_kernel<3, DAMP, COORD>; });
  });
}
auto draw_fn(int d, int coords) {
  if (coords == RSF_GRID_PRODUCT) return grid_draw_kernel<3, RSF_GRID_PRODUCT>;
  return with<1, 2, 3>(d, [](auto D) { return grid_draw_kernel<D, RSF_GRID_PLAIN>; });
}

}  // namespace

extern "C" {

int rsf_grid_logtarget(rsf_ctx *c, int32_t d, const int32_t *n, const double *x, const double *data, double shape, const double *lo,
                       const double *hi, int32_t coords, double *l, double *ssq) {
  RSF_ENTER(c, NEED_MODEL, n && x && data && lo && hi && l && ssq, "NULL argument");
  if (d != 1 && d != 3) return fail(RSF_ERR_INVALID, "rsf_grid_logtarget: need d = 1 or 3");
  int rc;
  int64_t N;
  if ((rc = grid_check(__func__, d, 1, n, x, nullptr, &N))) return rc;
  if ((rc = check_coords(__func__, d, coords))) return rc;
  if (!std::isfinite(shape) || !(shape > 0.0)) return fail(RSF_ERR_INVALID, "rsf_grid_logtarget: shape must be finite and > 0");
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "rsf_grid_logtarget: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)");
  GridTargetArgs A{};
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p])) return fail(RSF_ERR_INVALID, "rsf_grid_logtarget: need finite lo[%d] < hi[%d]", p, p);
    A.lo[p] = lo[p]; A.hi[p] = hi[p];
  }
  if (coords == RSF_GRID_PRODUCT && !(lo[1] > 0.0)) return fail(RSF_ERR_INVALID, "rsf_grid_logtarget: RSF_GRID_PRODUCT needs lo[1] > 0");
  Upload U;
  if ((rc = upload(c, d, n, x, nullptr, nullptr, 0, nullptr, 0, U))) return rc;
  A.N = N; A.G = U.G; A.shape = shape;
  const size_t nb = (size_t)N * sizeof(double);
  const double *ddata;
  if ((rc = stage_in(c, SLOT_GRID_OBS, data, (size_t)c->nout * sizeof(double), &ddata))) return rc;
  if ((rc = stage_out(c, SLOT_GRID_L, l, nb, &A.l))) return rc;
  if ((rc = stage_out(c, SLOT_GRID_SSQ, ssq, nb, &A.ssq))) return rc;
  // the shared chunking of the float64 tables (c->kc, c->lds_bytes), as rsf_evidence_logtarget's solve
  if ((rc = launch(c, logtarget_fn(c, d, coords), grid_for(c, N), c->block, c->lds_bytes, make_consts(c, ddata), A))) return rc;
  if ((rc = copy_back(c, SLOT_GRID_L, l, nb))) return rc;
  if ((rc = copy_back(c, SLOT_GRID_SSQ, ssq, nb))) return rc;
  return finish(c);
}

int rsf_grid_columns(rsf_ctx *c, int32_t d, const int32_t *n, const double *x, const double *w, const double *l, const double *ssq,
                     double center, double *lmax, double *fields, double *m0, double *cum0) {
  RSF_ENTER(c, NEED_NOTHING, n && x && w && l && ssq && lmax && fields, "NULL argument");
  int rc;
  int64_t N;
  if ((rc = grid_check(__func__, d, 1, n, x, w, &N))) return rc;
  if (!std::isfinite(center)) return fail(RSF_ERR_INVALID, "rsf_grid_columns: center is not finite");
  Upload U;
  if ((rc = upload(c, d, n, x, w, nullptr, 0, nullptr, 0, U))) return rc;
  GridColArgs A{};
  A.G = U.G; A.ncol = N / n[0]; A.center = center;
  const size_t nb = (size_t)N * sizeof(double), fb = (size_t)A.ncol * RSF_GRID_FIELDS * sizeof(double);
  double *dfields, *dm0, *dcum0;
  if ((rc = stage_in(c, SLOT_GRID_L, l, nb, &A.l))) return rc;
  if ((rc = stage_in(c, SLOT_GRID_SSQ, ssq, nb, &A.ssq))) return rc;
  if ((rc = stage_out(c, SLOT_GRID_FIELDS, fields, fb, &dfields))) return rc;
  if ((rc = stage_out(c, SLOT_GRID_M0, m0, (size_t)n[0] * sizeof(double), &dm0))) return rc;
  if ((rc = stage_out(c, SLOT_GRID_CUM0, cum0, nb, &dcum0))) return rc;
  // lmax: workspace, doubles: head[kGridHead] | the workgroups' partials
  const int blocks = (int)std::min<int64_t>(kGridBlocks, (N + kMaxBlock - 1) / kMaxBlock);
  if ((rc = ensure(c->pool, sizeof(double) * kGridHead * (kGridBlocks + 1)))) return rc;
  double *head = (double *)c->pool.p, h[kGridHead];
  if ((rc = launch(c, grid_max_kernel, blocks, kMaxBlock, 0, N, A.l, head + kGridHead))) return rc;
  if ((rc = launch(c, grid_max_finish_kernel, 1, 64, 0, blocks, head + kGridHead, head))) return rc;
  HIP_TRY(hipMemcpyAsync(h, head, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (h[1] + h[2] != (double)N) return fail(RSF_ERR_INVALID, "rsf_grid_columns: %lld of l are NaN or +inf", (long long)((double)N - h[1] - h[2]));
  *lmax = A.lmax = h[0];
  if ((rc = launch(c, grid_columns_kernel, (unsigned)A.ncol, kMaxBlock, 0, A, dfields))) return rc;
  if (dm0 && (rc = launch(c, grid_m0_kernel, blocks_of(n[0]), kMaxBlock, 0, A, dm0))) return rc;
  if (dcum0 && (rc = launch(c, grid_cum0_kernel, (unsigned)((A.ncol + 63) / 64), 64, 0, A, dcum0))) return rc;
  if ((rc = copy_back(c, SLOT_GRID_FIELDS, fields, fb))) return rc;
  if ((rc = copy_back(c, SLOT_GRID_M0, m0, (size_t)n[0] * sizeof(double)))) return rc;
  if ((rc = copy_back(c, SLOT_GRID_CUM0, cum0, nb))) return rc;
  return finish(c);
}

int rsf_grid_draw(rsf_ctx *c, int32_t d, const int32_t *n, const double *x, int32_t coords, const double *cum0, const double *cum1,
                  const double *cum2, uint64_t seed, int64_t offset, int64_t nd, double *q, int32_t *cell) {
  RSF_ENTER(c, NEED_NOTHING, n && x && cum0 && q, "NULL argument");
  int rc;
  int64_t N;
  if ((rc = grid_check(__func__, d, 1, n, x, nullptr, &N))) return rc;
  if ((rc = check_coords(__func__, d, coords))) return rc;
  if ((d > 1 && !cum1) || (d > 2 && !cum2)) return fail(RSF_ERR_INVALID, "rsf_grid_draw: NULL argument");
  if (nd < 1 || offset < 0) return fail(RSF_ERR_INVALID, "rsf_grid_draw: need nd >= 1 and offset >= 0");
  const size_t n1 = d > 1 ? (size_t)n[1] : 0, n2 = d > 2 ? (size_t)n[2] : 0;
  Upload U;
  if ((rc = upload(c, d, n, x, nullptr, d > 1 ? cum1 : nullptr, n1 * (d > 2 ? n2 : 1), d > 2 ? cum2 : nullptr, n2, U))) return rc;
  GridDrawArgs A{};
  A.G = U.G; A.nd = nd; A.offset = offset; A.seed = seed; A.cum1 = U.extra[0]; A.cum2 = U.extra[1];
  const size_t qb = (size_t)nd * d * sizeof(double), cb = (size_t)nd * d * sizeof(int32_t);
  if ((rc = stage_in(c, SLOT_GRID_CUM0, cum0, (size_t)N * sizeof(double), &A.cum0))) return rc;
  if ((rc = stage_out(c, SLOT_GRID_Q, q, qb, &A.q))) return rc;
  if ((rc = stage_out(c, SLOT_GRID_CELL, cell, cb, &A.cell))) return rc;
  if ((rc = launch(c, draw_fn(d, coords), blocks_of(nd), kMaxBlock, 0, A))) return rc;
  if ((rc = copy_back(c, SLOT_GRID_Q, q, qb))) return rc;
  if ((rc = copy_back(c, SLOT_GRID_CELL, cell, cb))) return rc;
  return finish(c);
}

int rsf_grid_cdf(rsf_ctx *c, int32_t d, const int32_t *n, const double *x, int32_t coords, const double *cum0, const double *pair, int64_t nx,
                 const double *xs, double *F) {
  RSF_ENTER(c, NEED_NOTHING, n && x && cum0 && pair && xs && F, "NULL argument");
  int rc;
  int64_t N;
  if ((rc = grid_check(__func__, d, 1, n, x, nullptr, &N))) return rc;
  if ((rc = check_coords(__func__, d, coords))) return rc;
  if (nx < 1) return fail(RSF_ERR_INVALID, "rsf_grid_cdf: need nx >= 1");
  const size_t ncol = (size_t)(N / n[0]);
  Upload U;
  if ((rc = upload(c, d, n, x, nullptr, pair, ncol, xs, (size_t)nx, U))) return rc;
  const double *dcum0;
  if ((rc = stage_in(c, SLOT_GRID_CUM0, cum0, (size_t)N * sizeof(double), &dcum0))) return rc;
  if ((rc = ensure(c->pool, (size_t)nx * sizeof(double)))) return rc;
  double *dF = (double *)c->pool.p;
  auto fn = with<RSF_GRID_PLAIN, RSF_GRID_PRODUCT>(coords, [](auto COORD) { return grid_cdf_kernel<COORD>; });
  if ((rc = launch(c, fn, blocks_of(nx), kMaxBlock, 0, U.G, dcum0, U.extra[0], nx, U.extra[1], dF))) return rc;
  HIP_TRY(hipMemcpyAsync(F, dF, (size_t)nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RSF_OK;
}

}  // extern "C"
