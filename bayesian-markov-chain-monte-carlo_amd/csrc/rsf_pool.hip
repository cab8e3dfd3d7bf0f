// rsf_pool.hip — posterior post-processing of the pooled draws: rsf_pool_summary / _kde / _histogram (kernels: rsf_kernels_pool.h)
// and their joint posterior, rsf_pool_joint_partials / _kde2d / _histogram2d (include/rsf_joint.h, kernels: rsf_kernels_joint.h);
// and rsfh::sum_in_order / sum_strided_tree, the last step of every unit's reductions (rsf_host.h).
#include <cmath>
#include <algorithm>
#include <vector>

#include "rsf_host.h"
#include "rsf_kernels_pool.h"
#include "rsf_kernels_joint.h"

using namespace rsfk;
using namespace rsfh;

namespace rsfh {

int sum_in_order(rsf_ctx *c, int64_t nblocks, int64_t per, int64_t nf, const double *part, double scale, double *out, unsigned grid_x) {
  if (!grid_x) grid_x = (unsigned)((nf + kMaxBlock - 1) / kMaxBlock);
  return launch(c, sum_in_order_kernel, dim3(grid_x, (unsigned)((nblocks + per - 1) / per)), kMaxBlock, 0, nblocks, per, nf, part, scale, out);
}

int sum_strided_tree(rsf_ctx *c, int nblocks, int nf, const double *part, double *out) {
  return launch(c, sum_strided_tree_kernel, nf, kMaxBlock, 0, nblocks, nf, part, out);
}

}  // namespace rsfh

extern "C" {

namespace {

// moments of x[i*stride] with x already a device pointer; result on the host
int pool_moments(rsf_ctx *c, int64_t n, const double *dx, int64_t stride, double out[5]) {
  int rc = ensure(c->pool, sizeof(PoolPartial) * kPoolBlocks);
  if (rc) return rc;
  double shift = 0.0;
  HIP_TRY(hipMemcpyAsync(&shift, dx, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int blocks = (int)std::min<int64_t>(kPoolBlocks, (n + kMaxBlock - 1) / kMaxBlock);
  if ((rc = launch(c, pool_moments_kernel, blocks, kMaxBlock, 0, n, dx, stride, shift, (PoolPartial *)c->pool.p))) return rc;
  std::vector<PoolPartial> h(blocks);
  HIP_TRY(hipMemcpyAsync(h.data(), c->pool.p, sizeof(PoolPartial) * blocks, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  double cnt = 0, sum = 0, sumsq = 0, mn = INFINITY, mx = -INFINITY;
  for (const auto &p : h) { cnt += p.cnt; sum += p.sum; sumsq += p.sumsq; mn = std::fmin(mn, p.mn); mx = std::fmax(mx, p.mx); }
  const double mean_s = sum / cnt;
  out[0] = cnt; out[1] = shift + mean_s;
  out[2] = cnt > 1 ? (sumsq - cnt * mean_s * mean_s) / (cnt - 1) : 0.0;
  out[3] = mn; out[4] = mx;
  // the non-finite rule of rsf_abi.h.  A NaN sample already makes both sums NaN; one infinite sample leaves sum = +-inf (a mean of
  // +-inf, and a variance of 0 at n = 1) unless x[0] is that sample: NaN in every case.  fmin/fmax skip NaN samples, so min and
  // max are those of the others, and the reduction's start values survive only when every sample is NaN.
  if (!std::isfinite(sum) || !std::isfinite(sumsq)) out[1] = out[2] = NAN;
  if (mn > mx) out[3] = out[4] = NAN;
  return RSF_OK;
}

}  // namespace

int rsf_pool_summary(rsf_ctx *c, int64_t n, const double *x, int64_t stride, double *out) {
  RSF_ENTER(c, NEED_NOTHING, x && out && n >= 1 && stride >= 1, "bad argument");
  int rc;
  const double *dx;
  if ((rc = stage_in(c, SLOT_X, x, (size_t)((n - 1) * stride + 1) * sizeof(double), &dx))) return rc;
  return pool_moments(c, n, dx, stride, out);
}

int rsf_pool_kde(rsf_ctx *c, int64_t n, const double *x, int64_t stride, int32_t m, const double *grid, double bw_factor,
                 double *density) {
  RSF_ENTER(c, NEED_NOTHING, x && grid && density && n >= 2 && m >= 1 && stride >= 1, "bad argument");
  int rc;
  const double *dx, *dg;
  double *dd;
  if ((rc = stage_in(c, SLOT_X, x, (size_t)((n - 1) * stride + 1) * sizeof(double), &dx))) return rc;
  if ((rc = stage_in(c, SLOT_GRID, grid, (size_t)m * sizeof(double), &dg))) return rc;
  if ((rc = stage_out(c, SLOT_POOL_OUT, density, (size_t)m * sizeof(double), &dd))) return rc;
  double s[5];
  if ((rc = pool_moments(c, n, dx, stride, s))) return rc;
  const double factor = bw_factor > 0.0 ? bw_factor : std::pow((double)n, -1.0 / 5.0);  // scipy scotts_factor, d = 1
  const double cov = s[2] * factor * factor;
  if (!std::isfinite(s[2])) return fail(RSF_ERR_INVALID, "rsf_pool_kde: a non-finite draw (or a variance beyond the range of a double)");
  if (!(cov > 0.0)) return fail(RSF_ERR_INVALID, "rsf_pool_kde: the samples have zero variance (singular KDE)");
  const int blocks = (int)std::min<int64_t>(kPoolBlocks, (n + kKdeTile - 1) / kKdeTile);
  DevBuf &ws = c->poolws;
  if ((rc = ensure(ws, (size_t)blocks * (size_t)m * sizeof(double)))) return rc;
  if ((rc = launch(c, pool_kde_kernel, blocks, kMaxBlock, 0, n, dx, stride, m, dg, 0.5 / cov, (double *)ws.p))) return rc;
  if ((rc = sum_in_order(c, blocks, blocks, m, (const double *)ws.p, 1.0 / ((double)n * std::sqrt(2.0 * 3.14159265358979323846 * cov)), dd))) return rc;
  if ((rc = copy_back(c, SLOT_POOL_OUT, density, (size_t)m * sizeof(double)))) return rc;
  return finish(c);
}

int rsf_pool_histogram(rsf_ctx *c, int64_t n, const double *x, int64_t stride, int32_t nbins, double lo, double hi, double *counts) {
  if (!c || !x || !counts || n < 1 || stride < 1 || nbins < 1 || nbins > kHistMaxBins || !(hi > lo) || !std::isfinite(hi - lo))
    return fail(RSF_ERR_INVALID, "rsf_pool_histogram: bad argument (1 <= nbins <= %d, finite lo < hi)", kHistMaxBins);
  RSF_ENTER(c, NEED_NOTHING);
  int rc;
  const double *dx;
  double *dout;
  const int nb = nbins + 2;
  if ((rc = stage_in(c, SLOT_X, x, (size_t)((n - 1) * stride + 1) * sizeof(double), &dx))) return rc;
  if ((rc = stage_out(c, SLOT_POOL_OUT, counts, (size_t)nb * sizeof(double), &dout))) return rc;
  DevBuf &ws = c->poolws;
  if ((rc = ensure(ws, (size_t)nb * sizeof(unsigned long long)))) return rc;
  HIP_TRY(hipMemsetAsync(ws.p, 0, (size_t)nb * sizeof(unsigned long long), c->stream));
  const int blocks = (int)std::min<int64_t>(kPoolBlocks, (n + kMaxBlock - 1) / kMaxBlock);
  if ((rc = launch(c, pool_hist_kernel, blocks, kMaxBlock, (size_t)nb * sizeof(unsigned int), n, dx, stride, nbins, lo, hi,
                   (double)nbins / (hi - lo), (hi - lo) / (double)nbins, (unsigned long long *)ws.p))) return rc;
  if ((rc = launch(c, pool_hist_finish_kernel, (nb + kMaxBlock - 1) / kMaxBlock, kMaxBlock, 0, nb, (const unsigned long long *)ws.p, dout))) return rc;
  if ((rc = copy_back(c, SLOT_POOL_OUT, counts, (size_t)nb * sizeof(double)))) return rc;
  return finish(c);
}

// ---- the joint posterior (include/rsf_joint.h) ------------------------------------------------------------------------

namespace {

// joint partials of the columns A.col[0..d) of x (a device pointer) about A.c; result on the host in the layout of rsf_joint.h
static int joint_moments(rsf_ctx *c, int64_t n, int d, const double *dx, const JointCols &A, double *partials) {
  static_assert(joint_fields(RSF_JOINT_MAX_PARAMS) <= kMaxBlock, "block_fields_store: one thread per field");
  const int nf = joint_fields(d);
  const int blocks = (int)std::min<int64_t>(kPoolBlocks, (n + kMaxBlock - 1) / kMaxBlock);
  int rc = ensure(c->pool, sizeof(double) * (size_t)nf * (size_t)(blocks + 1));
  if (rc) return rc;
  double *part = (double *)c->pool.p, *sum = part + (size_t)nf * blocks;
  auto fn = d == 1 ? pool_joint_moments_kernel<1, true> : d == 2 ? pool_joint_moments_kernel<2, true>
          : d == 3 ? pool_joint_moments_kernel<3, true> : pool_joint_moments_kernel<RSF_JOINT_MAX_PARAMS, false>;
  if ((rc = launch(c, fn, blocks, kMaxBlock, 0, n, d, dx, A, part))) return rc;
  if ((rc = sum_strided_tree(c, blocks, nf, part, sum))) return rc;
  HIP_TRY(hipMemcpyAsync(partials, sum, sizeof(double) * nf, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RSF_OK;
}

static bool bad_pair(int32_t d, int32_t pa, int32_t pb) { return d < 2 || pa < 0 || pb < 0 || pa >= d || pb >= d || pa == pb; }

}  // namespace

int rsf_pool_joint_partials(rsf_ctx *c, int64_t n, int32_t d, const double *x, const double *center, double *partials) {
  if (!c || !x || !center || !partials || n < 1 || d < 1 || d > RSF_JOINT_MAX_PARAMS)
    return fail(RSF_ERR_INVALID, "rsf_pool_joint_partials: bad argument (n >= 1, 1 <= d <= %d)", RSF_JOINT_MAX_PARAMS);
  JointCols A{};
  A.ld = d;
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(center[p])) return fail(RSF_ERR_INVALID, "rsf_pool_joint_partials: center[%d] is not finite", p);
    A.c[p] = center[p];
    A.col[p] = p;
  }
  RSF_ENTER(c, NEED_NOTHING);
  int rc;
  const double *dx;
  if ((rc = stage_in(c, SLOT_X, x, (size_t)n * (size_t)d * sizeof(double), &dx))) return rc;
  return joint_moments(c, n, d, dx, A, partials);
}

int rsf_pool_kde2d(rsf_ctx *c, int64_t n, int32_t d, const double *x, int32_t pa, int32_t pb, int32_t m, const double *points,
                   double bw_factor, const double *cov2, int64_t n_total, double *density) {
  if (!c || !x || !points || !density || n < 3 || m < 1 || bad_pair(d, pa, pb) || n_total < 0 || (n_total && n_total < n))
    return fail(RSF_ERR_INVALID, "rsf_pool_kde2d: bad argument (n >= 3, m >= 1, pa != pb in [0, d), n_total 0 or >= n)");
  RSF_ENTER(c, NEED_NOTHING);
  int rc;
  const double *dx, *dp;
  double *dd;
  if ((rc = stage_in(c, SLOT_X, x, (size_t)n * (size_t)d * sizeof(double), &dx))) return rc;
  if ((rc = stage_in(c, SLOT_GRID, points, (size_t)m * 2 * sizeof(double), &dp))) return rc;
  if ((rc = stage_out(c, SLOT_POOL_OUT, density, (size_t)m * sizeof(double), &dd))) return rc;
  // the centre of the whitening (and, without cov2, the bandwidth): the two columns' moments about the first row
  JointCols J{};
  J.ld = d;
  J.col[0] = pa; J.col[1] = pb;
  HIP_TRY(hipMemcpyAsync(&J.c[0], dx + pa, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(&J.c[1], dx + pb, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  double part[joint_fields(2)], o[RSF_JOINT_OUT(2)];
  if (!std::isfinite(J.c[0]) || !std::isfinite(J.c[1])) return fail(RSF_ERR_INVALID, "rsf_pool_kde2d: a non-finite draw");
  if ((rc = joint_moments(c, n, 2, dx, J, part))) return rc;
  if (part[1] != 0.0) return fail(RSF_ERR_INVALID, "rsf_pool_kde2d: %lld rows with a non-finite draw", (long long)part[1]);
  if ((rc = rsf_pool_joint_finish(2, part, J.c, o))) return rc;
  const double nt = (double)(n_total ? n_total : n);
  const double factor = bw_factor > 0.0 ? bw_factor : std::pow(nt, -1.0 / 6.0);  // scipy scotts_factor, d = 2
  const double *cv = cov2 ? cov2 : o + 2;
  const double f2 = factor * factor, h00 = cv[0] * f2, h01 = 0.5 * (cv[1] + cv[2]) * f2, h11 = cv[3] * f2, det = h00 * h11 - h01 * h01;
  if (!(h00 > 0.0) || !(h11 > 0.0) || !std::isfinite(h00) || !std::isfinite(h11) || !(det > 1e-12 * h00 * h11))
    return fail(RSF_ERR_INVALID, "rsf_pool_kde2d: the covariance of the two columns is not finite or not positive definite (singular KDE)");
  const double l00 = std::sqrt(h00), l10 = h01 / l00, l11 = std::sqrt(det / h00), r = std::sqrt(0.5);
  Kde2dArgs A{n, d, pa, pb, m, o[0], o[1], r / l00, -r * l10 / (l00 * l11), r / l11};
  const int64_t chunks = ((int64_t)m + kKde2dChunk - 1) / kKde2dChunk;
  const int slices = (int)std::max<int64_t>(1, std::min<int64_t>((n + kKdeTile - 1) / kKdeTile, (kPoolBlocks + chunks - 1) / chunks));
  DevBuf &ws = c->poolws;
  if ((rc = ensure(ws, (size_t)slices * (size_t)m * sizeof(double)))) return rc;
  if ((rc = launch(c, pool_kde2d_kernel, dim3((unsigned)chunks, (unsigned)slices), kMaxBlock, 0, A, dx, dp, (double *)ws.p))) return rc;
  if ((rc = sum_in_order(c, slices, slices, m, (const double *)ws.p, 1.0 / (nt * 2.0 * 3.14159265358979323846 * l00 * l11), dd))) return rc;
  if ((rc = copy_back(c, SLOT_POOL_OUT, density, (size_t)m * sizeof(double)))) return rc;
  return finish(c);
}

int rsf_pool_histogram2d(rsf_ctx *c, int64_t n, int32_t d, const double *x, int32_t pa, int32_t pb, int32_t nbx, double lo_a,
                         double hi_a, int32_t nby, double lo_b, double hi_b, double *counts) {
  const int64_t ncells = nbx >= 1 && nby >= 1 ? ((int64_t)nbx + 2) * ((int64_t)nby + 2) : 0;
  if (!c || !x || !counts || n < 1 || bad_pair(d, pa, pb) || ncells < 1 || ncells > RSF_HIST2D_MAX_CELLS || !(hi_a > lo_a) ||
      !std::isfinite(hi_a - lo_a) || !(hi_b > lo_b) || !std::isfinite(hi_b - lo_b))
    return fail(RSF_ERR_INVALID, "rsf_pool_histogram2d: bad argument (nbx >= 1, nby >= 1, (nbx + 2)(nby + 2) <= %d, finite lo < hi on "
                                 "both axes, pa != pb in [0, d))", RSF_HIST2D_MAX_CELLS);
  RSF_ENTER(c, NEED_NOTHING);
  int rc;
  const double *dx;
  double *dout;
  const int nb = (int)ncells;
  if ((rc = stage_in(c, SLOT_X, x, (size_t)n * (size_t)d * sizeof(double), &dx))) return rc;
  if ((rc = stage_out(c, SLOT_POOL_OUT, counts, (size_t)nb * sizeof(double), &dout))) return rc;
  DevBuf &ws = c->poolws;
  if ((rc = ensure(ws, (size_t)nb * sizeof(unsigned long long)))) return rc;
  HIP_TRY(hipMemsetAsync(ws.p, 0, (size_t)nb * sizeof(unsigned long long), c->stream));
  // a table above 32 KiB leaves room for two workgroups on a CU: half the grid, so that every workgroup is resident and
  // flushes its table once
  const int cap = (size_t)nb * sizeof(unsigned int) > 32 * 1024 ? kPoolBlocks / 2 : kPoolBlocks;
  const int blocks = (int)std::min<int64_t>(cap, (n + kMaxBlock - 1) / kMaxBlock);
  const Hist2dAxis A{pa, nbx, lo_a, hi_a, (double)nbx / (hi_a - lo_a), (hi_a - lo_a) / (double)nbx};
  const Hist2dAxis B{pb, nby, lo_b, hi_b, (double)nby / (hi_b - lo_b), (hi_b - lo_b) / (double)nby};
  const size_t lds = (size_t)nb * sizeof(unsigned int);
  if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)pool_hist2d_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if ((rc = launch(c, pool_hist2d_kernel, blocks, kMaxBlock, lds, n, dx, d, A, B, (unsigned long long *)ws.p))) return rc;
  if ((rc = launch(c, pool_hist_finish_kernel, (nb + kMaxBlock - 1) / kMaxBlock, kMaxBlock, 0, nb, (const unsigned long long *)ws.p, dout))) return rc;
  if ((rc = copy_back(c, SLOT_POOL_OUT, counts, (size_t)nb * sizeof(double)))) return rc;
  return finish(c);
}

}  // extern "C"
