// rsf_pool.hip — posterior post-processing of the pooled draws: rsf_pool_summary / _kde / _histogram (kernels: rsf_kernels_pool.h).
#include <cmath>
#include <algorithm>
#include <vector>

#include "rsf_host.h"
#include "rsf_kernels_pool.h"

using namespace rsfk;
using namespace rsfh;

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
  hipLaunchKernelGGL(pool_moments_kernel, dim3(blocks), dim3(kMaxBlock), 0, c->stream, n, dx, stride, shift, (PoolPartial *)c->pool.p);
  std::vector<PoolPartial> h(blocks);
  HIP_TRY(hipMemcpyAsync(h.data(), c->pool.p, sizeof(PoolPartial) * blocks, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  double cnt = 0, sum = 0, sumsq = 0, mn = INFINITY, mx = -INFINITY;
  for (const auto &p : h) { cnt += p.cnt; sum += p.sum; sumsq += p.sumsq; mn = std::fmin(mn, p.mn); mx = std::fmax(mx, p.mx); }
  const double mean_s = sum / cnt;
  out[0] = cnt; out[1] = shift + mean_s;
  out[2] = cnt > 1 ? (sumsq - cnt * mean_s * mean_s) / (cnt - 1) : 0.0;
  out[3] = mn; out[4] = mx;
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
  if (!(cov > 0.0)) return fail(RSF_ERR_INVALID, "rsf_pool_kde: the samples have zero variance (singular KDE)");
  const int blocks = (int)std::min<int64_t>(kPoolBlocks, (n + kKdeTile - 1) / kKdeTile);
  DevBuf &ws = c->poolws;
  if ((rc = ensure(ws, (size_t)blocks * (size_t)m * sizeof(double)))) return rc;
  hipLaunchKernelGGL(pool_kde_kernel, dim3(blocks), dim3(kMaxBlock), 0, c->stream, n, dx, stride, (int)m, dg, 0.5 / cov,
                     (double *)ws.p);
  hipLaunchKernelGGL(pool_kde_reduce_kernel, dim3((m + kMaxBlock - 1) / kMaxBlock), dim3(kMaxBlock), 0, c->stream, blocks, (int)m,
                     (const double *)ws.p, 1.0 / ((double)n * std::sqrt(2.0 * 3.14159265358979323846 * cov)), dd);
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
  hipLaunchKernelGGL(pool_hist_kernel, dim3(blocks), dim3(kMaxBlock), (size_t)nb * sizeof(unsigned int), c->stream, n, dx, stride,
                     (int)nbins, lo, hi, (double)nbins / (hi - lo), (hi - lo) / (double)nbins, (unsigned long long *)ws.p);
  hipLaunchKernelGGL(pool_hist_finish_kernel, dim3((nb + kMaxBlock - 1) / kMaxBlock), dim3(kMaxBlock), 0, c->stream, nb,
                     (const unsigned long long *)ws.p, dout);
  if ((rc = copy_back(c, SLOT_POOL_OUT, counts, (size_t)nb * sizeof(double)))) return rc;
  return finish(c);
}

}  // extern "C"
