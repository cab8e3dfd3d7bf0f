// rsf_fit_host.h — the host-side argument checks the least-squares entry points share (internal: not installed): rsf_fit.hip's
// rsf_fit_* and rsf_law_fit.hip's rsf_law_fit_*.  Host code only; the argument block FitArgs is rsf_kernels_fit.h's.
#pragma once
#include <cmath>

#include "rsf_host.h"
#include "rsf_kernels_fit.h"

#pragma GCC visibility push(hidden)

namespace rsfh {

using rsfk::FitArgs;

inline int set_box(const char *fn, int d, const double *lo, const double *hi, FitArgs &A) {
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p])) return fail(RSF_ERR_INVALID, "%s: need finite lo[%d] < hi[%d]", fn, p, p);
    A.lo[p] = lo[p]; A.hi[p] = hi[p];
  }
  return RSF_OK;
}

// what the calls with a solve share: the shape, the model's integrator, the split of the starts over the observation series
inline int set_solve(const char *fn, const rsf_ctx *c, int64_t n, int32_t d, int32_t n_groups, double fd, FitArgs &A) {
  if (n < 1 || (d != 1 && d != 3)) return fail(RSF_ERR_INVALID, "%s: need n >= 1 and d = 1 or 3", fn);
  if (!std::isfinite(fd) || !(fd > 0.0)) return fail(RSF_ERR_INVALID, "%s: fd must be finite and > 0", fn);
  if (c->m.flags & RSF_FLAG_DOP853)
    return fail(RSF_ERR_UNSUPPORTED, "%s: a model flagged RSF_FLAG_DOP853 is not supported (the solve is the float64 RK4)", fn);
  // a workgroup's starts share one observation series: rsf_mcmc_init's rule for chain groups
  if (n_groups < 1 || n % n_groups || (n_groups > 1 && (n / n_groups) % c->block))
    return fail(RSF_ERR_INVALID, "%s: need n_groups >= 1 and, with more than one, n/n_groups a whole multiple of a workgroup's threads (%d)", fn, c->block);
  A.n = n; A.fd = fd;
  A.group_starts = n_groups > 1 ? n / n_groups : 0;
  return RSF_OK;
}

// the iteration count and the tolerance of a fused run
inline int set_run(const char *fn, int32_t n_iter, double ftol, FitArgs &A) {
  if (n_iter < 1 || n_iter > RSF_FIT_MAX_ITER) return fail(RSF_ERR_INVALID, "%s: need 1 <= n_iter <= %d", fn, RSF_FIT_MAX_ITER);
  if (!std::isfinite(ftol) || ftol < 0.0) return fail(RSF_ERR_INVALID, "%s: ftol must be finite and >= 0", fn);
  A.ftol = ftol; A.n_iter = n_iter;
  return RSF_OK;
}

}  // namespace rsfh

#pragma GCC visibility pop
