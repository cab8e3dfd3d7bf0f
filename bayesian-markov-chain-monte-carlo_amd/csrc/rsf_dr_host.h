// rsf_dr_host.h — the host-side argument checks the delayed-rejection entry points share (internal: not installed): rsf_dr.hip's
// rsf_dr_*, rsf_law_dr.hip's rsf_law_dr_*, rsf_stiff.hip's rsf_stiff_* and rsf_kstiff.hip's rsf_kstiff_*.  Host code only; the argument block DrArgs is
// rsf_kernels_dr.h's, the wider one of the rsf_kstiff_* calls rsf_kernels_kstiff.h's.
#pragma once
#include <cmath>
#include <type_traits>

#include "../../include/rsf_observe.h"
#include "rsf_host.h"
#include "rsf_kernels_dr.h"

#pragma GCC visibility push(hidden)

namespace rsfh {

using rsfk::DrArgs;

// The trait of an argument block whose chains carry the stiffness as the LAST of d = 2 or 4 coordinates, in every call of the
// family; the unit that owns such a block says so by a specialisation (rsf_kstiff.hip for rsf_kernels_kstiff.h's KDrArgs).  Every
// other block takes rsf_dr.h's dimensions: d = 1 or 3 where the call solves, 1 to RSF_DR_MAX_PARAMS where it does not.
template <class ARGS> struct stiffness_last : std::false_type {};

// what the calls share: the chains and their groups, the box and the Philox stream; iterations first .. first + count - 1.
// whole_blocks: a group's chains are whole workgroups (the calls that solve)
// ARGS: DrArgs, or a family's own block; the dimensions a block takes are its trait's (stiffness_last)
template <class ARGS>
inline int set_chains(const char *fn, const rsf_ctx *c, int64_t n, int32_t d, bool solve, int32_t n_groups, const double *lo, const double *hi, uint64_t seed,
               int64_t offset, int64_t first, int64_t count, ARGS &A) {
  if constexpr (stiffness_last<ARGS>::value) {
    if (d != 2 && d != 4) return fail(RSF_ERR_INVALID, "%s: need d = 2 or 4", fn);
  } else if (solve ? (d != 1 && d != 3) : (d < 1 || d > RSF_DR_MAX_PARAMS)) {
    return fail(RSF_ERR_INVALID, "%s: need %s", fn, solve ? "d = 1 or 3" : "1 <= d <= 3");
  }
  if (n < 1) return fail(RSF_ERR_INVALID, "%s: need n >= 1", fn);
  if (n_groups < 1 || n_groups > RSF_DR_MAX_GROUPS) return fail(RSF_ERR_INVALID, "%s: need 1 <= n_groups <= %d", fn, RSF_DR_MAX_GROUPS);
  if (n_groups > 1 && (n % n_groups || (solve && (n / n_groups) % c->block)))
    return fail(RSF_ERR_INVALID, "%s: with n_groups > 1, n / n_groups must be a whole number%s", fn, solve ? " of workgroups (the ctx's block_threads)" : "");
  if (offset < 0) return fail(RSF_ERR_INVALID, "%s: offset must be >= 0", fn);
  if (first < 1 || first + count > ((int64_t)1 << 32)) return fail(RSF_ERR_INVALID, "%s: the Philox iterations must lie in 1 .. 2^32 - 1", fn);
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p])) return fail(RSF_ERR_INVALID, "%s: need finite lo[%d] < hi[%d]", fn, p, p);
    A.lo[p] = lo[p]; A.hi[p] = hi[p];
  }
  A.n = n; A.offset = offset; A.seed = seed; A.iter = (uint32_t)first;
  A.group_chains = n_groups > 1 ? n / n_groups : 0;
  return RSF_OK;
}

// chol[n_groups][d (d + 1) / 2], HOST: every entry finite, every diagonal entry positive → the ctx's poolws workspace, in A.chol.
// One copy; the stream is synchronised before the caller's array may go away.
template <class ARGS>
inline int set_factors(const char *fn, rsf_ctx *c, int32_t d, int32_t n_groups, const double *chol, ARGS &A) {
  const int ne = d * (d + 1) / 2;
  for (int g = 0; g < n_groups; ++g)
    for (int p = 0, e = 0; p < d; ++p)
      for (int r = 0; r <= p; ++r, ++e) {
        const double v = chol[g * ne + e];
        if (!std::isfinite(v) || (r == p && !(v > 0.0)))
          return fail(RSF_ERR_INVALID, "%s: chol of group %d is not a lower triangular factor with a positive finite diagonal (entry [%d][%d])", fn, g, p, r);
      }
  const size_t bytes = (size_t)n_groups * ne * sizeof(double);
  if (int rc = ensure(c->poolws, bytes)) return rc;
  HIP_TRY(hipMemcpyAsync(c->poolws.p, chol, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  A.chol = (const double *)c->poolws.p;
  return RSF_OK;
}

// the law and the observable of a call (rsf_law_dr.hip, rsf_stiff.hip, rsf_kstiff.hip): rsf_law_observe's checks and messages under the caller's name
inline int check_law(const char *fn, int32_t law, int32_t observable) {
  if (law != RSF_LAW_AGEING && law != RSF_LAW_SLIP) return fail(RSF_ERR_INVALID, "%s: law is RSF_LAW_AGEING (0) or RSF_LAW_SLIP (1), not %d", fn, law);
  if (observable != RSF_OBS_ACC && observable != RSF_OBS_MU && observable != RSF_OBS_THETA && observable != RSF_OBS_VELOCITY)
    return fail(RSF_ERR_INVALID, "%s: observable is RSF_OBS_ACC (0), RSF_OBS_MU (1), RSF_OBS_THETA (2) or RSF_OBS_VELOCITY (3), not %d", fn, observable);
  return RSF_OK;
}

inline bool good_gamma(double gamma) { return std::isfinite(gamma) && gamma > 0.0 && gamma <= 1.0; }

}  // namespace rsfh

#pragma GCC visibility pop
