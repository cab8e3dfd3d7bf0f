// rsf_finish.cpp — the host arithmetic that turns the device partials into the reported statistics: rsf_diag_finish,
// rsf_diag_rank_finish, rsf_predict_finish, rsf_predict_psis_finish, rsf_pool_joint_finish, rsf_pool_hpd_levels, rsf_evidence_finish,
// rsf_smc_section, rsf_smc_increment, rsf_smc_log_evidence, rsf_fit_laplace, rsf_grid_finish (and rsfh::grid_check, the grid's
// argument check, which rsf_grid.hip shares).  No ctx, no GPU:
// plain C++, the public headers and the standard library only.
#include <cmath>
#include <cstdint>
#include <algorithm>
#include <vector>

#include "../../include/rsf_abi.h"
#include "../../include/rsf_diag.h"
#include "../../include/rsf_evidence.h"
#include "../../include/rsf_fit.h"
#include "../../include/rsf_grid.h"
#include "../../include/rsf_joint.h"
#include "../../include/rsf_predict.h"
#include "../../include/rsf_psis.h"
#include "../../include/rsf_smc.h"

#pragma GCC visibility push(hidden)
namespace rsfh {
int fail(int code, const char *fmt, ...);  // rsf_hip.hip: formats rsf_last_error()'s message, returns code
int grid_check(const char *fn, int d, int dmin, const int32_t *n, const double *x, const double *w, int64_t *N);  // declared in rsf_host.h
}
#pragma GCC visibility pop
using rsfh::fail;

int rsfh::grid_check(const char *fn, int d, int dmin, const int32_t *n, const double *x, const double *w, int64_t *N) {
  if (d < dmin || d > RSF_GRID_MAX_PARAMS) return fail(RSF_ERR_INVALID, "%s: need %d <= d <= %d", fn, dmin, RSF_GRID_MAX_PARAMS);
  int64_t total = 1, at = 0;
  for (int p = 0; p < d; ++p) {
    if (n[p] < 2) return fail(RSF_ERR_INVALID, "%s: axis %d has %d nodes, fewer than 2", fn, p, (int)n[p]);
    total *= n[p];
    if (total >= (int64_t)1 << 31) return fail(RSF_ERR_INVALID, "%s: the grid has 2^31 nodes or more", fn);
    for (int k = 0; k < n[p]; ++k, ++at) {
      if (!std::isfinite(x[at]) || (k > 0 && !(x[at] > x[at - 1])))
        return fail(RSF_ERR_INVALID, "%s: the nodes of axis %d are not finite and strictly increasing (node %d)", fn, p, k);
      if (w && (!std::isfinite(w[at]) || !(w[at] > 0.0))) return fail(RSF_ERR_INVALID, "%s: weight %d of axis %d is not finite and > 0", fn, k, p);
    }
  }
  *N = total;
  return RSF_OK;
}

extern "C" {

int rsf_diag_finish(int64_t n, int32_t d, int64_t S, const double *center, const double *partials, int64_t n_lags, double *out) {
  if (!center || !partials || !out) return fail(RSF_ERR_INVALID, "rsf_diag_finish: NULL argument");
  if (n < 4 || d < 1 || d > RSF_MAX_PARAMS || S < 0)
    return fail(RSF_ERR_INVALID, "rsf_diag_finish: need n_iters >= 4, 1 <= n_params <= %d, chains_per_superchain >= 0", RSF_MAX_PARAMS);
  const int64_t N = n / 2;
  if (n_lags < 2 || n_lags > N) return fail(RSF_ERR_INVALID, "rsf_diag_finish: n_lags %lld outside [2, %lld]", (long long)n_lags, (long long)N);
  const double Nd = (double)N;
  std::vector<double> r((size_t)n_lags);
  for (int p = 0; p < d; ++p) {
    const double *q = partials + (int64_t)p * (RSF_DIAG_HEAD + n_lags);
    double *o = out + (int64_t)p * RSF_DIAG_OUT;
    for (int f = 0; f < RSF_DIAG_OUT; ++f) o[f] = NAN;
    o[RSF_DIAG_K] = q[4];
    o[RSF_DIAG_LAGS_COMPLETE] = 1.0;
    bool finite = std::isfinite(center[p]);
    for (int64_t f = 0; f < RSF_DIAG_HEAD + n_lags; ++f) finite = finite && std::isfinite(q[f]);
    if (!finite) continue;  // a non-finite draw: every statistic of this parameter is NaN
    const double Mp = q[0], ybar = q[1] / Mp, W = q[3] / Mp;
    const double BN = (q[2] - q[1] * ybar) / (Mp - 1.0);
    const double var_plus = (Nd - 1.0) / Nd * W + BN;
    o[RSF_DIAG_MEAN] = center[p] + ybar;
    o[RSF_DIAG_VAR_PLUS] = var_plus;
    o[RSF_DIAG_W] = W;
    o[RSF_DIAG_B_OVER_N] = BN;
    const double K = q[4];
    if (S > 0 && K > 1.0) {
      const double B_nu = (q[6] - q[5] * q[5] / K) / (K - 1.0), W_nu = (q[7] + q[8]) / K;
      if (W_nu > 0.0) o[RSF_DIAG_NESTED_RHAT] = std::sqrt(1.0 + B_nu / W_nu);
    }
    if (!(W > 0.0)) continue;  // every split chain constant
    o[RSF_DIAG_SPLIT_RHAT] = std::sqrt(var_plus / W);
    // ArviZ's _ess on the split chains, step by step (tests/diagnostics_reference.py), with the sequence cut at n_lags
    auto rho = [&](int64_t t) { return 1.0 - (W - q[RSF_DIAG_HEAD + t] / Mp) / var_plus; };
    std::fill(r.begin(), r.end(), 0.0);
    double ev = 1.0, od = rho(1);
    r[0] = ev; r[1] = od;
    int64_t t = 1;
    const int64_t lim = std::min(N - 3, n_lags - 2);  // the pair (t+1, t+2) needs lag t+2 < n_lags
    while (t < lim && ev + od > 0.0) {  // Geyer's initial positive sequence
      ev = rho(t + 1);
      od = rho(t + 2);
      if (ev + od >= 0.0) { r[t + 1] = ev; r[t + 2] = od; }
      t += 2;
    }
    o[RSF_DIAG_LAGS_COMPLETE] = (ev + od > 0.0 && t < N - 3) ? 0.0 : 1.0;
    const int64_t max_t = t - 2;
    if (ev > 0.0) r[max_t + 1] = ev;
    for (int64_t u = 1; u <= max_t - 2; u += 2)  // Geyer's initial monotone sequence
      if (r[u + 1] + r[u + 2] > r[u - 1] + r[u]) { r[u + 1] = 0.5 * (r[u - 1] + r[u]); r[u + 2] = r[u + 1]; }
    double tau = 0.0;
    for (int64_t u = 0; u <= max_t; ++u) tau += r[u];
    tau = -1.0 + 2.0 * tau + r[max_t + 1];
    const double MN = Mp * Nd;
    tau = std::max(tau, 1.0 / std::log10(MN));
    o[RSF_DIAG_TAU] = tau;
    o[RSF_DIAG_ESS] = MN / tau;
    o[RSF_DIAG_MCSE_MEAN] = std::sqrt(var_plus / o[RSF_DIAG_ESS]);
  }
  return RSF_OK;
}

int rsf_diag_rank_finish(int64_t n, int32_t d, const double *stats, int32_t n_probs, const double *partials, int64_t n_lags, double *out) {
  if (!stats || !partials || !out) return fail(RSF_ERR_INVALID, "rsf_diag_rank_finish: NULL argument");
  if (n < 4 || d < 1 || d > RSF_MAX_PARAMS || n_probs < 0)
    return fail(RSF_ERR_INVALID, "rsf_diag_rank_finish: need n_iters >= 4, 1 <= n_params <= %d, n_probs >= 0", RSF_MAX_PARAMS);
  const int64_t N = n / 2;
  if (n_lags < 2 || n_lags > N) return fail(RSF_ERR_INVALID, "rsf_diag_rank_finish: n_lags %lld outside [2, %lld]", (long long)n_lags, (long long)N);
  const double zero[RSF_MAX_PARAMS] = {0.0, 0.0, 0.0};
  std::vector<double> o((size_t)(RSF_DIAG_RANK_SERIES * d * RSF_DIAG_OUT));
  for (int q = 0; q < RSF_DIAG_RANK_SERIES; ++q) {
    const int rc = rsf_diag_finish(n, d, 0, zero, partials + (int64_t)q * d * (RSF_DIAG_HEAD + n_lags), n_lags, o.data() + q * d * RSF_DIAG_OUT);
    if (rc) return rc;
  }
  const int ns = RSF_DIAG_RANK_STATS + n_probs;
  for (int p = 0; p < d; ++p) {
    const double *st = stats + (int64_t)p * ns;
    double *r = out + (int64_t)p * RSF_DIAG_RANK_OUT;
    double ess[RSF_DIAG_RANK_SERIES], rh[RSF_DIAG_RANK_SERIES];
    bool complete = true;
    for (int q = 0; q < RSF_DIAG_RANK_SERIES; ++q) {
      const double *f = o.data() + (q * d + p) * RSF_DIAG_OUT;
      const double T = partials[((int64_t)q * d + p) * (RSF_DIAG_HEAD + n_lags)] * (double)N;  // M' N
      ess[q] = st[RSF_DIAG_RANK_CONST + q] != 0.0 ? T : f[RSF_DIAG_ESS];  // ArviZ _ess: a constant series has ess = M'N (tau = 1)
      rh[q] = f[RSF_DIAG_SPLIT_RHAT];
      complete = complete && f[RSF_DIAG_LAGS_COMPLETE] != 0.0;
    }
    for (int f = 0; f < RSF_DIAG_RANK_OUT; ++f) r[f] = NAN;
    r[RSF_DIAG_RANK_LAGS_COMPLETE] = complete ? 1.0 : 0.0;
    if (st[RSF_DIAG_RANK_NONFINITE] != 0.0) continue;
    auto nanmax = [](double a, double b) { return std::isnan(a) || std::isnan(b) ? NAN : std::max(a, b); };
    auto nanmin = [](double a, double b) { return std::isnan(a) || std::isnan(b) ? NAN : std::min(a, b); };
    r[RSF_DIAG_RANK_RHAT_BULK] = rh[0];
    r[RSF_DIAG_RANK_RHAT_TAIL] = rh[1];
    r[RSF_DIAG_RANK_RHAT] = nanmax(rh[0], rh[1]);
    r[RSF_DIAG_RANK_ESS_BULK] = ess[0];
    r[RSF_DIAG_RANK_ESS_Q05] = ess[2];
    r[RSF_DIAG_RANK_ESS_Q95] = ess[3];
    r[RSF_DIAG_RANK_ESS_TAIL] = nanmin(ess[2], ess[3]);
  }
  return RSF_OK;
}

int rsf_predict_finish(int64_t n_rows, const double *partials, const double *center_y, const double *center_l, double *out_rows,
                       double *out_totals) {
  if (!partials || !center_y || !center_l || !out_rows || !out_totals) return fail(RSF_ERR_INVALID, "rsf_predict_finish: NULL argument");
  if (n_rows < 1) return fail(RSF_ERR_INVALID, "rsf_predict_finish: n_rows < 1");
  const double n = partials[0];
  double elpd = 0.0, pw = 0.0;
  for (int64_t k = 0; k < n_rows; ++k) {
    const double *p = partials + RSF_PREDICT_HEAD + k * RSF_PREDICT_FIELDS;
    double *o = out_rows + k * RSF_PREDICT_OUT;
    bool finite = p[RSF_PREDICT_NONFINITE] == 0.0 && std::isfinite(center_y[k]) && std::isfinite(center_l[k]);
    for (int f = 0; f < RSF_PREDICT_NONFINITE; ++f) finite = finite && std::isfinite(p[f]);
    if (!finite) {  // a non-finite draw: every statistic of this output time is NaN
      for (int f = 0; f < RSF_PREDICT_OUT; ++f) o[f] = NAN;
    } else {
      const double my = p[RSF_PREDICT_SUM_Y] / n, ml = p[RSF_PREDICT_SUM_L] / n;
      o[RSF_PREDICT_MEAN] = center_y[k] + my;
      o[RSF_PREDICT_VAR] = (p[RSF_PREDICT_SUM_Y2] - p[RSF_PREDICT_SUM_Y] * my) / (n - 1.0);
      o[RSF_PREDICT_PIT] = p[RSF_PREDICT_SUM_PHI] / n;
      o[RSF_PREDICT_LPD] = center_l[k] + std::log(p[RSF_PREDICT_SUM_EXP] / n);
      o[RSF_PREDICT_P_WAIC] = (p[RSF_PREDICT_SUM_L2] - p[RSF_PREDICT_SUM_L] * ml) / (n - 1.0);
    }
    elpd += o[RSF_PREDICT_LPD] - o[RSF_PREDICT_P_WAIC];
    pw += o[RSF_PREDICT_P_WAIC];
  }
  const double nr = (double)n_rows, me = elpd / nr;
  double ss = 0.0;
  for (int64_t k = 0; k < n_rows; ++k) {
    const double e = out_rows[k * RSF_PREDICT_OUT + RSF_PREDICT_LPD] - out_rows[k * RSF_PREDICT_OUT + RSF_PREDICT_P_WAIC] - me;
    ss += e * e;
  }
  out_totals[RSF_PREDICT_MEAN_STD2] = partials[1] / n;
  out_totals[RSF_PREDICT_ELPD_WAIC] = elpd;
  out_totals[RSF_PREDICT_P_WAIC_TOTAL] = pw;
  out_totals[RSF_PREDICT_ELPD_WAIC_SE] = std::sqrt(nr * (ss / (nr - 1.0)));
  return RSF_OK;
}

int rsf_predict_psis_finish(int64_t nout, int64_t n, const double *psis_rows, const double *lpd_rows, double *out_totals) {
  if (!psis_rows || !lpd_rows || !out_totals) return fail(RSF_ERR_INVALID, "rsf_predict_psis_finish: NULL argument");
  if (nout < 1 || n < 1) return fail(RSF_ERR_INVALID, "rsf_predict_psis_finish: nout < 1 or n < 1");
  const double thr = n > 1 ? std::min(1.0 - 1.0 / std::log10((double)n), 0.7) : -INFINITY;
  double elpd = 0.0, p = 0.0, kmax = -INFINITY, high = 0.0;
  bool ok = true;
  for (int64_t k = 0; k < nout; ++k) {
    const double e = psis_rows[k * RSF_PSIS_OUT + RSF_PSIS_ELPD], pk = psis_rows[k * RSF_PSIS_OUT + RSF_PSIS_PARETO_K];
    ok = ok && std::isfinite(e) && !std::isnan(pk) && std::isfinite(lpd_rows[k]);
    elpd += e;
    p += lpd_rows[k] - e;
    kmax = std::max(kmax, pk);
    high += pk > thr ? 1.0 : 0.0;
  }
  const double nr = (double)nout, me = elpd / nr;
  double ss = 0.0;
  for (int64_t k = 0; k < nout; ++k) {
    const double e = psis_rows[k * RSF_PSIS_OUT + RSF_PSIS_ELPD] - me;
    ss += e * e;
  }
  out_totals[RSF_PSIS_ELPD_LOO] = ok ? elpd : NAN;
  out_totals[RSF_PSIS_P_LOO] = ok ? p : NAN;
  out_totals[RSF_PSIS_ELPD_LOO_SE] = ok ? std::sqrt(nr * (ss / (nr - 1.0))) : NAN;
  out_totals[RSF_PSIS_K_THRESHOLD] = thr;
  out_totals[RSF_PSIS_N_HIGH_K] = ok ? high : NAN;
  out_totals[RSF_PSIS_MAX_PARETO_K] = ok ? kmax : NAN;
  return RSF_OK;
}


int rsf_pool_joint_finish(int32_t d, const double *partials, const double *center, double *out) {
  if (!partials || !center || !out) return fail(RSF_ERR_INVALID, "rsf_pool_joint_finish: NULL argument");
  if (d < 1 || d > RSF_JOINT_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_pool_joint_finish: need 1 <= d <= %d", RSF_JOINT_MAX_PARAMS);
  const double n = partials[0], *s1 = partials + RSF_JOINT_HEAD, *s2 = s1 + d;
  double *mean = out, *cov = out + d, *corr = cov + d * d, sd[RSF_JOINT_MAX_PARAMS];
  for (int p = 0; p < d; ++p) mean[p] = center[p] + s1[p] / n;
  int e = 0;
  for (int p = 0; p < d; ++p)
    for (int q = p; q < d; ++q, ++e)
      cov[p * d + q] = cov[q * d + p] = n >= 2.0 ? (s2[e] - s1[p] * (s1[q] / n)) / (n - 1.0) : NAN;
  for (int p = 0; p < d; ++p) sd[p] = cov[p * d + p] > 0.0 ? std::sqrt(cov[p * d + p]) : NAN;  // zero variance: NaN row and column
  for (int p = 0; p < d; ++p)
    for (int q = 0; q < d; ++q) {
      const double r = cov[p * d + q] / (sd[p] * sd[q]);
      corr[p * d + q] = p == q && !std::isnan(r) ? 1.0 : std::fmax(-1.0, std::fmin(1.0, r));  // numpy.corrcoef clips too
      if (std::isnan(r)) corr[p * d + q] = NAN;  // (fmin and fmax drop a NaN)
    }
  return RSF_OK;
}

int rsf_pool_hpd_levels(int64_t m, const double *weights, int32_t n_probs, const double *probs, double *levels) {
  if (!weights || !probs || !levels) return fail(RSF_ERR_INVALID, "rsf_pool_hpd_levels: NULL argument");
  if (m < 1 || n_probs < 1) return fail(RSF_ERR_INVALID, "rsf_pool_hpd_levels: need m >= 1 and n_probs >= 1");
  for (int k = 0; k < n_probs; ++k)
    if (!(probs[k] > 0.0 && probs[k] < 1.0)) return fail(RSF_ERR_INVALID, "rsf_pool_hpd_levels: probs[%d] is not strictly inside (0, 1)", k);
  std::vector<double> w(weights, weights + m);
  for (int64_t i = 0; i < m; ++i)
    if (!(w[(size_t)i] >= 0.0) || !std::isfinite(w[(size_t)i]))
      return fail(RSF_ERR_INVALID, "rsf_pool_hpd_levels: weights[%lld] is negative or not finite", (long long)i);
  std::sort(w.begin(), w.end(), [](double a, double b) { return a > b; });
  std::vector<double> cum(w.size());
  double total = 0.0;
  for (size_t i = 0; i < w.size(); ++i) cum[i] = total += w[i];  // descending: the mass of {weight >= w[i]} once i is the last of its ties
  if (!(total > 0.0) || !std::isfinite(total)) return fail(RSF_ERR_INVALID, "rsf_pool_hpd_levels: the weights sum to 0 (or overflow)");
  for (int k = 0; k < n_probs; ++k) {
    // the first index whose running mass reaches p total: its value's ties reach it too, and no larger value does
    const size_t i = (size_t)(std::lower_bound(cum.begin(), cum.end(), probs[k] * total) - cum.begin());
    levels[k] = w[std::min(i, w.size() - 1)];
  }
  return RSF_OK;
}

int rsf_evidence_finish(const double *partials, double r, double lstar, double ess_factor, double shape, int32_t d, const double *lo,
                        const double *hi, double *out) {
  if (!partials || !out || (d > 0 && (!lo || !hi))) return fail(RSF_ERR_INVALID, "rsf_evidence_finish: NULL argument");
  const double n1 = partials[0], n2 = partials[1], n2f = partials[2];
  if (!(n1 >= 1.0) || !(n2 >= 1.0)) return fail(RSF_ERR_INVALID, "rsf_evidence_finish: need n1 >= 1 and n2 >= 1 draws in the summed partials");
  if (!std::isfinite(lstar) || !std::isfinite(r) || !(r > 0.0)) return fail(RSF_ERR_INVALID, "rsf_evidence_finish: need finite lstar and finite r > 0");
  if (!(ess_factor > 0.0 && ess_factor <= 1.0)) return fail(RSF_ERR_INVALID, "rsf_evidence_finish: ess_factor outside (0, 1]");
  if (!std::isfinite(shape) || !(shape > 0.0)) return fail(RSF_ERR_INVALID, "rsf_evidence_finish: shape must be finite and > 0");
  if (d < 0 || d > RSF_EVIDENCE_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_evidence_finish: d outside 0..%d", RSF_EVIDENCE_MAX_PARAMS);
  double logvol = 0.0;
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p])) return fail(RSF_ERR_INVALID, "rsf_evidence_finish: need finite lo[%d] < hi[%d]", p, p);
    logvol += std::log(hi[p] - lo[p]);
  }
  const double rn = n2f > 0.0 ? (partials[3] / n2) / (partials[4] / n1) : 0.0;
  out[0] = rn;
  out[1] = rn > 0.0 ? std::log(rn) + lstar : -INFINITY;
  out[2] = out[1] - logvol + std::lgamma(shape) - shape * std::log(3.14159265358979323846);
  if (n1 < 2.0 || n2 < 2.0 || !(n2f > 0.0)) {
    out[3] = INFINITY;  // no error estimate
  } else {
    const double e1 = partials[5] / n2, v1 = (partials[6] - partials[5] * e1) / (n2 - 1.0);
    const double e2 = partials[7] / n1, v2 = (partials[8] - partials[7] * e2) / (n1 - 1.0);
    const double re2 = std::fmax(v1, 0.0) / (n2 * e1 * e1) + std::fmax(v2, 0.0) / (ess_factor * n1 * e2 * e2);
    out[3] = std::sqrt(re2);
  }
  return RSF_OK;
}

int rsf_smc_section(double target, int32_t m, const double *sums, int32_t *k) {
  if (!sums || !k) return fail(RSF_ERR_INVALID, "rsf_smc_section: NULL argument");
  if (m < 1 || m > RSF_SMC_MAX_CANDIDATES || !(target >= 0.0)) return fail(RSF_ERR_INVALID, "rsf_smc_section: need 1 <= m <= %d and target >= 0", RSF_SMC_MAX_CANDIDATES);
  int32_t j = 0;
  while (j < m && sums[2 * j] * sums[2 * j] >= target * sums[2 * j + 1]) ++j;  // a NaN sum compares false: the search stops there
  *k = j;
  return RSF_OK;
}

int rsf_smc_increment(int64_t n, double sum_w, double delta, double lmax, double *out) {
  if (!out) return fail(RSF_ERR_INVALID, "rsf_smc_increment: NULL argument");
  if (n < 1 || !(sum_w > 0.0) || !std::isfinite(sum_w) || !std::isfinite(delta) || !std::isfinite(lmax))
    return fail(RSF_ERR_INVALID, "rsf_smc_increment: need n >= 1, finite sum_w > 0, finite delta and lmax");
  *out = std::log(sum_w / (double)n) + delta * lmax;
  return RSF_OK;
}

int rsf_smc_log_evidence(double log_integral, double shape, int32_t d, const double *lo, const double *hi, double *out) {
  if (!out || !lo || !hi) return fail(RSF_ERR_INVALID, "rsf_smc_log_evidence: NULL argument");
  if (!std::isfinite(shape) || !(shape > 0.0)) return fail(RSF_ERR_INVALID, "rsf_smc_log_evidence: shape must be finite and > 0");
  if (d < 1 || d > RSF_SMC_MAX_PARAMS) return fail(RSF_ERR_INVALID, "rsf_smc_log_evidence: d outside 1..%d", RSF_SMC_MAX_PARAMS);
  double logvol = 0.0;
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p])) return fail(RSF_ERR_INVALID, "rsf_smc_log_evidence: need finite lo[%d] < hi[%d]", p, p);
    logvol += std::log(hi[p] - lo[p]);
  }
  *out = log_integral - logvol + std::lgamma(shape) - shape * std::log(3.14159265358979323846);
  return RSF_OK;
}

int rsf_fit_laplace(int32_t d, int64_t n_obs, double shape, double ssq, const double *jtj, const double *lo, const double *hi, double *out) {
  if (!jtj || !lo || !hi || !out) return fail(RSF_ERR_INVALID, "rsf_fit_laplace: NULL argument");
  if (d < 1 || d > RSF_FIT_MAX_PARAMS || n_obs <= d) return fail(RSF_ERR_INVALID, "rsf_fit_laplace: need 1 <= d <= %d and n_obs > d", RSF_FIT_MAX_PARAMS);
  if (!std::isfinite(shape) || !(shape > 0.0) || !std::isfinite(ssq) || !(ssq > 0.0))
    return fail(RSF_ERR_INVALID, "rsf_fit_laplace: shape and ssq must be finite and > 0");
  // jtj = L L^T (lower triangle read); log det from the pivots, the inverse from L^-1
  double L[RSF_FIT_MAX_PARAMS * RSF_FIT_MAX_PARAMS] = {}, Li[RSF_FIT_MAX_PARAMS * RSF_FIT_MAX_PARAMS] = {}, logdet = 0.0;
  for (int p = 0; p < d; ++p)
    for (int r = 0; r <= p; ++r) {
      double s = jtj[p * d + r];
      for (int k = 0; k < r; ++k) s -= L[p * d + k] * L[r * d + k];
      if (r < p) { L[p * d + r] = s / L[r * d + r]; continue; }
      if (!(s > 0.0) || !std::isfinite(s)) return fail(RSF_ERR_NOT_POSDEF, "rsf_fit_laplace: jtj is not positive definite (pivot %d)", p);
      L[p * d + p] = std::sqrt(s);
      logdet += std::log(s);
    }
  for (int c = 0; c < d; ++c)  // column c of L^-1 by forward substitution
    for (int p = c; p < d; ++p) {
      double s = p == c ? 1.0 : 0.0;
      for (int k = c; k < p; ++k) s -= L[p * d + k] * Li[k * d + c];
      Li[p * d + c] = s / L[p * d + p];
    }
  const double s2 = ssq / (double)(n_obs - d);
  for (int p = 0; p < d; ++p)
    for (int r = 0; r < d; ++r) {
      double s = 0.0;
      for (int k = std::max(p, r); k < d; ++k) s += Li[k * d + p] * Li[k * d + r];  // (L^-T L^-1)_pr
      out[p * d + r] = s2 * s;
    }
  const double two_pi = 6.28318530717958647692;
  const double logi = -shape * std::log(ssq) + 0.5 * d * std::log(two_pi) - 0.5 * (logdet + d * std::log(2.0 * shape / ssq));
  out[d * d] = logi;
  return rsf_smc_log_evidence(logi, shape, d, lo, hi, out + d * d + 1);
}

// the trapezoid CDF of the node density m[k] / w[k] on the nodes x[n], the cells added in node order, divided by its last entry; all 0
// where there is no mass
static void grid_cum(int n, const double *x, const double *w, const double *m, int64_t stride, double *F) {
  double acc = 0.0;
  F[0] = 0.0;
  for (int k = 1; k < n; ++k) {
    acc += 0.5 * (m[(k - 1) * stride] / w[k - 1] + m[k * stride] / w[k]) * (x[k] - x[k - 1]);
    F[k] = acc;
  }
  if (acc > 0.0)
    for (int k = 1; k < n; ++k) F[k] /= acc;
}

int rsf_grid_finish(int32_t d, const int32_t *n, const double *x, const double *w, int32_t coords, double center, double shape, const double *lo,
                    const double *hi, double lmax, const double *fields, double *head, double *mass1, double *mass2, double *pair, double *cum1,
                    double *cum2) {
  if (!n || !x || !w || !lo || !hi || !fields || !head || !mass1 || !mass2 || !pair || !cum1 || !cum2)
    return fail(RSF_ERR_INVALID, "rsf_grid_finish: NULL argument");
  int64_t N;
  if (int rc = rsfh::grid_check(__func__, d, 1, n, x, w, &N)) return rc;
  if (coords != RSF_GRID_PLAIN && coords != RSF_GRID_PRODUCT) return fail(RSF_ERR_INVALID, "rsf_grid_finish: coords is neither RSF_GRID_PLAIN nor RSF_GRID_PRODUCT");
  if (coords == RSF_GRID_PRODUCT && d != 3) return fail(RSF_ERR_INVALID, "rsf_grid_finish: RSF_GRID_PRODUCT needs d = 3");
  if (!std::isfinite(shape) || !(shape > 0.0)) return fail(RSF_ERR_INVALID, "rsf_grid_finish: shape must be finite and > 0");
  if (!std::isfinite(center) || std::isnan(lmax) || lmax == INFINITY) return fail(RSF_ERR_INVALID, "rsf_grid_finish: need a finite center and lmax finite or -inf");
  double logvol = 0.0;
  for (int p = 0; p < d; ++p) {
    if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p])) return fail(RSF_ERR_INVALID, "rsf_grid_finish: need finite lo[%d] < hi[%d]", p, p);
    logvol += std::log(hi[p] - lo[p]);
  }
  if (coords == RSF_GRID_PRODUCT && !(lo[1] > 0.0)) return fail(RSF_ERR_INVALID, "rsf_grid_finish: RSF_GRID_PRODUCT needs lo[1] > 0");
  // an axis the grid lacks: one node 0 of weight 1
  const double one = 1.0, zero = 0.0;
  const int n1 = d > 1 ? n[1] : 1, n2 = d > 2 ? n[2] : 1;
  const double *x1 = d > 1 ? x + n[0] : &zero, *w1 = d > 1 ? w + n[0] : &one;
  const double *x2 = d > 2 ? x + n[0] + n[1] : &zero, *w2 = d > 2 ? w + n[0] + n[1] : &one;
  const int64_t ncol = (int64_t)n1 * n2;
  double neginf = 0.0;
  for (int64_t c = 0; c < ncol; ++c) neginf += fields[c * RSF_GRID_FIELDS + 5];
  for (int f = 0; f < RSF_GRID_HEAD; ++f) head[f] = NAN;
  head[3] = neginf;
  auto nan_fill = [](double *p, int64_t m) { std::fill(p, p + m, NAN); };
  double Z = 0.0;
  if (lmax != -INFINITY)
    for (int64_t c = 0; c < ncol; ++c) Z += (w1[c % n1] * w2[c / n1]) * fields[c * RSF_GRID_FIELDS];
  if (!(Z > 0.0) || !std::isfinite(Z)) {  // no finite node (or sums that are not numbers): no posterior to report
    head[1] = lmax == -INFINITY || Z == 0.0 ? -INFINITY : NAN;
    nan_fill(mass1, n1); nan_fill(mass2, n2); nan_fill(pair, ncol); nan_fill(cum1, ncol); nan_fill(cum2, n2);
    return RSF_OK;
  }
  head[0] = Z;
  head[1] = lmax + std::log(Z);
  head[2] = head[1] - logvol + std::lgamma(shape) - shape * std::log(3.14159265358979323846);
  // masses of the columns and of the upper axes' nodes
  std::fill(mass1, mass1 + n1, 0.0);
  std::fill(mass2, mass2 + n2, 0.0);
  double a1 = 0.0, m1 = 0.0, m2 = 0.0, sq = 0.0, sq2 = 0.0;
  for (int64_t c = 0; c < ncol; ++c) {
    const int i1 = (int)(c % n1), i2 = (int)(c / n1);
    const double W = w1[i1] * w2[i2], *f = fields + c * RSF_GRID_FIELDS;
    pair[c] = W * f[0] / Z;
    mass1[i1] += pair[c];
    mass2[i2] += pair[c];
    a1 += W * f[1];
    m1 += pair[c] * x1[i1];
    m2 += pair[c] * x2[i2];
    sq += W * f[3];
    sq2 += W * f[4];
  }
  const double mx0 = center + a1 / Z;  // the mean of x0
  // q0 - g summed per column: D1 = sum w0 e (q0 - g), D2 = sum w0 e (q0 - g)^2.  PLAIN: g = center.  PRODUCT: q0 = x0 / x1 and
  // q0 - g = ((x0 - center) + (center - g x1)) / x1 with g = E x0 / E x1, close to the mean of Dc
  const bool prod = coords == RSF_GRID_PRODUCT;
  const double g = prod ? mx0 / m1 : center;
  double d1 = 0.0, d2 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0, a2 = 0.0;
  for (int64_t c = 0; c < ncol; ++c) {
    const int i1 = (int)(c % n1), i2 = (int)(c / n1);
    const double W = w1[i1] * w2[i2], *f = fields + c * RSF_GRID_FIELDS;
    double D1 = f[1], D2 = f[2];
    if (prod) {
      const double e = center - g * x1[i1];
      D1 = (f[1] + e * f[0]) / x1[i1];
      D2 = (f[2] + 2.0 * e * f[1] + e * e * f[0]) / (x1[i1] * x1[i1]);
    }
    const double r1 = x1[i1] - m1, r2 = x2[i2] - m2;
    d1 += W * D1;
    d2 += W * D2;
    a2 += W * f[2];
    c01 += W * D1 * r1;
    c02 += W * D1 * r2;
    c11 += pair[c] * r1 * r1;
    c12 += pair[c] * r1 * r2;
    c22 += pair[c] * r2 * r2;
  }
  const double s0 = d1 / Z;  // E q0 - g
  double *mean = head + 4, *cov = head + 7;
  mean[0] = g + s0;
  cov[0] = d2 / Z - s0 * s0;
  if (d > 1) { mean[1] = m1; cov[1] = cov[3] = c01 / Z; cov[4] = c11; }
  if (d > 2) { mean[2] = m2; cov[2] = cov[6] = c02 / Z; cov[5] = cov[7] = c12; cov[8] = c22; }
  head[16] = mx0;
  head[17] = a2 / Z - (a1 / Z) * (a1 / Z);
  if (shape > 1.0) head[18] = 0.5 * (sq / Z) / (shape - 1.0);
  if (shape > 2.0) head[19] = 0.25 * (sq2 / Z) / ((shape - 1.0) * (shape - 2.0)) - head[18] * head[18];
  // the cumulative tables of the two upper axes
  if (d > 1) for (int i2 = 0; i2 < n2; ++i2) grid_cum(n1, x1, w1, pair + (int64_t)i2 * n1, 1, cum1 + (int64_t)i2 * n1);
  else cum1[0] = 0.0;
  if (d > 2) grid_cum(n2, x2, w2, mass2, 1, cum2);
  else cum2[0] = 0.0;
  return RSF_OK;
}

}  // extern "C"
