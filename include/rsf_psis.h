/*
 * rsf_psis.h — PSIS-LOO and the Pareto shape of pooled draws, per output time, on the series rsf_predict_partials leaves
 * (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson, Gelman, Yao, Gabry 2024).  Part of the posterior predictive checks: included
 * by rsf_predict.h, whose conventions and l_ik it shares.  Exported by librsf_hip.so only.
 */
#ifndef RSF_PSIS_H
#define RSF_PSIS_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ArviZ's psislw and _gpdfit per output time k; tests/psis_reference.py is the specification, step by step.  In short, with
 * x_i = -l_ik - max_i(-l_ik): tail_len = ceil(min(0.2 n, 3 sqrt(n / r_eff))), cutoff = max(x_(n - tail_len - 1), log(DBL_MIN))
 * (ascending order statistics, 0-based; n = 1: the index is clamped at 0), the tail is {x_i > cutoff}, strictly, n_tail its
 * size.  n_tail <= 4: pareto_k = +inf and nothing is smoothed (also a row whose ratios are all equal: ArviZ's behaviour).
 * Otherwise Zhang and Stephens' (2009) fit of the generalised Pareto distribution to exp(x) - exp(cutoff) of the tail gives
 * pareto_k, and, if it is finite, the tail is replaced by the fitted quantiles at (j + 0.5) / n_tail.  Then x = min(x, 0),
 * lw = x - logsumexp(x), elpd_loo_k = logsumexp_i(lw_i + l_ik), weight_ess_k = 1 / sum_i exp(2 lw_i).
 * A row k in which any y_ik (or l_ik) is not finite is NaN in all four, and so are the totals.
 * Tail ranks are global over the draws: nothing here is additive over shards; a multi-rank pool is gathered first. */
#define RSF_PSIS_ELPD 0
#define RSF_PSIS_PARETO_K 1
#define RSF_PSIS_N_TAIL 2
#define RSF_PSIS_WEIGHT_ESS 3
#define RSF_PSIS_OUT 4

/* rsf_predict_psis_finish out_totals[RSF_PSIS_TOTALS] */
#define RSF_PSIS_ELPD_LOO 0
#define RSF_PSIS_P_LOO 1       /* sum_k (lpd_k - elpd_loo_k) */
#define RSF_PSIS_ELPD_LOO_SE 2 /* sqrt(nout * var_k(elpd_loo_k)), ddof 1 as elpd_waic_se (ArviZ: ddof 0) */
#define RSF_PSIS_K_THRESHOLD 3 /* min(1 - 1 / log10(n), 0.7) */
#define RSF_PSIS_N_HIGH_K 4    /* rows with pareto_k > k_threshold; +inf counts */
#define RSF_PSIS_MAX_PARETO_K 5
#define RSF_PSIS_TOTALS 6

#define RSF_PSIS_MAX_TAIL 8192 /* largest tail_len: n = 4 194 304 draws at r_eff = 1 need 6144 */

/* series[nout][n] (time-major, as rsf_predict_partials leaves it), std2[n], data[nout]: ctx memory space;
 * out_rows[nout][RSF_PSIS_OUT]: a HOST array.  Needs no model.  Deterministic: the same input gives the same bits, host or
 * device memory alike.  RSF_ERR_INVALID: n < 1 or n >= 2^31, nout < 1, r_eff not finite or <= 0, a NULL pointer;
 * RSF_ERR_UNSUPPORTED: tail_len > RSF_PSIS_MAX_TAIL; RSF_ERR_NOMEM: the series' device copy of a RSF_MEM_HOST ctx. */
int rsf_predict_psis_loo(rsf_ctx *ctx, int64_t n, int64_t nout, const double *series, const double *std2, const double *data,
                         double r_eff, double *out_rows);

/* Host-only (no ctx, no GPU): the totals from psis_rows[nout][RSF_PSIS_OUT] and lpd_rows[nout] (RSF_PREDICT_LPD of
 * rsf_predict_finish), k = 0 included as in WAIC.  A NaN row makes every total but k_threshold NaN.
 * RSF_ERR_INVALID: nout < 1, n < 1, a NULL pointer. */
int rsf_predict_psis_finish(int64_t nout, int64_t n, const double *psis_rows, const double *lpd_rows, double *out_totals);

#ifdef __cplusplus
}
#endif
#endif /* RSF_PSIS_H */
