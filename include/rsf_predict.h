/*
 * rsf_predict.h — posterior predictive checks of pooled draws: the model series' credible spread, the probability
 * integral transform of the observation, the log pointwise predictive density and WAIC, exact credible bands, and PSIS-LOO
 * with the Pareto shape per output time (rsf_psis.h, included at the end), and the predictive band of an observation, noise
 * included (rsf_predict_noise.h, included at the end).
 *
 * Exported by librsf_hip.so only (the CPU checker implements rsf_abi.h alone; tests/predictive_reference.py is the
 * specification these entry points are tested against).  Same conventions as rsf_abi.h: int status, rsf_last_error(),
 * IEEE float64, caller-owned arrays, work ordered on the ctx stream.
 *
 * Given n draws (q_i, s2_i) — q_i = Dc (d = 1) or (Dc, a, b) (d = 3), s2_i the noise variance — and the observation data[nout]:
 * y_ik is the clean acceleration series of draw i at output time k (y_i0 = 0), solved with the float64 RK4 tiers (also for a
 * model flagged RSF_FLAG_FP32_SOLVE), and
 *     l_ik = -1/2 log(2 pi s2_i) - (data_k - y_ik)^2 / (2 s2_i).
 * Per output time k:
 *     mean_k, var_k   mean and ddof-1 variance of y_ik over the draws
 *     pit_k           mean_i Phi((data_k - y_ik) / sqrt(s2_i))
 *     lpd_k           log mean_i exp(l_ik)
 *     p_waic_k        ddof-1 variance of l_ik over the draws
 * Totals: mean_std2 = mean_i s2_i, elpd_waic = sum_k (lpd_k - p_waic_k), p_waic = sum_k p_waic_k,
 *     elpd_waic_se = sqrt(nout * var_k(lpd_k - p_waic_k)) (ddof 1), all including k = 0.
 * Non-finite: a row k in which any y_ik is not finite has every statistic NaN, and so have the totals.
 *
 * Additive partials, about caller-given centres c_y[k], c_l[k]: RSF_PREDICT_HEAD + nout * RSF_PREDICT_FIELDS doubles,
 *     [0] n   [1] sum_i s2_i
 *     row k at RSF_PREDICT_HEAD + k * RSF_PREDICT_FIELDS, sums over the draws whose y_ik is finite:
 *     [0] sum(y - c_y)  [1] sum(y - c_y)^2  [2] sum(l - c_l)  [3] sum(l - c_l)^2  [4] sum exp(l - c_l)  [5] sum Phi
 *     [6] the number of draws whose y_ik is not finite
 * Partials of disjoint shards of a pool taken about the same centres add (rsf_pool_allreduce_sum).
 */
#ifndef RSF_PREDICT_H
#define RSF_PREDICT_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_PREDICT_HEAD 2   /* n, sum s2 */
#define RSF_PREDICT_FIELDS 7 /* per output time */
#define RSF_PREDICT_SUM_Y 0
#define RSF_PREDICT_SUM_Y2 1
#define RSF_PREDICT_SUM_L 2
#define RSF_PREDICT_SUM_L2 3
#define RSF_PREDICT_SUM_EXP 4
#define RSF_PREDICT_SUM_PHI 5
#define RSF_PREDICT_NONFINITE 6

/* rsf_predict_finish out_rows[nout][RSF_PREDICT_OUT] */
#define RSF_PREDICT_MEAN 0
#define RSF_PREDICT_VAR 1
#define RSF_PREDICT_PIT 2
#define RSF_PREDICT_LPD 3
#define RSF_PREDICT_P_WAIC 4
#define RSF_PREDICT_OUT 5

/* rsf_predict_finish out_totals[RSF_PREDICT_TOTALS] */
#define RSF_PREDICT_MEAN_STD2 0
#define RSF_PREDICT_ELPD_WAIC 1
#define RSF_PREDICT_P_WAIC_TOTAL 2
#define RSF_PREDICT_ELPD_WAIC_SE 3
#define RSF_PREDICT_TOTALS 4

/* One forward solve per draw and the partials above.  q[n][d], std2[n], data[nout] and the optional series_out[nout][n]
 * (time-major; NULL = not wanted) are in the ctx memory space; center_y[nout], center_l[nout] and
 * partials[RSF_PREDICT_HEAD + nout * RSF_PREDICT_FIELDS] are HOST arrays in every mem_space.  Deterministic: the same draws
 * give the same bits, host or device memory alike, with or without series_out.
 * RSF_ERR_STATE without rsf_set_model; RSF_ERR_INVALID: n < 1, d not 1 or 3, n * nout too large, a NULL required pointer;
 * RSF_ERR_UNSUPPORTED: a model flagged RSF_FLAG_DOP853; RSF_ERR_NOMEM: the series' device copy of a RSF_MEM_HOST ctx
 * (n * nout doubles) cannot be allocated. */
int rsf_predict_partials(rsf_ctx *ctx, int64_t n, int32_t d, const double *q, const double *std2, const double *data,
                         const double *center_y, const double *center_l, double *partials, double *series_out);

/* Host-only (no ctx, no GPU): the statistics from summed partials.  out_rows[n_rows][RSF_PREDICT_OUT],
 * out_totals[RSF_PREDICT_TOTALS].  RSF_ERR_INVALID: n_rows < 1, a NULL pointer. */
int rsf_predict_finish(int64_t n_rows, const double *partials, const double *center_y, const double *center_l,
                       double *out_rows, double *out_totals);

/* np.quantile(series, probs, axis = 1), method "linear", exactly: the order statistics of every row by radix select, then
 * NumPy's _lerp.  series[nout][n]: ctx memory space; probs[n_probs] and out[n_probs][nout]: HOST arrays.  A row with a
 * non-finite value gives NaN.  RSF_ERR_INVALID: n < 1 or n >= 2^31, nout < 1, n_probs outside 1..RSF_PREDICT_MAX_PROBS, a
 * probability outside [0, 1], a NULL pointer. */
#define RSF_PREDICT_MAX_PROBS 16
int rsf_predict_quantiles(rsf_ctx *ctx, int64_t n, int64_t nout, const double *series, int32_t n_probs, const double *probs,
                          double *out);

#ifdef __cplusplus
}
#endif

/* PSIS-LOO and the Pareto shape per output time, on the series this header's entry points leave: declared in rsf_psis.h */
#include "rsf_psis.h"
/* The predictive band that includes the noise (quantiles of the mixture mean_i N(y_ik, s2_i)): declared in rsf_predict_noise.h */
#include "rsf_predict_noise.h"

#endif /* RSF_PREDICT_H */
