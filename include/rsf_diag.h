/*
 * rsf_diag.h — convergence diagnostics of chain pools: split R-hat, nested R-hat and the multi-chain ESS.
 *
 * Exported by librsf_hip.so only (the CPU checker implements rsf_abi.h alone; tests/diagnostics_reference.py is the
 * specification these entry points are tested against).  Same conventions as rsf_abi.h: int status, rsf_last_error(),
 * IEEE float64, caller-owned arrays.
 *
 * A trace is the iteration-major block x[n][C][d] that rsf_mcmc_run writes (d <= 3); chain c of parameter p is x[:, c, p].
 *
 * Definitions, per parameter, with N = floor(n/2):
 *   split chains   each chain's first N and last N draws (the middle draw is dropped when n is odd): M' = 2C chains of
 *                  length N with means xbar_m and variances s2_m (ddof 1).  W = mean_m s2_m, B/N = var_m(xbar_m) (ddof 1),
 *                  var_plus = (N-1)/N W + B/N, split_rhat = sqrt(var_plus / W).
 *   ESS            the non-rank-normalised multi-chain ("mean") ESS of Stan and ArviZ on the split chains:
 *                  acov_m(t) = 1/N sum_{i<N-t} (y_i - xbar_m)(y_{i+t} - xbar_m), A(t) = mean_m acov_m(t),
 *                  rho(t) = 1 - (W - A(t)) / var_plus; Geyer's initial positive, then initial monotone, sequence;
 *                  tau = max(-1 + 2 sum rho, 1/log10(M'N)), ess = M'N / tau, mcse_mean = sqrt(var_plus / ess).
 *   nested R-hat   (unsplit chains; Margossian et al. 2024) K superchains of S consecutive chains:
 *                  B_nu = 1/(K-1) sum_k (xbar_k - xbar)^2, Btilde_k = 1/(S-1) sum_m (xbar_mk - xbar_k)^2 (0 when S = 1),
 *                  Wtilde_k = mean of the chains' variances (ddof 1), W_nu = mean_k (Btilde_k + Wtilde_k),
 *                  nested_rhat = sqrt(1 + B_nu / W_nu); NaN without superchains (S = 0), with K = 1 or with W_nu = 0.
 *   degenerate     W = 0 (every split chain constant): split_rhat, ess, tau and mcse_mean are NaN.  A non-finite draw makes
 *                  every statistic of its parameter NaN.
 *
 * Additive partials: everything above is a function of per-parameter sums over chains, taken about a caller-given centre
 * c[p], that add across disjoint sets of chains (a superchain must not straddle two sets) — shards and ranks combine them
 * with a plain sum (rsf_pool_allreduce_sum).  Per parameter, RSF_DIAG_HEAD + L doubles:
 *   [0] M'   [1] sum(xbar_m - c)   [2] sum(xbar_m - c)^2   [3] sum s2_m
 *   [4] K    [5] sum_k(xbar_k - c) [6] sum_k(xbar_k - c)^2 [7] sum_k Btilde_k   [8] sum_k Wtilde_k
 *   [9 + j]  A_sum(lag_begin + j) = sum_m acov_m(lag_begin + j),  j < L = lag_end - lag_begin
 * (fields 4..8 are 0 when chains_per_superchain is 0).
 */
#ifndef RSF_DIAG_H
#define RSF_DIAG_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_DIAG_HEAD 9 /* fields of the partials before the lag sums */

/* rsf_diag_finish out[p][RSF_DIAG_OUT] */
#define RSF_DIAG_MEAN 0          /* c + sum(xbar_m - c) / M': the mean of the split chains' means */
#define RSF_DIAG_VAR_PLUS 1
#define RSF_DIAG_W 2
#define RSF_DIAG_B_OVER_N 3
#define RSF_DIAG_SPLIT_RHAT 4
#define RSF_DIAG_NESTED_RHAT 5
#define RSF_DIAG_K 6             /* number of superchains (0 without) */
#define RSF_DIAG_ESS 7
#define RSF_DIAG_TAU 8
#define RSF_DIAG_MCSE_MEAN 9
#define RSF_DIAG_LAGS_COMPLETE 10 /* 1, or 0 when the n_lags lags given ended before Geyer's truncation */
#define RSF_DIAG_OUT 11

/* Device passes over a trace in the ctx memory space: partials[d][RSF_DIAG_HEAD + lag_end - lag_begin] (HOST array in
 * every mem_space).  chains_per_superchain S: 0 = no superchains, else it must divide n_chains.  center[d] is a host array.
 * Reductions are deterministic: the same trace gives the same bits, host or device memory alike.
 * RSF_ERR_INVALID (checked before the device is touched): n_iters < 4, n_chains < 1, n_params outside 1..3, S < 0 or not a
 * divisor of n_chains, lag_begin < 0, lag_end <= lag_begin or lag_end > N, a NULL pointer, a non-finite centre. */
int rsf_diag_partials(rsf_ctx *ctx, int64_t n_iters, int64_t n_chains, int32_t n_params, const double *trace,
                      int64_t chains_per_superchain, const double *center, int64_t lag_begin, int64_t lag_end,
                      double *partials);

/* Host-only (no ctx, no GPU): the statistics from summed partials whose lags are [0, n_lags), 2 <= n_lags <= N.
 * out[d][RSF_DIAG_OUT].  With lags_complete = 0 the statistics are those of a sequence cut at the lags given; ask for more.
 * RSF_ERR_INVALID: n_iters < 4, n_params outside 1..3, chains_per_superchain < 0, n_lags outside [2, N], a NULL pointer. */
int rsf_diag_finish(int64_t n_iters, int32_t n_params, int64_t chains_per_superchain, const double *center,
                    const double *partials, int64_t n_lags, double *out);

/*
 * Rank-normalised diagnostics and order statistics (Vehtari et al. 2021, as ArviZ reports them; the specification is
 * tests/rank_diagnostics_reference.py).  Per parameter p, with A = n*C draws (the full set), N = floor(n/2) and the split set =
 * rows [0, N) and [n-N, n), T = 2CN draws (an odd n leaves out the middle row):
 *   order statistics  of the full set sorted ascending, s[0..A-1], -0.0 == +0.0: median (np.median); quantile(prob) with
 *                     h = (A-1) prob, lo = floor(h), g = h - lo, a = s[lo], b = s[min(lo+1, A-1)]: a + (b-a) g if g < 0.5,
 *                     else b - (b-a)(1-g) (np.quantile "linear"); HDI(prob): k = floor(prob A), the first i of the smallest
 *                     s[i+k] - s[i], i < A-k, gives (s[i], s[i+k]) (ArviZ, not circular).
 *   normal scores     r(v) = L + (E+1)/2 with L, E = split draws < v, == v (average ranks); z(v) = ndtri((r - 3/8) / (T + 1/4)).
 *   series            zb = z(x); zf = the normal scores of |x - median| among the split set's |x - median|; I_lo = [x <= q05];
 *                     I_hi = [x <= q95] (q05, q95: quantile(0.05), quantile(0.95)).  Each has the trace's shape; the middle row
 *                     holds 0 and is never read.
 *   statistics        each series through rsf_diag_partials (centre 0, no superchains) and rsf_diag_finish: rhat_bulk = split R-hat
 *                     of zb, rhat_tail = that of zf, rhat = max of the two (NaN if either is); ess_bulk = ESS of zb, ess_q05 / ess_q95
 *                     = ESS of I_lo / I_hi, ess_tail = their minimum.  A series whose split draws span less than 1e-15 (constant)
 *                     has ESS = T instead of NaN; its R-hat stays NaN.
 *   non-finite        a non-finite draw of p makes every output of p NaN (lags_complete excepted); other parameters are unaffected.
 * Ranks are global: the statistics of shards do not add.  Gather a multi-rank pool first.
 */
#define RSF_DIAG_RANK_SERIES 4 /* zb, zf, I_lo, I_hi: series-major [4][n][C][d] */

/* rsf_diag_rank_prepare stats[p][RSF_DIAG_RANK_STATS + n_probs] */
#define RSF_DIAG_RANK_MEDIAN 0
#define RSF_DIAG_RANK_Q05 1
#define RSF_DIAG_RANK_Q95 2
#define RSF_DIAG_RANK_HDI_LO 3
#define RSF_DIAG_RANK_HDI_HI 4
#define RSF_DIAG_RANK_NONFINITE 5  /* 1 when p has a non-finite draw (every other field NaN, constant flags 0) */
#define RSF_DIAG_RANK_CONST 6      /* 6..9: 1 when series zb, zf, I_lo, I_hi is constant over the split set */
#define RSF_DIAG_RANK_STATS 10     /* then quantile(probs[i]) for i < n_probs */

/* rsf_diag_rank_finish out[p][RSF_DIAG_RANK_OUT] */
#define RSF_DIAG_RANK_RHAT 0
#define RSF_DIAG_RANK_RHAT_BULK 1
#define RSF_DIAG_RANK_RHAT_TAIL 2
#define RSF_DIAG_RANK_ESS_BULK 3
#define RSF_DIAG_RANK_ESS_TAIL 4
#define RSF_DIAG_RANK_ESS_Q05 5
#define RSF_DIAG_RANK_ESS_Q95 6
#define RSF_DIAG_RANK_LAGS_COMPLETE 7 /* 1 when all four series reached Geyer's truncation within the lags given */
#define RSF_DIAG_RANK_OUT 8

/* Sorts every parameter's draws on the device once and keeps the four series in a ctx workspace (about 4x the trace plus
 * 24 B per draw; rsf_diag_rank_release or rsf_destroy frees it).  trace, series: ctx memory space; probs, stats: host.  series
 * (optional, NULL = device only) receives a copy of [4][n][C][d].  Deterministic: the same trace gives the same bits, host or
 * device memory alike.  RSF_ERR_INVALID (checked before the device is touched): n_iters < 4, n_chains < 1, n_params outside
 * 1..3, n_iters * n_chains >= 2^32, n_probs < 0, a probability outside [0, 1], hdi_prob outside (0, 1) or k = floor(hdi_prob*A)
 * outside [1, A), a NULL pointer (probs may be NULL when n_probs = 0). */
int rsf_diag_rank_prepare(rsf_ctx *ctx, int64_t n_iters, int64_t n_chains, int32_t n_params, const double *trace, int32_t n_probs,
                          const double *probs, double hdi_prob, double *stats, double *series);

/* rsf_diag_partials of each prepared series with centre 0 and no superchains: partials[4][d][RSF_DIAG_HEAD + L] (host).  Call it
 * for lag blocks until rsf_diag_rank_finish reports lags_complete.  RSF_ERR_INVALID: nothing prepared, the lag range as in
 * rsf_diag_partials, a NULL pointer. */
int rsf_diag_rank_partials(rsf_ctx *ctx, int64_t lag_begin, int64_t lag_end, double *partials);

/* Host-only: the statistics from prepare's stats and the four series' partials with lags [0, n_lags), out[d][RSF_DIAG_RANK_OUT].
 * RSF_ERR_INVALID: as rsf_diag_finish, n_probs < 0. */
int rsf_diag_rank_finish(int64_t n_iters, int32_t n_params, const double *stats, int32_t n_probs, const double *partials,
                         int64_t n_lags, double *out);

/* Frees the rank workspace; rsf_diag_rank_partials is invalid until the next prepare. */
int rsf_diag_rank_release(rsf_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* RSF_DIAG_H */
