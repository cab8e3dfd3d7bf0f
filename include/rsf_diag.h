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

#ifdef __cplusplus
}
#endif
#endif /* RSF_DIAG_H */
