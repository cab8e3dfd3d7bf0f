/*
 * rsf_predict_noise.h — the posterior predictive band that includes the noise: where an OBSERVATION is expected to lie, as
 * opposed to rsf_predict_quantiles' credible band of the clean model series.  Part of the posterior predictive checks:
 * included by rsf_predict.h, whose conventions and series it shares.  Exported by librsf_hip.so only;
 * tests/predictive_noise_reference.py is the specification.
 */
#ifndef RSF_PREDICT_NOISE_H
#define RSF_PREDICT_NOISE_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Most passes over a row: pass 0 (the bracket), then at most 64 bisections and 64 Newton steps.  A Newton step is taken only
 * while the steps halve, and 64 halvings take a bracket to 2^-64 of its width: below the spacing of float64 at its ends.  A
 * probability that is still running then gets the midpoint of its bracket. */
#define RSF_PREDICT_NOISE_MAX_PASSES 129

/* Quantiles of the posterior predictive distribution of an observation at every output time k: with s_i = sqrt(std2_i),
 *     F_k(t) = 1/n sum_i Phi((t - y_ki) / s_i),        out[j][k] = the t with F_k(t) = probs[j].
 * The root lies between min_i and max_i of y_ki + ndtri(p) s_i; a safeguarded Newton iteration from that bracket's midpoint finds
 * it, every pass one read of the row for all the probabilities.  The result is a float64 t whose residual |F_k(t) - p| is at the
 * rounding floor of the sum (about 1.4e-14 min(p, 1 - p), and the change of F_k over one ulp of t where that is larger); it is not
 * "the" float64 root, because F_k is flat to rounding near it.  A probability's result does not depend on the others of the call.
 * series[nout][n] (time-major, as rsf_predict_partials leaves it) and std2[n]: ctx memory space; probs[n_probs],
 * out[n_probs][nout] and passes_out[nout] (NULL = not wanted; the passes the kernel made over row k, <=
 * RSF_PREDICT_NOISE_MAX_PASSES): HOST arrays in every mem_space.  Needs no model.  Deterministic: the same input gives the same
 * bits, host or device memory alike.  A row with a non-finite y_ki gives NaN for every probability; a std2_i that is not finite
 * and > 0 makes every row NaN (that draw enters every row).
 * RSF_ERR_INVALID: n < 1 or n >= 2^31, nout < 1, n_probs outside 1..RSF_PREDICT_MAX_PROBS, a probability not strictly inside
 * (0, 1) (NaN included), a NULL required pointer; RSF_ERR_NOMEM: the series' device copy of a RSF_MEM_HOST ctx.
 * Ranks of draws do not enter, but F_k is a mean over ALL draws: a multi-rank pool is gathered first. */
int rsf_predict_noise_quantiles(rsf_ctx *ctx, int64_t n, int64_t nout, const double *series, const double *std2, int32_t n_probs,
                                const double *probs, double *out, int32_t *passes_out);

#ifdef __cplusplus
}
#endif
#endif /* RSF_PREDICT_NOISE_H */
