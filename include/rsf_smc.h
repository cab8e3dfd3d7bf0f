/*
 * rsf_smc.h — TEMPERED SEQUENTIAL MONTE CARLO over the box prior (Del Moral, Doucet & Jasra 2006; adaptive tempering by the
 * effective sample size, Jasra et al. 2011).  Exported by librsf_hip.so only; tests/smc_reference.py is the specification.
 *
 * With n0 = 0 the sampler's target is pi(q) ~ 1_box(q) SSq(q)^-shape (tests/posterior_reference.py).  n particles start uniform
 * in the strict box (lo, hi) and move through pi_beta(q) ~ 1_box(q) SSq(q)^(-shape beta), beta from 0 to 1.  Every particle carries
 * l = -shape log SSq (-inf where SSq is not finite or not positive).  One stage at the temperature beta:
 *     weights     w_j = exp(delta (l_j - lmax)), lmax the largest finite l; delta the largest step <= 1 - beta that keeps
 *                 (sum w)^2 / sum w^2 >= rho n_finite (rsf_smc_weight_sums, rsf_smc_section);
 *     evidence    log I += log(sum w / n) + delta lmax, from log I = log vol(box): at beta = 1, I = integral over the box of SSq^-shape,
 *                 the integral rsf_evidence_finish reports (rsf_smc_increment, rsf_smc_log_evidence);
 *     resampling  systematic, one uniform per stage (rsf_smc_resample);
 *     move        `steps` Metropolis steps on pi_(beta + delta) with the proposal N(q, L L^T) (rsf_smc_move, or rsf_smc_move_propose
 *                 and rsf_smc_move_accept around the caller's own sum of squares).
 * At beta = 1 the particles are an equally weighted sample of pi; rsf_smc_std2 completes them with sigma^2.
 *
 * Philox, as the sampler keys it: counter (particle = offset + j, iteration, slot), key = seed.  Iteration 0 is the start; the
 * Metropolis step k of stage s (both from 0, `steps` per stage) is iteration s steps + k + 1, which the caller passes.
 *
 * Arrays live in the ctx memory space unless marked HOST; particles are q[n][d] row-major.  d = 1 or 3 where a solve is involved,
 * 1..3 otherwise.  Every sum has a fixed order that depends on the shapes alone and no floating-point atomic is used: the same
 * call gives the same bits, host or device memory alike.  One ctx: the weight sums of shards taken with one lmax add, the
 * resampling is global.
 */
#ifndef RSF_SMC_H
#define RSF_SMC_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_SMC_MAX_PARAMS 3
#define RSF_SMC_MAX_CANDIDATES 16 /* steps delta evaluated in one read of l */
#define RSF_SMC_HEAD 3            /* rsf_smc_weight_sums' out before the sums: lmax, finite entries, -inf entries */
#define RSF_SMC_MAX_STEPS 64      /* Metropolis steps per rsf_smc_move call */

/* The start: q[j][p] = lo_p + u_p (hi_p - lo_p) in one fused multiply-add, strictly inside the box (a value that rounds onto an edge
 * moves one ulp in).  With w the four Philox words of (seed, offset + j, iteration 0, slot 2) and u53(a, b) = (((a << 32 | b) >> 11)
 * + 1) 2^-53: u_0 = u53(w0, w1) (the u of rsf_mcmc_draws), u_1 = u53(w2, w3), u_2 = u53 of the first two words of slot 3.
 * lo[d], hi[d]: HOST.  RSF_ERR_INVALID: n < 1, d outside 1..3, offset < 0, lo >= hi or not finite, a NULL pointer. */
int rsf_smc_init(rsf_ctx *ctx, int64_t n, int32_t d, const double *lo, const double *hi, uint64_t seed, int64_t offset, double *q);

/* For m <= RSF_SMC_MAX_CANDIDATES steps deltas[m] (HOST, each finite and >= 0), in one read of l[n]:
 *     out (HOST) = [ lmax, finite entries, -inf entries, (sum_j w_j, sum_j w_j^2) for each candidate ],  w_j = exp(delta (l_j - lmax)),
 * w_j = 0 for l_j = -inf.  lmax: the constant to use, or NaN for the largest finite l of this array (a pass of its own).
 * RSF_ERR_INVALID: n < 1, m outside 1..16, a bad delta, an l that is NaN or +inf, no finite l at all ("every particle has l = -inf"),
 * a NULL pointer. */
int rsf_smc_weight_sums(rsf_ctx *ctx, int64_t n, const double *l, int32_t m, const double *deltas, double lmax, double *out);

/* Host only.  sums[m][2] as rsf_smc_weight_sums leaves them for ascending candidates → *k = how many leading candidates keep
 * (sum w)^2 >= target sum w^2 (the effective sample size at least `target`); the search stops at the first that does not. */
int rsf_smc_section(double target, int32_t m, const double *sums, int32_t *k);
/* Host only.  *out = log(sum_w / n) + delta lmax, one stage's addition to log I.  RSF_ERR_INVALID: n < 1, sum_w not > 0. */
int rsf_smc_increment(int64_t n, double sum_w, double delta, double lmax, double *out);
/* Host only.  *out = log_integral - sum_p log(hi_p - lo_p) + lgamma(shape) - shape log(pi), rsf_evidence_finish's constant. */
int rsf_smc_log_evidence(double log_integral, double shape, int32_t d, const double *lo, const double *hi, double *out);

/* Systematic resampling at the step delta.  cum[n] (out): the inclusive prefix sum of w in the fixed order of
 * csrc/rsf_kernels_smc.h (eight consecutive weights per thread, 256 thread totals per tile, the tiles, each chain added one by one:
 * cum never decreases).  anc[n] (out, int64): anc[j] is the first i with cum_i > t_j, t_j = ((j + u) cum_{n-1}) / n evaluated in
 * that order in float64; t_j >= cum_{n-1}: the last particle that carries weight.  q_out[n][d], l_out[n]: q and l gathered through
 * anc (they must not overlap q and l).  u: the stage's uniform in (0, 1].
 * RSF_ERR_INVALID: n < 1, d outside 1..3, delta not finite or < 0, lmax not finite, u outside (0, 1], a NULL pointer. */
int rsf_smc_resample(rsf_ctx *ctx, int64_t n, int32_t d, const double *q, const double *l, double delta, double lmax, double u,
                     double *cum, int64_t *anc, double *q_out, double *l_out);

/* The fused hot path; needs a model (rsf_set_model).  `steps` Metropolis steps per particle on pi_beta, in place in q[n][d] and l[n]:
 * step k takes the d normals z and the uniform u that rsf_mcmc_draws(seed, offset + j, iter0 + k, d) reports, q' = q + L z
 * (fused multiply-adds, r ascending: the sampler's proposal); outside the strict box: rejected without a solve; else one float64 RK4
 * solve with a running sum of squares against data[nout], l' = -shape log SSq, accepted when log u < beta (l' - l); a non-finite
 * l' is rejected.  accepted[steps] (HOST, out): proposals accepted per step.  chol[d][d]: HOST, lower triangular, positive diagonal.
 * The solve is the float64 RK4 (with radiation damping if the model has it and k1 != 0), also for a model flagged
 * RSF_FLAG_FP32_SOLVE; a model flagged RSF_FLAG_DOP853 is refused (RSF_ERR_UNSUPPORTED).  A wave of 64 particles none of whose
 * proposals is inside the box does not solve.
 * RSF_ERR_STATE: no model.  RSF_ERR_INVALID: n < 1, d not 1 or 3, shape or beta not finite and > 0, steps outside 1..64, iter0 < 1,
 * offset < 0, the box or the factor as above, a NULL pointer. */
int rsf_smc_move(rsf_ctx *ctx, int64_t n, int32_t d, double *q, double *l, const double *data, double shape, const double *lo,
                 const double *hi, const double *chol, double beta, uint64_t seed, int64_t offset, int64_t iter0, int32_t steps,
                 int64_t *accepted);

/* The same step in two halves, for a caller that evaluates the sum of squares itself; no model needed, d = 1..3.
 * propose: q_new[n][d] and inbox[n] (uint8) of iteration `iter`.  accept: with ssq_new[n] (read where inbox is 1), q and l are
 * updated in place as rsf_smc_move updates them; *accepted (HOST, out). */
int rsf_smc_move_propose(rsf_ctx *ctx, int64_t n, int32_t d, const double *q, const double *lo, const double *hi, const double *chol,
                         uint64_t seed, int64_t offset, int64_t iter, double *q_new, uint8_t *inbox);
int rsf_smc_move_accept(rsf_ctx *ctx, int64_t n, int32_t d, double *q, double *l, const double *q_new, const uint8_t *inbox,
                        const double *ssq_new, double shape, double beta, uint64_t seed, int64_t offset, int64_t iter, int64_t *accepted);

/* sigma^2 of the final particles from its exact conditional InvGamma(shape, SSq / 2), SSq = exp(-l / shape):
 * std2[j] = 0.5 SSq_j / G_j, G_j the gamma variate of rsf_mcmc_draws(seed, offset + j, iter, ., shape).  shape >= 1.
 * RSF_ERR_INVALID: n < 1, shape not finite or < 1, offset < 0, iter < 0, a NULL pointer. */
int rsf_smc_std2(rsf_ctx *ctx, int64_t n, const double *l, double shape, uint64_t seed, int64_t offset, int64_t iter, double *std2);

#ifdef __cplusplus
}
#endif
#endif /* RSF_SMC_H */
