/*
 * rsf_evidence.h — the MARGINAL LIKELIHOOD of the pooled draws by bridge sampling (Meng & Wong 1996; the iterative scheme of
 * Gronau et al. 2017).  Exported by librsf_hip.so only; tests/evidence_reference.py is the specification.
 *
 * With n0 = 0 the sampler's target is pi(q) ~ 1_box(q) SSq(q)^-shape (tests/posterior_reference.py): the posterior under a uniform
 * box prior on q and p(sigma^2) ~ 1 / sigma^2, sigma^2 integrated out.  With N = nout observations and shape = N / 2,
 *     p(y | M) = Gamma(shape) pi^-shape / vol(box) * I,      I = integral over the box of SSq(q)^-shape dq.
 * The estimator works in coordinates phi_p = q_p or log q_p (transform[p] = 0 or 1) with a Gaussian proposal g = N(mean, L L^T)
 * there; the unnormalised target's log density in phi is -shape log SSq + sum over the logged parameters of log q_p.  With
 * l = log target - log g for the N1 posterior draws (l1) and the N2 proposal draws (l2), s1 = N1 / (N1 + N2), s2 = N2 / (N1 + N2):
 *     r  <-  [ 1/N2 sum_j e^(l2_j - l*) / (s1 e^(l2_j - l*) + s2 r) ]  /  [ 1/N1 sum_i 1 / (s1 e^(l1_i - l*) + s2 r) ],     log I = log r + l*.
 *
 * Arrays live in the ctx memory space unless marked HOST.  d <= RSF_EVIDENCE_MAX_PARAMS; points are [n][d] row-major in NATURAL
 * coordinates q.  chol is the lower Cholesky factor L, [d][d] row-major.  Every sum has a fixed order that depends on the shapes
 * alone and no floating-point atomic is used: the same call gives the same bits, host or device memory alike.
 */
#ifndef RSF_EVIDENCE_H
#define RSF_EVIDENCE_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_EVIDENCE_MAX_PARAMS 3
#define RSF_EVIDENCE_PARTIALS 9 /* n1, n2, n2_finite, sum num, sum den, sum f1, sum f1^2, sum f2, sum f2^2 */
#define RSF_EVIDENCE_OUT 4      /* r_next, log_integral, log_evidence, re */

/* n2 draws of the proposal.  Draw j takes the d standard normals z that rsf_mcmc_draws(seed, chain = offset + j, iteration = 0, d)
 * reports: phi_p = mean_p + sum_{r <= p} L_pr z_r (fused multiply-adds, r ascending), theta_p = phi_p or exp(phi_p).  Shards with
 * offsets 0 and k are the first k and the following draws of one stream.
 *     theta[n2][d]  natural coordinates;     logg[n2]  log g(phi), the density code of rsf_evidence_logg;
 *     inbox[n2]     1 where lo_p < theta_p < hi_p for every p (the sampler's strict box), else 0.
 * mean[d], chol[d][d], transform[d], lo[d], hi[d]: HOST.
 * RSF_ERR_INVALID: n2 < 1, d outside 1..3, offset < 0, a non-finite mean, a factor that is not lower triangular with a positive
 * finite diagonal, lo >= hi or not finite, a transform flag other than 0 and 1, transform[p] = 1 with lo[p] <= 0, a NULL pointer. */
int rsf_evidence_propose(rsf_ctx *ctx, int64_t n2, int32_t d, const double *mean, const double *chol, const int32_t *transform,
                         const double *lo, const double *hi, uint64_t seed, int64_t offset, double *theta, double *logg, uint8_t *inbox);

/* log g at n given points theta[n][d] (natural coordinates), for the posterior draws:
 *     logg = -1/2 |y|^2 - sum log L_pp - d/2 log(2 pi),    y = L^-1 (phi - mean) by forward substitution,   phi = transform(theta).
 * A logged parameter that is not positive gives NaN.  mean, chol, transform: HOST, checked as in rsf_evidence_propose. */
int rsf_evidence_logg(rsf_ctx *ctx, int64_t n, int32_t d, const double *theta, const double *mean, const double *chol,
                      const int32_t *transform, double *logg);

/* The fused hot path; needs a model (rsf_set_model).  One forward solve per point with a running sum of squares against
 * data[nout] — no series is materialised — and
 *     l[i] = -shape log SSq(theta_i) + sum over the logged p of log theta_ip - logg[i].
 * l[i] = -inf where theta_i is outside the strict box (lo, hi) or SSq is not finite or not positive.  d = 1 (Dc) or 3 (Dc, a, b).
 * The solve is the float64 RK4 (with radiation damping if the model has it and k1 != 0): the integrator of the float64 sampler, and
 * of rsf_predict_partials.  It is NOT built for a model flagged RSF_FLAG_DOP853 (RSF_ERR_UNSUPPORTED) nor for the float32 solve: in
 * the float32 mode the float64 RK4 runs, as rsf_mcmc_init's does, so the value belongs to the float64 sampler's target.
 * A wave of 64 points none of which is inside the box does not solve.  lo, hi, transform: HOST.
 * RSF_ERR_STATE: no model.  RSF_ERR_INVALID: n < 1, d not 1 or 3, shape not finite and > 0, the box or the transform as above. */
int rsf_evidence_logtarget(rsf_ctx *ctx, int64_t n, int32_t d, const double *theta, const double *data, double shape, const double *lo,
                           const double *hi, const int32_t *transform, const double *logg, double *l);

/* Additive partials of one bridge iteration at the ratio r > 0 (finite) and the constant lstar (finite), HOST:
 *     partials = [ n1, n2, n2_finite, sum_j t2_j, sum_i t1_i, sum_j f1_j, sum_j f1_j^2, sum_i f2_i, sum_i f2_i^2 ]
 *     t2_j = e^a / (s1 e^a + s2 r),  a = l2_j - lstar   (formed as 1 / (s1 + s2 r e^-a) for a > 0: bounded by 1 / s1, no inf / inf)
 *     t1_i = 1 / (s1 e^b + s2 r),    b = l1_i - lstar   (formed as e^-b / (s1 + s2 r e^-b) for b > 0: bounded by 1 / (s2 r))
 *     f1 = p / (s1 p + s2) = t2,   f2 = 1 / (s1 p + s2) = r t1,   p = e^(l - lstar) / r.
 * l2_j = -inf contributes 0 and is not counted in n2_finite.  s1 and s2 come from the caller: a shard passes the pool's
 * N1 / (N1 + N2) and N2 / (N1 + N2), and the partials of disjoint shards add (rsf_pool_allreduce_sum).  Either set may be empty
 * (n = 0, the pointer is then not read).
 * RSF_ERR_INVALID: n1 < 0, n2 < 0, r or lstar not finite, r <= 0, s1 or s2 outside (0, 1), an l1 that is not finite (no
 * posterior draw can lie outside the support), an l2 that is NaN or +inf, a NULL pointer. */
int rsf_evidence_partials(rsf_ctx *ctx, int64_t n1, const double *l1, int64_t n2, const double *l2, double lstar, double r, double s1,
                          double s2, double *partials);

/* Host only (no ctx, no GPU): summed partials taken at (r, lstar) → out = [ r_next, log_integral, log_evidence, re ].
 *     r_next = (sum t2 / n2) / (sum t1 / n1)   (0 when n2_finite = 0);      log_integral = log r_next + lstar  (-inf for r_next = 0)
 *     log_evidence = log_integral - sum_p log(hi_p - lo_p) + lgamma(shape) - shape log(pi)     (d = 0: no box term)
 *     re^2 = Var(f1) / (n2 E[f1]^2) + Var(f2) / (ess_factor n1 E[f2]^2)    (Fruehwirth-Schnatter 2004; Var with ddof = 1),
 * the approximate relative root-mean-squared error of I, evaluated at r.  re = +inf where it is not defined: n1 < 2, n2 < 2 or
 * n2_finite = 0.  ess_factor in (0, 1]: effective over actual number of posterior draws.
 * RSF_ERR_INVALID: n1 < 1 or n2 < 1, r or lstar as above, ess_factor outside (0, 1], shape not finite and > 0, d outside 0..3,
 * lo >= hi or not finite, a NULL pointer (lo, hi may be NULL for d = 0). */
int rsf_evidence_finish(const double *partials, double r, double lstar, double ess_factor, double shape, int32_t d, const double *lo,
                        const double *hi, double *out);

#ifdef __cplusplus
}
#endif
#endif /* RSF_EVIDENCE_H */
