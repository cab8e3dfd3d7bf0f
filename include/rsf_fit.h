/*
 * rsf_fit.h — MULTI-START LEVENBERG-MARQUARDT least squares of (Dc) or (Dc, a, b) over the strict box.  Exported by librsf_hip.so
 * only; tests/fit_reference.py is the specification.
 *
 * The normal equations at a point q (d = 1: Dc; d = 3: Dc, a, b), by rsf_mcmc_init's forward differences: parameter p times
 * (1 + fd), the perturbed value in the denominator, every sample k = 0 .. nout - 1 included:
 *     r_k = acc_k(q) - data_k        X_pk = (acc_k(q^(p)) - acc_k(q)) / (q^(p)_p fd)
 *     ssq = sum r_k^2                grad_p = sum X_pk r_k  (X^T r)              jtj_pr = sum X_pk X_rk  (X^T X)
 * One iteration of a start whose status is RSF_FIT_RUNNING:
 *     1. A = jtj + lam diag(jtj).  A pivot of its Cholesky factor that is not positive and finite: no trial point (ok = 0), the
 *        iteration is a rejection without a solve (6).
 *     2. delta = -A^-1 grad, q' = q + delta, every coordinate clamped into the strict box: a value <= lo becomes nextafter(lo, hi),
 *        a value >= hi becomes nextafter(hi, lo).
 *     3. the normal equations at q': ssq', grad', jtj'.
 *     4. accepted iff ssq' is finite and ssq' < ssq (a non-finite sum is a rejection, as in the sampler).
 *     5. accepted: (q, ssq, grad, jtj) <- (q', ssq', grad', jtj'), lam <- max(0.1 lam, 1e-12); the start is RSF_FIT_CONVERGED if
 *        (ssq - ssq') / ssq < ftol.
 *     6. rejected: lam <- 10 lam; the start is RSF_FIT_STALLED once lam > 1e12.
 *     7. iters += 1.
 * The caller sets lam (RSF_FIT_LAM0), iters = 0 and the status from rsf_fit_normal's ssq: RSF_FIT_FAILED where it is not finite,
 * such a start never moves.
 *
 * Arrays live in the ctx memory space unless marked HOST; points are q[n][d] row-major, grad[n][d], jtj[n][d][d] (full, symmetric),
 * status[n] and iters[n] int32.  Every sum has a fixed order and no floating-point atomic is used: the same call gives the same bits,
 * host or device memory alike.
 *
 * At d = 3 the series depends on Dc and a almost only through Dc a: the least-squares problem has a ridge, the estimate is ONE POINT
 * ON IT, and only its ssq and its product Dc a are reproducible between starts.
 */
#ifndef RSF_FIT_H
#define RSF_FIT_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_FIT_MAX_PARAMS 3
#define RSF_FIT_MAX_ITER 64 /* iterations per rsf_fit_run call */

#define RSF_FIT_RUNNING 0
#define RSF_FIT_CONVERGED 1
#define RSF_FIT_STALLED 2
#define RSF_FIT_FAILED 3

#define RSF_FIT_LAM0 1e-3    /* the damping a start begins with */
#define RSF_FIT_LAM_MIN 1e-12
#define RSF_FIT_LAM_MAX 1e12 /* a rejection that leaves lam above it: RSF_FIT_STALLED */
#define RSF_FIT_LAM_DOWN 0.1
#define RSF_FIT_LAM_UP 10.0

/* The normal equations at n points; needs a model (rsf_set_model).  d = 1 or 3.  data[n_groups][nout]: the points are split evenly
 * over the observation series in order; with n_groups > 1 a series' share n / n_groups must be a whole multiple of a workgroup's
 * threads (rsf_mcmc_init's rule for chain groups).  The solve is the float64 RK4 (with radiation damping if the model has it and
 * k1 != 0), also for a model flagged RSF_FLAG_FP32_SOLVE; a model flagged RSF_FLAG_DOP853 is refused (RSF_ERR_UNSUPPORTED).
 * ssq[n], grad[n][d], jtj[n][d][d]: out.  ssq is the value rsf_mcmc_init computes for the same point, to rounding.
 * RSF_ERR_STATE: no model.  RSF_ERR_INVALID: n < 1, d not 1 or 3, n_groups < 1 or the split above, fd not finite and > 0, a NULL
 * pointer. */
int rsf_fit_normal(rsf_ctx *ctx, int64_t n, int32_t d, const double *q, const double *data, int32_t n_groups, double fd, double *ssq,
                   double *grad, double *jtj);

/* The fused hot path; needs a model.  n_iter (1 .. RSF_FIT_MAX_ITER) iterations of every RUNNING start inside one launch, in place
 * in q, ssq, grad, jtj, lam, status and iters; each iteration is one group solve (the trial point and its d forward-difference
 * neighbours in adjacent lanes).  A start that is not RUNNING is not written: its arrays keep their bits.  lo[d], hi[d]: HOST.
 * RSF_ERR_INVALID: as rsf_fit_normal, and n_iter outside 1..64, ftol not finite or < 0, lo >= hi or not finite. */
int rsf_fit_run(rsf_ctx *ctx, int64_t n, int32_t d, double *q, const double *data, int32_t n_groups, const double *lo, const double *hi,
                double fd, double ftol, int32_t n_iter, double *ssq, double *grad, double *jtj, double *lam, int32_t *status,
                int32_t *iters);

/* The same iteration in two halves, for a caller that evaluates the residuals itself; no model needed, d = 1..3.
 * trial: steps 1-2 for the RUNNING starts → q_trial[n][d] and ok[n] (uint8: 1 where there is a trial point; 0 for a failed factor
 * and for a start that is not RUNNING, whose q_trial row is its q).
 * decide: steps 4-7 with the caller's ssq_new[n], grad_new[n][d], jtj_new[n][d][d] (read where ok is 1), in place. */
int rsf_fit_trial(rsf_ctx *ctx, int64_t n, int32_t d, const double *q, const double *grad, const double *jtj, const double *lam,
                  const double *lo, const double *hi, const int32_t *status, double *q_trial, uint8_t *ok);
int rsf_fit_decide(rsf_ctx *ctx, int64_t n, int32_t d, double *q, double *ssq, double *grad, double *jtj, double *lam, int32_t *status,
                   int32_t *iters, const double *q_trial, const uint8_t *ok, const double *ssq_new, const double *grad_new,
                   const double *jtj_new, double ftol);

/* Host only.  From a fit's ssq and jtj[d][d] at the optimum, with n_obs observations:
 *     out[0 .. d d)   cov = ssq / (n_obs - d) (jtj)^-1, the least-squares covariance (standard errors: sqrt of its diagonal)
 *     out[d d]        log I ~ -shape log ssq + (d / 2) log 2 pi - 1/2 log det(2 shape jtj / ssq), Laplace's approximation of the
 *                     integral of SSq^-shape (the Gauss-Newton Hessian of shape log SSq) — the integral rsf_evidence_finish and
 *                     the SMC calls estimate
 *     out[d d + 1]    log p(y | M) from it with rsf_smc_log_evidence's constant
 * The Laplace value IGNORES THE BOX: it is meaningful where the mode is interior and the Gaussian's mass lies inside (d = 1), not
 * on the ridge of d = 3.  RSF_ERR_NOT_POSDEF: jtj is not positive definite.  RSF_ERR_INVALID: d outside 1..3, n_obs <= d, shape or
 * ssq not finite and > 0, the box as rsf_smc_log_evidence, a NULL pointer. */
int rsf_fit_laplace(int32_t d, int64_t n_obs, double shape, double ssq, const double *jtj, const double *lo, const double *hi,
                    double *out);

#ifdef __cplusplus
}
#endif
#endif /* RSF_FIT_H */
