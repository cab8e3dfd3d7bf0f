/*
 * rsf_law_fit.h — the MULTI-START LEVENBERG-MARQUARDT fit of rsf_fit.h with the state-law solve in it: the least-squares fit of a
 * model under either state law (rsf_law.h: RSF_LAW_AGEING, RSF_LAW_SLIP) whose data is a series of any observable (rsf_observe.h:
 * RSF_OBS_ACC, RSF_OBS_MU, RSF_OBS_THETA, RSF_OBS_VELOCITY), under the loading table in use (rsf_set_loading).  Exported by
 * librsf_hip.so only; tests/law_fit_reference.py is the specification.
 *
 * The iteration, the points, the groups, the memory-space rules, the statuses and the constants are rsf_fit.h's, word for word:
 * rsf_law_fit_normal is rsf_fit_normal and rsf_law_fit_run is rsf_fit_run with `law` and `observable` in front, and the one thing that
 * differs is the solve.  The series s_k(q) is rsf_law_observe's: the plain float64 RK4 with a full evaluation of the right-hand side at
 * every stage (no tier, no guard; a trajectory that is not finite runs to its end and gives sums that are not finite).  The normal
 * equations are rsf_fit.h's with that series:
 *     r_k = s_k(q) - data_k        X_pk = (s_k(q^(p)) - s_k(q)) / (q^(p)_p fd)        q^(p): parameter p times (1 + fd)
 *     ssq = sum r_k^2              grad_p = sum X_pk r_k                               jtj_pr = sum X_pk X_rk
 * over EVERY sample k = 0 .. nout - 1.  Unlike the acceleration's, whose sample 0 is 0 in every trajectory, sample 0 of the friction
 * (mu_0 = k' ms_0) and of the state (theta_0 = x_0 Dc / V_ref) depends on the parameters: X_p0 is not 0 there, and sample 0 is summed
 * as every other sample is.
 *
 * Two contracts:
 *  1. ssq[i] is rsf_law_observe's SSq at q[i] BIT FOR BIT, whatever the starts beside it and the perturbed trajectories of its own
 *     group hold: the residual that is squared is the one rsf_law_observe forms, not one formed again from the stored sample (for
 *     RSF_OBS_ACC the two differ by an ulp of the sample).
 *  2. rsf_fit_trial -> rsf_law_fit_normal at the trial points -> rsf_fit_decide gives rsf_law_fit_run's iteration BIT FOR BIT, in
 *     every array, at every iteration.  rsf_fit_trial, rsf_fit_decide and rsf_fit_laplace take no model and serve this family as
 *     they are.
 *
 * RSF_FLAG_FP32_SOLVE runs the float64 solve; RSF_FLAG_DOP853: RSF_ERR_UNSUPPORTED.
 */
#ifndef RSF_LAW_FIT_H
#define RSF_LAW_FIT_H

#include "rsf_fit.h"
#include "rsf_law.h"
#include "rsf_observe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rsf_fit_normal under `law` against data[n_groups][nout] of `observable`; every other argument, rule and error is rsf_fit_normal's.
 * RSF_ERR_INVALID also: law not RSF_LAW_AGEING or RSF_LAW_SLIP; observable not one of RSF_OBS_*. */
int rsf_law_fit_normal(rsf_ctx *ctx, int32_t law, int32_t observable, int64_t n, int32_t d, const double *q, const double *data, int32_t n_groups,
                       double fd, double *ssq, double *grad, double *jtj);

/* rsf_fit_run under `law` against data of `observable`: n_iter (1 .. RSF_FIT_MAX_ITER) iterations of every RUNNING start inside one
 * launch, in place; every other argument, rule and error is rsf_fit_run's, and the two above. */
int rsf_law_fit_run(rsf_ctx *ctx, int32_t law, int32_t observable, int64_t n, int32_t d, double *q, const double *data, int32_t n_groups,
                    const double *lo, const double *hi, double fd, double ftol, int32_t n_iter, double *ssq, double *grad, double *jtj, double *lam,
                    int32_t *status, int32_t *iters);

#ifdef __cplusplus
}
#endif
#endif /* RSF_LAW_FIT_H */
