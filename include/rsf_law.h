/*
 * rsf_law.h — the two modelling choices of the forward model that rsf_abi.h fixes: the LOADING HISTORY V_l(t) and the STATE
 * EVOLUTION LAW.  Exported by librsf_hip.so only; tests/law_reference.py is the specification.
 *
 * Loading history.  rsf_set_model tabulates the built-in history V_l(t) = V_ref (1 + exp(-t / 20) sin 10 t) at the RK4 stage
 * times t_j = t_start + j (h / 2), h = delta_t / substeps, j = 0 .. 2 substeps (nout - 1): the float64 RK4 kernels of every
 * family read V_l from that table and from nowhere else.  rsf_set_loading replaces the table with the caller's values at the
 * same times, so every float64 RK4 entry point of the library (rsf_forward_batch, rsf_mcmc_*, rsf_predict_*, rsf_evidence_*,
 * rsf_smc_*, rsf_fit_*, rsf_mala_*, rsf_ensemble_*, rsf_grid_*, rsf_dr_*) then solves under the caller's history.  The
 * incremental tiers of those kernels start from an a-priori tier guess that assumes |V_l - v| <~ 1.2 V_ref; the guess costs
 * time when it is wrong, never accuracy: every incremental trip is accepted through its guard alone.
 *
 * State law.  In the project's state (ms = mu / k', x = V_ref theta / Dc) with w = v / V_ref = exp(e),
 * e = ms k'/a - mu_ref / a - (b / a) log x:
 *     RSF_LAW_AGEING   d(theta)/dt = 1 - w x                       (Dieterich; what every other kernel integrates)
 *     RSF_LAW_SLIP     d(theta)/dt = -(w x) log(w x) = -(w x)(e + log x)   (Ruina)
 * Everything downstream — the b / theta d(theta)/dt term, the single radiation-damping pass, dV/dt — is the same.
 * rsf_law_forward is the plain float64 solve under either law: classical RK4 with a full evaluation (log, exp, reciprocal) at
 * every stage, no tiers, no guard.  Under RSF_LAW_AGEING it is what the incremental tiers of rsf_forward_batch are checked
 * against on the device.
 */
#ifndef RSF_LAW_H
#define RSF_LAW_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_LAW_AGEING 0
#define RSF_LAW_SLIP 1

/* Replace the loading table of the ctx's model.  vl[n]: HOST, n = 2 substeps (nout - 1) + 1 values of V_l at the stage times
 * t_start + j (delta_t / substeps) / 2; copied before the call returns.  vl == NULL (n is then not read) restores the built-in
 * history.  The chains of an earlier rsf_mcmc_init are discarded, as rsf_set_model discards them; rsf_set_model itself always
 * resets the table to the built-in history.
 * RSF_ERR_STATE: no model.  RSF_ERR_INVALID: n is not the table's length, or a value is not finite.  RSF_ERR_UNSUPPORTED: the
 * model has RSF_FLAG_DOP853 (its adaptive steps evaluate the built-in formula off the table) or RSF_FLAG_FP32_SOLVE (its
 * incremental form has not been exercised off the built-in history). */
int rsf_set_loading(rsf_ctx *ctx, const double *vl, int64_t n);

/* The table in use → vl[n] (HOST), n = rsf_loading_size's.  RSF_ERR_STATE: no model.  RSF_ERR_INVALID: a wrong n.
 * RSF_ERR_UNSUPPORTED: RSF_FLAG_DOP853 (its table holds the twelve stage values of every step, not these times). */
int rsf_get_loading(rsf_ctx *ctx, double *vl, int64_t n);
int rsf_loading_size(rsf_ctx *ctx, int64_t *n);

/* n forward solves under `law` (RSF_LAW_AGEING or RSF_LAW_SLIP) and the table in use: one lane per parameter set, float64 RK4,
 * a full evaluation at every stage.  The arguments are rsf_forward_batch's: dc[n]; a[n], b[n] or NULL (the model's values);
 * data[nout] (needed with ssq_out); ssq_out[n] and / or acc_out[nout][n] (time-major; acc_out[0][i] = 0), either may be NULL;
 * all in the ctx memory space.  The sum of squares is the running sum of (acc_k - data_k)^2 from k = 0, each acc_k the
 * difference of the velocities at the interval's ends over delta_t.  A trajectory that goes non-finite runs to the end and
 * returns a non-finite sum.  RSF_FLAG_FP32_SOLVE: the float64 solve, as rsf_dr_run.
 * RSF_ERR_STATE: no model.  RSF_ERR_INVALID: an unknown law, n < 0, dc NULL, ssq_out without data.  RSF_ERR_UNSUPPORTED:
 * RSF_FLAG_DOP853. */
int rsf_law_forward(rsf_ctx *ctx, int32_t law, int64_t n, const double *dc, const double *a, const double *b, const double *data,
                    double *ssq_out, double *acc_out);

#ifdef __cplusplus
}
#endif
#endif /* RSF_LAW_H */
