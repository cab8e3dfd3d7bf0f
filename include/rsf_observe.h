/*
 * rsf_observe.h — the OBSERVABLE of the state-law solve.  Exported by librsf_hip.so only; tests/observe_reference.py is the
 * specification.
 *
 * rsf_law_forward (rsf_law.h) integrates three quantities — the friction coefficient mu, the state variable theta and the
 * slider velocity V — and returns one derived series, the acceleration acc_k = (V_k - V_{k-1}) / delta_t.  A laboratory
 * records mu(t), and sometimes V(t).  rsf_law_observe is the same solve (plain float64 RK4 under either state law and the
 * loading table in use, a full evaluation at every stage, no tiers, no guard) with the output sample chosen by the caller:
 *
 *     RSF_OBS_ACC        (V_k - V_{k-1}) / delta_t, sample 0 = 0: rsf_law_forward's series and sum, bit for bit
 *     RSF_OBS_MU         mu_k,    sample 0 = mu_t_zero
 *     RSF_OBS_THETA      theta_k, sample 0 = Dc / V_ref
 *     RSF_OBS_VELOCITY   V_k,     sample 0 = V_ref: the V whose differences RSF_OBS_ACC returns
 *
 * The kernel integrates ms = mu / k' (k' = 0.1 / Dc) and x = V_ref theta / Dc: mu_k is the product k' ms_k and theta_k the
 * product x_k (Dc (1 / V_ref)), each formed once per output sample.
 */
#ifndef RSF_OBSERVE_H
#define RSF_OBSERVE_H

#include "rsf_law.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_OBS_ACC 0
#define RSF_OBS_MU 1
#define RSF_OBS_THETA 2
#define RSF_OBS_VELOCITY 3

/* n forward solves under `law` (RSF_LAW_AGEING or RSF_LAW_SLIP) observed as `observable` (RSF_OBS_*).  The arguments are
 * rsf_law_forward's: dc[n]; a[n], b[n] or NULL (the model's values); data[nout] (needed with ssq_out), a series of the SAME
 * observable; ssq_out[n] and / or series_out[nout][n] (time-major), either may be NULL; all in the ctx memory space.  The sum
 * of squares is the running sum of (s_k - data_k)^2 from k = 0, s_0 the initial value above.  A trajectory that goes
 * non-finite runs to the end and returns a non-finite sum.  RSF_FLAG_FP32_SOLVE: the float64 solve, as rsf_law_forward.
 * RSF_ERR_STATE: no model.  RSF_ERR_INVALID: an unknown law or observable, n < 0, dc NULL, ssq_out without data.
 * RSF_ERR_UNSUPPORTED: RSF_FLAG_DOP853. */
int rsf_law_observe(rsf_ctx *ctx, int32_t law, int32_t observable, int64_t n, const double *dc, const double *a, const double *b,
                    const double *data, double *ssq_out, double *series_out);

#ifdef __cplusplus
}
#endif
#endif /* RSF_OBSERVE_H */
