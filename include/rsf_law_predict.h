/*
 * rsf_law_predict.h — the posterior predictive checks of rsf_predict.h for a model under either state law (rsf_law.h:
 * RSF_LAW_AGEING, RSF_LAW_SLIP) whose data is a series of any observable (rsf_observe.h: RSF_OBS_ACC, RSF_OBS_MU, RSF_OBS_THETA,
 * RSF_OBS_VELOCITY), under the loading table in use (rsf_set_loading); and the same partials from a series that already exists.
 * Exported by librsf_hip.so only.
 *
 * The statistics, the partials' layout (RSF_PREDICT_HEAD + nout * RSF_PREDICT_FIELDS doubles about caller-given centres), the
 * memory-space rules and the determinism promise are rsf_predict.h's, word for word; rsf_predict_finish finishes the partials of
 * both entry points, and rsf_predict_quantiles, rsf_predict_psis_loo and rsf_predict_noise_quantiles work on the series
 * rsf_law_predict_partials leaves as they do on rsf_predict_partials'.  The one thing that differs is the solve: y_ik is
 * rsf_law_observe's sample k of draw i BIT FOR BIT — the plain float64 RK4 with a full evaluation of the right-hand side at every
 * stage, no tier, no guard, sample 0 the observable's initial value; a trajectory that is not finite runs to its end and its
 * samples are counted in the rows' non-finite field.  data is a series of the same observable.
 *
 * rsf_predict_series_partials is the split path: rsf_law_observe's series (or any series of n draws) in, the same partials
 * out, bit for bit what rsf_law_predict_partials — and rsf_predict_partials, of the series it leaves — returns.
 *
 * RSF_FLAG_FP32_SOLVE runs the float64 solve; RSF_FLAG_DOP853: RSF_ERR_UNSUPPORTED.
 */
#ifndef RSF_LAW_PREDICT_H
#define RSF_LAW_PREDICT_H

#include "rsf_law.h"
#include "rsf_observe.h"
#include "rsf_predict.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rsf_predict_partials under `law` with y_ik the series of `observable`; every other argument, rule and error is
 * rsf_predict_partials's.  RSF_ERR_INVALID also: law not RSF_LAW_AGEING or RSF_LAW_SLIP; observable not one of RSF_OBS_*. */
int rsf_law_predict_partials(rsf_ctx *ctx, int32_t law, int32_t observable, int64_t n, int32_t d, const double *q, const double *std2,
                             const double *data, const double *center_y, const double *center_l, double *partials, double *series_out);

/* The partials of a materialised series[nout][n] (time-major), which with std2[n] and data[nout] is in the ctx memory space;
 * center_y[nout], center_l[nout] and partials[RSF_PREDICT_HEAD + nout * RSF_PREDICT_FIELDS] are HOST arrays in every mem_space.
 * Needs no model.  RSF_ERR_INVALID: n < 1, nout < 1, n * nout too large, a NULL pointer. */
int rsf_predict_series_partials(rsf_ctx *ctx, int64_t n, int64_t nout, const double *series, const double *std2, const double *data,
                                const double *center_y, const double *center_l, double *partials);

#ifdef __cplusplus
}
#endif
#endif /* RSF_LAW_PREDICT_H */
