/*
 * rsf_law_dr.h — the TWO-STAGE DELAYED-REJECTION sampler of rsf_dr.h with the state-law solve in it: the fused hot path for a
 * model under either state law (rsf_law.h: RSF_LAW_AGEING, RSF_LAW_SLIP) whose data is a series of any observable (rsf_observe.h:
 * RSF_OBS_ACC, RSF_OBS_MU, RSF_OBS_THETA, RSF_OBS_VELOCITY), under the loading table in use (rsf_set_loading).  Exported by
 * librsf_hip.so only.
 *
 * The chain, its draws, both stages, the decisions, the counters, the groups, the memory-space rules and the limits are rsf_dr.h's,
 * word for word: rsf_law_dr_run is rsf_dr_run and rsf_law_dr_ssq is rsf_dr_ssq with `law` and `observable` in front, and the one
 * thing that differs is the solve.  SSq(q) is rsf_law_observe's: the plain float64 RK4 with a full evaluation of the right-hand
 * side at every stage (no tier, no guard; a trajectory that is not finite runs to its end, gives an SSq that is not finite, hence
 * l = -inf, and is rejected), the sum of (s_k - data_k)^2 over every sample k = 0 .. nout - 1 of the observable, BIT FOR BIT what
 * rsf_law_observe returns for the same point whatever the lanes beside it hold.  So
 *     rsf_dr_propose -> rsf_law_dr_ssq (or rsf_law_observe on the masked-in points) -> rsf_dr_accept, stage 1 then stage 2,
 * gives rsf_law_dr_run's iteration bit for bit; rsf_dr_propose and rsf_dr_accept take no model and serve this family as they are.
 *
 * RSF_FLAG_FP32_SOLVE runs the float64 solve; RSF_FLAG_DOP853: RSF_ERR_UNSUPPORTED.
 */
#ifndef RSF_LAW_DR_H
#define RSF_LAW_DR_H

#include "rsf_dr.h"
#include "rsf_law.h"
#include "rsf_observe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rsf_dr_run under `law` against data[n_groups][nout] of `observable`; every other argument, rule and error is rsf_dr_run's.
 * RSF_ERR_INVALID also: law not RSF_LAW_AGEING or RSF_LAW_SLIP; observable not one of RSF_OBS_*. */
int rsf_law_dr_run(rsf_ctx *ctx, int32_t law, int32_t observable, int64_t n, int32_t d, double *q, double *l, const double *data, int32_t n_groups,
                   const double *lo, const double *hi, const double *chol, double gamma, int32_t stages, double shape, uint64_t seed, int64_t offset,
                   int64_t iter0, int32_t n_iter, int32_t *accepted1, int32_t *accepted2, int32_t *outbox1, int32_t *outbox2, int32_t *stuck,
                   double *trace_q, double *trace_l);

/* rsf_dr_ssq under `law` against data of `observable`: ssq[j] = SSq(y[j]) where mask[j] is 1, in rsf_law_dr_run's arrangement; every
 * other entry of ssq stays as it is.  Arguments and errors: rsf_dr_ssq's, and the two above. */
int rsf_law_dr_ssq(rsf_ctx *ctx, int32_t law, int32_t observable, int64_t n, int32_t d, const double *y, const uint8_t *mask, const double *data,
                   int32_t n_groups, double *ssq);

#ifdef __cplusplus
}
#endif
#endif /* RSF_LAW_DR_H */
