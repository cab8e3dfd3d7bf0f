/*
 * rsf_stiff.h — the state-law solve and its delayed-rejection sampler with the STIFFNESS OF THE APPARATUS a model constant,
 * independent of Dc.  Exported by librsf_hip.so only; tests/stiff_reference.py is the specification.
 *
 * Every other solve of this library integrates the reference's spring, whose stiffness is tied to the parameter being inferred:
 * k' = 1e-2 * 10 / Dc (RateStateModel.py:324).  In an experiment the stiffness is a constant of the apparatus: it does not move
 * when a sampler proposes another Dc, and k Dc is rarely 0.1.  The functions here are rsf_law_observe, rsf_law_dr_run and
 * rsf_law_dr_ssq with `stiffness` = k' in front of the points, under either state law (rsf_law.h), any observable (rsf_observe.h)
 * and the loading table in use (rsf_set_loading).
 *
 * Arithmetic: each lane forms kappa = stiffness * dc and ikappa = 1.0 / kappa (one IEEE division per lane per solve).  kappa
 * stands where the coupled solve has the literal 1e-2 * 10, ikappa where it has that literal's reciprocal:
 *     k' = kappa (1 / Dc)      beta = (b V_ref) ikappa      ms_0 = (mu_t_zero Dc) ikappa
 * and every other operation is rsf_law_observe's.  On a point where stiffness * dc == 0.1 exactly (Dc = 64 with stiffness
 * 0.1 / 64, say) the results are rsf_law_observe's bit for bit.
 *
 * A stiffness below the critical (b - a) / Dc gives stick-slip: the fixed-step solve then returns a series that is not finite on
 * some points.  Such a trajectory runs to its end and gives an SSq that is not finite, hence l = -inf in the sampler: the
 * proposal is rejected.  There is no guard.
 *
 * RSF_ERR_INVALID, with the function's name in rsf_last_error(): stiffness not finite or not > 0.  RSF_FLAG_FP32_SOLVE runs the
 * float64 solve; RSF_FLAG_DOP853: RSF_ERR_UNSUPPORTED.
 */
#ifndef RSF_STIFF_H
#define RSF_STIFF_H

#include "rsf_law_dr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rsf_law_observe with the spring's stiffness `stiffness`: every other argument, rule and error is rsf_law_observe's. */
int rsf_stiff_observe(rsf_ctx *ctx, int32_t law, int32_t observable, double stiffness, int64_t n, const double *dc, const double *a,
                      const double *b, const double *data, double *ssq_out, double *series_out);

/* rsf_law_dr_run with the spring's stiffness `stiffness`, the fused hot path: every other argument, rule and error is
 * rsf_law_dr_run's.  SSq(q) is rsf_stiff_observe's bit for bit, so
 *     rsf_dr_propose -> rsf_stiff_dr_ssq (or rsf_stiff_observe on the masked-in points) -> rsf_dr_accept, stage 1 then stage 2,
 * gives this call's iteration bit for bit. */
int rsf_stiff_dr_run(rsf_ctx *ctx, int32_t law, int32_t observable, double stiffness, int64_t n, int32_t d, double *q, double *l,
                     const double *data, int32_t n_groups, const double *lo, const double *hi, const double *chol, double gamma, int32_t stages,
                     double shape, uint64_t seed, int64_t offset, int64_t iter0, int32_t n_iter, int32_t *accepted1, int32_t *accepted2,
                     int32_t *outbox1, int32_t *outbox2, int32_t *stuck, double *trace_q, double *trace_l);

/* rsf_law_dr_ssq with the spring's stiffness `stiffness`: every other argument, rule and error is rsf_law_dr_ssq's. */
int rsf_stiff_dr_ssq(rsf_ctx *ctx, int32_t law, int32_t observable, double stiffness, int64_t n, int32_t d, const double *y, const uint8_t *mask,
                     const double *data, int32_t n_groups, double *ssq);

#ifdef __cplusplus
}
#endif
#endif /* RSF_STIFF_H */
