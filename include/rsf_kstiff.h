/*
 * rsf_kstiff.h — the delayed-rejection sampler of the state-law solve with the STIFFNESS OF THE APPARATUS AMONG THE PARAMETERS:
 * chains over (Dc, k) at d = 2 or (Dc, a, b, k) at d = 4, the stiffness always the LAST coordinate.  Exported by librsf_hip.so
 * only; tests/kstiff_reference.py is the specification.
 *
 * rsf_stiff.h takes the stiffness as a constant that is known exactly.  In a laboratory it comes from a calibration run and is
 * good to some 10-20 %, and a wrong fixed k moves the inferred Dc (18 % under a hold history at a 20 % error).  The functions here
 * are rsf_stiff_observe, rsf_stiff_dr_run and rsf_stiff_dr_ssq with the stiffness read per point instead of per call, and
 * rsf_dr_propose / rsf_dr_accept at d = 2 or 4, under either state law (rsf_law.h), any observable (rsf_observe.h) and the
 * loading table in use (rsf_set_loading).
 *
 * Arithmetic: rsf_stiff.h's, with the point's own k: kappa = k * dc and ikappa = 1.0 / kappa, one IEEE division per point per
 * solve.  A point whose k equals rsf_stiff_observe's `stiffness` gives that call's series and SSq bit for bit.  The chain logic
 * is rsf_dr.h's: the same draws (the second normal pair is drawn at d = 4 and its fourth normal used), the same decisions.
 *
 * A stiffness below the critical (b - a) / Dc gives a trajectory that is not finite on some points: it runs to its end and gives
 * an SSq that is not finite, hence l = -inf in the sampler, and the proposal is rejected.  There is no guard.
 *
 * RSF_ERR_INVALID, with the function's name in rsf_last_error(): d not 2 or 4; lo[d - 1] <= 0 (the stiffness's box lies in
 * k > 0: rsf_kstiff_dr_run, _propose, _accept); in rsf_kstiff_observe a k[i] that is not finite and > 0 (k is then a HOST
 * array or a device array: it is read on the host from a copy).  RSF_FLAG_FP32_SOLVE runs the float64 solve;
 * RSF_FLAG_DOP853: RSF_ERR_UNSUPPORTED.
 */
#ifndef RSF_KSTIFF_H
#define RSF_KSTIFF_H

#include "rsf_stiff.h"

#define RSF_KSTIFF_MAX_PARAMS 4

#ifdef __cplusplus
extern "C" {
#endif

/* rsf_stiff_observe with the stiffness k[n] of each point in place of the call's `stiffness`: every other argument, rule and
 * error is rsf_stiff_observe's.  k is validated on the host before the launch: for a caller with device memory (RSF_MEM_DEVICE) that
 * is a copy of k[n] to the host and a synchronise of the ctx stream, so the call is SYNCHRONOUS up to its launch for such a caller.
 * It is not on the sampler's path: rsf_kstiff_dr_run and rsf_kstiff_dr_ssq read the stiffness from the points and copy nothing. */
int rsf_kstiff_observe(rsf_ctx *ctx, int32_t law, int32_t observable, int64_t n, const double *dc, const double *a, const double *b,
                       const double *k, const double *data, double *ssq_out, double *series_out);

/* rsf_stiff_dr_run without the scalar stiffness, the fused hot path: q[n][d], d = 2 (Dc, k) or 4 (Dc, a, b, k); every other
 * argument, rule and error is rsf_stiff_dr_run's.  SSq(q) is rsf_kstiff_observe's bit for bit, so
 *     rsf_kstiff_dr_propose -> rsf_kstiff_dr_ssq (or rsf_kstiff_observe on the masked-in points) -> rsf_kstiff_dr_accept,
 * stage 1 then stage 2, gives this call's iteration bit for bit. */
int rsf_kstiff_dr_run(rsf_ctx *ctx, int32_t law, int32_t observable, int64_t n, int32_t d, double *q, double *l, const double *data,
                      int32_t n_groups, const double *lo, const double *hi, const double *chol, double gamma, int32_t stages, double shape,
                      uint64_t seed, int64_t offset, int64_t iter0, int32_t n_iter, int32_t *accepted1, int32_t *accepted2, int32_t *outbox1,
                      int32_t *outbox2, int32_t *stuck, double *trace_q, double *trace_l);

/* rsf_stiff_dr_ssq without the scalar stiffness: y[n][d], d = 2 or 4, the stiffness of a point its last coordinate. */
int rsf_kstiff_dr_ssq(rsf_ctx *ctx, int32_t law, int32_t observable, int64_t n, int32_t d, const double *y, const uint8_t *mask,
                      const double *data, int32_t n_groups, double *ssq);

/* rsf_dr_propose at d = 2 or 4: every other argument, rule and error is rsf_dr_propose's.  At d = 2 the results are
 * rsf_dr_propose's bit for bit. */
int rsf_kstiff_dr_propose(rsf_ctx *ctx, int64_t n, int32_t d, const double *q, const double *l, int32_t n_groups, const double *lo,
                          const double *hi, const double *chol, double gamma, int32_t stage, uint64_t seed, int64_t offset, int64_t iter,
                          const uint8_t *pending, double *y, uint8_t *mask);

/* rsf_dr_accept at d = 2 or 4: every other argument, rule and error is rsf_dr_accept's.  At d = 2 the results are
 * rsf_dr_accept's bit for bit. */
int rsf_kstiff_dr_accept(rsf_ctx *ctx, int64_t n, int32_t d, double *q, double *l, const double *lo, const double *hi, double gamma,
                         int32_t stage, double shape, uint64_t seed, int64_t offset, int64_t iter, const double *y, const uint8_t *mask,
                         const double *ssq, double *l1, uint8_t *pending, int32_t *accepted1, int32_t *accepted2, int32_t *outbox1,
                         int32_t *outbox2, int32_t *stuck);

#ifdef __cplusplus
}
#endif
#endif /* RSF_KSTIFF_H */
