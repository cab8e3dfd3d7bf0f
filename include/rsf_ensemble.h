/*
 * rsf_ensemble.h — AFFINE-INVARIANT ENSEMBLE SAMPLER IN ISLANDS over the strict box: the stretch move of Goodman & Weare (2010) in
 * the parallel form of Foreman-Mackey et al. (2013), one independent ensemble ("island") per workgroup.  It takes no proposal
 * covariance and no gradient, adapts nothing, costs one solve per proposal and its only constant is the stretch scale a.  Exported
 * by librsf_hip.so only; tests/ensemble_reference.py is the specification.
 *
 * Target: pi(q) ~ 1_box(q) SSq(q)^-shape (sigma^2 integrated out; rsf_smc_std2 with the walkers' l completes a state).
 * Walker state: q[d] and l = -shape log SSq(q) (-inf where SSq is not finite and > 0), as the SMC particles carry it.
 *
 * Islands.  B is the ctx's workgroup size (rsf_config.block_threads: 64, 128 or 256; 0 means 256).  n is a multiple of 2B; island k
 * holds the walkers k 2B .. (k + 1) 2B - 1 of q[n][d] (row-major), its first B walkers are half 0, the next B half 1.  Islands
 * never exchange anything: they are independent replicates, and because their walkers are consecutive a nested R-hat with
 * superchains of 2B walkers is the R-hat over islands.  Walker j uses the Philox particle g = offset + j, so island k run alone
 * with offset + k 2B reproduces its rows of the full run.
 *
 * Iteration t >= 1 is two half-steps h = 0, 1; in half-step h every walker j of half h of every island moves:
 *     1. Draws, all of (seed, g, t).  The four words w0..w3 of the accept slot (slot 2): U_a = u53(w0, w1), the u of rsf_mcmc_draws,
 *        and U_s = u53(w2, w3), rsf_smc_init's u_1.  The first word w0' of slot 3 (rsf_smc_init's third uniform's slot): the
 *        partner index r = (w0' B) >> 32 as a 64-bit product, in 0 .. B - 1.  r is not exactly uniform: an index's probability
 *        differs from 1/B by at most 2^-32 (relative bias <= B 2^-32 <= 6e-8).
 *     2. Partner y: walker r of the OTHER half of the same island, in its state at the start of this half-step (h = 0: after
 *        iteration t - 1; h = 1: after half-step 0 of iteration t).
 *     3. Coordinates.  Bit p of logmask chooses phi_p(q) = log q_p (bit set; needs lo_p >= 0) or q_p.  u = phi(x), v = phi(y).
 *     4. Stretch.  s = (a - 1) U_s + 1 (a product, then a sum), z = (s s) / a: the density g(z) ~ z^-1/2 on [1/a, a].
 *        u'_p = fma(z, u_p - v_p, v_p), one fused multiply-add; q'_p = exp(u'_p) under a mask bit, else u'_p.  Nothing is clamped:
 *        q' is inside iff lo_p < q'_p < hi_p for every p, and a proposal outside is rejected without a solve (outbox grows).
 *        J = (d - 1) log z, then + (u'_p - u_p) for every masked p in index order: the stretch's volume factor and the Jacobian
 *        of the log coordinates.
 *     5. Decide with l' = l(q'): log alpha = J + (l' - l); accepted iff l' is finite and min(log alpha, 0) > log U_a (a NaN
 *        compares false: rejected).  Accepted: (q, l) <- (q', l'), accepted grows.  A walker that does not move keeps its bits;
 *        q is stored, never u.
 * Given the other half, the move of one walker is Goodman & Weare's and leaves pi invariant in the phi coordinates; the walkers
 * of one half move simultaneously, each against the fixed other half, which is what makes the half-step parallel.
 *
 * Start states.  A walker whose q is not strictly inside the box, or whose l is not finite, is STUCK: in its half-step it makes
 * no proposal, nothing is solved for it and its stuck counter grows.  It is never a mover — but it may be drawn as a PARTNER,
 * and then its position (whatever it holds) enters the proposal of a healthy walker.  Hand in walkers inside the box with finite
 * l; the Python layer refuses any other start.
 *
 * Arrays live in the ctx memory space unless marked HOST (an RSF_MEM_HOST caller is staged through the ctx workspace, as
 * rsf_mala_run's).  accepted[n], outbox[n] and stuck[n] are int32 counters per walker, INCREMENTED in place (no atomic: a walker's
 * counters are written by one lane): per iteration at most one of them grows; a proposal inside the box that is rejected grows none.
 * No floating-point atomic, no sum across lanes: the same call gives the same bits, host or device memory alike.
 */
#ifndef RSF_ENSEMBLE_H
#define RSF_ENSEMBLE_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_ENSEMBLE_MAX_PARAMS 3
#define RSF_ENSEMBLE_MAX_ITER 64 /* iterations per rsf_ensemble_run call */

/* The fused hot path; needs a model, d = 1 (Dc) or 3 (Dc, a, b).  n_iter (1 .. RSF_ENSEMBLE_MAX_ITER) iterations inside one launch,
 * in place in q[n][d] and l[n]; iteration k = 0 .. n_iter - 1 uses the draws of Philox iteration iter0 + k (iter0 >= 1).  One
 * workgroup owns one island and a lane carries walker i of both halves; a half-step is one float64 RK4 solve per lane (damped or
 * not, also for RSF_FLAG_FP32_SOLVE; RSF_FLAG_DOP853: RSF_ERR_UNSUPPORTED).  data[n_groups][nout]: the walkers are split evenly
 * over the series in order, n / n_groups a multiple of 2B.  lo[d], hi[d]: HOST.  trace_q[n_iter][n][d] and trace_l[n_iter][n]: the
 * state after each iteration, iteration-major; both NULL, or both given.
 * RSF_ERR_STATE: no model.  RSF_ERR_INVALID: n < 1 or not a multiple of 2B (of 2B n_groups), d not 1 or 3, n_groups < 1, a not
 * finite or <= 1, shape not finite and > 0, a logmask bit at or beyond d, lo_p < 0 under a logmask bit, n_iter outside 1..64,
 * iter0 < 1 or iter0 + n_iter past 2^32, offset < 0, lo >= hi or not finite, a NULL pointer, one trace without the other. */
int rsf_ensemble_run(rsf_ctx *ctx, int64_t n, int32_t d, double *q, double *l, const double *data, int32_t n_groups, const double *lo,
                     const double *hi, double a, uint32_t logmask, double shape, uint64_t seed, int64_t offset, int64_t iter0,
                     int32_t n_iter, int32_t *accepted, int32_t *outbox, int32_t *stuck, double *trace_q, double *trace_l);

/* ONE HALF-STEP in two calls, for a caller that evaluates SSq itself; no model needed, d = 1..3.  Both touch the rows of the
 * walkers of half `half` (0 or 1) only and leave the other rows of every array as they are.
 * propose: q_new[n][d], inbox[n] (uint8) and logz_jac[n] = J of step 4.  inbox is 1 for a proposal inside the box, 0 for one
 * outside and for a stuck walker, whose q_new row is its own q and whose logz_jac is 0.
 * accept: the decision with the caller's ssq_new[n] (read where inbox is 1) at q_new (propose's, unchanged), in place in q, l and
 * the three counters.  It takes J from logz_jac and does not form the proposal again.
 * RSF_ERR_INVALID: as rsf_ensemble_run without the solve's arguments, d outside 1..3, iter < 1 or past 2^32 - 1, half not 0 or 1. */
int rsf_ensemble_propose(rsf_ctx *ctx, int64_t n, int32_t d, const double *q, const double *l, const double *lo, const double *hi, double a,
                         uint32_t logmask, uint64_t seed, int64_t offset, int64_t iter, int32_t half, double *q_new, uint8_t *inbox,
                         double *logz_jac);
int rsf_ensemble_accept(rsf_ctx *ctx, int64_t n, int32_t d, double *q, double *l, const double *lo, const double *hi, double shape,
                        uint64_t seed, int64_t offset, int64_t iter, int32_t half, const double *q_new, const uint8_t *inbox,
                        const double *logz_jac, const double *ssq_new, int32_t *accepted, int32_t *outbox, int32_t *stuck);

/* The solve of one half-step alone, between propose and accept, for a caller that wants the fused kernel's own SSq: needs a model,
 * d = 1 or 3.  ssq_new[j] = SSq(q_new[j]) for the walkers j of half `half` whose inbox is 1, solved in rsf_ensemble_run's
 * arrangement (one workgroup per island, lane i the mover i); every other entry of ssq_new stays as it is.  propose, this call and
 * accept for half 0 and then half 1 give rsf_ensemble_run's iteration BIT FOR BIT.  That needs this arrangement: the float64 RK4
 * tier code takes its tier decisions per wave, so the last bits of a trajectory depend on the trajectories it shares a wave
 * with, and a sum of squares from any other call (rsf_fit_normal, rsf_forward_batch) agrees to rounding only.
 * data, n_groups and the model's flags: rsf_ensemble_run's.  RSF_ERR_INVALID: n, d, n_groups or half as there, a NULL pointer. */
int rsf_ensemble_ssq(rsf_ctx *ctx, int64_t n, int32_t d, const double *q_new, const uint8_t *inbox, const double *data, int32_t n_groups,
                     int32_t half, double *ssq_new);

#ifdef __cplusplus
}
#endif
#endif /* RSF_ENSEMBLE_H */
