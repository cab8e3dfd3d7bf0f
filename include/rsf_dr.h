/*
 * rsf_dr.h — TWO-STAGE DELAYED-REJECTION METROPOLIS over the strict box (Mira 2001; the "DR" of Haario et al.'s DRAM): a random
 * walk whose chain, when its first proposal is rejected, makes a second, narrower one in the same iteration, with the correction
 * term that keeps the target exact.  A first proposal outside the box costs no solve.  It needs no gradient, no fit and no other
 * chain.  Exported by librsf_hip.so only; tests/dr_reference.py is the specification.
 *
 * Target: pi(q) ~ 1_box(q) SSq(q)^-shape (sigma^2 integrated out; rsf_smc_std2 with the chains' l completes a state).
 * Chain state: q[d] and l = -shape log SSq(q) (-inf where SSq is not finite and > 0), as the SMC particles carry it.
 *
 * Chain j of q[n][d] (row-major) uses the Philox particle g = offset + j.  Iteration t >= 1, with the factor L of the chain's
 * group (row-major lower triangle, d (d + 1) / 2 doubles: L00 | L10 L11 | L20 L21 L22) and the stage scale gamma in (0, 1]:
 *     1. Stage 1 draws, all of (seed, g, t): z1, the d normals of slots 0 and 1 as rsf_smc_move takes them; U1 = u53(w0, w1) of
 *        slot 2, the u of rsf_mcmc_draws.
 *     2. Stage 1 proposal: y1 = q + L z1 in rsf_smc_move's own arithmetic (one fused multiply-add per entry of L, in row order
 *        from q_p).  Nothing is clamped.  y1 outside the strict box: outbox1 grows, NO SOLVE, l1 = -inf, on to stage 2.  Inside:
 *        l1 = l(y1), -inf where SSq is not finite and > 0; accepted iff min(l1 - l, 0) > log U1 (a NaN compares false: rejected);
 *        then (q, l) <- (y1, l1), accepted1 grows and the iteration ends.
 *     3. Stage 2 draws (stages = 2 only): z2, the normals of slots 5 and 6 by the same Box-Muller pair (slot 5: components 0 and
 *        1, slot 6: component 2); U2 = u53(w2, w3) of slot 2's words.  Slots 3 and 4 belong to the ensemble sampler's partner
 *        and to the SMC resampling.
 *     4. Stage 2 proposal: v_p = L_p0 z2_0, then + L_pr z2_r for r = 1 .. p, each product and each sum rounded;
 *        y2_p = q_p + gamma v_p, a rounded product and a rounded sum.  y2 outside the box: outbox2 grows, the state is kept.
 *        Inside: l2 = l(y2); rejected if l2 is not finite.
 *     5. Stage 2 decision.  w_p = z1_p - gamma z2_p (a rounded product, a rounded difference); Sw = sum w_p w_p and S1 = sum
 *        z1_p z1_p, each from 0.0 in index order, every operation rounded; log q = -0.5 (Sw - S1), the exact logarithm of
 *        N(y1; y2, L L^T) / N(y1; q, L L^T).  T = 0 when l1 = -inf; the proposal is rejected when l1 >= l2; otherwise
 *        A = log(-expm1(l1 - l2)), B = log(-expm1(l1 - l)) (l1 < l: stage 1 was rejected).
 *        log alpha2 = (((l2 - l) + log q) + A) - B, without A and B when l1 = -inf; accepted iff min(log alpha2, 0) > log U2;
 *        then (q, l) <- (y2, l2) and accepted2 grows.
 * With stages = 1 an iteration ends after step 2 and is rsf_smc_move's at beta = 1 with the same factor, seed, offset and
 * iterations, BIT FOR BIT.
 *
 * Start states.  A chain whose q is not strictly inside the box, or whose l is not finite, is STUCK: it makes no proposal,
 * nothing is solved for it and its stuck counter grows.  The Python layer refuses such starts.
 *
 * Groups.  n_groups (1 .. RSF_DR_MAX_GROUPS) observation series data[n_groups][nout] and factors chol[n_groups][d (d + 1) / 2];
 * the chains are split evenly over them in order.  With n_groups > 1, n / n_groups is a multiple of the ctx's workgroup size B
 * (rsf_config.block_threads: 64, 128 or 256; 0 means 256); with one group n is any count >= 1.
 *
 * Arrays live in the ctx memory space unless marked HOST (an RSF_MEM_HOST caller is staged through the ctx workspace, as
 * rsf_ensemble_run's).  accepted1[n], accepted2[n], outbox1[n], outbox2[n] and stuck[n] are int32 counters per chain, INCREMENTED
 * in place by the chain's own lane.  No floating-point atomic, no sum across lanes: the same call gives the same bits, host or
 * device memory alike.
 */
#ifndef RSF_DR_H
#define RSF_DR_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_DR_MAX_PARAMS 3
#define RSF_DR_MAX_ITER 64   /* iterations per rsf_dr_run call */
#define RSF_DR_MAX_GROUPS 64 /* observation series, and factors, per call */

/* The fused hot path; needs a model, d = 1 (Dc) or 3 (Dc, a, b).  n_iter (1 .. RSF_DR_MAX_ITER) iterations inside one launch, in
 * place in q[n][d] and l[n]; iteration k = 0 .. n_iter - 1 uses the draws of Philox iteration iter0 + k (iter0 >= 1).  One lane per
 * chain; per iteration up to two float64 RK4 solves (damped or not, also for RSF_FLAG_FP32_SOLVE; RSF_FLAG_DOP853:
 * RSF_ERR_UNSUPPORTED), the second for the lanes rejected at stage 1 only; a wave in which no lane needs a solve skips it.
 * lo[d], hi[d], chol[n_groups][d (d + 1) / 2]: HOST.  trace_q[n_iter][n][d] and trace_l[n_iter][n]: the state after each iteration,
 * iteration-major; both NULL, or both given.
 * RSF_ERR_STATE: no model.  RSF_ERR_INVALID: gamma not in (0, 1]; stages not 1 or 2; a factor with a diagonal entry that is not
 * positive and finite (or any entry not finite); n < 1; n_groups outside 1 .. RSF_DR_MAX_GROUPS; with n_groups > 1, n not a multiple
 * of B n_groups; d not 1 or 3; shape not finite and > 0; n_iter outside 1 .. RSF_DR_MAX_ITER; iter0 < 1 or iter0 + n_iter past 2^32;
 * offset < 0; lo >= hi or not finite; a NULL pointer; one trace without the other. */
int rsf_dr_run(rsf_ctx *ctx, int64_t n, int32_t d, double *q, double *l, const double *data, int32_t n_groups, const double *lo,
               const double *hi, const double *chol, double gamma, int32_t stages, double shape, uint64_t seed, int64_t offset, int64_t iter0,
               int32_t n_iter, int32_t *accepted1, int32_t *accepted2, int32_t *outbox1, int32_t *outbox2, int32_t *stuck, double *trace_q,
               double *trace_l);

/* ONE STAGE of one iteration in two calls, for a caller that evaluates SSq itself; no model needed, d = 1..3, n any count >= 1 that
 * n_groups divides.  stage is 1 or 2.
 * propose: y[n][d] and mask[n] (uint8).  Stage 1: y = y1 and mask = 1 for a proposal inside the box; mask = 0 for one outside and
 * for a stuck chain, whose y row is its own q.  pending is not read (it may be NULL).  Stage 2: the chains whose pending[n]
 * (rsf_dr_accept's of stage 1) is 1 propose y = y2, mask = 1 inside the box; every other chain has y = q and mask = 0.
 * accept: the decision with the caller's ssq[n] (read where mask is 1) at y (propose's, unchanged), in place in q, l and the
 * counters.  Stage 1 WRITES l1[n] (l(y1), -inf outside the box) and pending[n] (1: not stuck and rejected at stage 1); stage 2
 * READS them.  It takes both stages' normals from the Philox stream and does not form a proposal again.
 * RSF_ERR_INVALID: as rsf_dr_run without the solve's arguments, d outside 1..3, n not a multiple of n_groups, stage not 1 or 2,
 * iter < 1 or past 2^32 - 1, pending NULL at stage 2. */
int rsf_dr_propose(rsf_ctx *ctx, int64_t n, int32_t d, const double *q, const double *l, int32_t n_groups, const double *lo, const double *hi,
                   const double *chol, double gamma, int32_t stage, uint64_t seed, int64_t offset, int64_t iter, const uint8_t *pending,
                   double *y, uint8_t *mask);
int rsf_dr_accept(rsf_ctx *ctx, int64_t n, int32_t d, double *q, double *l, const double *lo, const double *hi, double gamma, int32_t stage,
                  double shape, uint64_t seed, int64_t offset, int64_t iter, const double *y, const uint8_t *mask, const double *ssq, double *l1,
                  uint8_t *pending, int32_t *accepted1, int32_t *accepted2, int32_t *outbox1, int32_t *outbox2, int32_t *stuck);

/* The solve of one stage alone, between propose and accept, for a caller that wants the fused kernel's own SSq: needs a model,
 * d = 1 or 3.  ssq[j] = SSq(y[j]) for the chains whose mask is 1, solved in rsf_dr_run's arrangement (lane = chain, a masked-out
 * lane rides along with the same harmless point, a wave without a masked-in lane skips the solve); every other entry of ssq
 * stays as it is.  propose, this call and accept for stage 1 and then stage 2 give rsf_dr_run's iteration BIT FOR BIT.  That needs
 * this arrangement: the float64 RK4 tier code takes its tier decisions per wave (include/rsf_ensemble.h, rsf_ensemble_ssq).
 * data, n_groups and the model's flags: rsf_dr_run's.  RSF_ERR_INVALID: n, d or n_groups as there, a NULL pointer. */
int rsf_dr_ssq(rsf_ctx *ctx, int64_t n, int32_t d, const double *y, const uint8_t *mask, const double *data, int32_t n_groups, double *ssq);

#ifdef __cplusplus
}
#endif
#endif /* RSF_DR_H */
