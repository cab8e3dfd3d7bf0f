/*
 * rsf_mala.h — GAUSS-NEWTON MANIFOLD MALA over the strict box: the simplified manifold Metropolis-adjusted Langevin sampler of
 * Girolami & Calderhead (2011) with the Gauss-Newton metric, whose proposal is rebuilt from the normal equations at the chain's point
 * in every iteration.  It takes no proposal covariance, adapts nothing and its Metropolis-Hastings correction is exact.  Exported by
 * librsf_hip.so only; tests/mala_reference.py is the specification.
 *
 * Target: pi(q) ~ 1_box(q) SSq(q)^-shape (sigma^2 integrated out; rsf_smc_std2 with l = -shape log ssq completes a state).
 * Chain state: q[d], ssq, grad[d] = X^T r and jtj[d][d] = X^T X, exactly as rsf_fit_normal leaves them.
 * Constants: eps > 0 (step), lam >= 0 (damping of the metric), shape > 0.
 * Draws of chain i in iteration t: z (d normals) and u of rsf_mcmc_draws(seed, offset + i, t, d).
 *
 * Propose:
 *     1. A = jtj + lam diag(jtj) = L L^T, rsf_fit's factor in its operation order.  A pivot that is not positive and finite, or an
 *        ssq that is not finite and > 0: NO PROPOSAL, the chain is STUCK for this iteration and nothing is solved.
 *     2. delta = -A^-1 grad (the factor's two triangular solves), and w from L^T w = z.
 *     3. s = eps sqrt(ssq / (2 shape)).
 *     4. q'_p = (q_p + (0.5 eps^2) delta_p) + s w_p.  Nothing is clamped: q' is inside iff lo_p < q'_p < hi_p for every p, and a
 *        proposal outside is rejected without a solve.  ld = sum_p log L_pp.
 *    The mean is q plus half the Levenberg-Marquardt step scaled by eps^2 (2 shape / ssq cancels), the covariance
 *    eps^2 (ssq / 2 shape) A^-1.
 * Decide, with (ssq', grad', jtj') at q':
 *     1. rejected if ssq' is not finite and > 0, or A' = jtj' + lam diag(jtj') does not factor; else A' = L' L'^T.
 *     2. delta' = -A'^-1 grad', e = q - (q' + (0.5 eps^2) delta'), v = L'^T e, ld' = sum_p log L'_pp.
 *     3. log alpha = -(shape + d / 2) (log ssq' - log ssq) + (ld' - ld) + 1/2 sum z^2 - (shape / (ssq' eps^2)) sum v^2.
 *     4. accepted iff log u < log alpha (a NaN compares false: rejected).
 *     5. accepted: (q, ssq, grad, jtj) <- (q', ssq', grad', jtj').  A chain that does not move keeps its bits.
 * This is the Metropolis-Hastings ratio of the proposal N(m(q), eps^2 G(q)^-1), G = (2 shape / ssq) A, against pi.  Any
 * deterministic symmetric positive definite function of q is a valid metric: the noise of the forward differences in grad and jtj
 * changes the efficiency, not the target.
 *
 * Arrays live in the ctx memory space unless marked HOST (an RSF_MEM_HOST caller is staged through the ctx workspace, as
 * rsf_fit_decide's); q[n][d] row-major, grad[n][d], jtj[n][d][d] (full, symmetric).  accepted[n], outbox[n] and stuck[n] are
 * int32 counters per chain, INCREMENTED in place (no atomic: a chain's counters are written by one lane): per iteration at most one
 * of them grows, outbox for a proposal outside the box, stuck for no proposal; a proposal inside that is rejected grows none.  The
 * same call gives the same bits, host or device memory alike.
 */
#ifndef RSF_MALA_H
#define RSF_MALA_H

#include "rsf_fit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_MALA_MAX_PARAMS 3
#define RSF_MALA_MAX_ITER 64 /* iterations per rsf_mala_run call */

/* The fused hot path; needs a model, d = 1 or 3.  n_iter (1 .. RSF_MALA_MAX_ITER) iterations inside one launch, in place in q, ssq,
 * grad and jtj; iteration k = 0 .. n_iter - 1 uses the draws of Philox iteration iter0 + k (iter0 >= 1) and is one group solve
 * (q' and its d forward-difference neighbours in adjacent lanes).  data[n_groups][nout], fd, the split of the chains over the
 * series and the treatment of the model's flags: rsf_fit_normal's (float64 RK4, damped or not, also for RSF_FLAG_FP32_SOLVE;
 * RSF_FLAG_DOP853: RSF_ERR_UNSUPPORTED).  lo[d], hi[d]: HOST.  trace_q[n_iter][n][d] and trace_ssq[n_iter][n]: the state after
 * each iteration, iteration-major as rsf_mcmc_run's traces; both NULL, or both given.
 * RSF_ERR_STATE: no model.  RSF_ERR_INVALID: n < 1, d not 1 or 3, n_groups < 1 or the split, fd, eps or shape not finite and > 0,
 * lam not finite or < 0, n_iter outside 1..64, iter0 < 1 or iter0 + n_iter past 2^32, offset < 0, lo >= hi or not finite, a NULL
 * pointer, one trace without the other. */
int rsf_mala_run(rsf_ctx *ctx, int64_t n, int32_t d, double *q, double *ssq, double *grad, double *jtj, const double *data,
                 int32_t n_groups, const double *lo, const double *hi, double fd, double eps, double lam, double shape, uint64_t seed,
                 int64_t offset, int64_t iter0, int32_t n_iter, int32_t *accepted, int32_t *outbox, int32_t *stuck, double *trace_q,
                 double *trace_ssq);

/* The same iteration in two halves, for a caller that evaluates the residuals itself; no model needed, d = 1..3.
 * propose: q_new[n][d], inbox[n] and stuck[n] (uint8).  inbox is 1 for a proposal inside the box, 0 for one outside AND for a
 * stuck chain; stuck is 1 for a chain without a proposal.  The q_new row of a chain whose inbox is 0 is its own q.
 * accept: the decision with the caller's ssq_new[n], grad_new[n][d], jtj_new[n][d][d] (read where inbox is 1) at q_new (propose's,
 * unchanged), in place in q, ssq, grad and jtj, and the three counters.  It forms the factor at q again, so it takes the arguments
 * propose took.
 * RSF_ERR_INVALID: as rsf_mala_run without the solve's arguments, d outside 1..3, iter < 1 or past 2^32 - 1. */
int rsf_mala_propose(rsf_ctx *ctx, int64_t n, int32_t d, const double *q, const double *ssq, const double *grad, const double *jtj,
                     const double *lo, const double *hi, double eps, double lam, double shape, uint64_t seed, int64_t offset,
                     int64_t iter, double *q_new, uint8_t *inbox, uint8_t *stuck);
int rsf_mala_accept(rsf_ctx *ctx, int64_t n, int32_t d, double *q, double *ssq, double *grad, double *jtj, const double *lo,
                    const double *hi, double eps, double lam, double shape, uint64_t seed, int64_t offset, int64_t iter,
                    const double *q_new, const uint8_t *inbox, const double *ssq_new, const double *grad_new, const double *jtj_new,
                    int32_t *accepted, int32_t *outbox, int32_t *stuck);

#ifdef __cplusplus
}
#endif
#endif /* RSF_MALA_H */
