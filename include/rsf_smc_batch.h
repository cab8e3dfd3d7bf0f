/*
 * rsf_smc_batch.h — P INDEPENDENT POPULATIONS of the tempered sequential Monte Carlo sampler (rsf_smc.h) per call.  Exported by
 * librsf_hip.so only.  The specification is rsf_smc.h's single call: every population of a batched call equals, bit for bit, the
 * single call with that population's seed, offset, data row and parameters (tests/test_gpu_smc_batch.py).
 *
 * A population is n particles with a Philox stream (seed, offset), an observation series (a row `group[p]` of data[G][nout]) and its
 * own place on the temperature ladder (beta, delta, lmax, the stage's uniform, the iteration, the proposal factor).  A replicate is a
 * population with another seed, an observation group a population with another data row.  n, d, the box, the shape and the
 * number of Metropolis steps are the call's.
 *
 * Layout: populations p = 0 .. P - 1, q[P][n][d] and l[P][n] (and cum, anc, q_out, l_out, std2 alike) in the ctx memory space;
 * data[G][nout] in the ctx memory space; every per-population parameter array is HOST.  1 <= P <= RSF_SMC_BATCH_MAX.
 * active[P] (HOST, uint8) marks the populations a call works on.  An inactive population is left exactly as it was: its rows of q,
 * l, cum, anc, accepted and out are not touched, its parameters are not looked at, and where the result is another buffer
 * (rsf_smc_batch_resample's q_out, l_out) its particles are copied through.
 *
 * Geometry: the launch grid's x dimension is what the single call derives from n, y is the population; every sum keeps the single
 * call's order within a population and no floating-point atomic is used.  Host and device memory give the same bits.
 *
 * Status codes and argument rules are the single calls'; in addition RSF_ERR_INVALID for P outside 1..RSF_SMC_BATCH_MAX, a
 * group[p] outside 0..G-1, G < 1 and a NULL array.  A message about one population names it ("population p").
 */
#ifndef RSF_SMC_BATCH_H
#define RSF_SMC_BATCH_H

#include "rsf_smc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_SMC_BATCH_MAX 64 /* populations per call */

/* rsf_smc_init for each population: q[p] from (seeds[p], offsets[p]).  seeds[P] (uint64), offsets[P] (int64): HOST. */
int rsf_smc_batch_init(rsf_ctx *ctx, int32_t P, int64_t n, int32_t d, const double *lo, const double *hi, const uint64_t *seeds,
                       const int64_t *offsets, double *q);

/* The start's l[p][j] = -shape log SSq(q[p][j]) against data[group[p]] (-inf where q lies outside the strict box, or SSq is not
 * finite or not positive): the solve of rsf_smc_batch_move, what rsf_evidence_logtarget gives with no transform and logg = 0.
 * Needs a model; d = 1 or 3; group[P] (int32): HOST.  A model flagged RSF_FLAG_DOP853 is refused (RSF_ERR_UNSUPPORTED). */
int rsf_smc_batch_logtarget(rsf_ctx *ctx, int32_t P, int64_t n, int32_t d, const double *q, const double *data, int32_t G,
                            const int32_t *group, double shape, const double *lo, const double *hi, double *l);

/* rsf_smc_weight_sums for each active population: deltas[P][m] and lmax[P] HOST (lmax[p] NaN: the population's own largest finite l),
 * out[P][RSF_SMC_HEAD + 2 m] HOST.  A population whose l holds a NaN or +inf, or no finite entry at all, is that population's
 * error (the first such population is named; out is then not written). */
int rsf_smc_batch_weight_sums(rsf_ctx *ctx, int32_t P, int64_t n, const double *l, int32_t m, const double *deltas, const double *lmax,
                              const uint8_t *active, double *out);

/* rsf_smc_resample for each active population with delta[p], lmax[p], u[p] (HOST).  cum[P][n]; anc[P][n] (int64) is local to the
 * population, 0 .. n - 1; q_out[P][n][d], l_out[P][n] (they must not overlap q and l). */
int rsf_smc_batch_resample(rsf_ctx *ctx, int32_t P, int64_t n, int32_t d, const double *q, const double *l, const double *delta,
                           const double *lmax, const double *u, const uint8_t *active, double *cum, int64_t *anc, double *q_out,
                           double *l_out);

/* The fused hot path, rsf_smc_move for each active population in ONE launch: `steps` Metropolis steps per particle in place in q
 * and l, population p on pi_beta[p] against data[group[p]] with the proposal factor chol[p][d][d], the stream (seeds[p], offsets[p])
 * and the first iteration iter0[p].  chol, beta, seeds, offsets, iter0 (int64), group (int32): HOST.  accepted[P][steps] (HOST,
 * int64, out).  A workgroup belongs to one population; a wave none of whose proposals is inside the box does not solve. */
int rsf_smc_batch_move(rsf_ctx *ctx, int32_t P, int64_t n, int32_t d, double *q, double *l, const double *data, int32_t G,
                       const int32_t *group, double shape, const double *lo, const double *hi, const double *chol, const double *beta,
                       const uint64_t *seeds, const int64_t *offsets, const int64_t *iter0, int32_t steps, const uint8_t *active,
                       int64_t *accepted);

/* rsf_smc_std2 for each population: std2[p] from l[p] with the gamma variates of (seeds[p], offsets[p] + j, iter[p]). */
int rsf_smc_batch_std2(rsf_ctx *ctx, int32_t P, int64_t n, const double *l, double shape, const uint64_t *seeds, const int64_t *offsets,
                       const int64_t *iter, double *std2);

#ifdef __cplusplus
}
#endif
#endif /* RSF_SMC_BATCH_H */
