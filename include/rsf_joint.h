/*
 * rsf_joint.h — the JOINT posterior of the pooled draws: covariance and correlation of all parameters, and the pairwise
 * marginals a corner plot is made of (2-D Gaussian KDE, 2-D histogram, highest-density contour levels).  rsf_pool_summary,
 * rsf_pool_kde and rsf_pool_histogram (rsf_abi.h) look at one column; these look at the (n, d) block.  Exported by
 * librsf_hip.so only; tests/joint_reference.py is the specification.
 *
 * x is always the base of an (n, d) ROW-MAJOR block of float64 in the ctx memory space; pa and pb are column indices in
 * [0, d), pa != pb.  Every result is deterministic: sums have a fixed order that depends on the inputs' shape alone and no
 * floating-point atomic is used, so the same call gives the same bits, host or device memory alike.
 */
#ifndef RSF_JOINT_H
#define RSF_JOINT_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_JOINT_MAX_PARAMS 8      /* columns of a block whose joint moments are taken */
#define RSF_JOINT_HEAD 2            /* fields of the partials before the sums: n_finite, nonfinite */
#define RSF_HIST2D_MAX_CELLS 16384  /* (nbx + 2) (nby + 2): 64 KiB of 32-bit counters in a workgroup's LDS */
/* doubles of rsf_pool_joint_partials' partials and of rsf_pool_joint_finish's out, for d columns */
#define RSF_JOINT_PARTIALS(d) (RSF_JOINT_HEAD + (d) + (d) * ((d) + 1) / 2)
#define RSF_JOINT_OUT(d) ((d) + 2 * (d) * (d))

/* Additive partials of the joint moments of the d columns about center[d], 1 <= d <= RSF_JOINT_MAX_PARAMS:
 *     partials = [ n_finite, nonfinite, sum (x_p - c_p) for p < d, sum (x_p - c_p)(x_q - c_q) for p <= q (row-major upper triangle) ]
 * A row with any non-finite entry is counted in `nonfinite` and left out of every sum.  The partials are plain sums about a
 * centre the caller chooses: with the same centre the partials of shards add to the partials of their union
 * (rsf_pool_allreduce_sum).  Choose the centre within a few standard deviations of the mean (a draw of the pool will do): the
 * cancellation in rsf_pool_joint_finish grows with the square of that distance.
 * center[d] and partials[RSF_JOINT_PARTIALS(d)]: HOST arrays in every mem_space.
 * RSF_ERR_INVALID: n < 1, d outside 1..RSF_JOINT_MAX_PARAMS, a non-finite centre, a NULL pointer. */
int rsf_pool_joint_partials(rsf_ctx *ctx, int64_t n, int32_t d, const double *x, const double *center, double *partials);

/* Host only (no ctx, no GPU): out = [ mean[d], cov[d][d] (ddof = 1, numpy.cov), corr[d][d] (numpy.corrcoef) ] of summed partials
 * and the centre they were taken about.  n_finite < 2: cov and corr are NaN (n_finite = 0: the mean too).  A column of zero
 * variance has NaN in its row and column of corr, the diagonal included; elsewhere the diagonal of corr is 1. */
int rsf_pool_joint_finish(int32_t d, const double *partials, const double *center, double *out);

/* scipy.stats.gaussian_kde(np.vstack([x[:, pa], x[:, pb]]), bw_method).pdf(points.T) at m arbitrary points:
 *     density[j] = 1 / (n_total 2 pi sqrt(det H)) sum_i exp(-1/2 (p_j - x_i)^T H^-1 (p_j - x_i)),    H = cov f^2,
 * f = bw_factor if > 0, else Scott's factor for two dimensions n_total^(-1/6).  points[m][2] and density[m]: ctx memory space.
 * cov2 (HOST, row-major 2 x 2 of (pa, pb); NULL: the data covariance of these n rows, from the library's joint moments) and
 * n_total (0: n) let a shard of a larger pool be evaluated with the pool's bandwidth: the value is then
 * sum_{i in shard} K_H(p_j - x_i) / n_total, and the densities of disjoint shards ADD to the density of their union.
 * n >= 3.  Every row must be finite.  The kernel works on whitened, centred coordinates (the centre is the mean of these n
 * rows), so a parameter near 1000 with a spread of a few units loses nothing.  Points further than about 1e150 bandwidths
 * from every draw are outside the domain.
 * RSF_ERR_INVALID with "singular KDE" in the message, as rsf_pool_kde for zero variance: a covariance that is not finite
 * or not positive definite — in floating point: h00 <= 0, h11 <= 0 or det H <= 1e-12 h00 h11 (|correlation| within 5e-13 of
 * 1, where the determinant is rounding).  SciPy raises there.
 * RSF_ERR_INVALID: n < 3, m < 1, pa or pb outside [0, d) or equal, n_total < 0 or (not 0 and) < n, a NULL required pointer. */
int rsf_pool_kde2d(rsf_ctx *ctx, int64_t n, int32_t d, const double *x, int32_t pa, int32_t pb, int32_t m, const double *points,
                   double bw_factor, const double *cov2, int64_t n_total, double *density);

/* numpy.histogram2d(x[:, pa], x[:, pb], (nbx, nby), ((lo_a, hi_a), (lo_b, hi_b))) with the out-of-range counts:
 * counts[(nbx + 2)][(nby + 2)] row-major (ctx memory space), float64 holding exact integers.  Per axis the index is
 * rsf_pool_histogram's: 0 = below lo, 1 + b = numpy's bin b (edges numpy.linspace(lo, hi, nb + 1), edge cases included),
 * nb + 1 = above hi or NaN.  The interior [1:-1, 1:-1] is numpy's result; every row lands in exactly one cell, so the counts
 * sum to n, and counts of shards add (rsf_pool_allreduce_sum).
 * RSF_ERR_INVALID: nbx < 1, nby < 1, (nbx + 2)(nby + 2) > RSF_HIST2D_MAX_CELLS, lo < hi not finite on either axis, n < 1,
 * pa or pb outside [0, d) or equal, a NULL pointer. */
int rsf_pool_histogram2d(rsf_ctx *ctx, int64_t n, int32_t d, const double *x, int32_t pa, int32_t pb, int32_t nbx, double lo_a,
                         double hi_a, int32_t nby, double lo_b, double hi_b, double *counts);

/* Host only (no ctx, no GPU): the contour levels of a corner plot.  weights[m] >= 0 are histogram counts, or densities on a
 * regular grid.  levels[k] = the largest value w among the weights such that the sum of all weights >= w is >= probs[k] total:
 * the region {weight >= levels[k]} is the smallest union of cells that holds the mass probs[k] (ties enter together).
 * RSF_ERR_INVALID: m < 1, n_probs < 1, a negative or non-finite weight, total = 0, a probability not strictly inside (0, 1). */
int rsf_pool_hpd_levels(int64_t m, const double *weights, int32_t n_probs, const double *probs, double *levels);

#ifdef __cplusplus
}
#endif
#endif /* RSF_JOINT_H */
