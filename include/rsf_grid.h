/*
 * rsf_grid.h — the EXACT POSTERIOR on a tensor quadrature grid.  Exported by librsf_hip.so only; tests/grid_reference.py is the
 * specification.
 *
 * With n0 = 0 the sampler's target is pi(q) ~ 1_box(q) SSq(q)^-shape (tests/posterior_reference.py).  The parameter vector has at
 * most three entries, so pi is tabulated: one forward solve per node of a tensor grid, then fixed-order sums.
 *
 * Grid.  d axes; axis p has n[p] >= 2 nodes x_p (strictly increasing, finite) and weights w_p (finite, > 0): the quadrature rule is
 * the caller's.  x and w are HOST arrays, the axes one after the other (n[0] + .. + n[d-1] doubles each).  Node (i0, i1, i2) has
 * the flat index i = i0 + n0 (i1 + n1 i2), axis 0 fastest; N = prod n_p < 2^31.  A COLUMN is the n0 nodes of one (i1, i2); column
 * c = i1 + n1 i2; there are N / n0 of them.  An axis the grid does not have counts as one node of weight 1.
 *
 * Coordinates.  RSF_GRID_PLAIN: q = x.  RSF_GRID_PRODUCT (d = 3): x0 = Dc a, q = (x0 / x1, x1, x2); the density in x is pi(q) / x1.
 *
 * Log density of node i:  l_i = fma(-shape, log SSq(q_i), -[PRODUCT] log x1); -inf where q_i is outside the CLOSED box
 * lo <= q <= hi (a node on a face carries a quadrature weight) or SSq is not finite or not > 0.
 * Weights:  e_i = exp(l_i - lmax) (0 for -inf), lmax the largest finite l;  W_i = ((w0 w1) w2) e_i;  Z = sum W;
 * log_integral = lmax + log Z.
 *
 * Arrays live in the ctx memory space unless marked HOST.  Every sum has a fixed order that depends on the shapes alone and no
 * floating-point atomic is used: the same call gives the same bits, host or device memory alike.
 */
#ifndef RSF_GRID_H
#define RSF_GRID_H

#include "rsf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_GRID_MAX_PARAMS 3
#define RSF_GRID_PLAIN 0
#define RSF_GRID_PRODUCT 1
#define RSF_GRID_FIELDS 6 /* per column: sums over i0 of w0 e times 1, (x0 - c), (x0 - c)^2, SSq, SSq^2; then the count of -inf nodes */
#define RSF_GRID_HEAD 20  /* rsf_grid_finish's head, see there */

/* The fused hot path; needs a model (rsf_set_model).  One lane per node, the node formed from the flat index; one float64 RK4 solve
 * per node inside the box with a running sum of squares against data[nout].  l[N] as defined above; ssq[N]: the sum of squares,
 * NaN for a node outside the box.  d = 1 (Dc) or 3 (Dc, a, b).  The solve is rsf_evidence_logtarget's (float64 RK4, damped if the
 * model is and k1 != 0, also for a float32 model); RSF_FLAG_DOP853 is refused (RSF_ERR_UNSUPPORTED).  A wave of 64 nodes none of
 * which is inside the box does not solve.  n[d], x, lo[d], hi[d]: HOST.
 * RSF_ERR_STATE: no model.  RSF_ERR_INVALID: d not 1 or 3, n[p] < 2, N >= 2^31, nodes not finite or not increasing, coords not
 * PLAIN or PRODUCT, PRODUCT with d != 3 or lo[1] <= 0, shape not finite and > 0, lo >= hi or not finite, a NULL pointer. */
int rsf_grid_logtarget(rsf_ctx *ctx, int32_t d, const int32_t *n, const double *x, const double *data, double shape, const double *lo,
                       const double *hi, int32_t coords, double *l, double *ssq);

/* The reductions over any l[N], ssq[N] (ssq is read where l is finite); d = 1..3.  center: c of the column fields.
 *     *lmax (HOST)       the largest finite l, a pass of its own; -inf when no l is finite (every output below is then 0 but the counts)
 *     fields[N / n0][RSF_GRID_FIELDS]   per column, thread t of 256 adds nodes t, t + 256, .. in that order, then the wave's descending
 *                        shuffle tree, then the four waves in index order
 *     m0[n0]             sum over the columns in index order of (w1 w2) e, one thread per i0
 *     cum0[N]            per column the trapezoid CDF along axis 0 of the node density e: F[0] = 0, F[k+1] = F[k] + 1/2 (e_k + e_{k+1})
 *                        (x_{k+1} - x_k) added in node order, then every entry divided by F[n0-1]; all 0 for a column without mass
 * m0 and cum0 may be NULL (not computed).
 * RSF_ERR_INVALID: the grid as above, a weight not finite or not > 0, center not finite, an l that is NaN or +inf, a NULL pointer. */
int rsf_grid_columns(rsf_ctx *ctx, int32_t d, const int32_t *n, const double *x, const double *w, const double *l, const double *ssq,
                     double center, double *lmax, double *fields, double *m0, double *cum0);

/* Host only (no ctx, no GPU).  fields: rsf_grid_columns' (HOST), taken at (center, lmax); the columns are added in index order.
 *     head[RSF_GRID_HEAD] = [ Z, log_integral, log_evidence, nodes with l = -inf, mean[3], cov[3][3], mean and variance of x0 (Dc a in
 *                             PRODUCT), mean and variance of sigma^2 ]
 *       log_evidence = log_integral - sum_p log(hi_p - lo_p) + lgamma(shape) - shape log(pi)         (rsf_evidence_finish's)
 *       mean, cov: of q (in PRODUCT q0 = x0 / x1, a per-column divisor); unused entries of a d < 3 grid are NaN
 *       sigma^2 ~ the mixture over the nodes of InvGamma(shape, SSq / 2): E = sum W SSq / 2 / (shape - 1) / Z, second raw moment
 *       sum W (SSq / 2)^2 / ((shape - 1)(shape - 2)) / Z (NaN for shape <= 2)
 *     mass1[n1], mass2[n2]   node masses of axes 1 and 2 (sum 1);     pair[n2][n1]   the column masses (sum 1)
 *     cum1[n2][n1]   for each axis-2 node the trapezoid CDF along axis 1 of pair[i2][.] / w1, normalised by its last entry (0: no mass)
 *     cum2[n2]       the trapezoid CDF of mass2 / w2, normalised
 * lmax = -inf (no finite node): log_integral = -inf, every other output NaN but the count, and RSF_OK.
 * RSF_ERR_INVALID: the grid or the box as above, shape not finite and > 0, center not finite, lmax NaN or +inf, a NULL pointer. */
int rsf_grid_finish(int32_t d, const int32_t *n, const double *x, const double *w, int32_t coords, double center, double shape,
                    const double *lo, const double *hi, double lmax, const double *fields, double *head, double *mass1, double *mass2,
                    double *pair, double *cum1, double *cum2);

/* nd independent draws.  Draw j takes the uniforms u_0, u_1, u_2 rsf_smc_init defines for (seed, offset + j) (rsf_smc.h); shards with
 * offsets 0 and k form one stream.  The top axis t = d - 1 is inverted from its table with u_t: k the largest index <= n - 2 with
 * F[k] <= u, x = x[k] + (u - F[k]) / (F[k+1] - F[k]) (x[k+1] - x[k]), x = x[k] where the cell has no mass.  The next axis is drawn
 * conditional on the node nearest to x (a tie: the lower node): axis 1 from cum1[i2], axis 0 from cum0[., i1, i2].
 *     q[nd][d]      the draw in q (PRODUCT: (x0 / x1, x1, x2));     cell[nd][d] (int32, may be NULL)   k of each axis
 * cum1[n2][n1], cum2[n2]: HOST, rsf_grid_finish's (not read for the axes a d < 3 grid lacks; may then be NULL).
 * RSF_ERR_INVALID: the grid as above, nd < 1, offset < 0, a NULL pointer. */
int rsf_grid_draw(rsf_ctx *ctx, int32_t d, const int32_t *n, const double *x, int32_t coords, const double *cum0, const double *cum1,
                  const double *cum2, uint64_t seed, int64_t offset, int64_t nd, double *q, int32_t *cell);

/* The CDF of q0 at the points xs[nx] (HOST): F[k] (HOST) = sum over the columns in index order of pair[c] F0(xs_k x1 | c) in PRODUCT,
 * pair[c] F0(xs_k | c) in PLAIN; F0 is cum0's column, linearly interpolated, 0 to the left and 1 to the right.  One thread per
 * point.  pair[N / n0]: HOST, rsf_grid_finish's.
 * Resolution: in PRODUCT, F0(x x1 | c) is, as a function of x1, a step about as wide as the posterior of x0 is narrow; the sum is as
 * good as the axis-1 nodes resolve that step, which takes more nodes than the moments do (at 65 nodes Dc's 0.975
 * quantile was 0.32 Monte-Carlo SE of a 262 144-draw pool off, at 129 nodes 0.013).  A caller may refine axis 1 by interpolating the
 * columns of cum0 and the masses between neighbouring nodes and pass the refined grid, as GridPosterior.dc_cdf (engine.py) does. */
int rsf_grid_cdf(rsf_ctx *ctx, int32_t d, const int32_t *n, const double *x, int32_t coords, const double *cum0, const double *pair,
                 int64_t nx, const double *xs, double *F);

#ifdef __cplusplus
}
#endif
#endif /* RSF_GRID_H */
