/*
 * rsf_law_grid.h — the EXACT POSTERIOR OF A STATE-LAW MODEL on a tensor grid laid in the coordinates of a fit.  Exported by
 * librsf_hip.so only; tests/law_grid_reference.py is the specification.
 *
 * The target is rsf_grid.h's, pi(q) ~ 1_box(q) SSq(q)^-shape, with SSq the sum of squares of rsf_law_observe: either state law, any
 * of the four observables, the loading table in use.  On laboratory data its mass is a small oblique ellipsoid, so the grid is a
 * tensor grid in WHITENED coordinates z, mapped to the parameters by the fit:
 *
 *     phi = m + L z        m[d] the fit's point, L[d (d + 1) / 2] the row-major lower triangle of the factor of its covariance
 *     q_perm[p] = phi_p, or exp(phi_p) where tr[p] != 0        perm[d]: which of (Dc, a, b) phi_p is — a permutation of 0 .. d - 1
 *
 * Formation of a node (one definition on the device, law_grid_point):  m_p + sum_{r <= p} L_pr z_r is accumulated as an unevaluated
 * sum s + e (the products split exactly, the sums by TwoSum);  phi_p = s + e rounded once, err_p its rounding error;  q = phi_p, or
 * fma(E, err_p, E) with E = exp(phi_p): q is within 4 ulp of the exactly formed value, also where the window cancels m against L z.
 *
 * Grid: rsf_grid.h's — d axes of n[p] >= 2 nodes z_p (strictly increasing, finite), node (i0, i1, i2) at the flat index
 * i0 + n0 (i1 + n1 i2), N = prod n_p < 2^31, a column the n0 nodes of one (i1, i2).  L is lower-triangular, so parameter perm[0] is a
 * monotone function of z_0 alone: rsf_grid_columns, rsf_grid_finish, rsf_grid_draw and rsf_grid_cdf serve the z-grid as they are
 * (RSF_GRID_PLAIN), and the integral over q is theirs over z times prod L_pp (the Jacobian of tr is in l).
 *
 * Log density:  l = fma(-shape, log SSq, J) - logg;  J = sum over tr of log q_perm[p], for a node as for a given point: at a node that is
 * phi_p to the rounding of exp and log, and a node given back as a point (q_out) has the same l bit for bit.
 * -inf where q is outside the CLOSED box lo <= q <= hi or SSq is not finite or not > 0.  lo, hi, theta, q_out and center are in the
 * order (Dc, a, b) whatever perm is.
 *
 * Arrays live in the ctx memory space unless marked HOST.  Every sum has a fixed order that depends on the shapes alone and no
 * floating-point atomic is used.
 */
#ifndef RSF_LAW_GRID_H
#define RSF_LAW_GRID_H

#include "rsf_abi.h"
#include "rsf_observe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSF_LAW_GRID_MAX_PARAMS 3
/* per column: sums of W = ((w0 w1) w2) e times 1, dq_0, dq_1, dq_2, dq_0 dq_0, dq_0 dq_1, dq_0 dq_2, dq_1 dq_1, dq_1 dq_2, dq_2 dq_2, SSq, SSq^2 */
#define RSF_LAW_GRID_FIELDS 12

/* The fused hot path; needs a model (rsf_set_model).  One lane per point: one float64 RK4 solve under `law` (RSF_LAW_*) with a
 * running sum of squares of `observable` (RSF_OBS_*) against data[nout], sample 0 included — rsf_law_observe's, bit for bit.
 * The N points come from one of two sources:
 *     theta == NULL   the nodes of the grid (d, n[d], z: HOST, the axes one after the other) under the map (m, L, tr, perm: HOST);
 *                     N = prod n_p
 *     theta != NULL   theta[npoints][d] as given, N = npoints; n and z are not read.  m and L are not read; tr and perm say which
 *                     parameters' logarithms enter J
 * logg[N] (may be NULL: 0) is subtracted.  l[N], ssq[N] (NaN outside the box); q_out[N][d] (may be NULL): the point each lane solved.
 * d = 1 (Dc; a and b the model's) or 3.  The solve is damped if the model is and k1 != 0.  A wave of 64 points none of which is inside
 * the box does not solve.  lo[d], hi[d]: HOST.
 * RSF_ERR_STATE: no model.  RSF_ERR_UNSUPPORTED: a model flagged RSF_FLAG_DOP853.  RSF_ERR_INVALID: law or observable unknown, d not
 * 1 or 3, the grid as rsf_grid_logtarget refuses it, npoints < 1 with theta, m or L not finite, a diagonal entry of L not > 0, perm
 * not a permutation, shape not finite and > 0, lo >= hi or not finite, a logged parameter with lo <= 0, a NULL pointer. */
int rsf_law_logtarget(rsf_ctx *ctx, int32_t law, int32_t observable, int32_t d, const int32_t *n, const double *z, const double *m,
                      const double *L, const int32_t *tr, const int32_t *perm, int64_t npoints, const double *theta, const double *logg,
                      const double *data, double shape, const double *lo, const double *hi, double *l, double *ssq, double *q_out);

/* The moments in natural coordinates of any l[N], ssq[N] on the grid (ssq is read where l is finite); no model needed.  z, w: HOST,
 * the axes' nodes and weights; lmax: rsf_grid_columns'; center[d] (HOST): c of dq = q - c, in the order (Dc, a, b).
 *     fields[N / n0][RSF_LAW_GRID_FIELDS]   per column: thread t of 256 adds nodes t, t + 256, .. in that order, then the wave's descending
 *                                           shuffle tree, then the four waves in index order; the node's q is re-formed from its index
 *     total[RSF_LAW_GRID_FIELDS] (HOST)     the columns added in index order from 0
 * Entries of dq a d = 1 grid lacks are 0.  fields may be NULL.
 * RSF_ERR_INVALID: the grid and the map as above, a weight not finite or not > 0, lmax NaN or +inf, center not finite, a NULL pointer. */
int rsf_law_grid_moments(rsf_ctx *ctx, int32_t d, const int32_t *n, const double *z, const double *w, const double *m, const double *L,
                         const int32_t *tr, const int32_t *perm, const double *l, const double *ssq, double lmax, const double *center,
                         double *fields, double *total);

#ifdef __cplusplus
}
#endif
#endif /* RSF_LAW_GRID_H */
