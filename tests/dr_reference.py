"""
Specification of include/rsf_dr.h in NumPy (TEST INFRASTRUCTURE ONLY, no GPU): two-stage delayed-rejection Metropolis (Mira 2001)
over the strict box, on a supplied ssq_fn(points (m, d)) → SSq (m,).  Chain j draws from the Philox particle offset + j
(tests/smc_reference.py: words, u53, normals).

Iteration t >= 1 of a chain at (q, l), l = -shape log SSq(q), with the factor L (d, d) lower triangular and the stage scale gamma:
    stage 1     z1 = the normals of slots 0 and 1, U1 = u53(w0, w1) of slot 2: smc_reference.move_step's own draws.
                y1 = q + L z1 (smc_reference.propose).  Outside the strict box: outbox1 grows, no solve, l1 = -inf.  Inside:
                l1 = l(y1), -inf where SSq is not finite and > 0; accepted iff min(l1 - l, 0) > log U1.
    stage 2     (stages = 2, stage 1 rejected.)  z2 = the normals of slots 5 (components 0, 1) and 6 (component 2) by the same
                Box-Muller pair, U2 = u53(w2, w3) of slot 2's words.  v_p = L_p0 z2_0 + L_p1 z2_1 + .. in index order, every product
                and sum rounded to float64; y2_p = q_p + gamma v_p.  Outside the box: outbox2 grows.  Inside: l2 = l(y2), rejected if
                not finite.
    decision    w = z1 - gamma z2, log q = -0.5 (sum w^2 - sum z1^2), both sums from 0.0 in index order: the exact logarithm of
                N(y1; y2, L L^T) / N(y1; q, L L^T) (y1 - y2 = L w and y1 - q = L z1, so no triangular solve is needed).
                log alpha2 = (((l2 - l) + log q) + A) - B,  A = log(1 - alpha1(y2, y1)) = log(-expm1(l1 - l2)),
                B = log(1 - alpha1(q, y1)) = log(-expm1(l1 - l)), alpha1(x, y) = min(1, exp(l(y) - l(x))).  l1 = -inf: A = B = 0 and
                neither is added.  l1 >= l2: alpha1(y2, y1) = 1, rejected.  Accepted iff min(log alpha2, 0) > log U2.
    stuck       a chain not strictly inside the box, or with a non-finite l, makes no proposal: stuck grows.

Why the rule keeps pi (Mira 2001, Tierney & Mira 1999): the second stage's acceptance probability
    alpha2 = min(1, pi(y2) q1(y2, y1) q2(y2, y1, q) (1 - alpha1(y2, y1)) / (pi(q) q1(q, y1) q2(q, y1, y2) (1 - alpha1(q, y1))))
makes the two-stage kernel reversible for pi.  Here q2(x, ., y) = N(y; x, gamma^2 L L^T) does not depend on y1 and is symmetric
in (x, y), so it cancels; q1(y2, y1) / q1(q, y1) = exp(log q); and a y1 outside the box has pi(y1) = 0, alpha1 = 0 from either end.

`mutant`: "no_reject_terms" drops A, B and the l1 >= l2 rejection, "no_logq" drops log q — two wrong rules the target tests must
catch (tests/test_dr_reference.py).
"""
import numpy as np

import smc_reference as smc

SLOT_Z01_2, SLOT_Z2_2 = 5, 6


def pack(L):
    """L (d, d) → its row-major lower triangle (d (d + 1) / 2,), the layout of rsf_dr_run's chol"""
    L = np.atleast_2d(np.asarray(L, np.float64))
    return np.concatenate([L[p, :p + 1] for p in range(L.shape[0])])


def unpack(tri, d):
    L = np.zeros((d, d))
    L[np.tril_indices(d)] = np.asarray(tri, np.float64).reshape(-1)
    return L


def normals2(seed, particles, iteration, d):
    """the second stage's normals: slots 5 and 6 through smc_reference.normals' Box-Muller pair"""
    out = []
    for slot in (SLOT_Z01_2, SLOT_Z2_2)[:1 if d <= 2 else 2]:
        w = smc.words(seed, particles, iteration, slot)
        r = np.sqrt(-2.0 * np.log(smc.u53(w[:, 0], w[:, 1])))
        a = 2.0 * np.pi * smc.u53(w[:, 2], w[:, 3])
        out += [r * np.cos(a), r * np.sin(a)]
    return np.stack(out[:d], axis=1)


def uniforms(seed, particles, iteration):
    """→ (U1, U2) of the accept slot's four words"""
    w = smc.words(seed, particles, iteration, smc.SLOT_U)
    return smc.u53(w[:, 0], w[:, 1]), smc.u53(w[:, 2], w[:, 3])


def stage2_point(q, L, z2, gamma):
    """y2 = q + gamma (L z2) in float64, in the stated order"""
    q, L, z2 = np.asarray(q, np.float64), np.asarray(L, np.float64), np.asarray(z2, np.float64)
    y = np.empty_like(q)
    for p in range(q.shape[1]):
        v = L[p, 0] * z2[:, 0]
        for r in range(1, p + 1):
            v = v + L[p, r] * z2[:, r]
        y[:, p] = q[:, p] + gamma * v
    return y


def log_q(z1, z2, gamma):
    sw, s1 = np.zeros(z1.shape[0]), np.zeros(z1.shape[0])
    for p in range(z1.shape[1]):
        w = z1[:, p] - gamma * z2[:, p]
        sw = sw + w * w
        s1 = s1 + z1[:, p] * z1[:, p]
    return -0.5 * (sw - s1)


def log_alpha2(l, l1, l2, logq, mutant=None):
    """→ (log alpha2, rejected outright: l2 not finite, or l1 >= l2)"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        la = (l2 - l) if mutant == "no_logq" else (l2 - l) + logq
        fin1 = ~np.isneginf(l1)
        out = ~np.isfinite(l2)
        if mutant != "no_reject_terms":
            A = np.log(-np.expm1(np.where(fin1, l1 - l2, -1.0)))
            B = np.log(-np.expm1(np.where(fin1, l1 - l, -1.0)))
            la = np.where(fin1, (la + A) - B, la)
            out = out | (fin1 & (l1 >= l2))
    return la, out


def accept_test(la, log_u):
    """csrc/rsf_kernel_common.h: min(log alpha, 0) > log u, a NaN rejected"""
    with np.errstate(invalid="ignore"):
        return np.where(la > 0.0, 0.0, la) > log_u


def new_counters(n):
    return {k: np.zeros(n, np.int32) for k in ("accepted1", "accepted2", "outbox1", "outbox2", "stuck")}


def _logt(ssq_fn, pts, where, shape, dtype, fix=None):
    """l at the rows of pts where `where`, -inf elsewhere; ssq → the raw sums of squares (1 elsewhere), after fix(ssq (n,)) if given"""
    l, ssq = np.full(pts.shape[0], -np.inf), np.ones(pts.shape[0])
    if where.any():
        ssq[where] = np.asarray(ssq_fn(pts[where]), np.float64).reshape(-1)
    if fix is not None:
        ssq = fix(ssq)
    if where.any():
        l[where] = smc.log_target(ssq[where], shape, dtype)
    return l, ssq


def step(q, l, ssq_fn, lo, hi, L, gamma, stages, shape, seed, offset, iteration, counters, dtype=np.float64, mutant=None, variates=None,
         fix=None):
    """One iteration IN PLACE in q (n, d), l (n,) and the counters → dict of what happened, per chain: stuck, y1, in1, l1, ssq1, acc1,
    margin1 (log alpha1 - log U1), pending, y2, in2, l2, ssq2, acc2, margin2, log_q.  variates: (z1, U1, z2, U2) in place of the
    Philox stream's (for the tests of the rule on other variates).  fix(stage, ssq (n,)) → ssq: sums of squares a test plants at chosen rows."""
    n, d = q.shape
    L = np.asarray(L, np.float64).reshape(d, d)
    ids = (offset + np.arange(n)).astype(np.uint64)
    if variates is None:
        z1, z2 = smc.normals(seed, ids, iteration, d), normals2(seed, ids, iteration, d)
        u1, u2 = uniforms(seed, ids, iteration)
    else:
        z1, u1, z2, u2 = variates
    log_u1, log_u2 = np.log(u1), np.log(u2)
    ok = smc.inbox(q, lo, hi) & np.isfinite(l)
    y1 = smc.propose(q, L, z1, dtype)
    y1[~ok] = q[~ok]
    in1 = ok & smc.inbox(y1, lo, hi)
    l1, ssq1 = _logt(ssq_fn, y1, in1, shape, dtype, fix and (lambda v: fix(1, v)))
    with np.errstate(invalid="ignore"):
        la1 = np.where(in1, l1 - l, -np.inf)
    acc1 = in1 & accept_test(la1, log_u1)
    pend = ok & ~acc1 & (stages == 2)
    y2 = stage2_point(q, L, z2, gamma)
    y2[~pend] = q[~pend]
    in2 = pend & smc.inbox(y2, lo, hi)
    l2, ssq2 = _logt(ssq_fn, y2, in2, shape, dtype, fix and (lambda v: fix(2, v)))
    lq = log_q(z1, z2, gamma)
    la2, out2 = log_alpha2(l, l1, l2, lq, mutant)
    acc2 = in2 & ~out2 & accept_test(la2, log_u2)
    counters["stuck"][~ok] += 1
    counters["outbox1"][ok & ~in1] += 1
    counters["accepted1"][acc1] += 1
    counters["outbox2"][pend & ~in2] += 1
    counters["accepted2"][acc2] += 1
    q[acc1], l[acc1] = y1[acc1], l1[acc1]
    q[acc2], l[acc2] = y2[acc2], l2[acc2]
    with np.errstate(invalid="ignore"):
        m1, m2 = np.where(la1 > 0, 0.0, la1) - log_u1, np.where(la2 > 0, 0.0, la2) - log_u2
    return dict(stuck=~ok, y1=y1, in1=in1, l1=l1, ssq1=ssq1, acc1=acc1, margin1=m1, pending=pend, y2=y2, in2=in2, l2=l2, ssq2=ssq2, acc2=acc2,
                margin2=m2, rejected2=out2, log_q=lq)


def start_l(q, ssq_fn, shape, dtype=np.float64):
    return smc.log_target(np.asarray(ssq_fn(np.asarray(q, np.float64)), np.float64).reshape(-1), shape, dtype)


def run(ssq_fn, q0, lo, hi, L, n_iter, shape, gamma=0.2, stages=2, seed=0, offset=0, iter0=1, checkpoints=(), dtype=np.float64, mutant=None, rng=None):
    """n_iter iterations from q0 (n, d) → dict(q, l, the five counters, at={iteration: (q, l) copies}).  rng: NumPy variates in
    place of the Philox stream's."""
    q = np.array(q0, dtype=np.float64).reshape(len(q0), -1)
    n, d = q.shape
    l = start_l(q, ssq_fn, shape, dtype)
    cnt, at = new_counters(n), {}
    for it in range(iter0, iter0 + n_iter):
        var = None if rng is None else (rng.standard_normal((n, d)), 1.0 - rng.uniform(size=n), rng.standard_normal((n, d)), 1.0 - rng.uniform(size=n))
        step(q, l, ssq_fn, lo, hi, L, gamma, stages, shape, seed, offset, it, cnt, dtype, mutant, var)
        if it in checkpoints:
            at[it] = (q.copy(), l.copy())
    return dict(q=q, l=l, at=at, **cnt)


def n_solves(n_iter, counters, stages=2):
    """forward solves of a run: stage 1 solves every proposal inside the box, stage 2 (stages = 2) every proposal inside the box of a
    chain whose first was not accepted"""
    c = {k: np.asarray(counters[k], np.int64) for k in ("accepted1", "outbox1", "outbox2", "stuck")}
    first = int((n_iter - c["stuck"] - c["outbox1"]).sum())
    return first + (int((n_iter - c["stuck"] - c["accepted1"] - c["outbox2"]).sum()) if stages == 2 else 0)


def adapted_factor(states, lo, hi, old):
    """The burn-in adaptation of one group: states (m, d) pooled over chains and iterations → chol((2.38^2 / d) cov(states) +
    diag((1e-6 (hi - lo))^2)) (np.cov, ddof 1), or `old` where that matrix has no Cholesky factor"""
    x = np.asarray(states, np.float64)
    d = x.shape[1]
    lo, hi = np.atleast_1d(np.asarray(lo, np.float64)), np.atleast_1d(np.asarray(hi, np.float64))
    cov = np.atleast_2d(np.cov(x.T))
    try:
        return np.linalg.cholesky((2.38 ** 2 / d) * cov + np.diag((1e-6 * (hi - lo)) ** 2))
    except np.linalg.LinAlgError:
        return np.asarray(old, np.float64)
