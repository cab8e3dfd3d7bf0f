"""
Specification of the adaptive delayed-rejection run under a state law (a test helper; TEST INFRASTRUCTURE ONLY, no GPU) — what
Engine.law_gn_factor, Engine.law_dr and MCMC.sample_law are checked against, and how the expectation figures quoted in
tests/test_gpu_law_dr.py were made.  Nothing new is specified here: the iteration is tests/dr_reference.py's `step`, the
adaptation its `adapted_factor`, the solve tests/observe_reference.py's `forward`; this file only puts them in Engine.law_dr's
order — launches of iters_per_launch iterations, the factor adapted after each of the first adapt_launches launches from every
state traced so far — and adds the forward-difference Gauss-Newton factor.
"""
import numpy as np

import dr_reference as dr
import observe_reference as O

# the common problem of tests/test_gpu_law_dr.py: truth (Dc, a, b) = (20, 0.011, 0.014) on the step history
TRUTH3 = np.array([20.0, 0.011, 0.014])
LO3, HI3 = np.array([8.0, 0.009, 0.012]), np.array([60.0, 0.013, 0.016])


def ssq_fn(m, vl, law, observable, data):
    """points (k, 1) of Dc or (k, 3) of (Dc, a, b) → SSq (k,) of the float64 specification"""
    def fn(pts):
        pts = np.asarray(pts, np.float64).reshape(len(pts), -1)
        ab = (pts[:, 1], pts[:, 2]) if pts.shape[1] == 3 else (None, None)
        return O.forward(m, pts[:, 0], vl, law, observable, a=ab[0], b=ab[1], data=data)[1]
    return fn


def gn_factor(m, vl, law, observable, q, data, rel_step=1e-4):
    """→ (L, cov, ssq) at the point q (d,): J by forward differences with step rel_step q_p, cov = (SSq / nout) (J^T J)^-1,
    L = chol((2.38^2 / d) cov)"""
    q = np.asarray(q, np.float64).reshape(-1)
    d = q.size
    h = rel_step * q
    pts = np.tile(q, (1 + d, 1))
    pts[1:] += np.diag(h)
    ab = (pts[:, 1], pts[:, 2]) if d == 3 else (None, None)
    series = O.forward(m, pts[:, 0], vl, law, observable, a=ab[0], b=ab[1])[0]
    r = series[:, 0] - data
    ssq = float(r @ r)
    J = (series[:, 1:] - series[:, :1]) / h
    cov = (ssq / data.size) * np.linalg.inv(J.T @ J)
    return np.linalg.cholesky((2.38 ** 2 / d) * cov), cov, ssq


def run(fn, q0, lo, hi, L, n_iter, shape, gamma=0.2, stages=2, seed=0, offset=0, iters_per_launch=16, adapt_launches=0):
    """Engine.law_dr's run on the specification → dict(q, l, the five counters, trace_q (n_iter, n, d), chol)"""
    q = np.array(q0, np.float64).reshape(len(q0), -1)
    lo, hi = np.atleast_1d(np.asarray(lo, np.float64)), np.atleast_1d(np.asarray(hi, np.float64))
    L = np.array(L, np.float64).reshape(q.shape[1], q.shape[1])
    l = dr.start_l(q, fn, shape)
    cnt, trace, done, launch = dr.new_counters(q.shape[0]), [], 0, 0
    while done < n_iter:
        k = min(iters_per_launch, n_iter - done)
        for it in range(done + 1, done + k + 1):
            dr.step(q, l, fn, lo, hi, L, gamma, stages, shape, seed, offset, it, cnt)
            trace.append(q.copy())
        if launch < adapt_launches:
            L = dr.adapted_factor(np.concatenate(trace), lo, hi, L)
        done += k
        launch += 1
    return dict(q=q, l=l, trace_q=np.stack(trace), chol=L, **cnt)
