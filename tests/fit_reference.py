"""
The specification of the multi-start Levenberg-Marquardt fit (include/rsf_fit.h), in NumPy (a test helper; TEST INFRASTRUCTURE ONLY).

A forward solve is a function  solve(points (m, d) float64) -> series (N, m)  (float64 or longdouble): the closed-form models of
the tests, the checker's rsf_forward_batch, or the extended-precision RK4 (tests/rk4_extended.py).  The normal equations at the
points q (n, d), by rsf_mcmc_init's forward differences (parameter p times (1 + fd), the perturbed value in the denominator, every
sample included, k = 0 too):
    r_k = acc_k(q) - data_k      X_pk = (acc_k(q^(p)) - acc_k(q)) / (q^(p)_p fd)
    ssq = sum r_k^2              g_p = sum X_pk r_k  (X^T r)        H_pr = sum X_pk X_rk  (X^T X)
The differences r and X are formed in the solve's own precision; the sums are taken in np.longdouble and rounded once.

State per start: q[d], ssq, g[d], H[d][d], lam, status, iters.  One iteration of a RUNNING start (`iterate`):
    1. A = H + lam diag(H).  A pivot of its Cholesky factor that is not positive and finite: no trial point; the iteration is a
       rejection without a solve (6).
    2. delta = -A^-1 g, q' = q + delta; every coordinate clamped into the strict box: a value <= lo becomes nextafter(lo, hi), a
       value >= hi becomes nextafter(hi, lo).
    3. the normal equations at q': ssq', g', H'.
    4. accepted iff ssq' is finite and ssq' < ssq (the sampler's rule: a non-finite sum is a rejection).
    5. accepted: (q, ssq, g, H) <- (q', ssq', g', H'), lam <- max(0.1 lam, 1e-12); CONVERGED if (ssq - ssq') / ssq < ftol.
    6. rejected: lam <- 10 lam; STALLED once lam > 1e12.
    7. iters += 1.
lam starts at 1e-3; a start whose first ssq is not finite is FAILED and never moves.  (A failed factor takes the rejection's branch
so that a start whose X^T X never factors ends STALLED after sixteen iterations instead of running forever.)

The factor, the two triangular solves and the clamp are float64, written out in the order csrc/rsf_kernels_fit.h takes them.
"""
import math

import numpy as np

LD = np.longdouble

RUNNING, CONVERGED, STALLED, FAILED = 0, 1, 2, 3
LAM0, LAM_MIN, LAM_MAX, LAM_DOWN, LAM_UP = 1e-3, 1e-12, 1e12, 0.1, 10.0
FTOL = 1e-9  # above the noise of SSq(q) near its minimum, 1e-12 .. 1.3e-11 relative on the real model


def perturbed(q, fd):
    """-> (d + 1, n, d) float64: row 0 the points, row p + 1 parameter p times (1 + fd), rounded as the kernel rounds it"""
    q = np.asarray(q, dtype=np.float64)
    n, d = q.shape
    pq = np.repeat(q[None], d + 1, axis=0)
    for p in range(d):
        pq[p + 1, :, p] = pq[p + 1, :, p] * (1 + fd)
    return pq


def normal(solve, q, data, fd, out=np.float64):
    """-> (ssq (n,), g (n, d), H (n, d, d)) of dtype `out`.  data: one series (N,), or one per group (G, N), the points split
    evenly over the groups in order."""
    q = np.asarray(q, dtype=np.float64)
    n, d = q.shape
    data = np.atleast_2d(np.asarray(data, dtype=np.float64))
    G, N = data.shape
    assert n % G == 0, (n, G)
    pq = perturbed(q, fd)
    acc = np.asarray(solve(pq.reshape(-1, d)))
    wide = LD if acc.dtype == LD else np.float64
    acc = acc.reshape(N, d + 1, n)
    obs = data[np.arange(n) // (n // G)].T.astype(wide)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (acc[:, 0] - obs).astype(LD)
        X = np.stack([((acc[:, p + 1] - acc[:, 0]) / (pq[p + 1, :, p].astype(wide) * wide(fd))).astype(LD) for p in range(d)])
        ssq = (r * r).sum(axis=0)
        g = np.einsum("pkc,kc->cp", X, r)
        H = np.einsum("pkc,rkc->cpr", X, X)
    return tuple(np.ascontiguousarray(x, dtype=out) for x in (ssq, g, H))


def trial(q, g, H, lam, lo, hi):
    """steps 1-2 for one start -> (ok, q' (d,)); float64 throughout"""
    d = len(q)
    L = np.zeros((d, d))
    for p in range(d):
        for r in range(p + 1):
            s = H[p][r]
            if r == p:
                s = s + lam * s
            for k in range(r):
                s = s - L[p][k] * L[r][k]
            if r == p:
                if not (s > 0.0 and s < math.inf):
                    return False, np.array(q, dtype=np.float64)
                L[p][p] = math.sqrt(s)
            else:
                L[p][r] = s / L[r][r]
    y = np.zeros(d)
    for p in range(d):
        s = -g[p]
        for k in range(p):
            s = s - L[p][k] * y[k]
        y[p] = s / L[p][p]
    for p in range(d - 1, -1, -1):
        s = y[p]
        for k in range(p + 1, d):
            s = s - L[k][p] * y[k]
        y[p] = s / L[p][p]
    qt = np.empty(d)
    for p in range(d):
        v = q[p] + y[p]
        if v <= lo[p]:
            v = np.nextafter(lo[p], hi[p])
        elif v >= hi[p]:
            v = np.nextafter(hi[p], lo[p])
        qt[p] = v
    return True, qt


def new_state(q0, ssq, g, H):
    """the state the caller builds from the first normal equations"""
    q0 = np.array(q0, dtype=np.float64)
    n = q0.shape[0]
    return {"q": q0, "ssq": np.array(ssq, dtype=np.float64), "g": np.array(g, dtype=np.float64), "H": np.array(H, dtype=np.float64),
            "lam": np.full(n, LAM0), "status": np.where(np.isfinite(ssq), RUNNING, FAILED).astype(np.int32), "iters": np.zeros(n, dtype=np.int32)}


def trials(st, lo, hi):
    """steps 1-2 for every start -> (q_trial (n, d), ok (n,) bool): a start that is not RUNNING has its q and ok False"""
    qt, ok = st["q"].copy(), np.zeros(st["q"].shape[0], dtype=bool)
    for i in np.flatnonzero(st["status"] == RUNNING):
        ok[i], qt[i] = trial(st["q"][i], st["g"][i], st["H"][i], st["lam"][i], lo, hi)
    return qt, ok


def decide(st, qt, ok, ssq_n, g_n, H_n, ftol=FTOL):
    """steps 4-7, in place -> accepted (n,) bool"""
    acc = np.zeros(ok.shape, dtype=bool)
    for i in np.flatnonzero(st["status"] == RUNNING):
        a = bool(ok[i]) and bool(np.isfinite(ssq_n[i])) and bool(ssq_n[i] < st["ssq"][i])
        acc[i] = a
        st["iters"][i] += 1
        if a:
            if (st["ssq"][i] - ssq_n[i]) / st["ssq"][i] < ftol:
                st["status"][i] = CONVERGED
            st["q"][i], st["ssq"][i], st["g"][i], st["H"][i] = qt[i], ssq_n[i], g_n[i], H_n[i]
            st["lam"][i] = max(LAM_DOWN * st["lam"][i], LAM_MIN)
        else:
            st["lam"][i] = LAM_UP * st["lam"][i]
            if st["lam"][i] > LAM_MAX:
                st["status"][i] = STALLED
    return acc


def iterate(normal_fn, st, lo, hi, ftol=FTOL):
    """one iteration of every RUNNING start; normal_fn(points (n, d)) -> (ssq, g, H) -> (ok, accepted, ssq' (n,))"""
    qt, ok = trials(st, lo, hi)
    ssq_n, g_n, H_n = normal_fn(qt)
    acc = decide(st, qt, ok, ssq_n, g_n, H_n, ftol)
    return ok, acc, ssq_n


def fit(normal_fn, q0, lo, hi, ftol=FTOL, max_iter=100, history=None):
    """the whole fit -> state; history (a list): one (ok, accepted, ssq', ssq before) per iteration"""
    q0 = np.asarray(q0, dtype=np.float64).reshape(len(q0), -1)
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1)
    st = new_state(q0, *normal_fn(q0))
    for _ in range(int(max_iter)):
        if not (st["status"] == RUNNING).any():
            break
        before = st["ssq"].copy()
        ok, acc, ssq_n = iterate(normal_fn, st, lo, hi, ftol)
        if history is not None:
            history.append((ok, acc, ssq_n, before))
    return st


def laplace(d, n_obs, shape, ssq, jtj, lo, hi):
    """rsf_fit_laplace in longdouble -> (cov (d, d), log_integral, log_evidence)"""
    from init_extended import inverse3

    H = np.asarray(jtj, dtype=LD).reshape(d, d)
    ssq, shape = LD(ssq), LD(shape)
    if d == 1:
        inv, det = 1 / H, H[0, 0]
    else:
        P = np.eye(3, dtype=LD)
        P[:d, :d] = H
        inv = inverse3(P)[:d, :d]
        det = H[0, 0] * H[1, 1] - H[0, 1] * H[1, 0] if d == 2 else (
            H[0, 0] * (H[1, 1] * H[2, 2] - H[1, 2] * H[2, 1]) - H[0, 1] * (H[1, 0] * H[2, 2] - H[1, 2] * H[2, 0])
            + H[0, 2] * (H[1, 0] * H[2, 1] - H[1, 1] * H[2, 0]))
    cov = ssq / LD(n_obs - d) * inv
    two_pi = 2 * LD(np.pi) if np.finfo(LD).eps >= 2e-16 else LD("6.283185307179586476925286766559005768")
    logi = -shape * np.log(ssq) + LD(d) / 2 * np.log(two_pi) - (np.log(det) + d * np.log(2 * shape / ssq)) / 2
    logvol = np.log(np.asarray(hi, dtype=LD) - np.asarray(lo, dtype=LD)).sum()
    pi = two_pi / 2
    lgam = LD(math.lgamma(float(shape)))  # float64's lgamma: the library's own, exact to an ulp of a value of order 1e3
    return cov, logi, logi - logvol + lgam - shape * np.log(pi)
