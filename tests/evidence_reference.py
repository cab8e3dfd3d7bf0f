"""
Specification of include/rsf_evidence.h in NumPy with np.longdouble arithmetic (TEST INFRASTRUCTURE ONLY, no GPU): the Gaussian
proposal in working coordinates and its density, the log target minus log proposal from a sum of squares, one bridge iteration's
additive partials, the finish, the iteration — and the independent truth, a tensor Gauss-Legendre quadrature of SSq^-shape over
the box.  Every function takes `dtype`: np.longdouble is the specification, np.float64 the restatement whose distance from it
sizes the GPU tolerances (tests/evidence_cases.py).

The sampler's target with n0 = 0 is pi(q) ~ 1_box(q) SSq(q)^-shape (tests/posterior_reference.py), so with N = 2 shape observations
    p(y | M) = Gamma(shape) pi^-shape / vol(box) * I,      I = integral over the box of SSq^-shape.
Bridge sampling (Meng & Wong 1996; Gronau et al. 2017): with l = log target - log proposal in the working coordinates
phi_p = q_p or log q_p (the log-Jacobian sum log q_p over the logged parameters belongs to the target),
    r <- [1/N2 sum_j e^(l2_j - l*) / (s1 e^(l2_j - l*) + s2 r)] / [1/N1 sum_i 1 / (s1 e^(l1_i - l*) + s2 r)],   log I = log r + l*.
"""
import math

import numpy as np

LD = np.longdouble
MAX_PARAMS = 3
PARTIALS = ("n1", "n2", "n2_finite", "sum_num", "sum_den", "sum_f1", "sum_f1_sq", "sum_f2", "sum_f2_sq")
OUT = ("r_next", "log_integral", "log_evidence", "re")
MAX_ITER = 1000
RTOL = 1e-10


def to_phi(theta, tr, dtype=LD):
    """natural coordinates (n, d) → working coordinates: log of the flagged columns (NaN where not positive)"""
    th = np.asarray(theta, dtype=dtype).reshape(-1, len(tr))
    phi = th.copy()
    for p in np.flatnonzero(np.asarray(tr)):
        with np.errstate(invalid="ignore", divide="ignore"):
            phi[:, p] = np.where(th[:, p] > 0, np.log(np.where(th[:, p] > 0, th[:, p], 1)), np.nan)
    return phi


def logg_phi(phi, mean, chol, dtype=LD):
    """log N(phi; mean, L L^T): y = L^-1 (phi - mean) by forward substitution, -1/2 |y|^2 - sum log L_pp - d/2 log 2 pi"""
    phi = np.asarray(phi, dtype=dtype)
    m, L = np.asarray(mean, dtype=dtype).reshape(-1), np.asarray(chol, dtype=dtype)
    d = m.size
    L = L.reshape(d, d)
    y = np.zeros_like(phi)
    ss = np.zeros(phi.shape[0], dtype=dtype)
    for p in range(d):
        s = phi[:, p] - m[p]
        for r in range(p):
            s = s - L[p, r] * y[:, r]
        y[:, p] = s / L[p, p]
        ss = ss + y[:, p] * y[:, p]
    logc = -sum(np.log(L[p, p]) for p in range(d)) - dtype(d) / 2 * np.log(2 * dtype(np.pi) if dtype is np.float64 else 2 * np.arccos(dtype(-1)))
    return logc - ss / 2


def logg(theta, mean, chol, tr, dtype=LD):
    return logg_phi(to_phi(theta, tr, dtype), mean, chol, dtype)


def propose(z, mean, chol, tr, lo, hi, dtype=LD):
    """normals z (n, d) → (theta (n, d) natural, logg (n,), inbox (n,) bool): phi = mean + L z, theta = phi or exp(phi)"""
    z = np.asarray(z, dtype=dtype)
    d = z.shape[1]
    m, L = np.asarray(mean, dtype=dtype).reshape(-1), np.asarray(chol, dtype=dtype).reshape(d, d)
    phi = np.empty_like(z)
    for p in range(d):
        s = np.full(z.shape[0], m[p], dtype=dtype)
        for r in range(p + 1):
            s = s + L[p, r] * z[:, r]
        phi[:, p] = s
    theta = phi.copy()
    for p in np.flatnonzero(np.asarray(tr)):
        theta[:, p] = np.exp(phi[:, p])
    return theta, logg_phi(phi, mean, chol, dtype), inbox(theta, lo, hi)


def inbox(theta, lo, hi):
    th = np.asarray(theta).reshape(-1, np.size(lo))
    return np.all((th > np.asarray(lo)) & (th < np.asarray(hi)), axis=1)  # the sampler's strict box


def logtarget(theta, ssq, shape, lo, hi, tr, logg_, dtype=LD):
    """l = -shape log SSq + sum over the logged p of log theta_p - logg; -inf outside the strict box or where SSq is not finite
    and positive"""
    th = np.asarray(theta, dtype=dtype).reshape(-1, len(tr))
    ssq = np.asarray(ssq, dtype=dtype).reshape(-1)
    ok = inbox(np.asarray(theta, dtype=np.float64).reshape(-1, len(tr)), lo, hi) & np.isfinite(ssq) & (ssq > 0)
    jac = np.zeros(th.shape[0], dtype=dtype)
    for p in np.flatnonzero(np.asarray(tr)):
        jac = jac + np.log(np.where(ok, th[:, p], 1))
    with np.errstate(invalid="ignore"):
        l = -dtype(shape) * np.log(np.where(ok, ssq, 1)) + jac - np.asarray(logg_, dtype=dtype)
    return np.where(ok, l, -np.inf)


def partials(l1, l2, lstar, r, s1=None, s2=None, dtype=LD):
    """the additive partials of one iteration at (r, lstar), PARTIALS order.  Each term through exp(-|l - lstar|): a spread of
    1e4 gives 0 or the bound 1 / s1, 1 / (s2 r), never inf / inf."""
    l1, l2 = np.asarray(l1, dtype=dtype).reshape(-1), np.asarray(l2, dtype=dtype).reshape(-1)
    n1, n2 = l1.size, l2.size
    if s1 is None:
        s1, s2 = dtype(n1) / (n1 + n2), dtype(n2) / (n1 + n2)
    s1, s2r, r = dtype(s1), dtype(s2) * dtype(r), dtype(r)
    if not np.isfinite(l1).all() or np.isnan(l2).any() or np.isposinf(l2).any():
        raise ValueError("l1 must be finite; l2 finite or -inf")
    fin = np.isfinite(l2)
    a = np.where(fin, l2, 0) - dtype(lstar)
    e = np.exp(-np.abs(a))
    t2 = np.where(fin, np.where(a > 0, 1 / (s1 + s2r * e), e / (s1 * e + s2r)), 0)
    b = l1 - dtype(lstar)
    e = np.exp(-np.abs(b))
    t1 = np.where(b > 0, e / (s1 + s2r * e), 1 / (s1 * e + s2r))
    return np.array([n1, n2, fin.sum(), t2.sum(), t1.sum(), t2.sum(), (t2 * t2).sum(), r * t1.sum(), r * r * (t1 * t1).sum()], dtype=dtype)


def finish(part, r, lstar, ess_factor=1.0, shape=None, lo=None, hi=None, dtype=LD):
    """summed partials taken at (r, lstar) → dict of OUT (log_evidence None without shape, lo, hi)"""
    part = np.asarray(part, dtype=dtype)
    n1, n2, n2f = part[0], part[1], part[2]
    rn = (part[3] / n2) / (part[4] / n1) if n2f > 0 else dtype(0)
    logi = np.log(rn) + dtype(lstar) if rn > 0 else dtype(-np.inf)
    logz = None
    if shape is not None:
        logz = logi - sum(np.log(dtype(h) - dtype(l)) for l, h in zip(np.ravel(lo), np.ravel(hi))) + dtype(math.lgamma(shape)) \
            - dtype(shape) * np.log(np.arccos(dtype(-1)))
    if n1 < 2 or n2 < 2 or not n2f > 0:
        re = dtype(np.inf)
    else:
        e1, e2 = part[5] / n2, part[7] / n1
        v1, v2 = (part[6] - part[5] * e1) / (n2 - 1), (part[8] - part[7] * e2) / (n1 - 1)
        re = np.sqrt(max(v1, 0) / (n2 * e1 * e1) + max(v2, 0) / (dtype(ess_factor) * n1 * e2 * e2))
    return {"r_next": rn, "log_integral": logi, "log_evidence": logz, "re": re}


def bridge(l1, l2, ess_factor=1.0, lstar=None, shape=None, lo=None, hi=None, dtype=LD):
    """the iteration from r = 1 → dict(log_integral, log_evidence, re, iterations, n2_in_box, converged, r, lstar)"""
    if lstar is None:
        lstar = float(np.median(np.asarray(l1, dtype=np.float64)))
    r, it, conv = dtype(1), 0, False
    while it < MAX_ITER:
        part = partials(l1, l2, lstar, r, dtype=dtype)
        res = finish(part, r, lstar, ess_factor, shape, lo, hi, dtype)
        it += 1
        rn = res["r_next"]
        if not rn > 0:
            r = dtype(0)
            break
        conv = bool(abs(rn - r) < dtype(RTOL) * rn)
        r = rn
        if conv:
            break
    return {"log_integral": res["log_integral"], "log_evidence": res["log_evidence"], "re": res["re"], "iterations": it,
            "n2_in_box": int(part[2]), "converged": conv, "r": r, "lstar": lstar}


def evidence(q, ssq_fn, lo, hi, shape, z, tr=None, fit_fraction=0.5, ess_factor=1.0, dtype=LD):
    """the whole estimator on a flat pool q (n, d) with the normals z (n2, d) supplied: the first part fits the proposal (mean
    and np.cov of the working coordinates), the second enters the estimator.  ssq_fn(q (m, d)) → (m,), called inside the box only."""
    q = np.asarray(q, dtype=np.float64).reshape(len(q), -1)
    d = q.shape[1]
    tr = np.zeros(d, dtype=int) if tr is None else np.asarray(tr)
    k = int(round(fit_fraction * q.shape[0]))
    phi = np.asarray(to_phi(q[:k], tr, np.float64))
    mean, chol = phi.mean(0), np.linalg.cholesky(np.atleast_2d(np.cov(phi.T)))
    theta, g2, inb = propose(z, mean, chol, tr, lo, hi, dtype)
    th64 = np.asarray(theta, dtype=np.float64)
    ssq2 = np.full(th64.shape[0], np.nan)
    ssq2[inb] = ssq_fn(th64[inb])
    l2 = logtarget(th64, ssq2, shape, lo, hi, tr, g2, dtype)
    l1 = logtarget(q[k:], ssq_fn(q[k:]), shape, lo, hi, tr, logg(q[k:], mean, chol, tr, dtype), dtype)
    res = bridge(l1, l2, ess_factor, None, shape, lo, hi, dtype)
    res.update(l1=l1, l2=l2, mean=mean, chol=chol)
    return res


def quadrature_log_integral(ssq_fn, lo, hi, shape, nodes):
    """log of the tensor Gauss-Legendre quadrature of SSq^-shape over the box with `nodes` nodes per axis; ssq_fn(q (m, d))"""
    lo, hi = np.atleast_1d(np.asarray(lo, np.float64)), np.atleast_1d(np.asarray(hi, np.float64))
    d = lo.size
    t, w = np.polynomial.legendre.leggauss(nodes)
    axes = [lo[p] + (hi[p] - lo[p]) * (t + 1) / 2 for p in range(d)]
    ws = [w * (hi[p] - lo[p]) / 2 for p in range(d)]
    total, lmax = LD(0), None
    first = axes[0]
    rest = np.stack(np.meshgrid(*axes[1:], indexing="ij"), axis=-1).reshape(-1, d - 1) if d > 1 else np.zeros((1, 0))
    wrest = np.ones(1) if d == 1 else np.prod(np.stack(np.meshgrid(*ws[1:], indexing="ij"), axis=-1).reshape(-1, d - 1), axis=1)
    logs = []
    for i, x0 in enumerate(first):  # one slab of the first axis at a time
        q = np.column_stack([np.full(rest.shape[0], x0), rest])
        logs.append(-shape * np.log(ssq_fn(q)))
    lmax = max(l.max() for l in logs)
    for i, l in enumerate(logs):
        total += LD(ws[0][i]) * np.sum(np.asarray(wrest, dtype=LD) * np.exp(np.asarray(l - lmax, dtype=LD)))
    return float(np.log(total) + lmax)
