"""
The exact posterior of a state-law model on a tensor grid in the coordinates of a fit, in NumPy: the specification of
include/rsf_law_grid.h (a test helper; TEST INFRASTRUCTURE ONLY, no GPU).  The z-grid sums are tests/grid_reference.py's, the solve
tests/observe_reference.py's `forward`, the fit tests/law_fit_reference.py's; what is specified here is the map — phi = m + L z,
q_perm[p] = phi_p or exp(phi_p) — the target on it, the moments in natural coordinates and the evidence.  Every sum that a test
compares is taken in np.longdouble.

What tests/test_law_grid_reference.py (CPU) and tests/test_gpu_law_grid.py share is here too: the end-to-end problems, solved ONCE
per process.
"""
import functools
import math

import numpy as np

import fit_reference as F
import grid_reference as G
import law_fit_reference as LF
import observe_cases as OC
import observe_reference as O

LD = np.longdouble
FIELDS = 12  # W times 1, dq_0..2, dq_0 dq_0, dq_0 dq_1, dq_0 dq_2, dq_1 dq_1, dq_1 dq_2, dq_2 dq_2, SSq, SSq^2
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
E2E_N, E2E_WINDOW = (33, 17, 17), 6.0  # the end-to-end grid: 9 537 solves


def axes(n, window_sd):
    """Simpson axes of odd n[p] nodes on [-window_sd, window_sd] -> (z, w) lists"""
    zw = [G.simpson(-float(window_sd), float(window_sd), int(k)) for k in n]
    return [a[0] for a in zw], [a[1] for a in zw]


def factor(point, cov, log_coords=None, first=0):
    """The map of a fit: its point q (d,) and covariance (d, d) in natural coordinates, the parameters named in log_coords (indices)
    logged, parameter `first` on axis 0 and the others behind it in their order -> (m (d,), L (d, d) lower, tr (d,), perm (d,)).
    The covariance of phi is J cov J with J = diag(1 / q_p) over the logged parameters (first order)."""
    q = np.asarray(point, dtype=np.float64).reshape(-1)
    d = q.size
    logged = np.zeros(d, dtype=bool)
    logged[list(log_coords or ())] = True
    perm = np.array([first] + [p for p in range(d) if p != first], dtype=np.int32)
    J = np.where(logged, 1.0 / q, 1.0)
    C = (np.asarray(cov, dtype=np.float64).reshape(d, d) * J[:, None] * J[None, :])[np.ix_(perm, perm)]
    return np.where(logged, np.log(q), q)[perm], np.linalg.cholesky(C), logged[perm].astype(np.int32), perm


def nodes(z, m, L, tr, perm, dtype=np.float64):
    """The nodes of the grid in flat-index order -> (q (N, d) in the order (Dc, a, b), jac (N,), phi (N, d)).  np.longdouble:
    phi = m + L z and q = exp(phi) from the float64 inputs widened exactly.  float64: the library's formation — phi is the sum
    rounded ONCE (the library carries it as an unevaluated sum; here it is long double's, rounded), err its rounding error, and
    q = phi, or E + E err with E = exp(phi), where the library has one fused multiply-add."""
    d = len(z)
    Z = np.stack([np.ravel(a, order="F") for a in np.meshgrid(*[np.asarray(a, dtype=np.float64) for a in z], indexing="ij")], axis=1).astype(LD)
    m, L = np.asarray(m, dtype=np.float64).astype(LD), np.asarray(L, dtype=np.float64).reshape(d, d).astype(LD)
    q, phi, jac = np.zeros((Z.shape[0], d), dtype), np.zeros((Z.shape[0], d), dtype), np.zeros(Z.shape[0], dtype)
    for p in range(d):
        wide = m[p] + np.zeros(Z.shape[0], LD)
        for r in range(p + 1):
            wide = wide + L[p, r] * Z[:, r]
        phi[:, p] = wide.astype(dtype)
        if tr[p]:
            e = np.exp(phi[:, p])
            q[:, int(perm[p])] = e + e * (wide - phi[:, p].astype(LD)).astype(dtype) if dtype == np.float64 else e
            jac = jac + phi[:, p]
        else:
            q[:, int(perm[p])] = phi[:, p]
    return q, jac, phi


def in_box(q, lo, hi):
    """inside the CLOSED box"""
    return ((q >= np.asarray(lo)) & (q <= np.asarray(hi))).all(axis=1)


def log_target(ssq, jac, inb, shape, logg=0.0, dtype=np.float64):
    """l = -shape log SSq + jac - logg; -inf outside the box and where SSq is not finite or not > 0"""
    ssq = np.asarray(ssq, dtype=dtype)
    ok = inb & np.isfinite(ssq) & (ssq > 0)
    with np.errstate(all="ignore"):
        return np.where(ok, -dtype(shape) * np.log(np.where(ok, ssq, 1)) + jac - logg, -np.inf)


def solve(m, vl, law, observable, data, q, inb, dtype=np.float64):
    """SSq (N,) of tests/observe_reference.forward at the points q (N, 1) or (N, 3) inside the box, NaN elsewhere"""
    q = np.asarray(q, dtype=np.float64)
    ssq = np.full(q.shape[0], np.nan, dtype=dtype)
    if inb.any():
        ab = (q[inb, 1], q[inb, 2]) if q.shape[1] == 3 else (None, None)
        ssq[inb] = O.forward(m, q[inb, 0], vl, law, observable, a=ab[0], b=ab[1], data=data, dtype=dtype)[1]
    return ssq


def weights(w):
    """((w0 w1) w2) of every node in flat-index order, in long double"""
    _, w = G.pad([np.zeros(a.size) for a in w], w)
    W = w[0].astype(LD)[None, None, :] * w[1].astype(LD)[None, :, None] * w[2].astype(LD)[:, None, None]
    return W.reshape(-1)


def z_sums(z, w, l):
    """The z-grid sums in long double -> dict(lmax, Z, log_integral, n_neginf, mass (per axis the node masses, sum 1), edge_mass
    (the largest share of any axis' marginal mass on that axis' two end nodes) and edge_axis)"""
    n = [a.size for a in z] + [1] * (3 - len(z))
    l = np.asarray(l, dtype=np.float64)
    fin = np.isfinite(l)
    out = {"n_neginf": int((l == -np.inf).sum())}
    if not fin.any():
        out.update(lmax=-np.inf, Z=LD(0), log_integral=-np.inf, mass=None, edge_mass=np.nan, edge_axis=-1)
        return out
    lmax = l[fin].max()
    e = np.where(fin, np.exp(np.where(fin, l.astype(LD) - LD(lmax), 0)), 0).astype(LD)
    We = (weights(w) * e).reshape(n[2], n[1], n[0])
    Z = We.sum()
    mass = [We.sum(axis=(0, 1)) / Z, We.sum(axis=(0, 2)) / Z, We.sum(axis=(1, 2)) / Z][:len(z)]
    edge = [float(a[0] + a[-1]) for a in mass]
    out.update(lmax=float(lmax), Z=Z, log_integral=LD(lmax) + np.log(Z), mass=mass, edge_mass=max(edge), edge_axis=int(np.argmax(edge)))
    return out


def moments(w, l, ssq, q, lmax, center):
    """rsf_law_grid_moments' totals in long double: the sums over every node of W e times {1, dq_p, dq_p dq_r, SSq, SSq^2}, dq = q -
    center (entries a d = 1 grid lacks are 0) -> (FIELDS,)"""
    l = np.asarray(l, dtype=np.float64)
    fin = np.isfinite(l)
    e = np.where(fin, np.exp(np.where(fin, l.astype(LD) - LD(lmax), 0)), 0).astype(LD)
    W = weights(w) * e
    dq = np.zeros((l.size, 3), LD)
    q = np.asarray(q, dtype=np.float64).reshape(l.size, -1)
    dq[:, :q.shape[1]] = q.astype(LD) - np.asarray(center, dtype=np.float64).astype(LD)[None, :q.shape[1]]
    sq = np.where(fin, np.asarray(ssq, dtype=np.float64), 0.0).astype(LD)
    return np.array([W.sum()] + [(W * dq[:, p]).sum() for p in range(3)] + [(W * dq[:, p] * dq[:, r]).sum() for p, r in PAIRS]
                    + [(W * sq).sum(), (W * sq * sq).sum()], dtype=LD)


def summary(total, center, d, shape):
    """mean (d,), cov (d, d), std2_mean of the posterior from moments' totals about `center`"""
    t = np.asarray(total, dtype=LD)
    m1 = t[1:4] / t[0]
    cov = np.zeros((3, 3), LD)
    for k, (p, r) in enumerate(PAIRS):
        cov[p, r] = cov[r, p] = t[4 + k] / t[0] - m1[p] * m1[r]
    return {"mean": (np.asarray(center, dtype=np.float64).astype(LD) + m1[:d]), "cov": cov[:d, :d], "std2_mean": 0.5 * t[10] / t[0] / (LD(shape) - 1)}


def log_evidence(log_integral_z, L, lo, hi, shape):
    """log p(y | M) with the constants of rsf_grid_finish: the z-integral times prod L_pp is the integral over q (the Jacobian of
    the logged parameters is in l)"""
    d = len(lo)
    L = np.asarray(L, dtype=np.float64).reshape(d, d)
    return (LD(log_integral_z) + np.log(np.diag(L).astype(LD)).sum() - np.log(np.asarray(hi, dtype=LD) - np.asarray(lo, dtype=LD)).sum()
            + LD(math.lgamma(shape)) - LD(shape) * np.log(LD(np.pi)))


def posterior(ssq_at, z, w, m, L, tr, perm, lo, hi, shape):
    """The whole specification: ssq_at(q (k, d) inside the box) -> SSq (k,).  -> dict(q, jac, inb, ssq, l, the entries of z_sums,
    log_evidence, total, center, mean, cov, sd, std2_mean)"""
    d = len(z)
    q, jac, _ = nodes(z, m, L, tr, perm)
    inb = in_box(q, lo, hi)
    ssq = np.full(q.shape[0], np.nan)
    if inb.any():
        ssq[inb] = ssq_at(q[inb])
    l = log_target(ssq, jac, inb, shape)
    out = {"q": q, "jac": jac, "inb": inb, "ssq": ssq, "l": l}
    out.update(z_sums(z, w, l))
    if out["mass"] is None:
        return out
    center = nodes([np.zeros(1)] * d, m, L, tr, perm)[0][0]  # the fit's point
    total = moments(w, l, ssq, q, out["lmax"], center)
    out.update(summary(total, center, d, shape))
    out.update(total=total, center=center, sd=np.sqrt(np.diag(out["cov"])), log_evidence=log_evidence(out["log_integral"], L, lo, hi, shape))
    return out


# ---- the end-to-end problems -----------------------------------------------------------------------------------------------------
def fit_map(truth, law, log_coords=None, first=0):
    """observe_cases.friction_problem(truth) fitted under `law`: the true law's fit is law_fit_reference.fit_d3's, the other law's the
    same fit under that law -> (m, L, tr, perm, point, cov)"""
    st = fit_state(truth, law)
    i = int(np.argmin(np.where(st["status"] != F.FAILED, st["ssq"], np.inf)))
    n_obs = OC.friction_problem(truth)["data"].size
    cov = np.asarray(F.laplace(3, n_obs, 1.0, st["ssq"][i], st["H"][i], *LF.BOX[3])[0], dtype=np.float64)
    return factor(st["q"][i], cov, log_coords, first) + (st["q"][i].copy(), cov)


@functools.lru_cache(maxsize=None)
def fit_state(truth, law):
    if law == truth:
        return LF.fit_d3(truth)
    p = OC.friction_problem(truth)
    return LF.fit(p["m"], p["vl"], law, "mu", np.array(LF.STARTS3), p["data"], *LF.BOX[3], LF.FD[3], max_iter=60)


@functools.lru_cache(maxsize=None)
def e2e(truth, law, first=0, n=E2E_N, window_sd=E2E_WINDOW):
    """the specification's posterior of friction_problem(truth) under `law` at d = 3 on the grid of the fit, parameter `first` on axis
    0 -> posterior's dict with z, w, m, L, tr, perm, lo, hi, shape"""
    p = OC.friction_problem(truth)
    m, L, tr, perm, _, _ = fit_map(truth, law, None, first)
    z, w = axes(n, window_sd)
    lo, hi = LF.BOX[3]
    shape = 0.5 * p["data"].size
    ssq_at = lambda q: O.forward(p["m"], q[:, 0], p["vl"], law, "mu", a=q[:, 1], b=q[:, 2], data=p["data"])[1]
    out = posterior(ssq_at, z, w, m, L, tr, perm, lo, hi, shape)
    out.update(z=z, w=w, m=m, L=L, tr=tr, perm=perm, lo=lo, hi=hi, shape=shape)
    return out
