"""
Specification of the state-law solve with the STIFFNESS AMONG THE PARAMETERS (a test helper; TEST INFRASTRUCTURE ONLY, no GPU) —
what include/rsf_kstiff.h's rsf_kstiff_observe, rsf_kstiff_dr_run and rsf_kstiff_dr_ssq and MCMC.sample_stiffness are checked
against.  Nothing new is solved here: a point is (Dc, k) or (Dc, a, b, k), the stiffness LAST, and its series is
tests/stiff_reference.py's trajectory_lane with k one value per lane (it broadcasts k over the lanes; an array works as it is),
its sum of squares formed sample by sample so that a lane's SSq is the same bits alone and among others.  Added: the
forward-difference Gauss-Newton normal equations (Engine.kstiff_gn_factor's rule), a damped Gauss-Newton least-squares fit on them,
and the two yardsticks of the target tests:

    quadrature2   d = 2: tensor Simpson quadrature of SSq^-shape over a window of +-nsd Laplace SDs about a centre
    importance4   d = 4: self-normalised importance sampling from a multivariate t5 about the least-squares point
"""
import numpy as np

import stiff_reference as S


def columns(pts):
    """points (m, 2) of (Dc, k) or (m, 4) of (Dc, a, b, k) -> (dc, a, b, k); a and b None at d = 2"""
    pts = np.asarray(pts, np.float64)
    pts = pts.reshape(1, -1) if pts.ndim == 1 else pts
    if pts.ndim != 2 or pts.shape[1] not in (2, 4):
        raise ValueError(f"points are (m, 2) of (Dc, k) or (m, 4) of (Dc, a, b, k), not {pts.shape}")
    return (pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]) if pts.shape[1] == 4 else (pts[:, 0], None, None, pts[:, 1])


def trajectory_lane(m, pts, vl=None, law="aging"):
    """-> {observable: series [nout, m]}: stiff_reference.trajectory_lane with each point's own k"""
    dc, a, b, k = columns(pts)
    return S.trajectory_lane(m, k, dc, vl, law, a, b)


def ssq_in_order(series, data):
    """-> SSq [m] of series [nout, m] against data [nout], the squares added sample by sample from 0.0: a lane's sum does not depend
    on how many lanes stand beside it (NumPy's own sum over an axis pairs its terms by the array's width)"""
    s = np.zeros(series.shape[1])
    with np.errstate(all="ignore"):
        for row, obs in zip(series, np.asarray(data, np.float64)):
            r = row - obs
            s = s + r * r
    return s


def forward_lane(m, pts, vl=None, law="aging", observable="acc", data=None):
    """-> (series [nout, m], ssq [m] or None): stiff_reference.trajectory_lane's series with each point's own k, and ssq_in_order"""
    series = trajectory_lane(m, pts, vl, law)[S.ALIASES[observable]]
    return series, None if data is None else ssq_in_order(series, data)


def ssq_fn(m, vl, law, observable, data):
    """points (m, d) with the stiffness last -> SSq (m,) of the float64 specification"""
    return lambda pts: forward_lane(m, pts, vl, law, observable, data)[1]


def normal(m, vl, law, observable, q, data, rel_step=1e-4):
    """-> (J (nout, d), r (nout,), ssq) at the point q (d,): J by forward differences with step rel_step q_p, from ONE solve of
    1 + d lanes (Engine.kstiff_gn_factor's rule)"""
    q = np.asarray(q, np.float64).reshape(-1)
    h = rel_step * q
    pts = np.tile(q, (1 + q.size, 1))
    pts[1:] += np.diag(h)
    series = forward_lane(m, pts, vl, law, observable)[0]
    r = series[:, 0] - data
    return (series[:, 1:] - series[:, :1]) / h, r, float(r @ r)


def laplace(J, ssq, nout):
    """-> (cov, sd, condition number of the scaled Jacobian): cov = (SSq / nout) (J^T J)^-1"""
    cov = (ssq / nout) * np.linalg.inv(J.T @ J)
    return cov, np.sqrt(np.diag(cov)), float(np.linalg.cond(J / np.linalg.norm(J, axis=0)))


def gn_factor(m, vl, law, observable, q, data, rel_step=1e-4):
    """-> (L, cov, ssq): L = chol((2.38^2 / d) cov), law_dr_reference.gn_factor's rule at d = 2 or 4"""
    J, _, ssq = normal(m, vl, law, observable, q, data, rel_step)
    cov = laplace(J, ssq, data.size)[0]
    return np.linalg.cholesky((2.38 ** 2 / np.size(q)) * cov), cov, ssq


def fit(m, vl, law, observable, q0, data, iters=40, tol=1e-12):
    """The least-squares point from q0 by damped Gauss-Newton (Levenberg-Marquardt on the scaled normal equations) -> (q, J, ssq);
    stops when a step changes no coordinate by more than tol of its value"""
    q = np.asarray(q0, np.float64).reshape(-1).copy()
    J, r, ssq = normal(m, vl, law, observable, q, data)
    lam = 1e-3
    for _ in range(iters):
        s = np.linalg.norm(J, axis=0)
        A, g = (J / s).T @ (J / s), (J / s).T @ r
        step = -np.linalg.solve(A + lam * np.eye(q.size), g) / s
        Jn, rn, ssqn = normal(m, vl, law, observable, q + step, data)
        if np.isfinite(ssqn) and ssqn <= ssq:
            q, J, r, ssq, lam = q + step, Jn, rn, ssqn, max(lam / 10.0, 1e-12)
            if (np.abs(step) <= tol * np.abs(q)).all():
                break
        else:
            lam *= 10.0
            if lam > 1e8:
                break
    return q, J, ssq


def _simpson(lo, hi, n):
    assert n % 2 == 1 and n >= 3
    w = np.full(n, 2.0)
    w[1::2] = 4.0
    w[0] = w[-1] = 1.0
    return np.linspace(lo, hi, n), w * (hi - lo) / (n - 1) / 3.0


def quadrature2(fn, center, sd, shape, n=(129, 65), nsd=8.0):
    """The exact posterior pi(Dc, k) ~ SSq^-shape by tensor Simpson quadrature on n[0] x n[1] nodes over center +- nsd sd; fn(points
    (m, 2)) -> SSq (m,) -> dict(mean (2,), sd (2,), edge: the largest weight on the window's edge over the largest weight,
    x, y: the axes, l: -shape log SSq on the grid)"""
    (x, wx), (y, wy) = (_simpson(center[p] - nsd * sd[p], center[p] + nsd * sd[p], n[p]) for p in (0, 1))
    X, Y = np.meshgrid(x, y, indexing="ij")
    ssq = np.asarray(fn(np.column_stack([X.ravel(), Y.ravel()])), np.float64).reshape(X.shape)
    assert np.isfinite(ssq).all() and (ssq > 0).all(), "a non-finite SSq inside the window"
    l = -shape * np.log(ssq)
    f = np.exp(l - l.max())
    W = wx[:, None] * wy[None, :] * f
    W /= W.sum()
    mean = np.array([(W * X).sum(), (W * Y).sum()])
    var = np.array([(W * (X - mean[0]) ** 2).sum(), (W * (Y - mean[1]) ** 2).sum()])
    edge = max(f[0].max(), f[-1].max(), f[:, 0].max(), f[:, -1].max())
    return dict(mean=mean, sd=np.sqrt(var), edge=float(edge), x=x, y=y, l=l)


def importance4(fn, center, cov, shape, lo, hi, n=16384, seed=0, nu=5, scale=1.5):
    """The posterior pi(q) ~ 1_box SSq^-shape by self-normalised importance sampling: n draws from the multivariate t_nu at
    `center` with the scale matrix scale^2 cov; fn(points (n, d)) -> SSq -> dict(mean (d,), sd (d,), se (d,): the delta-method
    standard error of mean, ess, wmax: the largest normalised weight, inbox, finite: every draw inside the box / finite)"""
    rng = np.random.default_rng(seed)
    center = np.asarray(center, np.float64)
    d = center.size
    Lc = scale * np.linalg.cholesky(cov)
    z = rng.standard_normal((n, d)) / np.sqrt(rng.chisquare(nu, n) / nu)[:, None]
    q = center + z @ Lc.T
    inbox = bool(((q > lo) & (q < hi)).all())
    ssq = np.asarray(fn(q), np.float64)
    finite = bool(np.isfinite(ssq).all() and (ssq > 0).all())
    with np.errstate(all="ignore"):
        lw = np.where(((q > lo) & (q < hi)).all(axis=1) & np.isfinite(ssq) & (ssq > 0), -shape * np.log(ssq), -np.inf)
    lw = lw + 0.5 * (nu + d) * np.log1p((z * z).sum(axis=1) / nu)  # over the proposal's density, up to a constant
    w = np.exp(lw - lw.max())
    w /= w.sum()
    mean = w @ q
    c = q - mean
    return dict(mean=mean, sd=np.sqrt(w @ (c * c)), se=np.sqrt((w * w) @ (c * c)), ess=float(1.0 / (w @ w)), wmax=float(w.max()), inbox=inbox,
                finite=finite, q=q, w=w)
