"""
The exact posterior on a tensor quadrature grid, in NumPy: the specification of include/rsf_grid.h (a test helper; TEST
INFRASTRUCTURE ONLY, no GPU).  Every sum that a test compares is taken in np.longdouble.

Grid: `n` (d,), `x` and `w` lists of d arrays; node (i0, i1, i2) has the flat index i0 + n0 (i1 + n1 i2), a COLUMN is the n0 nodes
of one (i1, i2), column c = i1 + n1 i2.  An axis the grid lacks counts as one node 0 of weight 1.  Coordinates PLAIN: q = x;
PRODUCT (d = 3): x0 = Dc a, q = (x0 / x1, x1, x2), density pi(q) / x1.
"""
import math

import numpy as np

import smc_reference

LD = np.longdouble
PLAIN, PRODUCT = 0, 1
FIELDS = 6  # per column: sums over i0 of w0 e times 1, (x0 - c), (x0 - c)^2, SSq, SSq^2; the count of -inf nodes
HEAD = ("Z", "log_integral", "log_evidence", "n_neginf")


def simpson(lo, hi, n):
    """n (odd) uniform nodes on [lo, hi] and their composite Simpson weights"""
    assert n % 2 == 1 and n >= 3
    x = np.linspace(lo, hi, n)
    w = np.full(n, 2.0)
    w[1::2] = 4.0
    w[0] = w[-1] = 1.0
    return x, w * ((hi - lo) / (n - 1) / 3.0)


def trapezoid(x):
    """trapezoid weights on the (uneven) nodes x"""
    x = np.asarray(x, dtype=np.float64)
    w = np.zeros_like(x)
    w[:-1] += 0.5 * np.diff(x)
    w[1:] += 0.5 * np.diff(x)
    return w


def gauss_legendre(lo, hi, n):
    t, g = np.polynomial.legendre.leggauss(n)
    return lo + (hi - lo) * (t + 1) / 2, g * (hi - lo) / 2


def pad(x, w=None):
    """the axes of a d <= 3 grid as three: a missing axis is one node 0 of weight 1"""
    x = [np.asarray(a, dtype=np.float64) for a in x] + [np.zeros(1)] * (3 - len(x))
    w = None if w is None else [np.asarray(a, dtype=np.float64) for a in w] + [np.ones(1)] * (3 - len(w))
    return x, w


def nodes(x, coords=PLAIN):
    """the points q (N, d) of the grid in flat-index order"""
    d = len(x)
    X = np.meshgrid(*x, indexing="ij")  # X[p][i0, i1, i2]
    flat = [np.ravel(a, order="F") for a in X]
    if coords == PRODUCT:
        assert d == 3
        flat[0] = flat[0] / flat[1]
    return np.stack(flat, axis=1)


def log_density(q, ssq, shape, lo, hi, coords=PLAIN):
    """l (N,) from the sums of squares at the nodes q (N, d): -shape log SSq - [PRODUCT] log x1; -inf outside the CLOSED box and
    where SSq is not finite or not > 0"""
    q, ssq = np.asarray(q, dtype=np.float64), np.asarray(ssq, dtype=np.float64)
    inb = ((q >= np.asarray(lo)) & (q <= np.asarray(hi))).all(axis=1)
    ok = inb & np.isfinite(ssq) & (ssq > 0)
    jac = np.log(q[:, 1]) if coords == PRODUCT else 0.0
    return np.where(ok, -shape * np.log(np.where(ok, ssq, 1.0)) - jac, -np.inf)


def columns(x, w, l, ssq, center, dtype=LD):
    """→ dict(lmax, fields (ncol, FIELDS), m0 (n0,), cum0 (ncol, n0)) of rsf_grid_columns"""
    x, w = pad(x, w)
    n0, n1, n2 = (a.size for a in x)
    L = np.asarray(l, dtype=np.float64).reshape(n2 * n1, n0)
    S = np.asarray(ssq, dtype=np.float64).reshape(n2 * n1, n0)
    fin = np.isfinite(L)
    assert not (np.isnan(L) | (L == np.inf)).any()
    lmax = L[fin].max() if fin.any() else -np.inf
    e = np.where(fin, np.exp(np.where(fin, L.astype(dtype) - dtype(lmax), 0)), 0).astype(dtype) if fin.any() else np.zeros(L.shape, dtype)
    we = w[0].astype(dtype)[None, :] * e
    dx = (x[0].astype(dtype) - dtype(center))[None, :]
    sq = np.where(fin, S, 0.0).astype(dtype)
    fields = np.stack([we.sum(axis=1), (we * dx).sum(axis=1), (we * dx * dx).sum(axis=1), (we * sq).sum(axis=1), (we * sq * sq).sum(axis=1),
                       (L == -np.inf).sum(axis=1).astype(dtype)], axis=1)
    W = (w[1].astype(dtype)[None, :] * w[2].astype(dtype)[:, None]).reshape(-1)
    m0 = (W[:, None] * e).sum(axis=0)
    cells = 0.5 * (e[:, :-1] + e[:, 1:]) * np.diff(x[0].astype(dtype))[None, :]
    cum0 = np.concatenate([np.zeros((e.shape[0], 1), dtype), np.cumsum(cells, axis=1)], axis=1)
    tot = cum0[:, -1:]
    cum0 = np.where(tot > 0, cum0 / np.where(tot > 0, tot, 1), 0)
    return {"lmax": float(lmax), "fields": fields, "m0": m0, "cum0": cum0}


def cum_table(x, w, m, dtype=LD):
    """the trapezoid CDF of the node density m / w on the nodes x, normalised by its last entry (all 0 without mass)"""
    x, f = np.asarray(x, dtype=dtype), np.asarray(m, dtype=dtype) / np.asarray(w, dtype=dtype)
    F = np.concatenate([[dtype(0)], np.cumsum(0.5 * (f[:-1] + f[1:]) * np.diff(x))])
    return F / F[-1] if F[-1] > 0 else np.zeros_like(F)


def finish(x, w, coords, center, shape, lo, hi, lmax, fields, dtype=LD):
    """rsf_grid_finish: → dict(Z, log_integral, log_evidence, n_neginf, mean (d,), cov (d, d), x0_mean, x0_var, std2_mean,
    std2_var, mass1, mass2, pair (n2, n1), cum1 (n2, n1), cum2 (n2,))"""
    d = len(x)
    x, w = pad(x, w)
    n0, n1, n2 = (a.size for a in x)
    f = np.asarray(fields, dtype=dtype).reshape(n2 * n1, FIELDS)
    out = {"n_neginf": int(f[:, 5].sum())}
    W = (w[1].astype(dtype)[None, :] * w[2].astype(dtype)[:, None]).reshape(-1)
    Z = (W * f[:, 0]).sum() if np.isfinite(lmax) else dtype(0)
    if not Z > 0:
        out.update(Z=np.nan, log_integral=-np.inf, log_evidence=np.nan)
        return out
    logi = dtype(lmax) + np.log(Z)
    out.update(Z=Z, log_integral=logi,
               log_evidence=logi - np.log(np.asarray(hi, dtype=dtype) - np.asarray(lo, dtype=dtype)).sum() + math.lgamma(shape) - shape * np.log(dtype(np.pi)))
    X1 = np.tile(x[1].astype(dtype), n2)
    X2 = np.repeat(x[2].astype(dtype), n1)
    c = dtype(center)
    # per column the sum over i0 of w0 e q0 from the fields about the centre
    q1 = f[:, 1] + c * f[:, 0]
    x0_mean = (W * q1).sum() / Z
    out["x0_mean"], out["x0_var"] = x0_mean, (W * (f[:, 2] + 2 * (c - x0_mean) * f[:, 1] + (c - x0_mean) ** 2 * f[:, 0])).sum() / Z
    if coords == PRODUCT:
        q1 = q1 / X1
    pair = W * f[:, 0] / Z
    mean = np.array([(W * q1).sum() / Z, (pair * X1).sum(), (pair * X2).sum()], dtype=dtype)
    r1, r2 = X1 - mean[1], X2 - mean[2]
    # the second moment of q0 about its mean from the centred fields: q0 - mean = ((x0 - c) + (c - mean x1)) / x1 in PRODUCT
    e = c - mean[0] * (X1 if coords == PRODUCT else 1)
    v0 = (W * (f[:, 2] + 2 * e * f[:, 1] + e * e * f[:, 0]) / (X1 * X1 if coords == PRODUCT else 1)).sum() / Z
    cov = np.array([[v0, (W * q1 * r1).sum() / Z, (W * q1 * r2).sum() / Z],
                    [0, (pair * r1 * r1).sum(), (pair * r1 * r2).sum()],
                    [0, 0, (pair * r2 * r2).sum()]], dtype=dtype)
    cov = cov + np.triu(cov, 1).T
    out["mean"], out["cov"] = mean[:d], cov[:d, :d]
    sq, sq2 = (W * f[:, 3]).sum() / Z, (W * f[:, 4]).sum() / Z
    out["std2_mean"] = 0.5 * sq / (shape - 1)
    out["std2_var"] = 0.25 * sq2 / ((shape - 1) * (shape - 2)) - out["std2_mean"] ** 2
    P = pair.reshape(n2, n1)
    out["pair"], out["mass1"], out["mass2"] = P, P.sum(axis=0), P.sum(axis=1)
    out["cum1"] = np.stack([cum_table(x[1], w[1], P[i2], dtype) for i2 in range(n2)]) if d > 1 else np.zeros((1, 1), dtype)
    out["cum2"] = cum_table(x[2], w[2], out["mass2"], dtype) if d > 2 else np.zeros(1, dtype)
    return out


def invert(F, x, u):
    """One axis: F (n,) or per draw (m, n), nodes x (n,), uniforms u (m,) → (value, cell k, nearest node) per draw.  k is the largest
    index <= n - 2 with F[k] <= u; a cell without mass gives x[k]; a tie between two nodes goes to the lower"""
    F, x, u = np.asarray(F, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    n = x.size
    if F.ndim == 1:
        F = np.broadcast_to(F, (u.size, n))
    k = np.clip((F[:, : n - 1] <= u[:, None]).sum(axis=1) - 1, 0, n - 2)
    r = np.arange(u.size)
    Fk, Fk1 = F[r, k], F[r, k + 1]
    dF = Fk1 - Fk
    v = np.where(dF > 0, x[k] + (u - Fk) / np.where(dF > 0, dF, 1.0) * (x[k + 1] - x[k]), x[k])
    node = np.where(v - x[k] <= x[k + 1] - v, k, k + 1)
    return v, k, node


def draw(x, coords, cum0, cum1, cum2, seed, offset, nd, chunk=8192):
    """rsf_grid_draw from the tables (float64, as the library holds them) → dict(q (nd, d), cell (nd, d) int, u (nd, d), margin (nd,):
    the smallest distance of a draw's u from an entry of the table row it was inverted from)"""
    if nd > chunk:
        parts = [draw(x, coords, cum0, cum1, cum2, seed, offset + s, min(chunk, nd - s)) for s in range(0, nd, chunk)]
        return {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    d = len(x)
    x, _ = pad(x)
    n0, n1, n2 = (a.size for a in x)
    u = smc_reference.start_uniforms(seed, np.arange(offset, offset + nd, dtype=np.uint64), d)
    v, k = np.zeros((nd, 3)), np.zeros((nd, 3), dtype=np.int64)
    i1 = i2 = np.zeros(nd, dtype=np.int64)
    margin = np.full(nd, np.inf)
    cum0 = np.asarray(cum0, dtype=np.float64).reshape(n2 * n1, n0)
    if d > 2:
        F = np.asarray(cum2, dtype=np.float64)
        v[:, 2], k[:, 2], i2 = invert(F, x[2], u[:, 2])
        margin = np.minimum(margin, np.abs(F[None, :] - u[:, 2:3]).min(axis=1))
    if d > 1:
        F = np.asarray(cum1, dtype=np.float64).reshape(n2, n1)[i2]
        v[:, 1], k[:, 1], i1 = invert(F, x[1], u[:, 1])
        margin = np.minimum(margin, np.abs(F - u[:, 1:2]).min(axis=1))
    F = cum0[i2 * n1 + i1]
    v[:, 0], k[:, 0], _ = invert(F, x[0], u[:, 0])
    margin = np.minimum(margin, np.abs(F - u[:, 0:1]).min(axis=1))
    if coords == PRODUCT:
        v[:, 0] = v[:, 0] / v[:, 1]
    return {"q": v[:, :d], "cell": k[:, :d], "u": u, "margin": margin}


def cdf(x, coords, cum0, pair, xs, dtype=LD):
    """rsf_grid_cdf: F(xs) = sum over the columns of pair[c] F0(xs [x1] | c), F0 the column of cum0 linearly interpolated"""
    x, _ = pad(x)
    n0, n1, n2 = (a.size for a in x)
    cum0 = np.asarray(cum0, dtype=np.float64).reshape(n2 * n1, n0)
    pair = np.asarray(pair, dtype=dtype).reshape(-1)
    out = np.zeros(np.size(xs), dtype)
    for c in range(n2 * n1):
        t = np.asarray(xs, dtype=np.float64) * (x[1][c % n1] if coords == PRODUCT else 1.0)
        out += pair[c] * np.interp(t, x[0], cum0[c], left=0.0, right=1.0)
    return out


def posterior(ssq_fn, x, w, lo, hi, shape, coords=PLAIN, center=None, dtype=LD):
    """The whole specification on the host: ssq_fn(*q columns) → SSq.  → (columns' dict, finish's dict, l, ssq)"""
    q = nodes(x, coords)
    inb = ((q >= np.asarray(lo)) & (q <= np.asarray(hi))).all(axis=1)
    ssq = np.full(q.shape[0], np.nan)
    ssq[inb] = ssq_fn(*q[inb].T)
    l = log_density(q, ssq, shape, lo, hi, coords)
    center = float(x[0][len(x[0]) // 2]) if center is None else center
    col = columns(x, w, l, ssq, center, dtype)
    return col, finish(x, w, coords, center, shape, lo, hi, col["lmax"], col["fields"], dtype), l, ssq
