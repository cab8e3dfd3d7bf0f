"""
Specification of the posterior predictive band that includes the noise (include/rsf_predict_noise.h), restated in NumPy and
SciPy.  Nothing here calls the library.

For a row y = series[k, :] of the materialised series (n draws) and s_i = sqrt(std2_i), the posterior predictive distribution of
an observation at output time k is the mixture mean_i N(y_i, s_i^2):

    F(t) = 1/n sum_i Phi((t - y_i) / s_i)          strictly increasing, F(-inf) = 0, F(+inf) = 1
    Q(p) = the t with F(t) = p,  0 < p < 1

Bracket.  With z = ndtri(p) and e_i = y_i + z s_i:  F(min_i e_i) <= p <= F(max_i e_i), because at t = min e every component has
(t - y_i) / s_i <= z, so Phi <= p, and at t = max e every component has Phi >= p.  For n = 1 the bracket is the answer.

Root.  scipy.optimize.brentq on F - p over that bracket widened by one ulp at each end, xtol tiny, rtol = 4 eps.

Non-finite.  A row with a non-finite y_i gives NaN for every probability.  If any std2_i is not finite and > 0, every row is NaN:
that draw enters every row.  Row k = 0 (every y_i = 0) is a scale mixture at 0, an ordinary row.

Element functions are float64 (scipy.special.ndtr, ndtri); every sum over draws is math.fsum, which is exact.

The library's result is not "the" float64 root — F is flat to rounding near it — but a float64 t whose residual |F(t) - p| is
small; `residual` measures it.  `scheme` is the float64 restatement of the library's iteration (bracket, safeguarded Newton, the
three stopping rules, the sums in 256 strided partials and a tree), from which the tests take their bounds on the passes.
"""
import math

import numpy as np
from scipy.optimize import brentq
from scipy.special import erfc, ndtr, ndtri

MAX_PASSES = 129   # RSF_PREDICT_NOISE_MAX_PASSES
TOL = 2.0 ** -46   # the library's stopping rule (a), relative to min(p, 1 - p)


def cdf(y, s, t):
    """F(t) of one row: y (n,), s (n,) = sqrt(std2)."""
    return math.fsum(ndtr((t - np.asarray(y, dtype=np.float64)) / np.asarray(s, dtype=np.float64))) / len(y)


def bracket(y, s, p):
    e = np.asarray(y, dtype=np.float64) + ndtri(p) * np.asarray(s, dtype=np.float64)
    return float(e.min()), float(e.max())


def std2_ok(std2):
    s2 = np.asarray(std2, dtype=np.float64)
    return bool(np.all(np.isfinite(s2) & (s2 > 0.0)))


def quantile_row(y, s, p):
    """Q(p) of one row (finite y, good s)."""
    lo, hi = bracket(y, s, p)
    if cdf(y, s, lo) - p >= 0.0:  # (F(lo) <= p by the bracket: equal as far as float64 tells, so the end is the root; n = 1 always)
        return lo
    if cdf(y, s, hi) - p <= 0.0:
        return hi
    lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    return float(brentq(lambda t: cdf(y, s, t) - p, lo, hi, xtol=5e-324, rtol=4 * np.finfo(np.float64).eps, maxiter=500))


def quantiles(series, std2, probs, rows=None):
    """(len(probs), nout) — NaN rows as defined; rows: compute only these (the others NaN)."""
    y = np.asarray(series, dtype=np.float64)
    nout, n = y.shape
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if not np.all((probs > 0.0) & (probs < 1.0)):
        raise ValueError("probabilities lie strictly inside (0, 1)")
    out = np.full((probs.size, nout), np.nan)
    if not std2_ok(std2):
        return out
    s = np.sqrt(np.asarray(std2, dtype=np.float64))
    for k in (range(nout) if rows is None else rows):
        if np.isfinite(y[k]).all():
            out[:, k] = [quantile_row(y[k], s, p) for p in probs]
    return out


def residual(series, std2, probs, got):
    """|F_k(got[j, k]) - probs[j]| (len(probs), nout), F evaluated once per entry; NaN where got is NaN."""
    y = np.asarray(series, dtype=np.float64)
    s = np.sqrt(np.asarray(std2, dtype=np.float64))
    got = np.asarray(got, dtype=np.float64)
    out = np.full(got.shape, np.nan)
    for k in range(y.shape[0]):
        for j, p in enumerate(probs):
            if np.isfinite(got[j, k]):
                out[j, k] = abs(cdf(y[k], s, got[j, k]) - p)
    return out


# ---- the library's iteration in float64 NumPy ---------------------------------------------------------------------------------
def _tree(v, op):
    """256 per-thread values: a butterfly over each wave's 64 lanes (= the pairwise tree), then the four waves in order."""
    w = np.asarray(v, dtype=np.float64).reshape(4, 64)
    while w.shape[1] > 1:
        w = op(w[:, 0::2], w[:, 1::2])
    w = w[:, 0]
    return op(op(op(w[0], w[1]), w[2]), w[3])


def _strided(x, fill, op):
    """per-thread strides i = t, t + 256, ... in order, then the tree"""
    pad = (-len(x)) % 256
    a = np.concatenate([x, np.full(pad, fill)]).reshape(-1, 256)
    acc = a[0].copy()
    for r in a[1:]:
        acc = op(acc, r)
    return _tree(acc, op)


def scheme(y, s, p, max_passes=MAX_PASSES):
    """The library's iteration for one row and one probability → (t, passes over the row)."""
    y, s = np.asarray(y, dtype=np.float64), np.asarray(s, dtype=np.float64)
    n = len(y)
    r = 1.0 / (s * 1.41421356237309504880)
    e = y + ndtri(p) * s
    lo, hi = -_strided(-e, -np.inf, np.maximum), _strided(e, -np.inf, np.maximum)
    pad = 2.0 ** -49 * (abs(lo) + abs(hi))
    lo, hi = lo - pad, hi + pad
    neg = p > 0.5
    q = 1.0 - p if neg else p
    t = res = lo + 0.5 * (hi - lo)
    prev = hi - lo
    passes = 1
    if not (lo < t < hi):
        return res, passes
    while passes < max_passes:
        passes += 1
        x = (y - t) * r
        if neg:
            x = -x
        H = _strided(erfc(x), 0.0, np.add)
        D = _strided(np.exp(-(x * x)) * r, 0.0, np.add)
        Hn = H / (2.0 * n)
        g = Hn - q
        fg = -g if neg else g
        fd = D * 0.56418958354775628695 / n
        if fg < 0.0:
            lo = t
        if fg > 0.0:
            hi = t
        if abs(g) <= TOL * q:
            return t, passes  # (a)
        with np.errstate(divide="ignore", invalid="ignore"):
            step = (-Hn if neg else Hn) * np.log1p(g / q) / np.float64(fd)  # Newton on log(mass) = log q
        tn = t - step
        inside = fd > 0.0 and lo < tn < hi
        if fd > 0.0 and abs(step) <= abs(t) * 2.0 ** -52:
            return (tn if inside else t), passes  # (b)
        if not (inside and abs(step) <= 0.5 * abs(prev)):
            tn = lo + 0.5 * (hi - lo)
            if not (lo < tn < hi):
                return t, passes  # (c)
        prev, t = tn - t, tn
        res = lo + 0.5 * (hi - lo)
    return res, passes
