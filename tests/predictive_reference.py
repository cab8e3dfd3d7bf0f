"""
Specification of the posterior predictive checks (include/rsf_predict.h), restated in NumPy.  Nothing here calls the library.

Given n draws (q_i, s2_i) and the observation data[nout]; y[k, i] is the clean acceleration series of draw i at output time k
(y[0, i] = 0), time-major as the library materialises it, and

    l[k, i] = -1/2 log(2 pi s2_i) - (data_k - y[k, i])^2 / (2 s2_i)

the Gaussian log likelihood the sampler's sum of squares and inverse-gamma update assume.  Per output time k:

    mean_k, var_k   mean and ddof = 1 variance of y[k, :] (the model series' credible spread)
    pit_k           mean_i Phi((data_k - y[k, i]) / sqrt(s2_i)): the probability integral transform of the observation under
                    the posterior predictive, the noise integrated analytically
    lpd_k           log mean_i exp(l[k, i]), the log pointwise predictive density
    p_waic_k        ddof = 1 variance of l[k, :] (Gelman, Hwang, Vehtari 2014; R loo's waic)
    quantiles[j,k]  np.quantile(y[k, :], probs[j]), method "linear"

Totals: mean_std2 = mean_i s2_i, elpd_waic = sum_k (lpd_k - p_waic_k), p_waic = sum_k p_waic_k,
elpd_waic_se = sqrt(nout * var_k(lpd_k - p_waic_k)) with ddof = 1 (R's var), all including k = 0.

Non-finite: if any y[k, i] of row k is not finite, every statistic of row k is NaN, and so are the totals that include it.

Additive partials about centres c_y[k], c_l[k] (HEAD + nout * FIELDS doubles): [0] n, [1] sum_i s2_i, then per row, over the
draws whose y[k, i] is finite: sum(y - c_y), sum(y - c_y)^2, sum(l - c_l), sum(l - c_l)^2, sum exp(l - c_l), sum Phi, and the
number of draws whose y[k, i] is not finite.

Element functions are float64 (scipy.special.ndtr, np.exp, np.log); every sum over draws is math.fsum, which is exact.
"""
import math

import numpy as np
from scipy.special import ndtr

HEAD = 2
FIELDS = 7
OUT = ("mean", "var", "pit", "lpd", "p_waic_k")
TOTALS = ("mean_std2", "elpd_waic", "p_waic", "elpd_waic_se")


def loglik(series, std2, data):
    """l[k, i]"""
    y = np.asarray(series, dtype=np.float64)
    s2 = np.asarray(std2, dtype=np.float64)[None, :]
    r = np.asarray(data, dtype=np.float64)[:, None] - y
    with np.errstate(invalid="ignore", over="ignore"):
        return -0.5 * np.log(2.0 * np.pi * s2) - (r * r) / (2.0 * s2)


def phi(series, std2, data):
    y = np.asarray(series, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ndtr((np.asarray(data, dtype=np.float64)[:, None] - y) / np.sqrt(np.asarray(std2, dtype=np.float64))[None, :])


def partials(series, std2, data, center_y, center_l):
    """The additive partials of a series (nout, n), flat (HEAD + nout * FIELDS,)."""
    y = np.asarray(series, dtype=np.float64)
    nout, n = y.shape
    l, p = loglik(y, std2, data), phi(y, std2, data)
    out = np.zeros(HEAD + nout * FIELDS)
    out[0], out[1] = n, math.fsum(np.asarray(std2, dtype=np.float64))
    for k in range(nout):
        ok = np.isfinite(y[k])
        dy, dl = y[k, ok] - center_y[k], l[k, ok] - center_l[k]
        with np.errstate(over="ignore"):
            row = [math.fsum(dy), math.fsum(dy * dy), math.fsum(dl), math.fsum(dl * dl), math.fsum(np.exp(dl)), math.fsum(p[k, ok]),
                   float(n - ok.sum())]
        out[HEAD + k * FIELDS:HEAD + (k + 1) * FIELDS] = row
    return out


def scales(want):
    """Per-entry scale of reference partials: a sum that may cancel is measured against sqrt(n * sum of squares)."""
    w = np.abs(np.asarray(want, dtype=np.float64))
    s = w.copy()
    rows, ws = s[HEAD:].reshape(-1, FIELDS), w[HEAD:].reshape(-1, FIELDS)
    rows[:, 0] = np.sqrt(w[0] * ws[:, 1])
    rows[:, 2] = np.sqrt(w[0] * ws[:, 3])
    rows[:, 6] = 1.0  # a count: exact
    return np.maximum(s, 1e-300)


def finish(part, center_y, center_l):
    """The statistics from (summed) partials, in float64 as the library's host-only finish computes them."""
    part = np.asarray(part, dtype=np.float64)
    n = part[0]
    rows = part[HEAD:].reshape(-1, FIELDS)
    nout = rows.shape[0]
    res = {name: np.full(nout, np.nan) for name in OUT}
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(nout):
            sy, sy2, sl, sl2, se, sp, bad = rows[k]
            if bad != 0 or not np.isfinite(rows[k]).all():
                continue
            res["mean"][k] = center_y[k] + sy / n
            res["var"][k] = (sy2 - sy * (sy / n)) / (n - 1.0)
            res["pit"][k] = sp / n
            res["lpd"][k] = center_l[k] + np.log(se / n)
            res["p_waic_k"][k] = (sl2 - sl * (sl / n)) / (n - 1.0)
        e = res["lpd"] - res["p_waic_k"]
        res["mean_std2"] = part[1] / n
        res["elpd_waic"] = math.fsum(e) if np.isfinite(e).all() else float("nan")
        res["p_waic"] = math.fsum(res["p_waic_k"]) if np.isfinite(e).all() else float("nan")
        res["elpd_waic_se"] = float(np.sqrt(nout * np.var(e, ddof=1))) if nout > 1 else float("nan")
    return res


def statistics(series, std2, data, probs=()):
    """The definitions, straight from the series (no partials, no centres): every sum over draws exact."""
    y = np.asarray(series, dtype=np.float64)
    nout, n = y.shape
    l, p = loglik(y, std2, data), phi(y, std2, data)
    res = {name: np.full(nout, np.nan) for name in OUT}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(nout):
            if not np.isfinite(y[k]).all():
                continue
            my, ml = math.fsum(y[k]) / n, math.fsum(l[k]) / n
            res["mean"][k] = my
            res["var"][k] = math.fsum((y[k] - my) ** 2) / (n - 1.0) if n > 1 else np.nan
            res["pit"][k] = math.fsum(p[k]) / n
            mx = l[k].max()
            res["lpd"][k] = mx + np.log(math.fsum(np.exp(l[k] - mx)) / n)
            res["p_waic_k"][k] = math.fsum((l[k] - ml) ** 2) / (n - 1.0) if n > 1 else np.nan
        e = res["lpd"] - res["p_waic_k"]
        ok = np.isfinite(e).all()
        res["mean_std2"] = math.fsum(np.asarray(std2, dtype=np.float64)) / n
        res["elpd_waic"] = math.fsum(e) if ok else float("nan")
        res["p_waic"] = math.fsum(res["p_waic_k"]) if ok else float("nan")
        res["elpd_waic_se"] = float(np.sqrt(nout * np.var(e, ddof=1))) if nout > 1 else float("nan")
        if len(probs):
            res["quantiles"] = np.quantile(y, np.asarray(probs, dtype=np.float64), axis=1)
    return res
