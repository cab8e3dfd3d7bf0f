"""
Specification of PSIS-LOO and the Pareto shape of pooled draws (include/rsf_psis.h, rsf_predict_psis_loo and
rsf_predict_psis_finish), restated in NumPy.  Nothing here calls the library.  It is ArviZ's psislw and _gpdfit written out
(Vehtari, Gelman, Gabry 2017; Vehtari, Simpson, Gelman, Yao, Gabry 2024; Zhang and Stephens 2009), evaluated in `dtype`:
np.longdouble is the specification, np.float64 the plain restatement whose distance from it sizes the tests' bounds.

For one output time k, n draws, r_eff (default 1), l_i = -1/2 log(2 pi s2_i) - (data_k - y_ik)^2 / (2 s2_i):

1.  x_i = -l_i, then x_i -= max_i x_i.
2.  tail_len = ceil(min(0.2 n, 3 sqrt(n / r_eff))); cutoff = max(x_(n - tail_len - 1), log(DBL_MIN)), x_(j) the ascending order
    statistics, 0-based.  The tail is {i : x_i > cutoff}, strictly; n_tail its size (values tied with the cutoff stay out, so
    n_tail <= tail_len).  n = 1 has no such order statistic (tail_len = 1, index -1; ArviZ raises there): the index is clamped
    at 0, the tail is empty.
3.  n_tail <= 4: pareto_k = +inf and no smoothing.  This includes a row whose ratios are all equal, as row k = 0 is when every
    s2_i is equal: ArviZ's behaviour, kept.
4.  Otherwise t_j = exp(x) - exp(cutoff) of the tail, ascending, N = n_tail, and Zhang and Stephens' fit:
        m = 30 + floor(sqrt(N));  b_j = 1 - sqrt(m / (j - 0.5)), j = 1..m;  b_j /= 3 t[floor(N/4 + 0.5) - 1];  b_j += 1 / t[N-1]
        k_j = mean_i log1p(-b_j t_i);  L_j = N (log(-b_j / k_j) - k_j - 1);  w_j = 1 / sum_l exp(L_l - L_j)
        (an overflow to +inf in exp(L_l - L_j) is meant: it gives w_j = 0)
        drop every w_j < 10 DBL_EPSILON, normalise the rest to sum 1
        b = sum w_j b_j;  k = mean_i log1p(-b t_i);  sigma = -k / b;  pareto_k = (N k + 5) / (N + 10)
    and, if pareto_k is finite, with p_j = (j + 0.5) / N, j = 0..N-1, the tail member of rank j gets
        x = log(sigma expm1(-pareto_k log1p(-p_j)) / pareto_k + exp(cutoff)).
5.  x_i = min(x_i, 0);  lw_i = x_i - logsumexp(x);  elpd_loo_k = logsumexp_i(lw_i + l_i);  weight_ess_k = 1 / sum_i exp(2 lw_i).

A row that holds a non-finite y_ik is NaN in all four outputs.  Totals over the rows, with lpd_k of the predictive statistics
and k = 0 included as in WAIC: elpd_loo = sum_k elpd_loo_k, p_loo = sum_k (lpd_k - elpd_loo_k),
elpd_loo_se = sqrt(nout var_k(elpd_loo_k)) with ddof 1 (the convention of elpd_waic_se here; ArviZ uses ddof 0),
k_threshold = min(1 - 1 / log10(n), 0.7), n_high_k = #{k : pareto_k > k_threshold} (+inf counts), max_pareto_k.
"""
import math

import numpy as np

OUT = ("elpd_loo_k", "pareto_k", "n_tail", "weight_ess")
TOTALS = ("elpd_loo", "p_loo", "elpd_loo_se", "k_threshold", "n_high_k", "max_pareto_k")
LOG_DBL_MIN = math.log(np.finfo(np.float64).tiny)
EPS = float(np.finfo(np.float64).eps)
MAX_TAIL = 8192  # RSF_PSIS_MAX_TAIL


def tail_len(n, r_eff=1.0):
    return int(math.ceil(min(0.2 * n, 3.0 * math.sqrt(n / r_eff))))


def loglik_row(y, std2, obs, dtype=np.longdouble):
    """l_i of one output time, in dtype from the float64 inputs."""
    y, s2 = np.asarray(y, dtype=np.float64).astype(dtype), np.asarray(std2, dtype=np.float64).astype(dtype)
    r = dtype(np.float64(obs)) - y
    pi = dtype(np.pi) if dtype is np.float64 else np.longdouble(4) * np.arctan(np.longdouble(1))
    with np.errstate(invalid="ignore", over="ignore"):
        return -np.log(2 * pi * s2) / 2 - (r * r) / (2 * s2)


def _logsumexp(v):
    m = v.max()
    return m + np.log(np.sum(np.exp(v - m)))


def gpdfit(t, dtype=np.longdouble):
    """Step 4's fit of an ascending tail t → (pareto_k, sigma)."""
    t = np.asarray(t, dtype=dtype)
    N = t.size
    m = 30 + int(math.floor(math.sqrt(N)))
    with np.errstate(all="ignore"):
        b = 1 - np.sqrt(dtype(m) / (np.arange(1, m + 1, dtype=dtype) - dtype(0.5)))
        b = b / (3 * t[int(N / 4 + 0.5) - 1])
        b = b + 1 / t[-1]
        kj = np.log1p(-b[:, None] * t).mean(axis=1)
        L = N * (np.log(-b / kj) - kj - 1)
        w = 1 / np.exp(L - L[:, None]).sum(axis=1)
        keep = w >= 10 * EPS
        w, b = w[keep], b[keep]
        w = w / w.sum()
        bb = np.sum(w * b)
        k = np.log1p(-bb * t).mean()
        sigma = -k / bb
        k = (N * k + 5) / (N + 10)
    return k, sigma


def psis_row(loglik, r_eff=1.0, dtype=np.longdouble, return_weights=False):
    """Steps 1 to 5 for the log likelihoods l_i of one output time → (elpd_loo_k, pareto_k, n_tail, weight_ess_k)."""
    l = np.asarray(loglik, dtype=dtype)
    n = l.size
    x = -l
    x = x - x.max()
    cutoff = max(np.sort(x)[max(n - tail_len(n, r_eff) - 1, 0)], dtype(LOG_DBL_MIN))
    tail = np.nonzero(x > cutoff)[0]
    n_tail = tail.size
    k = dtype(np.inf)
    if n_tail > 4:
        order = np.argsort(x[tail], kind="stable")
        tail = tail[order]
        with np.errstate(all="ignore"):
            ecut = np.exp(cutoff)
            k, sigma = gpdfit(np.exp(x[tail]) - ecut, dtype)
            if np.isfinite(k):
                p = (np.arange(n_tail, dtype=dtype) + dtype(0.5)) / n_tail
                x[tail] = np.log(sigma * np.expm1(-k * np.log1p(-p)) / k + ecut)
    with np.errstate(all="ignore"):
        x = np.minimum(x, 0)
        lw = x - _logsumexp(x)
        elpd = _logsumexp(lw + l)
        ess = 1 / np.sum(np.exp(2 * lw))
    if return_weights:
        return lw
    return elpd, k, n_tail, ess


def psis_rows(series, std2, data, r_eff=1.0, dtype=np.longdouble):
    """The four row outputs of a series (nout, n) → dict of (nout,) arrays in dtype (n_tail float64; NaN rows as specified)."""
    y = np.asarray(series, dtype=np.float64)
    nout = y.shape[0]
    res = {name: np.full(nout, np.nan, dtype=dtype) for name in OUT}
    for k in range(nout):
        if not np.isfinite(y[k]).all():
            continue
        row = psis_row(loglik_row(y[k], std2, data[k], dtype), r_eff, dtype)
        for name, v in zip(OUT, row):
            res[name][k] = v
    return res


def finish(rows, lpd, n):
    """The totals from the rows and lpd_k, in float64 as the library's host-only finish computes them."""
    e = np.asarray(rows["elpd_loo_k"], dtype=np.float64)
    pk = np.asarray(rows["pareto_k"], dtype=np.float64)
    lpd = np.asarray(lpd, dtype=np.float64)
    nout = e.size
    ok = bool(np.isfinite(e).all() and not np.isnan(pk).any() and np.isfinite(lpd).all())
    with np.errstate(all="ignore"):
        thr = min(1.0 - 1.0 / math.log10(n), 0.7) if n > 1 else -math.inf
        nan = float("nan")
        return {"elpd_loo": math.fsum(e) if ok else nan,
                "p_loo": math.fsum(lpd - e) if ok else nan,
                "elpd_loo_se": float(np.sqrt(nout * np.var(e, ddof=1))) if ok and nout > 1 else nan,
                "k_threshold": thr,
                "n_high_k": float(np.sum(pk > thr)) if ok else nan,
                "max_pareto_k": float(pk.max()) if ok else nan}


def gpd_quantile_tail(k, N, sigma=1.0, dtype=np.longdouble):
    """Exact generalised-Pareto quantiles at the mid-points p_j = (j + 0.5) / N: a tail whose shape is k by construction."""
    p = (np.arange(N, dtype=dtype) + dtype(0.5)) / N
    return dtype(sigma) * np.expm1(-dtype(k) * np.log1p(-p)) / dtype(k)
