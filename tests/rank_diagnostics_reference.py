"""
NumPy/SciPy restatement of the rank-normalised diagnostics and order statistics of include/rsf_diag.h (rsf_diag_rank_*): the
specification that tests/test_rank_diagnostics_reference.py and tests/test_gpu_rank_diagnostics.py hold the library to.  These
are ArviZ's definitions (rhat(method="rank"), ess(method="bulk" / "tail"), hdi) and NumPy's (median, quantile(method="linear")),
written out so that neither ArviZ nor a copy of it is needed.

For each parameter p of a trace x[n][C][d] (iteration-major, as rsf_mcmc_run writes it), with N = n // 2:

Full set: all A = n*C draws of p.  Split set: rows [0, N) and [n-N, n), T = 2*C*N draws; an odd n leaves out the middle row.

Non-finite: if any draw of p is not finite, every output for p is NaN (lags_complete excepted); other parameters are unaffected.

Order statistics of the full set sorted ascending, s[0..A-1], with -0.0 == +0.0:
  median     s[(A-1)/2] for odd A, else (s[A/2-1] + s[A/2]) / 2 (np.median);
  quantile   h = (A-1)*prob, lo = floor(h), g = h - lo, a = s[lo], b = s[min(lo+1, A-1)]; a + (b-a)*g if g < 0.5 else
             b - (b-a)*(1-g) (np.quantile, NumPy's _lerp);
  HDI        k = floor(prob*A), 1 <= k < A; widths w_i = s[i+k] - s[i] for i < A-k; i* = the first index of the minimum;
             (s[i*], s[i*+k]) (ArviZ's _hdi, not circular).

Average ranks over the split set: r(v) = L + (E+1)/2, L = #split draws < v, E = #split draws == v (scipy.stats.rankdata
"average").  Normal scores z(v) = ndtri((r(v) - 3/8) / (T + 1/4)).

Four derived series, each with the trace's shape; the middle row holds 0 and is never read:
  bulk    zb = z(x);
  folded  zf = the normal scores of |x - median| (float64), ranked among the split set's |x - median|;
  q05     I_lo = 1.0 if x <= quantile(0.05) else 0.0;
  q95     I_hi = 1.0 if x <= quantile(0.95) else 0.0.

Statistics: each series goes through diagnostics_reference (centre 0, no superchains; Geyer's truncation) in long double.
rhat_bulk = split R-hat of zb, rhat_tail = split R-hat of zf, rhat = max of the two (NaN if either is NaN), ess_bulk = ESS of zb,
ess_q05 / ess_q95 = ESS of I_lo / I_hi, ess_tail = min(ess_q05, ess_q95).  A series whose split draws are all equal
(max - min < 1e-15, ArviZ _ess) has ess = T and tau = 1 instead of NaN; its R-hat stays NaN.

Ranks are global: these statistics do not add across shards of chains.
"""
import numpy as np
from scipy import special, stats

import diagnostics_reference as dref

LD = dref.LD
SERIES = ("bulk", "folded", "q05", "q95")
STATS = ("median", "q05", "q95", "hdi_lo", "hdi_hi", "nonfinite", "const_bulk", "const_folded", "const_q05", "const_q95")
OUT = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "lags_complete")
CONST_TOL = 1e-15


def _trace(trace):
    x = np.asarray(trace, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3 or x.shape[0] < 4:
        raise ValueError("a trace is (n >= 4, C[, d])")
    return x


def split_rows(n):
    """Row indices of the split set: [0, N) and [n - N, n)."""
    N = n // 2
    return np.r_[0:N, n - N:n]


def quantile(v, prob):
    return np.quantile(np.asarray(v, dtype=np.float64).ravel(), prob, method="linear")


def hdi(v, prob):
    """ArviZ's non-circular HDI of the flattened draws: (s[i*], s[i*+k]), k = floor(prob*A), i* the first narrowest window."""
    s = np.sort(np.asarray(v, dtype=np.float64).ravel())
    A = s.size
    k = int(np.floor(prob * A))
    if not 1 <= k < A:
        raise ValueError("need 1 <= floor(prob * A) < A")
    w = s[k:] - s[: A - k]
    i = int(np.argmin(w))
    return s[i], s[i + k]


def normal_scores(v):
    """z of every value of v among the values of v: ndtri((average rank - 3/8) / (size + 1/4))."""
    v = np.asarray(v, dtype=np.float64)
    r = stats.rankdata(v.ravel(), method="average")
    return special.ndtri((r - 0.375) / (v.size + 0.25)).reshape(v.shape)


def prepare(trace, probs=(), hdi_prob=0.94):
    """The stats (d, len(STATS) + len(probs)) and the four series (4, n, C, d), float64."""
    x = _trace(trace)
    n, C, d = x.shape
    rows = split_rows(n)
    mid = np.setdiff1d(np.arange(n), rows)
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    st = np.zeros((d, len(STATS) + probs.size))
    series = np.zeros((4, n, C, d))
    for p in range(d):
        xp = x[:, :, p]
        if not np.all(np.isfinite(xp)):
            st[p] = np.nan
            st[p, STATS.index("nonfinite")] = 1.0
            st[p, STATS.index("const_bulk"):len(STATS)] = 0.0
            series[:, :, :, p] = np.nan
            continue
        m = np.median(xp)
        q05, q95 = quantile(xp, 0.05), quantile(xp, 0.95)
        series[0, rows, :, p] = normal_scores(xp[rows])
        series[1, rows, :, p] = normal_scores(np.abs(xp[rows] - m))
        series[2, :, :, p] = np.where(xp <= q05, 1.0, 0.0)
        series[3, :, :, p] = np.where(xp <= q95, 1.0, 0.0)
        series[2:, mid, :, p] = 0.0
        lo, hi = hdi(xp, hdi_prob)
        st[p, :6] = m, q05, q95, lo, hi, 0.0
        for q in range(4):
            v = series[q, rows, :, p]
            st[p, 6 + q] = 1.0 if v.max() - v.min() < CONST_TOL else 0.0
        if probs.size:
            st[p, len(STATS):] = quantile(xp, probs)
    return st, series


def finish(st, series_stats):
    """The statistics from prepare's stats and diagnostics_reference's dicts of the four series (series_stats[q][p], each with
    "T", the split-set size, added)."""
    res = []
    nan = LD("nan")
    for p, row in enumerate(st):
        r = dict.fromkeys(OUT, nan)
        r["lags_complete"] = all(series_stats[q][p]["lags_complete"] for q in range(4))
        res.append(r)
        if row[STATS.index("nonfinite")]:
            continue
        ess, rh = [], []
        for q in range(4):
            s = series_stats[q][p]
            ess.append(LD(s["T"]) if row[6 + q] else s["ess"])
            rh.append(s["split_rhat"])
        r["rhat_bulk"], r["rhat_tail"] = rh[0], rh[1]
        r["rhat"] = nan if np.isnan(rh[0]) or np.isnan(rh[1]) else max(rh[0], rh[1])
        r["ess_bulk"], r["ess_q05"], r["ess_q95"] = ess[0], ess[2], ess[3]
        r["ess_tail"] = nan if np.isnan(ess[2]) or np.isnan(ess[3]) else min(ess[2], ess[3])
    return res


def rank_diagnostics(trace, probs=(0.025, 0.5, 0.975), hdi_prob=0.94, n_lags=None, lag_block=64):
    """One dict per parameter, as Engine.rank_diagnostics returns it (statistics in long double).  Without n_lags each series'
    lags are computed `lag_block` at a time until Geyer's truncation; the statistics do not depend on lags past it."""
    x = _trace(trace)
    n, C, d = x.shape
    probs = tuple(float(v) for v in probs)
    st, series = prepare(x, probs, hdi_prob)
    per = []
    for q in range(4):
        ds = dref.diagnostics(series[q], None, 0.0, n_lags=n_lags, lag_block=lag_block)
        for s in ds:
            s["T"] = 2 * C * (n // 2)
        per.append(ds)
    res = finish(st, per)
    for p, r in enumerate(res):
        r["n_lags"] = max(per[q][p]["n_lags"] for q in range(4))
        r["median"] = st[p, 0]
        r["quantiles"] = {pr: st[p, len(STATS) + i] for i, pr in enumerate(probs)}
        r["hdi"] = (st[p, 3], st[p, 4])
    return res
