"""
Specification of the posterior predictive checks under a state law (include/rsf_law_predict.h; a test helper).  Nothing new
numerically, and nothing here calls the library: the series is tests/observe_reference.py's `forward` — the reference's own
recurrence under either law, any observable, the loading table given — and everything made of it is
tests/predictive_reference.py's `partials`, `finish` and `statistics`, tests/psis_reference.py's PSIS-LOO and
tests/predictive_noise_reference.py's band.

The end-to-end problem is tests/observe_cases.friction_problem(truth): friction data at nsteps 500 under the step history, truth
Dc = 20, noise 5 % of the friction's excursion, the box (5, 200).  `exact_draws` draws from the EXACT one-parameter posterior of
either law on that problem's 4001 quadrature nodes, pi(Dc) ~ SSq^-N/2, and sigma^2 | Dc ~ InvGamma(N / 2, SSq / 2) — the target
MCMC.sample_law samples — so the conditions of the end-to-end test can be checked on the specification alone, without a sampler.
"""
import functools

import numpy as np

import law_reference as R
import observe_cases as OC
import observe_reference as O
import predictive_noise_reference as NR
import predictive_reference as P
import psis_reference as PS


def series(m, q, vl=None, law="aging", observable="acc"):
    """y (nout, n) of the draws q (n,), (n, 1) of Dc or (n, 3) of (Dc, a, b): observe_reference.forward's, float64"""
    q = np.asarray(q, dtype=np.float64)
    q = q.reshape(-1, 1) if q.ndim < 2 else q
    ab = (q[:, 1], q[:, 2]) if q.shape[1] == 3 else (None, None)
    return np.asarray(O.forward(m, q[:, 0], vl, law, observable, a=ab[0], b=ab[1])[0], dtype=np.float64)


def default_center(m, q, std2, data, vl=None, law="aging", observable="acc"):
    """Engine.law_predictive's default centres: the series at the draws' mean point, and its log density under the mean sigma^2"""
    q = np.asarray(q, dtype=np.float64)
    q = q.reshape(-1, 1) if q.ndim < 2 else q
    cy = series(m, q.mean(0).reshape(1, -1), vl, law, observable)[:, 0]
    ms = float(np.mean(std2))
    return cy, -0.5 * np.log(2.0 * np.pi * ms) - (np.asarray(data, dtype=np.float64) - cy) ** 2 / (2.0 * ms)


def partials(m, q, std2, data, center_y, center_l, vl=None, law="aging", observable="acc"):
    return P.partials(series(m, q, vl, law, observable), std2, data, center_y, center_l)


def predictive(y, std2, data, center_y, center_l, loo=False, r_eff=1.0, noise_probs=(), psis_dtype=np.longdouble):
    """Engine.law_predictive's result from a series y (nout, n): predictive_reference.finish of its partials, with loo
    psis_reference's rows and totals, with noise_probs predictive_noise_reference's quantiles"""
    part = P.partials(y, std2, data, center_y, center_l)
    res = P.finish(part, center_y, center_l)
    res["partials"] = part
    if loo:
        rows = PS.psis_rows(y, std2, data, r_eff=r_eff, dtype=psis_dtype)
        res.update({k: np.asarray(v, dtype=np.float64) for k, v in rows.items()})
        res.update(PS.finish(rows, res["lpd"], y.shape[1]))
    if len(noise_probs):
        res["noise_quantiles"] = NR.quantiles(y, std2, noise_probs)
    return res


# ---- the end-to-end conditions ---------------------------------------------------------------------------------------------------
def coverage(data, lo, hi):
    """the share of observations inside [lo, hi], and the bound the issue sets on its distance from 0.9: 4 sqrt(0.9 0.1 / nout)"""
    data = np.asarray(data, dtype=np.float64)
    return float(np.mean((data >= lo) & (data <= hi))), 4.0 * np.sqrt(0.9 * 0.1 / data.size)


def elpd_difference(elpd_k_true, elpd_k_other):
    """(delta, se): sum of the pointwise differences elpd_loo_k(true law) - elpd_loo_k(other law) and its paired standard error
    sqrt(nout var_k(difference)), ddof 1 (the se of elpd_loo itself is formed the same way)"""
    dlt = np.asarray(elpd_k_true, dtype=np.float64) - np.asarray(elpd_k_other, dtype=np.float64)
    return float(dlt.sum()), float(np.sqrt(dlt.size * dlt.var(ddof=1)))


@functools.lru_cache(maxsize=None)
def exact_draws(truth, law, n=1024, seed=11):
    """n draws (Dc, sigma^2) from the exact posterior of `law` on friction_problem(truth)'s nodes → (q (n, 1), std2 (n,)):
    Dc by inversion of the piecewise-linear CDF of the trapezoid rule, sigma^2 = (SSq / 2) / Gamma(N / 2), SSq interpolated"""
    p = OC.friction_problem(truth)
    x = np.linspace(R.BF_BOX[0], R.BF_BOX[1], R.BF_NODES)
    ssq = np.asarray(p["ssq"][law], dtype=np.float64)
    shape = 0.5 * len(p["data"])
    ok = np.isfinite(ssq) & (ssq > 0)
    l = np.where(ok, -shape * np.log(np.where(ok, ssq, 1.0)), -np.inf)
    f = np.exp(l - l.max())
    F = np.concatenate([[0.0], np.cumsum(0.5 * (f[1:] + f[:-1]) * np.diff(x))])
    rng = np.random.default_rng([seed, R.LAWS.index(truth), R.LAWS.index(law)])
    q = np.interp(rng.uniform(0.0, 1.0, n) * F[-1], F, x)
    s = np.interp(q, x[ok], ssq[ok])
    return np.ascontiguousarray(q.reshape(n, 1)), 0.5 * s / rng.gamma(shape, 1.0, n)


@functools.lru_cache(maxsize=None)
def exact_check(truth, law, n=1024):
    """the specification's law_predictive(loo=True, noise_probs=(0.05, 0.95)) of exact_draws(truth, law) on friction_problem(truth)"""
    p = OC.friction_problem(truth)
    q, s2 = exact_draws(truth, law, n)
    y = series(p["m"], q, p["vl"], law, "mu")
    cy, cl = default_center(p["m"], q, s2, p["data"], p["vl"], law, "mu")
    res = predictive(y, s2, p["data"], cy, cl, loo=True, noise_probs=(0.05, 0.95), psis_dtype=np.float64)
    res["series"] = y
    return res
