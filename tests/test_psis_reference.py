"""
CPU tests of the PSIS-LOO specification itself (tests/psis_reference.py): the fit on tails of known shape, a model whose exact
leave-one-out predictive density is closed form, the edge rules, the totals, and the measurement that sizes the GPU test's bounds.
"""
import math

import numpy as np
import pytest

import psis_cases as cases
import psis_reference as ref

LD = np.longdouble

# The fit's own discretisation, |k_hat - (N k + 5) / (N + 10)| on exact GPD quantile tails, largest over k in {-0.3, 0.2, 0.5, 0.9}
# (attained at k = -0.3).  Measured with the long double reference: 1.04e-2 at N = 300, 1.93e-3 at N = 1536, 3.3e-4 at N = 6000:
# it falls about as 1 / N.  k_hat itself: -0.2638, 0.2145, 0.5014, 0.8840 at N = 300; -0.2929, 0.2028, 0.5003, 0.8968 at N = 1536.
DISCRETISATION = {300: 1.1e-2, 1536: 2.0e-3}


def test_fit_recovers_the_shape_of_exact_gpd_tails():
    ks = (-0.3, 0.2, 0.5, 0.9)
    worst = {}
    for N in (300, 1536):
        got = [float(ref.gpdfit(ref.gpd_quantile_tail(k, N))[0]) for k in ks]
        assert got == sorted(got), got
        disc = [abs(g - (N * k + 5.0) / (N + 10.0)) for g, k in zip(got, ks)]
        worst[N] = max(disc)
        print(f"N = {N}: k_hat {got}, discretisation {disc}")
        for g, k, dd in zip(got, ks, disc):
            assert dd <= DISCRETISATION[N]
            # the shrink of the prior term plus the discretisation (the triangle inequality of the line above)
            assert abs(g - k) <= abs(5.0 - 10.0 * k) / (N + 10.0) + DISCRETISATION[N]
    assert worst[1536] < 0.25 * worst[300]


def test_fit_is_scale_equivariant():
    t = ref.gpd_quantile_tail(0.4, 500)
    k1, s1 = ref.gpdfit(t)
    k2, s2 = ref.gpdfit(7.5 * t)
    assert abs(float(k1 - k2)) < 1e-15 and abs(float(s2 / s1) - 7.5) < 1e-14


def test_conjugate_normal_mean_model():
    """y_j ~ N(theta, sigma^2), sigma known, flat prior: theta | y ~ N(mean y, sigma^2 / J) and the exact leave-one-out predictive
    density of y_j is N(mean of the others, sigma^2 (1 + 1 / (J - 1))).  elpd_loo_k from n = 4000 exact posterior draws lies
    within |z| < 4.5 of it; the standard error is the delta method's for the self-normalised estimate p_hat = sum w_i p_i,
    sqrt(sum w_i (p_i - p_hat)^2 / weight_ess_k) / p_hat.  Measured: max |z| = 0.58 (pareto_k between 0.03 and 0.23)."""
    rng = np.random.default_rng(3)
    J, n, sig = 20, 4000, 1.3
    y = rng.normal(0.4, sig, J)
    theta = rng.normal(y.mean(), sig / np.sqrt(J), n)
    for j in range(J):
        l = -0.5 * np.log(2 * np.pi * sig ** 2) - (y[j] - theta) ** 2 / (2 * sig ** 2)
        elpd, k, n_tail, ess = ref.psis_row(l)
        w = np.exp(ref.psis_row(l, return_weights=True))
        assert abs(float(w.sum()) - 1.0) < 1e-15 and n_tail == ref.tail_len(n) and float(k) < 0.7
        p = np.exp(l.astype(LD))
        p_hat = np.sum(w * p)
        se = np.sqrt(np.sum(w * (p - p_hat) ** 2) / ess) / p_hat
        m, v = (y.sum() - y[j]) / (J - 1), sig ** 2 * (1.0 + 1.0 / (J - 1))
        exact = -0.5 * np.log(2 * np.pi * v) - (y[j] - m) ** 2 / (2 * v)
        z = float((elpd - exact) / se)
        print(f"y_{j}: elpd_loo {float(elpd):.5f}, exact {exact:.5f}, pareto_k {float(k):.3f}, weight_ess {float(ess):.0f}, z {z:+.2f}")
        assert abs(z) < 4.5


def _plain_importance_sampling(l):
    """elpd and ESS of the raw ratios 1 / p_i: the harmonic mean, what a row that is not smoothed must give."""
    l = np.asarray(l, dtype=LD)
    x = -l - (-l).max()
    lw = x - np.log(np.sum(np.exp(x)))
    return np.log(np.sum(np.exp(lw + l))), 1 / np.sum(np.exp(2 * lw))


def _rows(name):
    (series, r_eff), = [(s, r) for nm, s, r in cases.crafted() if nm == name]
    n = series.shape[1]
    return series, ref.psis_rows(series, np.full(n, cases.STD2), np.zeros(series.shape[0]), r_eff), r_eff


def test_at_most_four_tail_members_are_not_smoothed():
    for name, n_tails in (("n1", (0, 0)), ("n5", (1, 1)), ("all_equal", (0, 1))):
        series, rows, _ = _rows(name)
        n = series.shape[1]
        assert tuple(rows["n_tail"]) == n_tails
        assert np.all(np.isposinf(rows["pareto_k"].astype(np.float64)))
        for k in range(series.shape[0]):
            e, ess = _plain_importance_sampling(ref.loglik_row(series[k], np.full(n, cases.STD2), 0.0))
            assert abs(float(rows["elpd_loo_k"][k] - e)) < 1e-17 * n + 1e-18 and abs(float(rows["weight_ess"][k] / ess) - 1) < 1e-17
    # an all-equal row: every weight 1 / n
    series, rows, _ = _rows("all_equal")
    assert abs(float(rows["weight_ess"][0]) - series.shape[1]) < 1e-12
    assert abs(float(rows["elpd_loo_k"][0]) - float(ref.loglik_row(series[0, :1], [cases.STD2], 0.0)[0])) < 1e-15
    # n = 25: tail_len = 5, the smallest tail that is fitted
    _, rows, _ = _rows("n25")
    assert tuple(rows["n_tail"]) == (5, 5) and np.isfinite(rows["pareto_k"].astype(np.float64)).all()


def test_ties_at_the_cutoff_stay_out_and_their_order_is_immaterial():
    series, rows, _ = _rows("repeats")
    assert ref.tail_len(series.shape[1]) == 195 and tuple(rows["n_tail"]) == (182, 182)
    for name in ("elpd_loo_k", "pareto_k", "weight_ess"):  # the sorted pool and the shuffled one: sums in another order only
        assert abs(float(rows[name][0] - rows[name][1])) <= 1e-16 * abs(float(rows[name][0])), name


def test_cutoff_is_clamped_at_log_dbl_min():
    series, rows, _ = _rows("clamped_cutoff")
    n = series.shape[1]
    x = -ref.loglik_row(series[0], np.full(n, cases.STD2), 0.0)
    assert float(np.sort(x - x.max())[n - ref.tail_len(n) - 1]) < ref.LOG_DBL_MIN - 500.0  # the order statistic is far below it
    assert ref.tail_len(n) == 95 and tuple(rows["n_tail"]) == (50, 50)  # unclamped, all 95 above x_(904) would be the tail
    assert np.isfinite(rows["elpd_loo_k"].astype(np.float64)).all()


def test_r_eff_sets_the_tail_length():
    series, rows, r_eff = _rows("r_eff")
    assert ref.tail_len(4099) == 193 and ref.tail_len(4099, r_eff) == 316 and tuple(rows["n_tail"]) == (316, 316)
    _, rows, r_eff = _rows("long_tail")
    assert tuple(rows["n_tail"]) == (6000,) and ref.tail_len(4194304) == 6144 <= ref.MAX_TAIL


def test_heavy_tails_are_ranked():
    _, rows, _ = _rows("heavy_tail")
    k = rows["pareto_k"].astype(np.float64)
    assert k[0] < k[1] < k[2] and abs(k[0] - 0.2) < 0.15 and abs(k[1] - 0.5) < 0.15 and abs(k[2] - 0.9) < 0.3


def test_totals():
    rows = {"elpd_loo_k": np.array([-1.0, -2.0, -4.0]), "pareto_k": np.array([0.1, np.inf, 0.69])}
    lpd = np.array([-0.5, -1.5, -3.0])
    tot = ref.finish(rows, lpd, 100000)
    assert tot["elpd_loo"] == -7.0 and tot["p_loo"] == 2.0 and tot["k_threshold"] == 0.7
    assert tot["elpd_loo_se"] == pytest.approx(math.sqrt(3 * np.var([-1.0, -2.0, -4.0], ddof=1)))
    assert tot["n_high_k"] == 1 and tot["max_pareto_k"] == np.inf
    assert ref.finish(rows, lpd, 1000)["k_threshold"] == pytest.approx(1 - 1 / 3) and ref.finish(rows, lpd, 1000)["n_high_k"] == 2
    rows["elpd_loo_k"][1] = rows["pareto_k"][1] = np.nan
    tot = ref.finish(rows, lpd, 1000)
    assert all(np.isnan(tot[name]) for name in ref.TOTALS if name != "k_threshold")


def test_float64_distance_sizes_the_bounds(pkg, cpu_engine):
    """The reference in plain float64 NumPy against long double, on the inputs of tests/test_gpu_psis.py (the real draws' series
    from the CPU restatement): n_tail equal, and the distances recorded in psis_cases.py — 8 x those are the GPU test's bounds.
    NumPy's float64 element functions differ in the last bit between builds, so the re-measurement is held to twice the record."""
    worst = [0.0, 0.0]
    inputs = [(name, s, np.full(s.shape[1], cases.STD2), np.zeros(s.shape[0]), r) for name, s, r in cases.crafted()]
    for d, n in cases.REAL:
        _, q, std2, data = cases.real_draws(pkg, cpu_engine, n, d, 400 + d + n)
        inputs.append((f"real d={d} n={n}", cases.restatement_series(cpu_engine, q), std2, data, 1.0))
    for name, series, std2, data, r_eff in inputs:
        a, b = ref.psis_rows(series, std2, data, r_eff, LD), ref.psis_rows(series, std2, data, r_eff, np.float64)
        np.testing.assert_array_equal(a["n_tail"], b["n_tail"])
        fin = np.isfinite(a["pareto_k"].astype(np.float64))
        np.testing.assert_array_equal(fin, np.isfinite(b["pareto_k"]))
        e = float((np.abs(b["elpd_loo_k"] - a["elpd_loo_k"]) / np.maximum(np.abs(a["elpd_loo_k"]), 1)).max())
        s = float((np.abs(b["weight_ess"] - a["weight_ess"]) / np.abs(a["weight_ess"])).max())
        k = float(np.abs(b["pareto_k"][fin] - a["pareto_k"][fin]).max()) if fin.any() else 0.0
        print(f"{name}: elpd_loo_k {e:.3e} (scaled), weight_ess {s:.3e} (relative), pareto_k {k:.3e} (absolute)")
        worst = [max(worst[0], e, s), max(worst[1], k)]
    print(f"largest: scaled {worst[0]:.4e}, pareto_k {worst[1]:.4e}")
    assert worst[0] <= 2 * cases.DIST_SCALED and worst[1] <= 2 * cases.DIST_K
    assert cases.TOL_SCALED == 8 * cases.DIST_SCALED and cases.TOL_K == 8 * cases.DIST_K
