"""
CPU tests of the specification of the posterior predictive checks under a state law (tests/law_predictive_reference.py): the
composition — observe_reference.forward's series through predictive_reference.partials and finish — agrees with the definitions
taken straight from the series, and the conditions of the end-to-end GPU test (tests/test_gpu_law_predictive.py, test 9) hold
for the specification alone, on draws from the exact posterior.  No GPU, no library.
"""
import numpy as np
import pytest

import law_cases as C
import law_predictive_reference as LP
import law_reference as R
import observe_cases as OC
import observe_reference as O
import predictive_reference as P


def _draws(n, d, seed):
    rng = np.random.default_rng(seed)
    q = np.column_stack([rng.uniform(15.0, 25.0, n), rng.uniform(0.0105, 0.0115, n), rng.uniform(0.0135, 0.0145, n)])[:, :d]
    return np.ascontiguousarray(q), rng


@pytest.mark.parametrize("observable", O.OBSERVABLES)
@pytest.mark.parametrize("law", R.LAWS)
def test_composition_agrees_with_the_definitions(law, observable):
    m = C.spec()
    vl = R.table(m, "step")
    for d in (1, 3):
        q, rng = _draws(37, d, [d, R.LAWS.index(law)])
        y = LP.series(m, q, vl, law, observable)
        assert y.shape == (R.nout(m), 37) and np.isfinite(y).all()
        # the series is forward's, lane for lane, and its sample 0 the observable's initial value
        one = O.forward(m, q[5:6, 0], vl, law, observable, a=q[5:6, 1] if d == 3 else None, b=q[5:6, 2] if d == 3 else None)[0][:, 0]
        np.testing.assert_array_equal(y[:, 5], one)
        first = {"acc": 0.0, "velocity": m.V_ref, "mu": m.mu_t_zero}
        np.testing.assert_array_equal(y[0], q[:, 0] / m.V_ref if observable == "theta" else first[observable])
        amp = np.abs(y - y[0]).max()
        data = y[:, 0] + 0.05 * amp * rng.standard_normal(y.shape[0])
        std2 = (rng.uniform(0.03, 0.1, 37) * amp) ** 2
        cy, cl = LP.default_center(m, q, std2, data, vl, law, observable)
        part = LP.partials(m, q, std2, data, cy, cl, vl, law, observable)
        np.testing.assert_array_equal(part, P.partials(y, std2, data, cy, cl))
        got, want = P.finish(part, cy, cl), P.statistics(y, std2, data)
        for name in P.OUT:
            np.testing.assert_allclose(got[name], want[name], rtol=1e-9, atol=1e-12 * np.abs(want[name]).max(), err_msg=name)
        for name in P.TOTALS:
            assert got[name] == pytest.approx(want[name], rel=1e-9), name
        res = LP.predictive(y, std2, data, cy, cl)
        np.testing.assert_array_equal(res["partials"], part)
        assert set(P.OUT) | set(P.TOTALS) <= set(res)


def test_shards_add_and_a_nonfinite_draw_is_counted():
    m = C.spec()
    vl = R.table(m, "step")
    q, rng = _draws(20, 1, 3)
    q[7, 0] = 0.2  # the plain RK4 of this Dc is not finite
    y = LP.series(m, q, vl, "aging", "mu")
    bad = ~np.isfinite(y[:, 7])
    assert bad.any() and not bad[0] and np.isfinite(np.delete(y, 7, axis=1)).all()
    data, std2 = y[:, 0] + 1e-3 * rng.standard_normal(y.shape[0]), np.full(20, 1e-6)
    cy, cl = LP.default_center(m, q[:7], std2[:7], data, vl, "aging", "mu")
    whole = P.partials(y, std2, data, cy, cl)
    np.testing.assert_array_equal(whole[P.HEAD:].reshape(-1, P.FIELDS)[:, 6], bad.astype(float))
    halves = P.partials(y[:, :9], std2[:9], data, cy, cl) + P.partials(y[:, 9:], std2[9:], data, cy, cl)
    assert (np.abs(halves - whole) / P.scales(whole)).max() < 1e-14
    res = P.finish(whole, cy, cl)
    for name in P.OUT:
        assert np.isnan(res[name][bad]).all() and np.isfinite(res[name][~bad]).all(), name
    assert np.isnan(res["elpd_waic"])


@pytest.mark.parametrize("truth", R.LAWS)
def test_end_to_end_conditions_hold_for_the_specification(truth):
    """Test 9's conditions on 1024 draws from the exact posterior of either law (law_predictive_reference.exact_draws).
    Measured: coverage of the 90 % noise band under the true law 0.906 (ageing) and 0.908 (slip), bound 0.9 +- 0.0537;
    n_high_k 0 in all four fits, the largest Pareto k 0.31; delta elpd_loo 676.0 (paired se 32.1, ratio 21.1) with the ageing
    law true and 667.0 (se 24.2, ratio 27.5) with the slip law true — the log Bayes factors of the same data are -672.5 and +664.7."""
    p = OC.friction_problem(truth)
    other = [law for law in R.LAWS if law != truth][0]
    fit = {law: LP.exact_check(truth, law) for law in R.LAWS}
    cov, bound = LP.coverage(p["data"], fit[truth]["noise_quantiles"][0], fit[truth]["noise_quantiles"][1])
    delta, se = LP.elpd_difference(fit[truth]["elpd_loo_k"], fit[other]["elpd_loo_k"])
    print(f"truth {truth}: coverage {cov:.4f} (0.9 +- {bound:.4f}), n_high_k {fit[truth]['n_high_k']:.0f}, max k {fit[truth]['max_pareto_k']:.3f}, "
          f"delta elpd_loo {delta:.2f}, paired se {se:.2f}, ratio {delta / se:.2f}; log Bayes factor {p['log_bayes_factor']:+.1f}")
    assert abs(cov - 0.9) <= bound
    assert fit[truth]["n_high_k"] == 0
    assert delta > 4.0 * se
    # the two answers to "which law" agree in sign and in size: elpd_loo differs from the log evidence by the prior's share only
    assert abs(delta - abs(p["log_bayes_factor"])) < 4.0 * se
    # the credible quantities are the posterior's: the series' mean lies within the noise of the data
    assert np.abs(fit[truth]["mean"] - p["data"]).max() < 6.0 * np.sqrt(fit[truth]["mean_std2"])
