"""
GPU tests of the posterior predictive checks under either state law and any observable (include/rsf_law_predict.h:
rsf_law_predict_partials / rsf_predict_series_partials; Engine.law_predictive_partials / series_partials / law_predictive;
PosteriorPool.law_predictive / law_loo):
  1. the series is rsf_law_observe's, bit for bit, with the partials the same bits with and without it, host or device memory;
  2. the fused kernel equals the split path (law_observe's series through series_partials), bit for bit;
  3. series_partials of the series rsf_predict_partials leaves equals that call's partials, bit for bit;
  4. the partials and the finished statistics against the specification;
  5. the quantiles are np.quantile of the returned series; the PSIS-LOO and noise-band entries are the series entry points';
  6. shards add;
  7. a draw whose trajectory is not finite;
  8. the refusals through ctypes;
  9. end to end on friction data: the noise band's coverage, the Pareto k, and delta elpd_loo between the laws.
The model is law_cases.spec() at nsteps 500 (500 output samples: 62 tiles of 8 and a remainder of 4); the draws are
default_rng uniform in [15, 25] x [0.0105, 0.0115] x [0.0135, 0.0145], the starts of tests/test_gpu_law_dr.py.

Tests 4 and 9 measure the REDUCTION and the element functions, as tests/test_gpu_predictive.py does: the
specification's sums (tests/predictive_reference.py, exact fsum) are evaluated on the series the kernel returned, which test 1
ties bit for bit to rsf_law_observe, whose own distance from the long-double solve is tests/test_gpu_observe.py's subject.
"""
import numpy as np
import pytest

import law_cases as C
import law_predictive_reference as LP
import law_reference as R
import observe_cases as OC
import observe_reference as O
import predictive_reference as P

pytestmark = pytest.mark.gpu

TOL = 1e-12      # DESIGN 4c's bound on the partials and the finished rows, scaled (predictive_reference.scales)
TOL_TOTALS = 1e-11
PAIRS = (("aging", "mu"), ("slip", "mu"), ("slip", "acc"), ("aging", "theta"), ("slip", "velocity"), ("aging", "acc"))


def _model(pkg, nsteps=500, substeps=1, history="step", **attrs):
    m = pkg.RateStateModel(number_time_steps=nsteps)
    m.substeps = substeps
    if history == "step":
        m.loading = R.step_history
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _bits(x):
    x = np.ascontiguousarray(np.asarray(x.cpu() if hasattr(x, "cpu") else x, dtype=np.float64))
    return x.view(np.int64)


def _draws(d, n, seed=7):
    rng = np.random.default_rng([seed, d, n])
    q = np.column_stack([rng.uniform(15.0, 25.0, n), rng.uniform(0.0105, 0.0115, n), rng.uniform(0.0135, 0.0145, n)])[:, :d]
    return np.ascontiguousarray(q), rng


def _observe(eng, law, obs, q):
    """law_observe's series (nout, n) of the draws, in the engine's memory space"""
    d = q.shape[1]
    ab = [np.ascontiguousarray(q[:, p]) for p in (1, 2)] if d == 3 else [None, None]
    return eng.law_observe(law, obs, np.ascontiguousarray(q[:, 0]), ab[0], ab[1])[1]


def _problem(eng, law, obs, d, n):
    """draws, noise variances, data and centres for the model set on `eng`: the data the series of the box's midpoint plus noise of
    5 % of its excursion; the centres the series of ANOTHER point moved by a tenth of the excursion.  Not the draws' mean: with
    n = 1 that is the draw itself, and y - c_y, l - c_l would be differences of two roundings, which no scale describes.  And
    moved, because under the step history the acceleration and the velocity do not depend on the parameters before the step:
    there every point's series is the same to an ulp, and l - c_l of a single draw would again be such a difference."""
    q, rng = _draws(d, n)
    truth = np.asarray(_observe(eng, law, obs, np.array([[20.0, 0.011, 0.014]])[:, :d]))[:, 0]
    amp = np.abs(truth - truth[0]).max()
    data = truth + 0.05 * amp * rng.standard_normal(truth.size)
    std2 = (rng.uniform(0.05, 0.2, n) * amp) ** 2
    cy = np.asarray(_observe(eng, law, obs, np.array([[21.0, 0.0112, 0.0142]])[:, :d]))[:, 0] + 0.1 * amp
    cl = P.loglik(cy[:, None], [std2.mean()], data)[:, 0]
    assert np.isfinite(truth).all() and np.isfinite(cy).all()
    return q, std2, data, cy, cl


def _scaled(got, want):
    return float((np.abs(np.asarray(got) - want) / P.scales(want)).max())


def _finish_errors(got, part_ref, cy, cl):
    """tests/test_gpu_predictive.py's measure: the largest scaled error of the finished rows and of the totals against the
    specification's finish of the specification's partials; a finished statistic inherits the scale of the partials it is made of"""
    want = P.finish(part_ref, cy, cl)
    n = part_ref[0]
    rows = part_ref[P.HEAD:].reshape(-1, P.FIELDS)
    sc = {"mean": np.maximum(np.abs(want["mean"]), np.sqrt(rows[:, 1] / n)), "var": np.maximum(np.abs(want["var"]), rows[:, 1] / n),
          "pit": np.abs(want["pit"]), "lpd": np.maximum(np.abs(want["lpd"]), 1.0), "p_waic_k": np.maximum(np.abs(want["p_waic_k"]), rows[:, 3] / n)}
    ok = np.isfinite(want["lpd"])
    worst_row = 0.0
    for name in P.OUT:
        np.testing.assert_array_equal(np.isnan(got[name]), np.isnan(want[name]), err_msg=name)
        both = ok & np.isfinite(want[name])
        if both.any():
            worst_row = max(worst_row, float((np.abs(got[name][both] - want[name][both]) / np.maximum(sc[name][both], 1e-300)).max()))
    worst_tot = 0.0
    if ok.all() and n > 1:
        tsc = {"mean_std2": abs(want["mean_std2"]), "elpd_waic": (sc["lpd"] + sc["p_waic_k"]).sum(), "p_waic": sc["p_waic_k"].sum(),
               "elpd_waic_se": abs(want["elpd_waic_se"])}
        for name in P.TOTALS:
            worst_tot = max(worst_tot, abs(got[name] - want[name]) / tsc[name])
    elif not ok.all():
        for name in ("elpd_waic", "p_waic", "elpd_waic_se"):
            assert np.isnan(got[name]), name
    return worst_row, worst_tot


# ---- 1. the series is rsf_law_observe's ----------------------------------------------------------------------------------------
def _series_is_observe(eng, law, obs, d, n, tag):
    q, std2, data, cy, cl = _problem(eng, law, obs, d, n)
    want = _observe(eng, law, obs, q)
    part, series = eng.law_predictive_partials(law, obs, q, std2, data, cy, cl, return_series=True)
    assert tuple(series.shape) == (eng.nout, n), tag
    assert np.array_equal(_bits(series), _bits(want)), (tag, law, obs, d, n)
    alone = eng.law_predictive_partials(law, obs, q, std2, data, cy, cl)
    assert np.array_equal(_bits(alone), _bits(part)), (tag, law, obs, d, n)
    assert part[0] == n and not np.isnan(part).any(), tag  # (a sum of exp(l - c_l) may overflow: the centres are not the draws')
    return q, std2, data, cy, cl, part


def _non_default():
    """tests/golden/forward_nondefault.json's V_ref, mu_ref, mu_t_zero and k1, the step history as a table in the model's units"""
    attrs = dict(V_ref=1.7, mu_ref=0.55, mu_t_zero=0.58, k1=3e-7)
    return dict(attrs, loading=R.table(C.spec(**attrs), "step"))


@pytest.mark.parametrize("obs", O.OBSERVABLES)
@pytest.mark.parametrize("law", R.LAWS)
def test_series_is_law_observe_bit_for_bit(pkg, law, obs):
    kept = {}
    with pkg.Engine(mem="host") as eng:
        for tag, attrs in (("damped", {}), ("k1 = 0", dict(k1=0.0)), ("undamped", dict(RadiationDamping=False)), ("built-in loading", dict(history=None)),
                           ("non-default", _non_default())):
            eng.set_model(_model(pkg, **attrs), 1)
            for d in (1, 3):
                for n in (1, 63, 65):
                    res = _series_is_observe(eng, law, obs, d, n, tag)
                    if tag == "damped" and n == 65:
                        kept[d] = res
        # the table in more than one chunk of the kernel's own chunking (kPredTableBudget: 4863 doubles, 607 output samples at substeps 4)
        eng.set_model(_model(pkg, 900, 4), 4)
        assert 2 * 4 * (eng.nout - 1) + 1 > 38 * 1024 // 8
        for d in (1, 3):
            _series_is_observe(eng, law, obs, d, 65, "two chunks")
    with pkg.Engine(mem="host", block_threads=64) as eng:
        eng.set_model(_model(pkg), 1)
        for d in (1, 3):
            _series_is_observe(eng, law, obs, d, 133, "workgroups of one wave")
    # device memory: the same bits
    with pkg.Engine(mem="device") as eng:
        eng.set_model(_model(pkg), 1)
        for d in (1, 3):
            q, std2, data, cy, cl, want = kept[d]
            part, series = eng.law_predictive_partials(law, obs, q, std2, data, cy, cl, return_series=True)
            assert np.array_equal(_bits(part), _bits(want)), (law, obs, d)
            assert np.array_equal(_bits(series), _bits(_observe(eng, law, obs, q))), (law, obs, d)
            assert np.array_equal(_bits(eng.law_predictive_partials(law, obs, q, std2, data, cy, cl)), _bits(want)), (law, obs, d)


# ---- 2. fused equals split -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law,obs", PAIRS)
def test_fused_equals_split_bit_for_bit(pkg, law, obs):
    with pkg.Engine(mem="host") as eng:
        for tag, model, sizes in (("resident", _model(pkg), (1, 63, 65, 4161)), ("undamped", _model(pkg, RadiationDamping=False), (65,)),
                                  ("two chunks", _model(pkg, 900, 4), (65,))):
            eng.set_model(model, model.substeps)
            for d in (1, 3):
                for n in sizes:
                    q, std2, data, cy, cl = _problem(eng, law, obs, d, n)
                    fused = eng.law_predictive_partials(law, obs, q, std2, data, cy, cl)
                    split = eng.series_partials(_observe(eng, law, obs, q), std2, data, cy, cl)
                    assert fused.shape == split.shape == (P.HEAD + eng.nout * P.FIELDS,)
                    assert np.array_equal(_bits(fused), _bits(split)), (tag, law, obs, d, n)
    with pkg.Engine(mem="host", block_threads=64) as eng:
        eng.set_model(_model(pkg), 1)
        q, std2, data, cy, cl = _problem(eng, law, obs, 3, 133)
        assert np.array_equal(_bits(eng.law_predictive_partials(law, obs, q, std2, data, cy, cl)),
                              _bits(eng.series_partials(_observe(eng, law, obs, q), std2, data, cy, cl)))


# ---- 3. the series kernel equals the existing code -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 4161])
@pytest.mark.parametrize("d", [1, 3])
def test_series_partials_equals_predict_partials_bit_for_bit(pkg, gpu_engine, d, n):
    """rsf_predict_partials (the ageing model, the acceleration, the tier code) leaves a series; series_partials of it is that
    call's partials: the new reduction is pinned to code already tested against the CPU restatement"""
    eng = gpu_engine
    eng.set_model(pkg.RateStateModel(number_time_steps=500), 1)
    rng = np.random.default_rng([3, d, n])
    q = np.ascontiguousarray(np.column_stack([rng.uniform(600.0, 1600.0, n), rng.uniform(0.009, 0.013, n), rng.uniform(0.013, 0.017, n)])[:, :d])
    mid = np.array([[1100.0, 0.011, 0.015]])[:, :d]
    cy = np.asarray(eng.forward(mid[:, 0], a=mid[:, 1] if d == 3 else None, b=mid[:, 2] if d == 3 else None)[1])[:, 0]
    amp = np.abs(cy).max()
    data = cy + 0.05 * amp * rng.standard_normal(cy.size)
    std2 = (rng.uniform(0.05, 0.3, n) * amp) ** 2
    cl = P.loglik(cy[:, None], [std2.mean()], data)[:, 0]
    part, series = eng.predictive_partials(q, std2, data, cy, cl, return_series=True)
    assert np.isfinite(part).all()
    assert np.array_equal(_bits(eng.series_partials(series, std2, data, cy, cl)), _bits(part)), (d, n)


# ---- 4. against the specification ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law,obs", PAIRS[:5])
def test_partials_and_finished_statistics_against_the_specification(pkg, gpu_engine, law, obs):
    """Measured on an MI355X when this was written: see DESIGN 4q."""
    eng = gpu_engine
    eng.set_model(_model(pkg), 1)
    for d, n in ((1, 1), (3, 65), (1, 1037), (3, 1037)):
        q, std2, data, cy, cl = _problem(eng, law, obs, d, n)
        part, series = eng.law_predictive_partials(law, obs, q, std2, data, cy, cl, return_series=True)
        want = P.partials(np.asarray(series), std2, data, cy, cl)
        err = _scaled(part, want)
        rows, tot = _finish_errors(eng.predictive_finish(part, cy, cl), want, cy, cl)
        print(f"{law} {obs} d={d} n={n}: partials' scaled error {err:.3e}; finished rows {rows:.3e}, totals {tot:.3e}")
        assert err <= TOL
        assert rows <= TOL and tot <= TOL_TOTALS


# ---- 5. the composition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law,obs,d", [("slip", "mu", 3), ("aging", "velocity", 1)])
def test_law_predictive_composes_the_series_entry_points(pkg, gpu_engine, law, obs, d):
    eng = gpu_engine
    eng.set_model(_model(pkg), 1)
    q, std2, data, _, _ = _problem(eng, law, obs, d, 1037)
    probs, noise = (0.0, 0.05, 0.5, 0.95, 1.0, 1.0 / np.pi), (0.05, 0.5, 0.95)
    res = eng.law_predictive(law, obs, q, std2, data, probs=probs, return_series=True, loo=True, r_eff=0.7, noise_probs=noise)
    series = np.asarray(res["series"])
    assert np.array_equal(_bits(series), _bits(_observe(eng, law, obs, q)))
    np.testing.assert_array_equal(res["quantiles"], np.quantile(series, probs, axis=1))
    loo = eng.psis_loo(res["series"], std2, data, res["lpd"], r_eff=0.7)
    for name in pkg._abi.PSIS_OUT + pkg._abi.PSIS_TOTALS:
        assert np.array_equal(_bits(res[name]), _bits(loo[name])), name
    assert np.array_equal(_bits(res["noise_quantiles"]), _bits(eng.predictive_noise_quantiles(res["series"], std2, noise)))
    # the default centres: one law_observe call at the draws' mean point, the log density under the mean sigma^2
    cy = np.asarray(_observe(eng, law, obs, q.mean(0).reshape(1, d)))[:, 0]
    assert np.array_equal(_bits(res["center_y"]), _bits(cy))
    np.testing.assert_array_equal(res["center_l"], -0.5 * np.log(2.0 * np.pi * std2.mean()) - (data - cy) ** 2 / (2.0 * std2.mean()))
    assert np.array_equal(_bits(res["partials"]), _bits(eng.series_partials(res["series"], std2, data, res["center_y"], res["center_l"])))
    # and the statistics are the definitions' on that series
    want = P.statistics(series, std2, data)
    for name in P.OUT:
        np.testing.assert_allclose(res[name], want[name], rtol=1e-9, atol=1e-12 * np.abs(want[name]).max(), err_msg=name)
    for name in P.TOTALS:
        assert res[name] == pytest.approx(want[name], rel=1e-9), name
    assert res["n"] == 1037 and res["n_high_k"] >= 0
    # without the extras the result has predictive's keys and no more
    plain = eng.law_predictive(law, obs, q, std2, data)
    assert set(plain) == set(P.OUT) | set(P.TOTALS) | {"n", "partials", "center_y", "center_l"}
    assert np.array_equal(_bits(plain["partials"]), _bits(res["partials"]))


# ---- 6. shards add -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law,obs,d", [("slip", "mu", 1), ("aging", "theta", 3)])
def test_partials_of_shards_add(pkg, gpu_engine, law, obs, d):
    eng = gpu_engine
    eng.set_model(_model(pkg), 1)
    q, std2, data, cy, cl = _problem(eng, law, obs, d, 1037)
    whole = eng.law_predictive_partials(law, obs, q, std2, data, cy, cl)
    halves = eng.law_predictive_partials(law, obs, q[:500], std2[:500], data, cy, cl) + eng.law_predictive_partials(law, obs, q[500:], std2[500:], data, cy, cl)
    err = _scaled(halves, whole)
    print(f"{law} {obs} d={d}: two shards against the whole, scaled {err:.3e}")
    assert err <= TOL
    assert halves[0] == 1037


# ---- 7. a draw that is not finite ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", R.LAWS)
def test_a_nonfinite_draw(pkg, gpu_engine, law):
    """Dc = 0.2: observe_reference.forward's plain RK4 of it is not finite under either law, and neither is the kernel's, which
    runs the trajectory to its end.  The rows it spoils and the totals are NaN, the other rows the specification's, the count exact."""
    spec = LP.series(C.spec(), np.array([[0.2]]), R.table(C.spec(), "step"), law, "mu")[:, 0]
    assert not np.isfinite(spec).all() and np.isfinite(spec[0])
    eng = gpu_engine
    eng.set_model(_model(pkg), 1)
    q, std2, data, cy, cl = _problem(eng, law, "mu", 1, 133)
    q[70, 0] = 0.2
    part, series = eng.law_predictive_partials(law, "mu", q, std2, data, cy, cl, return_series=True)
    series = np.asarray(series)
    bad = ~np.isfinite(series[:, 70])
    print(f"{law}: first row that is not finite: kernel {int(np.argmax(bad))}, specification {int(np.argmax(~np.isfinite(spec)))}; {int(bad.sum())} rows")
    assert bad.any() and not bad[0] and np.isfinite(np.delete(series, 70, axis=1)).all()
    np.testing.assert_array_equal(part[P.HEAD:].reshape(-1, P.FIELDS)[:, 6], bad.astype(np.float64))
    want = P.partials(series, std2, data, cy, cl)
    assert _scaled(part, want) <= TOL
    res = eng.predictive_finish(part, cy, cl)
    rows, _ = _finish_errors(res, want, cy, cl)
    assert rows <= TOL
    for name in P.OUT:
        assert np.isnan(res[name][bad]).all() and np.isfinite(res[name][~bad]).all(), name
    # the split path counts the same, and a NaN put into a series by hand is counted where it is
    assert np.array_equal(_bits(eng.series_partials(series, std2, data, cy, cl)), _bits(part))
    series[3, 5], series[499, 132] = np.nan, np.inf
    got = eng.series_partials(series, std2, data, cy, cl)[P.HEAD:].reshape(-1, P.FIELDS)[:, 6]
    np.testing.assert_array_equal(got, bad.astype(np.float64) + (np.arange(500) == 3) + (np.arange(500) == 499))


# ---- 8. the refusals through ctypes ----------------------------------------------------------------------------------------------
def test_refusals(pkg):
    P_ = lambda x: x.ctypes.data
    dp = lambda x: x.ctypes.data_as(pkg._abi._DP)
    with pkg.Engine(mem="host", block_threads=64) as eng:
        lib, ctx = eng.lib, eng._ctx
        n, nout = 128, 500
        q, q3, s2, data, c = np.full(n, 1000.0), np.tile([1000.0, 0.011, 0.014], (n, 1)), np.ones(n), np.zeros(nout), np.zeros(nout)
        part, series = np.zeros(P.HEAD + nout * P.FIELDS), np.zeros((nout, n))
        fused = lambda law=1, obs=1, n=n, d=1: [ctx, law, obs, n, d, P_(q3 if d == 3 else q), P_(s2), P_(data), dp(c), dp(c), dp(part), P_(series)]
        split = lambda n=n, nout=nout: [ctx, n, nout, P_(series), P_(s2), P_(data), dp(c), dp(c), dp(part)]
        # no model: the fused entry needs one, the series entry does not
        assert lib.rsf_law_predict_partials(*fused()) == -3 and b"rsf_law_predict_partials" in lib.rsf_last_error()
        assert lib.rsf_predict_series_partials(*split()) == 0
        eng.set_model(pkg.RateStateModel(number_time_steps=500), 1)
        assert eng.nout == nout
        ok = fused()
        assert lib.rsf_law_predict_partials(*ok) == 0 and lib.rsf_law_predict_partials(*fused(d=3)) == 0 and part[0] == n
        # the law and the observable: rsf_law_observe's messages under this function's name
        for law in (-1, 2, 7):
            assert lib.rsf_law_predict_partials(*fused(law=law)) == -1 and b"rsf_law_predict_partials: law is RSF_LAW_AGEING" in lib.rsf_last_error()
        for obs in (-1, 4):
            assert lib.rsf_law_predict_partials(*fused(obs=obs)) == -1 and b"rsf_law_predict_partials: observable is RSF_OBS_ACC" in lib.rsf_last_error()
        # rsf_predict_partials' argument errors
        for d in (0, 2, 4):
            assert lib.rsf_law_predict_partials(*fused(d=d)) == -1 and b"rsf_law_predict_partials: need n >= 1 and d = 1 or 3" in lib.rsf_last_error()
        for bad_n in (0, -5):
            assert lib.rsf_law_predict_partials(*fused(n=bad_n)) == -1 and b"rsf_law_predict_partials" in lib.rsf_last_error()
        for i in (5, 6, 7, 8, 9, 10):
            bad = list(ok)
            bad[i] = None
            assert lib.rsf_law_predict_partials(*bad) == -1 and b"rsf_law_predict_partials: NULL argument" in lib.rsf_last_error(), i
        assert lib.rsf_law_predict_partials(None, *ok[1:]) == -1 and b"rsf_law_predict_partials" in lib.rsf_last_error()
        no_series = list(ok)
        no_series[11] = None
        assert lib.rsf_law_predict_partials(*no_series) == 0
        # the series entry's own checks
        for kw in (dict(n=0), dict(n=-1), dict(nout=0), dict(nout=-3), dict(n=2 ** 31), dict(n=2 ** 30, nout=2 ** 30)):
            assert lib.rsf_predict_series_partials(*split(**kw)) == -1 and b"rsf_predict_series_partials" in lib.rsf_last_error(), kw
        for i in range(3, 9):
            bad = split()
            bad[i] = None
            assert lib.rsf_predict_series_partials(*bad) == -1 and b"rsf_predict_series_partials: NULL argument" in lib.rsf_last_error(), i
        assert lib.rsf_predict_series_partials(None, *split()[1:]) == -1
        # the DOP853 flag: refused, the series entry serves its series
        m = pkg.RateStateModel(number_time_steps=500)
        m.integrator = "dop853"
        eng.set_model(m, 1)
        assert lib.rsf_law_predict_partials(*ok) == -5 and b"rsf_law_predict_partials: a model flagged RSF_FLAG_DOP853" in lib.rsf_last_error()
        acc = np.ascontiguousarray(eng.forward(q)[1])
        assert lib.rsf_predict_series_partials(ctx, n, nout, P_(acc), P_(s2), P_(data), dp(c), dp(c), dp(part)) == 0 and part[0] == n
        # the float32 flag runs the float64 solve
        m = pkg.RateStateModel(number_time_steps=500)
        m.precision = "float32"
        eng.set_model(m, 1)
        got = np.zeros_like(part)
        assert lib.rsf_law_predict_partials(*(ok[:10] + [dp(got), None])) == 0
        eng.set_model(pkg.RateStateModel(number_time_steps=500), 1)
        assert lib.rsf_law_predict_partials(*no_series) == 0 and np.array_equal(_bits(got), _bits(part))


# ---- 9. end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("truth", R.LAWS)
def test_end_to_end_on_friction_data(pkg, truth):
    """observe_cases.friction_problem(truth) fitted under both laws by MCMC.sample_law(256, 200, nburn=96, seed=9), then
    PosteriorPool.law_predictive(model, data, noise_probs=(0.05, 0.95), loo=True).  Conditions (each met by the CPU specification
    alone on draws from the exact posterior, tests/test_law_predictive_reference.py: coverage 0.906 / 0.908, n_high_k 0, delta
    elpd_loo 676 / 667 at 21 / 27 paired standard errors): the share of observations inside the 90 % noise band within
    4 sqrt(0.9 0.1 / nout) of 0.9; n_high_k = 0 under the true law; delta elpd_loo favours the true law by more than 4 paired se."""
    p = OC.friction_problem(truth)
    other = [law for law in R.LAWS if law != truth][0]
    res, pools, models = {}, {}, {}
    for law in R.LAWS:
        model = _model(pkg, observable="mu", state_law=law)
        model.loading = p["vl"]
        mc = pkg.MCMC(model, p["data"], R.BF_TRUTH, ["Uniform", *R.BF_BOX], R.BF_TRUTH, nsamples=10, verbose=False)
        pools[law], models[law] = mc.sample_law(256, 200, nburn=96, seed=9), model
        res[law] = pools[law].law_predictive(model, p["data"], noise_probs=(0.05, 0.95), loo=True)
        assert (res[law]["law"], res[law]["observable"], res[law]["n"]) == (law, "mu", 104 * 256)
        assert np.array_equal(_bits(res[law]["elpd_loo_k"]), _bits(pools[law].law_loo(model, p["data"])["elpd_loo_k"]))
    fit = res[truth]
    cov, bound = LP.coverage(p["data"], fit["noise_quantiles"][0], fit["noise_quantiles"][1])
    delta, se = LP.elpd_difference(fit["elpd_loo_k"], res[other]["elpd_loo_k"])
    print(f"truth {truth}: coverage {cov:.4f} (0.9 +- {bound:.4f}); n_high_k {fit['n_high_k']:.0f}, max k {fit['max_pareto_k']:.3f}; elpd_loo {fit['elpd_loo']:.2f} "
          f"(se {fit['elpd_loo_se']:.2f}) against {res[other]['elpd_loo']:.2f}: delta {delta:.2f}, paired se {se:.2f}, ratio {delta / se:.2f}; "
          f"log Bayes factor {p['log_bayes_factor']:+.1f}; elpd_waic {fit['elpd_waic']:.2f}, p_waic {fit['p_waic']:.2f}, p_loo {fit['p_loo']:.2f}")
    assert abs(cov - 0.9) <= bound
    assert fit["n_high_k"] == 0
    assert delta > 4.0 * se
    # the figures are the specification's, to test 4's bounds, on an evenly strided subset of the draws (the specification's
    # sums are exact and slow): the engine's result for the subset against predictive_reference on the series it returns
    q, s2 = pools[truth]._draws(2048)
    with pkg.Engine(mem="host") as eng:
        eng.set_model(models[truth], 1)
        sub = eng.law_predictive(truth, "mu", q, s2, p["data"], return_series=True)
    want = P.partials(np.asarray(sub["series"]), s2, p["data"], sub["center_y"], sub["center_l"])
    err = _scaled(sub["partials"], want)
    rows, tot = _finish_errors(sub, want, sub["center_y"], sub["center_l"])
    cpu = P.finish(LP.partials(p["m"], q, s2, p["data"], sub["center_y"], sub["center_l"], p["vl"], truth, "mu"), sub["center_y"], sub["center_l"])
    print(f"truth {truth}, 2048 draws: partials' scaled error {err:.3e}; finished rows {rows:.3e}, totals {tot:.3e}; elpd_waic {sub['elpd_waic']:.6f}, "
          f"the specification's own solve {cpu['elpd_waic']:.6f}")
    assert err <= TOL and rows <= TOL and tot <= TOL_TOTALS
