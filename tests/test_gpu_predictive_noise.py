"""
GPU tests of the posterior predictive band that includes the noise (include/rsf_predict_noise.h, rsf_predict_noise_quantiles)
against the specification tests/predictive_noise_reference.py.

The criterion is the residual: the library's t has |F_ref(t) - p| <= 1e-12 (tests/predictive_noise_cases.py derives the bound and
states the condition on the inputs it rests on), F_ref evaluated once per (row, probability).  The distance to the brentq root
is printed, not asserted: where F' is tiny the root is ill-conditioned by nature.

Measured on an MI355X (profiles/noise_band/gpu_noise_tests.log):
    real draws, nsteps 500, probabilities (0.025, 0.05, 0.5, 0.95, 0.975):
        d, n          largest residual    passes mean / max    largest distance to the brentq root (every 25th row), in min_i s_i
        1,  1037      6.4e-15             6.21 / 8             2.4e-14
        3,  1037      6.9e-15             6.45 / 9             6.9e-14
        1, 16421      7.0e-15             6.22 / 8             3.6e-14
        3, 16421      6.4e-15             6.50 / 8             3.1e-14
    crafted rows: largest residual 2.8e-15 (`tight`); passes tight 6, wide 13, bimodal 14, k0 7, n1 2, n5 10, scales 7, extreme_p 11:
    on every case the count of the float64 NumPy restatement (predictive_noise_reference.scheme) on the same input.
    end to end: 0.896 of the observations inside the 90 % band, 0.052 inside the credible band of the model series; 0 rows excused.
"""
import ctypes

import numpy as np
import pytest
from scipy.special import ndtri

import predictive_noise_cases as cases
import predictive_noise_reference as ref
import psis_cases

pytestmark = pytest.mark.gpu


def _check(got, passes, series, std2, probs, label):
    res = ref.residual(series, std2, probs, got)
    worst = float(np.nanmax(res)) if np.isfinite(res).any() else 0.0
    print(f"{label}: largest residual {worst:.3e}; passes mean {passes.mean():.2f}, max {passes.max()}")
    assert np.all(np.diff(got, axis=0)[:, np.isfinite(got).all(axis=0)] >= 0), "not monotone in p"
    assert passes.min() >= 1 and passes.max() <= ref.MAX_PASSES
    return worst


@pytest.fixture(scope="module")
def real(pkg, oracle_lib):
    """The series of predictive_partials for psis_cases.REAL and the library's band of it: computed once, shared, not changed."""
    memo = {}

    def get(d, n):
        if (d, n) not in memo:
            with pkg.Engine(lib=oracle_lib) as cpu:
                model, q, std2, data = psis_cases.real_draws(pkg, cpu, n, d, 400 + d + n)
            with pkg.Engine(mem="host") as eng:
                eng.set_model(model, 1)
                series = eng.predictive(q, std2, data, return_series=True)["series"]
                got, passes = eng.predictive_noise_quantiles(series, std2, cases.REAL_PROBS, return_passes=True)
            for a in (series, std2, got, passes):
                a.setflags(write=False)
            memo[d, n] = (series, std2, got, passes)
        return memo[d, n]

    return get


@pytest.mark.parametrize("d,n", psis_cases.REAL)
def test_real_draws(real, d, n):
    series, std2, got, passes = real(d, n)
    cases.check_condition(series, std2)
    assert got.shape == (len(cases.REAL_PROBS), series.shape[0]) and np.isfinite(got).all()
    worst = _check(got, passes, series, std2, cases.REAL_PROBS, f"real draws d={d} n={n}")
    rows = list(range(0, series.shape[0], 25))
    want = ref.quantiles(series, std2, cases.REAL_PROBS, rows=rows)
    dist = np.abs(got[:, rows] - want[:, rows]) / np.sqrt(std2).min()
    print(f"real draws d={d} n={n}: distance to the brentq root on every 25th row, in min_i s_i: largest {dist.max():.3e} "
          f"(per probability {[float(f'{v:.2e}') for v in dist.max(axis=1)]})")
    assert worst <= cases.TOL_RESIDUAL


@pytest.mark.parametrize("name", [c[0] for c in cases.crafted()])
def test_crafted_rows(gpu_engine, name):
    (series, std2, probs), = [(y, s2, p) for nm, y, s2, p in cases.crafted() if nm == name]
    got, passes = gpu_engine.predictive_noise_quantiles(series, std2, probs, return_passes=True)
    assert np.isfinite(got).all()
    worst = _check(got, passes, series, std2, probs, name)
    assert worst <= cases.TOL_RESIDUAL
    if name != "bimodal":
        assert passes.max() <= cases.SCHEME_PASSES[name] + cases.PASS_MARGIN
    if name == "n1":
        s = np.sqrt(std2)[0]
        want = series[:, 0][None, :] + ndtri(np.asarray(probs))[:, None] * s
        # rule (a) stops within 2^-46 q / F' of the root: at most 2^-46 sqrt(2 pi) / 2 s = 1.8e-14 s (p = 1/2); then the rounding of t
        assert np.all(np.abs(got - want) <= 2e-14 * s + 4 * np.spacing(np.abs(want)))
    if name == "k0":
        assert got[probs.index(0.5), 0] == 0.0 and passes[0] >= 2  # (p = 1/2 stops in pass 0; the other targets go on)


def test_seventeen_probabilities_equal_one_at_a_time(real, gpu_engine):
    """Two calls (16 + 1) with the 16-target kernel against 17 calls with the 4-target kernel: a target's result depends neither
    on the other targets of its call nor on which instantiation runs it."""
    series, std2, _, _ = real(3, 1037)
    probs = np.concatenate([[1e-6, 0.001], np.linspace(0.025, 0.975, 13), [0.999, 1.0 - 1e-6]])
    assert probs.size == 17
    both, passes = gpu_engine.predictive_noise_quantiles(series, std2, probs, return_passes=True)
    each = [gpu_engine.predictive_noise_quantiles(series, std2, [p], return_passes=True) for p in probs]
    np.testing.assert_array_equal(both, np.vstack([e[0] for e in each]))
    np.testing.assert_array_equal(passes, np.max([e[1] for e in each], axis=0))
    assert np.all(np.diff(both, axis=0) >= 0)
    three = gpu_engine.predictive_noise_quantiles(series, std2, probs[[3, 16, 8]])
    np.testing.assert_array_equal(three, both[[3, 16, 8]])


def test_a_non_finite_draw_and_a_bad_std2(pkg, gpu_engine, cpu_engine):
    """One draw with Dc = 0.2, whose fixed-step series is not finite: exactly its rows are NaN.  One std2 = 0: every
    row is NaN."""
    model, q, std2, data = psis_cases.real_draws(pkg, cpu_engine, 100, 1, 31)
    q[17, 0] = 0.2
    gpu_engine.set_model(model, 1)
    res = gpu_engine.predictive(q, std2, data, return_series=True, noise_probs=(0.05, 0.95))
    bad = ~np.isfinite(res["series"]).all(axis=1)
    assert bad.any() and not bad[0]
    got = res["noise_quantiles"]
    assert np.isnan(got[:, bad]).all() and np.isfinite(got[:, ~bad]).all()
    series = np.where(np.isfinite(res["series"]), res["series"], 0.0)
    assert np.isfinite(gpu_engine.predictive_noise_quantiles(series, std2, (0.05, 0.95))).all()
    for v in (0.0, -1.0, np.inf, np.nan):
        s2 = std2.copy()
        s2[41] = v
        got, passes = gpu_engine.predictive_noise_quantiles(series, s2, (0.05, 0.95), return_passes=True)
        assert np.isnan(got).all() and (passes == 1).all(), v


def test_bits_are_reproducible_in_host_and_device_memory(pkg, real, gpu_engine):
    series, std2, got, passes = real(3, 16421)
    a = gpu_engine.predictive_noise_quantiles(series, std2, cases.REAL_PROBS, return_passes=True)
    np.testing.assert_array_equal(a[0], got)
    np.testing.assert_array_equal(a[1], passes)
    with pkg.Engine(mem="device") as dev:
        b = dev.predictive_noise_quantiles(series, std2, cases.REAL_PROBS, return_passes=True)
    np.testing.assert_array_equal(b[0], got)
    np.testing.assert_array_equal(b[1], passes)


def test_predictive_with_noise_probs_composes(pkg, gpu_engine, cpu_engine):
    """predictive(noise_probs=...) is predictive(return_series=True) followed by predictive_noise_quantiles, bit for bit; without
    noise_probs the keys and values are what they were."""
    model, q, std2, data = psis_cases.real_draws(pkg, cpu_engine, 1037, 3, 5)
    gpu_engine.set_model(model, 1)
    plain = gpu_engine.predictive(q, std2, data, probs=(0.05, 0.95), return_series=True)
    assert set(plain) == {"mean", "var", "pit", "lpd", "p_waic_k", "mean_std2", "elpd_waic", "p_waic", "elpd_waic_se", "n", "partials",
                          "center_y", "center_l", "probs", "quantiles", "series"}
    band = gpu_engine.predictive_noise_quantiles(plain["series"], std2, (0.05, 0.5, 0.95))
    both = gpu_engine.predictive(q, std2, data, probs=(0.05, 0.95), noise_probs=(0.05, 0.5, 0.95))
    assert set(both) == (set(plain) - {"series"}) | {"noise_probs", "noise_quantiles"}
    np.testing.assert_array_equal(both["noise_quantiles"], band)
    np.testing.assert_array_equal(both["noise_probs"], (0.05, 0.5, 0.95))
    for name in set(plain) - {"series"}:
        np.testing.assert_array_equal(both[name], plain[name], err_msg=name)
    only = gpu_engine.predictive(q, std2, data, noise_probs=(0.5,))
    assert set(only) == (set(plain) - {"series", "probs", "quantiles"}) | {"noise_probs", "noise_quantiles"}
    np.testing.assert_array_equal(only["noise_quantiles"][0], band[1])
    # the band of an observation contains the band of the model series
    assert np.all(both["noise_quantiles"][0] <= both["quantiles"][0]) and np.all(both["noise_quantiles"][2] >= both["quantiles"][1])
    for bad in ((0.0,), (1.0,), (float("nan"),), (0.5, 1.5)):
        with pytest.raises(ValueError):
            gpu_engine.predictive(q, std2, data, noise_probs=bad)


def test_end_to_end_band_contains_the_data_where_the_pit_says_so(pkg, cpu_engine):
    """The shape and seeds of test_end_to_end_well_specified_run.  F_k(data_k) = pit_k by definition, so data_k lies inside
    [noise_q05_k, noise_q95_k] exactly when 0.05 <= pit_k <= 0.95; asserted for every k whose pit_k is further than 1e-9 from both
    ends, and at most 1 % of the rows may be excused."""
    model = pkg.RateStateModel(number_time_steps=500)
    model.RadiationDamping = True
    cpu_engine.set_model(model, 1)
    truth = psis_cases.restatement_series(cpu_engine, np.array([[1000.0]]))[:, 0]
    sigma0 = 0.01 * np.abs(truth).max()
    data = truth + sigma0 * np.random.default_rng(1).standard_normal(truth.size)
    mc = pkg.MCMC(model, data, 1000.0, ["Uniform", 0.0, 1.0e4], 1000.0, nsamples=200, verbose=False)
    pool = mc.sample_batched(4096, seed=7)
    res = pool.predictive(model, data, probs=(), noise_probs=(0.05, 0.95), max_draws=32768)
    assert res["n"] == 32768 and "quantiles" not in res
    lo, hi = res["noise_quantiles"]
    pit = res["pit"]
    inside = (data >= lo) & (data <= hi)
    clear = np.minimum(np.abs(pit - 0.05), np.abs(pit - 0.95)) > 1e-9
    excused = int((~clear).sum())
    clean = pool.predictive(model, data, probs=(0.05, 0.95), max_draws=32768)
    np.testing.assert_array_equal(clean["pit"], pit)
    in_clean = (data >= clean["quantiles"][0]) & (data <= clean["quantiles"][1])
    print(f"end to end: {inside.mean():.3f} of the {data.size} observations inside the 90 % posterior predictive band, "
          f"{in_clean.mean():.3f} inside the 90 % credible band of the model series; {excused} rows excused (pit within 1e-9 of an end)")
    assert excused <= 0.01 * data.size
    np.testing.assert_array_equal(inside[clear], ((pit >= 0.05) & (pit <= 0.95))[clear])


def test_validation_through_a_real_ctx(pkg, gpu_engine):
    lib, dbl, i32 = gpu_engine.lib, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    series, s2 = np.ones((3, 50)), np.full(50, 0.5)
    pr, out, ps = np.array([0.05, 0.95]), np.zeros((2, 3)), np.zeros(3, dtype=np.int32)

    def call(n=50, rows=3, s=series, std2=s2, np_=2, p=pr, o=out, passes=ps, ctx=gpu_engine._ctx):
        return lib.rsf_predict_noise_quantiles(ctx, n, rows, None if s is None else s.ctypes.data, None if std2 is None else std2.ctypes.data, np_,
                                               None if p is None else p.ctypes.data_as(dbl), None if o is None else o.ctypes.data_as(dbl),
                                               None if passes is None else passes.ctypes.data_as(i32))

    assert call() == 0  # needs no model
    z = 1.6448536269514722 * np.sqrt(0.5)
    assert np.abs(out - np.array([[1 - z] * 3, [1 + z] * 3])).max() <= 2e-15 and (ps >= 1).all()
    assert call(passes=None) == 0  # passes_out is optional
    many = np.linspace(0.1, 0.9, 17)
    for kw in (dict(n=0), dict(n=2 ** 31), dict(rows=0), dict(np_=0), dict(np_=17, p=many), dict(s=None), dict(std2=None), dict(p=None),
               dict(o=None), dict(p=np.array([0.0, 0.5])), dict(p=np.array([0.5, 1.0])), dict(p=np.array([-0.1, 0.5])),
               dict(p=np.array([0.5, float("nan")]))):
        assert call(**kw) == -1 and b"rsf_predict_noise_quantiles" in lib.rsf_last_error(), kw
    assert call(ctx=None) == -1
    assert call(np_=16, p=many, o=np.zeros((16, 3))) == 0
    for args in ((series, s2[:49], pr), (np.zeros(5), s2, pr), (series, s2, ())):
        with pytest.raises(ValueError):
            gpu_engine.predictive_noise_quantiles(*args)
    for bad in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError):
            gpu_engine.predictive_noise_quantiles(series, s2, (0.5, bad))
    assert pkg._abi.PREDICT_NOISE_MAX_PASSES == ref.MAX_PASSES
