"""
GPU tests of PSIS-LOO and the Pareto shape (include/rsf_psis.h, rsf_predict_psis_loo / _finish) against the long double
specification tests/psis_reference.py, applied to the same series.

Bounds (tests/psis_cases.py, where the measurement is recorded; re-measured by tests/test_psis_reference.py): 8 x the distance of
the reference in plain float64 NumPy from the reference in long double on these inputs,
    elpd_loo_k over max(|elpd_loo_k|, 1) and weight_ess_k relative:  8 x 1.458e-13 = 1.1664e-12   (TOL_SCALED)
    pareto_k absolute:                                              8 x 1.736e-13 = 1.3888e-12   (TOL_K)
and n_tail equal as an integer.
"""
import ctypes

import numpy as np
import pytest

import predictive_reference as pref
import psis_cases as cases
import psis_reference as ref

pytestmark = pytest.mark.gpu

LD = np.longdouble


def _compare(got, series, std2, data, r_eff, label):
    want = ref.psis_rows(series, std2, data, r_eff, LD)
    nan = np.isnan(want["elpd_loo_k"].astype(np.float64))
    for name in ref.OUT:
        np.testing.assert_array_equal(np.isnan(got[name]), nan, err_msg=name)
    ok = ~nan
    np.testing.assert_array_equal(got["n_tail"][ok], want["n_tail"][ok].astype(np.float64))
    wk = want["pareto_k"].astype(np.float64)
    fin = ok & np.isfinite(wk)
    np.testing.assert_array_equal(np.isposinf(got["pareto_k"]), np.isposinf(wk))
    e = float((np.abs(got["elpd_loo_k"][ok] - want["elpd_loo_k"][ok]) / np.maximum(np.abs(want["elpd_loo_k"][ok]), 1)).max()) if ok.any() else 0.0
    s = float((np.abs(got["weight_ess"][ok] - want["weight_ess"][ok]) / np.abs(want["weight_ess"][ok])).max()) if ok.any() else 0.0
    k = float(np.abs(got["pareto_k"][fin] - want["pareto_k"][fin]).max()) if fin.any() else 0.0
    print(f"{label}: elpd_loo_k {e:.3e} (scaled), weight_ess {s:.3e} (relative), pareto_k {k:.3e} (absolute; k in "
          f"[{wk[ok].min():.3g}, {wk[ok].max():.3g}]), n_tail equal")
    return e, s, k, want


@pytest.mark.parametrize("d,n", cases.REAL)
def test_real_draws(pkg, gpu_engine, cpu_engine, d, n):
    """The series of predictive_partials (nsteps 500); rows and totals from the library against the reference on that series."""
    model, q, std2, data = cases.real_draws(pkg, cpu_engine, n, d, 400 + d + n)
    gpu_engine.set_model(model, 1)
    res = gpu_engine.predictive(q, std2, data, return_series=True)
    series = res["series"]
    got = gpu_engine.psis_loo(series, std2, data, res["lpd"])
    e, s, k, want = _compare(got, series, std2, data, 1.0, f"real draws d={d} n={n}")
    assert e <= cases.TOL_SCALED and s <= cases.TOL_SCALED
    assert k <= cases.TOL_K
    tot = ref.finish({name: got[name] for name in ref.OUT}, res["lpd"], n)  # the finish alone: from the library's own rows
    for name in ref.TOTALS:
        assert got[name] == pytest.approx(tot[name], rel=1e-13, abs=1e-13), name
    assert got["n"] == n and got["k_threshold"] == min(1.0 - 1.0 / np.log10(n), 0.7)
    assert got["p_loo"] > 0 and got["elpd_loo"] <= res["lpd"].sum()


@pytest.mark.parametrize("name", [c[0] for c in cases.crafted()])
def test_crafted_rows(gpu_engine, name):
    """A heavy tail of known shape; a pool with repeated draws straddling the cutoff (n_tail < tail_len); n = 1, 5, 25; an
    all-equal row; a range of x beyond 708 (the cutoff clamps); r_eff != 1, up to the longest tail one workgroup holds."""
    (series, r_eff), = [(s, r) for nm, s, r in cases.crafted() if nm == name]
    rows, n = series.shape
    std2, data = np.full(n, cases.STD2), np.zeros(rows)
    lpd = pref.statistics(series, std2, data)["lpd"]
    got = gpu_engine.psis_loo(series, std2, data, lpd, r_eff=r_eff)
    e, s, k, want = _compare(got, series, std2, data, r_eff, name)
    assert e <= cases.TOL_SCALED and s <= cases.TOL_SCALED
    assert k <= cases.TOL_K
    if name == "repeats":
        assert tuple(got["n_tail"]) == (182.0, 182.0)
    if name in ("n1", "n5", "all_equal"):
        assert np.isposinf(got["pareto_k"]).all() and got["n_high_k"] == rows and got["max_pareto_k"] == np.inf
    if name == "clamped_cutoff":
        assert tuple(got["n_tail"]) == (50.0, 50.0)
    if name == "long_tail":
        assert tuple(got["n_tail"]) == (6000.0,)


def test_a_non_finite_draw_makes_its_rows_and_the_totals_nan(pkg, gpu_engine, cpu_engine):
    """One draw with Dc = 0.2, whose fixed-step series is not finite: exactly its rows are NaN, and the totals."""
    model, q, std2, data = cases.real_draws(pkg, cpu_engine, 100, 1, 31)
    q[17, 0] = 0.2
    gpu_engine.set_model(model, 1)
    res = gpu_engine.predictive(q, std2, data, loo=True, return_series=True)
    series = res["series"]
    bad = ~np.isfinite(series).all(axis=1)
    assert bad.any() and not bad[0]
    for name in ref.OUT:
        assert np.isnan(res[name][bad]).all() and not np.isnan(res[name][~bad]).any(), name
    e, s, k, _ = _compare(res, series, std2, data, 1.0, "non-finite draw")
    assert e <= cases.TOL_SCALED and s <= cases.TOL_SCALED and k <= cases.TOL_K
    for name in ref.TOTALS:
        assert np.isnan(res[name]) == (name != "k_threshold"), name


def test_bits_are_reproducible_in_host_and_device_memory(pkg, gpu_engine, cpu_engine):
    model, q, std2, data = cases.real_draws(pkg, cpu_engine, 5037, 3, 11)
    gpu_engine.set_model(model, 1)
    res = gpu_engine.predictive(q, std2, data, return_series=True)
    a = gpu_engine.psis_loo(res["series"], std2, data, res["lpd"])
    b = gpu_engine.psis_loo(res["series"], std2, data, res["lpd"])
    with pkg.Engine(mem="device") as dev:
        c = dev.psis_loo(res["series"], std2, data, res["lpd"])
        dev.set_model(model, 1)
        rd = dev.predictive(q, std2, data, loo=True)
    for name in ref.OUT + ref.TOTALS:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
        np.testing.assert_array_equal(a[name], c[name], err_msg=name)
        if name != "p_loo":  # (lpd_k is formed about centres at the draws' mean, which the two engines average in another order)
            np.testing.assert_array_equal(a[name], rd[name], err_msg=name)


def test_predictive_with_loo_composes(pkg, gpu_engine, cpu_engine):
    """predictive(loo=True) is predictive() followed by psis_loo on its series, bit for bit; loo=False has today's keys."""
    model, q, std2, data = cases.real_draws(pkg, cpu_engine, 1037, 3, 5)
    gpu_engine.set_model(model, 1)
    plain = gpu_engine.predictive(q, std2, data, probs=(0.05, 0.95), return_series=True)
    assert set(plain) == {"mean", "var", "pit", "lpd", "p_waic_k", "mean_std2", "elpd_waic", "p_waic", "elpd_waic_se", "n", "partials",
                          "center_y", "center_l", "probs", "quantiles", "series"}
    assert set(gpu_engine.predictive(q, std2, data)) == set(plain) - {"probs", "quantiles", "series"}
    loo = gpu_engine.psis_loo(plain["series"], std2, data, plain["lpd"])
    both = gpu_engine.predictive(q, std2, data, probs=(0.05, 0.95), loo=True)
    assert set(both) == (set(plain) - {"series"}) | set(ref.OUT) | set(ref.TOTALS)
    for name in ref.OUT + ref.TOTALS:
        np.testing.assert_array_equal(both[name], loo[name], err_msg=name)
    for name in pref.OUT + pref.TOTALS + ("quantiles",):
        np.testing.assert_array_equal(both[name], plain[name], err_msg=name)
    r = gpu_engine.predictive(q, std2, data, loo=True, r_eff=0.5)
    assert np.all(r["n_tail"] <= ref.tail_len(1037, 0.5)) and r["n_tail"].max() == ref.tail_len(1037, 0.5) > ref.tail_len(1037)


# h: n_high_k of the long double reference alone on the CPU restatement's draws at this shape and seed (see the docstring)
END_TO_END_HIGH_K = 0


def test_end_to_end_well_specified_run(pkg, cpu_engine):
    """The shape and seed of test_end_to_end_pit_is_calibrated: data = y(Dc = 1000) + sigma0 eps, sigma0 = 0.01 max|y|, data seed
    1, nsteps 500, 4096 chains x 200 iterations (the last 100 kept), sampler seed 7; pool.loo on an evenly strided subset of
    32 768 draws.  elpd_loo <= sum lpd_k, p_loo > 0 and n_high_k <= h.  h = 0 is what tests/psis_reference.py alone gave, in long
    double and in float64, on the CPU restatement's chains (same start, seed and iterations, run through the checker engine) and
    the restatement's series of the same strided subset: pareto_k between -0.184 and 0.121 (median -0.049) against the threshold
    0.7, elpd_loo 4012.98 +- 17.28, p_loo 2.238, sum lpd_k 4015.22."""
    model = pkg.RateStateModel(number_time_steps=500)
    model.RadiationDamping = True
    cpu_engine.set_model(model, 1)
    truth = cases.restatement_series(cpu_engine, np.array([[1000.0]]))[:, 0]
    sigma0 = 0.01 * np.abs(truth).max()
    data = truth + sigma0 * np.random.default_rng(1).standard_normal(truth.size)
    mc = pkg.MCMC(model, data, 1000.0, ["Uniform", 0.0, 1.0e4], 1000.0, nsamples=200, verbose=False)
    pool = mc.sample_batched(4096, seed=7)
    res = pool.loo(model, data, max_draws=32768)
    pk = res["pareto_k"]
    print(f"end to end: elpd_loo {res['elpd_loo']:.2f} +- {res['elpd_loo_se']:.2f} (elpd_waic {res['elpd_waic']:.2f}), p_loo {res['p_loo']:.3f} "
          f"(p_waic {res['p_waic']:.3f}), n_high_k {res['n_high_k']:.0f} of {data.size} (threshold {res['k_threshold']:.2f}), pareto_k "
          f"quantiles 0 / 0.5 / 0.9 / 1: {np.quantile(pk, [0, 0.5, 0.9, 1])}")
    assert res["n"] == 32768
    assert res["elpd_loo"] <= res["lpd"].sum()
    assert res["p_loo"] > 0
    assert res["n_high_k"] <= END_TO_END_HIGH_K


def test_validation_through_a_real_ctx(pkg, gpu_engine):
    lib, dbl = gpu_engine.lib, ctypes.POINTER(ctypes.c_double)
    series, s2, row, out = np.ones((3, 50)), np.full(50, 0.5), np.zeros(3), np.zeros((3, 4))

    def loo(n=50, rows=3, s=series, std2=s2, data=row, r_eff=1.0, o=out):
        return lib.rsf_predict_psis_loo(gpu_engine._ctx, n, rows, *(None if x is None else x.ctypes.data for x in (s, std2, data)), r_eff,
                                        None if o is None else o.ctypes.data_as(dbl))

    assert loo() == 0  # needs no model
    assert np.isposinf(out[:, 1]).all() and (out[:, 2] == 0).all()
    for kw in (dict(n=0), dict(n=2 ** 31), dict(rows=0), dict(r_eff=0.0), dict(r_eff=-1.0), dict(r_eff=float("nan")), dict(r_eff=float("inf")),
               dict(s=None), dict(std2=None), dict(data=None), dict(o=None)):
        assert loo(**kw) == -1 and b"rsf_predict_psis_loo" in lib.rsf_last_error(), kw
    assert lib.rsf_predict_psis_loo(None, 50, 3, series.ctypes.data, s2.ctypes.data, row.ctypes.data, 1.0, out.ctypes.data_as(dbl)) == -1
    # a tail beyond RSF_PSIS_MAX_TAIL: n = 50 000 at r_eff = 0.001 is min(10 000, 21 214); refused before anything is read
    assert loo(n=50000, r_eff=0.001) == -5 and b"RSF_PSIS_MAX_TAIL" in lib.rsf_last_error()
    tot, lpd = np.zeros(6), np.zeros(3)
    P = lambda x: None if x is None else x.ctypes.data_as(dbl)
    assert lib.rsf_predict_psis_finish(3, 50, P(out), P(lpd), P(tot)) == 0
    for args in ((0, 50, out, lpd, tot), (3, 0, out, lpd, tot), (3, 50, None, lpd, tot), (3, 50, out, None, tot), (3, 50, out, lpd, None)):
        assert lib.rsf_predict_psis_finish(args[0], args[1], *(P(x) for x in args[2:])) == -1 and b"rsf_predict_psis_finish" in lib.rsf_last_error()
    # the composed path needs the model
    with pytest.raises(RuntimeError, match="set_model"):
        gpu_engine.predictive(np.full(4, 1000.0), np.full(4, 1e-4), np.zeros(500), loo=True)
    for args in ((series, s2[:49], row, row), (series, s2, row[:2], row), (series, s2, row, row[:2]), (np.zeros(5), s2, row, row)):
        with pytest.raises(ValueError):
            gpu_engine.psis_loo(*args)
    with pytest.raises(ValueError):
        gpu_engine.psis_loo(series, s2, row, row, r_eff=0.0)
