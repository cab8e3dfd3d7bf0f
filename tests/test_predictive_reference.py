"""
CPU tests of the posterior predictive checks: the NumPy specification (tests/predictive_reference.py) against independent
forms, the library's host-only rsf_predict_finish (librsf_hip.so loads without a GPU) against the specification's finish, and
include/rsf_predict.h against the binding.
"""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.special import logsumexp
from scipy.stats import norm

import predictive_reference as ref
from conftest import ROOT


def _case(seed, nout=7, n=23, spread=0.3):
    rng = np.random.default_rng(seed)
    base = rng.normal(0.0, 2.0, nout)
    series = base[:, None] + spread * rng.standard_normal((nout, n))
    series[0] = 0.0
    std2 = rng.uniform(0.05, 0.4, n)
    data = base + 0.4 * rng.standard_normal(nout)
    return series, std2, data


def _centres(series, std2, data, shift=0.0):
    cy = series.mean(axis=1) + shift
    cl = ref.loglik(cy[:, None], [float(np.mean(std2))], data)[:, 0] - 3.0 * shift
    return cy, cl


def test_reference_against_scipy_brute_force():
    series, std2, data = _case(1)
    nout, n = series.shape
    got = ref.statistics(series, std2, data, probs=(0.05, 0.5))
    sd = np.sqrt(std2)[None, :]
    logpdf = norm.logpdf(data[:, None], loc=series, scale=sd)
    np.testing.assert_allclose(got["mean"], series.mean(axis=1), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(got["var"], series.var(axis=1, ddof=1), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(got["pit"], norm.cdf(data[:, None], loc=series, scale=sd).mean(axis=1), rtol=1e-13)
    np.testing.assert_allclose(got["lpd"], logsumexp(logpdf, axis=1) - np.log(n), rtol=1e-13)
    np.testing.assert_allclose(got["p_waic_k"], logpdf.var(axis=1, ddof=1), rtol=1e-11)
    e = got["lpd"] - got["p_waic_k"]
    assert got["elpd_waic"] == pytest.approx(e.sum(), rel=1e-13)
    assert got["p_waic"] == pytest.approx(logpdf.var(axis=1, ddof=1).sum(), rel=1e-11)
    assert got["elpd_waic_se"] == pytest.approx(np.sqrt(nout * e.var(ddof=1)), rel=1e-13)
    assert got["mean_std2"] == pytest.approx(std2.mean(), rel=1e-14)
    np.testing.assert_array_equal(got["quantiles"], np.quantile(series, [0.05, 0.5], axis=1))


def test_identical_draws_have_no_spread():
    series, std2, data = _case(2)
    series = np.repeat(series[:, :1], 8, axis=1)  # a power of two: the mean of identical values is exact
    std2 = np.full(8, 0.2)
    got = ref.statistics(series, std2, data)
    np.testing.assert_array_equal(got["var"], 0.0)
    np.testing.assert_array_equal(got["p_waic_k"], 0.0)
    np.testing.assert_allclose(got["lpd"], ref.loglik(series[:, :1], std2[:1], data)[:, 0], rtol=1e-14)
    assert got["p_waic"] == 0.0


def test_finished_statistics_do_not_depend_on_the_centres():
    series, std2, data = _case(3, nout=11, n=200)
    want = ref.statistics(series, std2, data)
    for shift in (0.0, 0.05, -0.2):
        cy, cl = _centres(series, std2, data, shift)
        got = ref.finish(ref.partials(series, std2, data, cy, cl), cy, cl)
        for name in ref.OUT:
            np.testing.assert_allclose(got[name], want[name], rtol=1e-9, atol=1e-12, err_msg=f"{name}, shift {shift}")
        for name in ref.TOTALS:
            assert got[name] == pytest.approx(want[name], rel=1e-9), (name, shift)


def test_partials_of_shards_add():
    series, std2, data = _case(4, n=50)
    cy, cl = _centres(series, std2, data)
    whole = ref.partials(series, std2, data, cy, cl)
    parts = ref.partials(series[:, :13], std2[:13], data, cy, cl) + ref.partials(series[:, 13:], std2[13:], data, cy, cl)
    assert (np.abs(parts - whole) / ref.scales(whole)).max() < 1e-14


def _lib_finish(lib, part, cy, cl):
    dbl = ctypes.POINTER(ctypes.c_double)
    part, cy, cl = (np.ascontiguousarray(x, dtype=np.float64) for x in (part, cy, cl))
    rows = (part.size - ref.HEAD) // ref.FIELDS
    out, tot = np.empty((rows, len(ref.OUT))), np.empty(len(ref.TOTALS))
    rc = lib.rsf_predict_finish(rows, part.ctypes.data_as(dbl), cy.ctypes.data_as(dbl), cl.ctypes.data_as(dbl), out.ctypes.data_as(dbl),
                                tot.ctypes.data_as(dbl))
    assert rc == 0, lib.rsf_last_error()
    res = {name: out[:, j].copy() for j, name in enumerate(ref.OUT)}
    res.update(zip(ref.TOTALS, tot))
    return res


def _same(got, want, rows=1e-13, totals=1e-12):
    for name in ref.OUT:
        np.testing.assert_allclose(got[name], want[name], rtol=rows, atol=1e-300, equal_nan=True, err_msg=name)
    for name in ref.TOTALS:
        np.testing.assert_allclose(got[name], want[name], rtol=totals, equal_nan=True, err_msg=name)


def test_library_finish_matches_the_reference(pkg):
    lib = pkg._abi.load()
    series, std2, data = _case(5, nout=40, n=300)
    cy, cl = _centres(series, std2, data, 0.01)
    part = ref.partials(series, std2, data, cy, cl)
    _same(_lib_finish(lib, part, cy, cl), ref.finish(part, cy, cl))
    # the same through the Engine-level wrapper's layout constants
    assert pkg._abi.PREDICT_HEAD == ref.HEAD and len(pkg._abi.PREDICT_FIELDS) == ref.FIELDS
    assert pkg._abi.PREDICT_OUT == ref.OUT and pkg._abi.PREDICT_TOTALS == ref.TOTALS


def test_library_finish_nan_row_rule(pkg):
    lib = pkg._abi.load()
    series, std2, data = _case(6, nout=9, n=31)
    series[3, 4] = np.nan
    series[6, 0] = np.inf
    cy, cl = _centres(np.nan_to_num(series, nan=0.0, posinf=0.0), std2, data)
    part = ref.partials(series, std2, data, cy, cl)
    got, want = _lib_finish(lib, part, cy, cl), ref.finish(part, cy, cl)
    _same(got, want)
    direct = ref.statistics(series, std2, data)
    for name in ref.OUT:
        assert np.isnan(got[name][[3, 6]]).all() and np.isfinite(np.delete(got[name], [3, 6])).all(), name
        np.testing.assert_allclose(np.delete(got[name], [3, 6]), np.delete(direct[name], [3, 6]), rtol=1e-9, atol=1e-12)
    for name in ("elpd_waic", "p_waic", "elpd_waic_se"):
        assert np.isnan(got[name]) and np.isnan(direct[name]), name
    assert np.isfinite(got["mean_std2"])


def test_library_finish_single_draw(pkg):
    lib = pkg._abi.load()
    series, std2, data = _case(7, nout=5, n=1)
    cy, cl = _centres(series, std2, data, 0.1)
    part = ref.partials(series, std2, data, cy, cl)
    got = _lib_finish(lib, part, cy, cl)
    _same(got, ref.finish(part, cy, cl))
    assert np.isnan(got["var"]).all() and np.isnan(got["p_waic_k"]).all() and np.isnan(got["elpd_waic"])  # ddof = 1 with one draw
    np.testing.assert_allclose(got["mean"], series[:, 0], rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(got["lpd"], ref.loglik(series, std2, data)[:, 0], rtol=1e-13)


def test_library_finish_validates(pkg):
    lib = pkg._abi.load()
    dbl = ctypes.POINTER(ctypes.c_double)
    x = np.zeros(16)
    p = x.ctypes.data_as(dbl)
    assert lib.rsf_predict_finish(0, p, p, p, p, p) == -1 and b"rsf_predict_finish" in lib.rsf_last_error()
    assert lib.rsf_predict_finish(1, None, p, p, p, p) == -1 and b"rsf_predict_finish" in lib.rsf_last_error()


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "rsf_predict.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rsf_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_declare_the_same_symbols(pkg):
    assert _declared_symbols() == sorted(pkg._abi.PREDICT_PROTOTYPES)
    assert len(_declared_symbols()) == 3
    lib = pkg._abi.load()
    for name in _declared_symbols():
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == pkg._abi.PREDICT_PROTOTYPES[name][1]
    text = open(os.path.join(ROOT, "include", "rsf_predict.h")).read()
    for macro, value in (("RSF_PREDICT_HEAD", pkg._abi.PREDICT_HEAD), ("RSF_PREDICT_FIELDS", len(pkg._abi.PREDICT_FIELDS)),
                         ("RSF_PREDICT_OUT", len(pkg._abi.PREDICT_OUT)), ("RSF_PREDICT_TOTALS", len(pkg._abi.PREDICT_TOTALS)),
                         ("RSF_PREDICT_MAX_PROBS", pkg._abi.PREDICT_MAX_PROBS)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == value, macro


def test_header_compiles_as_c(tmp_path):
    import subprocess

    src = tmp_path / "t.c"
    src.write_text('#include "rsf_predict.h"\nint main(void) { return RSF_PREDICT_FIELDS == 7 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_pool_predictive_strided_subset(pkg):
    """PosteriorPool.predictive flattens (n_keep, C, d) to draws, takes an evenly strided subset without an RNG and
    sets the model on the engine it is given (here: an engine object that records, no GPU)."""
    seen = {}

    class Fake:
        def set_model(self, model, substeps):
            seen["substeps"] = substeps

        def predictive(self, q, std2, data, probs=()):
            seen.update(q=q, std2=std2, probs=probs)
            return {}

    samples = np.arange(5 * 4 * 3, dtype=np.float64).reshape(5, 4, 3)
    from bayesian_markov_chain_monte_carlo_amd.MCMC import PosteriorPool

    pool = PosteriorPool(samples, np.arange(20.0).reshape(5, 4), 0.3, {}, 0)
    model = type("M", (), {"substeps": 2})()
    pool.predictive(model, np.zeros(3), max_draws=5, engine=Fake())
    np.testing.assert_array_equal(seen["std2"], [0.0, 4.0, 8.0, 12.0, 16.0])
    np.testing.assert_array_equal(seen["q"], samples.reshape(20, 3)[[0, 4, 8, 12, 16]])
    assert seen["substeps"] == 2 and tuple(seen["probs"]) == (0.05, 0.5, 0.95)
    pool.predictive(model, np.zeros(3), engine=Fake(), substeps=1)
    assert seen["q"].shape == (20, 3) and seen["substeps"] == 1
    with pytest.raises(ValueError):
        pool.predictive(model, np.zeros(3), max_draws=0, engine=Fake())
