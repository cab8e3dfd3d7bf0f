"""
CPU tests of the convergence diagnostics (include/rsf_diag.h): the long-double reference itself (tests/diagnostics_reference.py)
is pinned to hand-computed values, to known closed forms and to the ESS of processes whose autocorrelation is known; then the
library's host-only finish (rsf_diag_finish, librsf_hip.so — it loads on a host without a GPU) is held to the reference's
finish on the same partials, and every argument check of it is exercised.
"""
import ctypes
import os
from fractions import Fraction as F

import numpy as np
import pytest

import diagnostics_reference as ref

LD = np.longdouble


def test_reference_is_extended_precision():
    assert np.finfo(LD).nmant >= 63


# --- the reference ---------------------------------------------------------------------------------------------------------
def test_hand_computed_two_chains_four_draws():
    # chain 0: 1 3 | 2 4, chain 1: 3 5 | 6 8.  Split chains [1,3] [3,5] [2,4] [6,8]: means 2 4 3 7, every s2 = 2.
    # W = 2, B/N = var(2, 4, 3, 7) = 14/3, var_plus = (1/2) 2 + 14/3 = 17/3, split_rhat = sqrt(17/6).
    # Whole chains: means 5/2 and 11/2, variances 5/3 and 13/3.  S = 1: K = 2, B_nu = (3/2)^2 * 2 / 1 = 9/2, Btilde = 0,
    # W_nu = (5/3 + 13/3)/2 = 3, nested_rhat = sqrt(1 + 3/2) = sqrt(5/2).  N = 2: Geyer's loop never runs (t = 1 is not < N - 3),
    # so tau = -1 + rho(0) = 0 -> 1/log10(M'N) = 1/log10(8), ess = 8 log10(8), mcse = sqrt(var_plus / ess).
    x = np.array([[1, 3], [3, 5], [2, 6], [4, 8]], dtype=np.float64)
    r = ref.diagnostics(x, superchain_size=1)[0]
    exact = dict(W=F(2), B_over_N=F(14, 3), var_plus=F(17, 3), mean=F(4))
    for k, v in exact.items():
        assert r[k] == LD(v.numerator) / LD(v.denominator), k
    assert abs(r["split_rhat"] - np.sqrt(LD(17) / 6)) < 1e-18
    assert abs(r["nested_rhat"] - np.sqrt(LD(5) / 2)) < 1e-18
    assert r["K"] == 2 and r["lags_complete"]
    assert abs(r["ess"] - 8 * np.log10(LD(8))) < 1e-17
    assert abs(r["tau"] - 1 / np.log10(LD(8))) < 1e-18
    assert abs(r["mcse_mean"] - np.sqrt(LD(17) / 3 / (8 * np.log10(LD(8))))) < 1e-18
    # without superchains nested R-hat is undefined
    assert np.isnan(ref.diagnostics(x)[0]["nested_rhat"])


def test_iid_normal():
    x = np.random.default_rng(11).standard_normal((2048, 2048))  # M'N = 4096 * 1024 = 2^22
    r = ref.diagnostics(x)[0]
    assert abs(r["split_rhat"] - 1) < 1e-3
    assert 0.9 <= r["ess"] / 2**22 <= 1.1


def test_ar1_ess():
    phi, n, C = 0.9, 4096, 1024  # M'N = 2048 * 2048 = 2^22
    rng = np.random.default_rng(12)
    x = np.empty((n, C))
    x[0] = rng.standard_normal(C) / np.sqrt(1 - phi * phi)  # stationary start
    e = rng.standard_normal((n, C))
    for i in range(1, n):
        x[i] = phi * x[i - 1] + e[i]
    r = ref.diagnostics(x)[0]
    expect = 2**22 * (1 - phi) / (1 + phi)
    assert abs(r["ess"] / expect - 1) < 0.05, (r["ess"], expect)
    assert r["lags_complete"]


def test_offset_chains_closed_form():
    # every chain is the same base series plus c * delta; the base series' two halves have the same mean and variance (the
    # second is the first reversed), so W = s2 of a half and the split means are m + c delta, each c twice
    N, C, delta = 50, 7, 0.37
    half = np.random.default_rng(13).standard_normal(N)
    base = np.concatenate([half, half[::-1]])
    x = base[:, None] + delta * np.arange(C)[None, :]
    r = ref.diagnostics(x)[0]
    s2 = np.var(half.astype(LD), ddof=1)
    BN = LD(delta) ** 2 * C * (C * C - 1) / (6 * (2 * C - 1))
    expect = np.sqrt(((N - 1) / LD(N) * s2 + BN) / s2)
    assert abs(r["split_rhat"] / expect - 1) < 1e-15


def test_nested_rhat_with_one_chain_per_superchain():
    x = np.random.default_rng(14).standard_normal((101, 9)) + np.linspace(0, 1, 9)
    r = ref.diagnostics(x, superchain_size=1)[0]
    assert abs(r["nested_rhat"] ** 2 - (ref.unsplit_rhat(x)[0] ** 2 + LD(1) / 101)) < 1e-15


def test_partials_add_over_disjoint_chain_sets():
    x = np.random.default_rng(15).standard_normal((40, 12, 2))
    c = ref.default_center(x)
    whole = ref.partials(x, 3, c)
    parts = ref.partials(x[:, :6], 3, c) + ref.partials(x[:, 6:], 3, c)
    np.testing.assert_allclose(np.asarray(parts, np.float64), np.asarray(whole, np.float64), rtol=1e-15, atol=1e-15)


# --- rsf_diag_finish against the reference -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip_lib(pkg):
    if not os.path.exists(pkg._abi.LIB_PATH):
        pytest.skip("librsf_hip.so not built (run __graft_entry__.build())")
    return pkg._abi.load()


def _finish(lib, n, part, center, S, n_lags):
    d = part.shape[0]
    part = np.ascontiguousarray(part, dtype=np.float64)
    c = np.ascontiguousarray(np.broadcast_to(np.asarray(center, np.float64), (d,)))
    out = np.empty((d, 11))
    dbl = ctypes.POINTER(ctypes.c_double)
    rc = lib.rsf_diag_finish(n, d, S, c.ctypes.data_as(dbl), part.ctypes.data_as(dbl), n_lags, out.ctypes.data_as(dbl))
    assert rc == 0, lib.rsf_last_error()
    return out


def _compare(lib, n, part, center, S, n_lags, rtol=1e-13):
    part64 = np.asarray(part, dtype=np.float64)[:, : ref.HEAD + n_lags]
    got = _finish(lib, n, part64, center, S, n_lags)
    want = ref.finish(n, part64, center, S, n_lags)  # the same float64 partials, finished in long double
    for p, w in enumerate(want):
        for i, k in enumerate(ref.OUT):
            g, e = got[p, i], float(w[k])
            if np.isnan(e):
                assert np.isnan(g), (p, k, g)
            else:
                assert abs(g - e) <= rtol * max(abs(e), 1e-300), (p, k, g, e)
    return got, want


def _ar1(n, C, d, phi, seed):
    rng = np.random.default_rng(seed)
    x = np.empty((n, C, d))
    x[0] = rng.standard_normal((C, d)) / np.sqrt(1 - phi * phi)
    for i in range(1, n):
        x[i] = phi * x[i - 1] + rng.standard_normal((C, d))
    return x + 1000.0


@pytest.mark.parametrize("n", [200, 201])
def test_finish_truncated_sequence(hip_lib, n):
    x = _ar1(n, 16, 3, 0.5, n)
    tr = ref.Trace(x, superchain_size=4)
    got, want = _compare(hip_lib, n, tr.partials(), tr.center, 4, n // 2)
    assert all(w["lags_complete"] for w in want) and np.all(got[:, 10] == 1)
    assert np.all(np.isfinite(got[:, :10]))


@pytest.mark.parametrize("n", [10, 11])
def test_finish_untruncated_sequence(hip_lib, n):
    # N = 5: Geyer's loop takes the pair (2, 3) and stops at t = 3 = N - 2 by length, its pair still positive
    x = _ar1(n, 64, 1, 0.9, n)
    tr = ref.Trace(x)
    _compare(hip_lib, n, tr.partials(), tr.center, 0, n // 2)
    w = ref.finish(n, tr.partials(), tr.center)[0]
    rho = 1 - (w["W"] - tr.lag_sums(0, n // 2)[0] / (2 * 64)) / w["var_plus"]
    assert rho[2] + rho[3] > 0 and w["lags_complete"]


def test_finish_lags_incomplete(hip_lib):
    x = _ar1(400, 8, 1, 0.95, 3)
    tr = ref.Trace(x)
    got, want = _compare(hip_lib, 400, tr.partials(0, 6), tr.center, 0, 6)
    assert not want[0]["lags_complete"] and got[0, 10] == 0
    full = ref.finish(400, tr.partials(), tr.center)[0]
    assert full["lags_complete"] and full["tau"] > want[0]["tau"]


def test_finish_constant_chains_and_nonfinite(hip_lib):
    x = np.tile(np.array([5.0, 6.0, 7.0])[None, :, None], (12, 1, 2))
    x[3, 1, 1] = np.nan
    tr = ref.Trace(x, superchain_size=3)
    got, _ = _compare(hip_lib, 12, tr.partials(), tr.center, 3, 6)
    assert np.all(np.isnan(got[0, [4, 7, 8, 9]])) and got[0, 2] == 0.0  # W = 0
    assert np.all(np.isnan(got[1, [0, 1, 2, 3, 4, 5, 7, 8, 9]]))        # a NaN draw
    assert got[1, 6] == 1 and got[1, 10] == 1


def test_finish_validates_arguments(hip_lib):
    part = np.zeros((1, ref.HEAD + 4))
    c = np.zeros(3)
    out = np.empty((3, 11))
    dbl = ctypes.POINTER(ctypes.c_double)
    P, Cp, O = part.ctypes.data_as(dbl), c.ctypes.data_as(dbl), out.ctypes.data_as(dbl)
    f = hip_lib.rsf_diag_finish
    assert f(8, 1, 0, Cp, P, 4, O) == 0
    for args in [(3, 1, 0, Cp, P, 2, O), (8, 0, 0, Cp, P, 4, O), (8, 4, 0, Cp, P, 4, O), (8, 1, -1, Cp, P, 4, O),
                 (8, 1, 0, Cp, P, 1, O), (8, 1, 0, Cp, P, 5, O), (8, 1, 0, None, P, 4, O), (8, 1, 0, Cp, None, 4, O),
                 (8, 1, 0, Cp, P, 4, None)]:
        assert f(*args) == -1, args
        assert hip_lib.rsf_last_error()
