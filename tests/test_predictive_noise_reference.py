"""
CPU tests of the specification of the predictive band with noise itself (tests/predictive_noise_reference.py): closed forms, the
bracket, the round trip, monotonicity, the non-finite rules, the measurement that sizes the GPU test's pass bounds, and the
agreement of the C header with the ctypes table.
"""
import math
import os
import re

import numpy as np
import pytest
from scipy.special import ndtri

import predictive_noise_cases as cases
import predictive_noise_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (1e-6, 0.025, 0.05, 0.5, 0.95, 0.999, 1.0 - 1e-6)


def _ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


def test_one_draw_is_its_normal_quantile():
    for y, s in ((0.7, 0.05), (-3.0, 2.0), (0.0, 1e-3)):
        for p in PROBS:
            got = ref.quantile_row(np.array([y]), np.array([s]), p)
            want = y + ndtri(p) * s
            assert _ulps(got, want) <= 2 if want != 0.0 else got == 0.0, (y, s, p, got, want)


def test_equal_draws_are_one_normal():
    """n equal components are one component: the same closed form.  (The bracket is a point; F_ref sums n equal terms exactly.)"""
    for n in (5, 1037):
        y, s = np.full(n, -1.3), np.full(n, 0.2)
        for p in PROBS:
            assert _ulps(ref.quantile_row(y, s, p), -1.3 + ndtri(p) * 0.2) <= 2


def test_symmetric_two_point_mixture_has_its_median_in_the_middle():
    y, s = np.array([-1.0, 3.0]), np.array([0.5, 0.5])
    assert abs(ref.quantile_row(y, s, 0.5) - 1.0) <= 4 * np.finfo(np.float64).eps
    # closer components, where F' at the middle is not small
    y = np.array([0.75, 1.25])
    assert abs(ref.quantile_row(y, s, 0.5) - 1.0) <= 4 * np.finfo(np.float64).eps


def test_round_trip_on_random_rows():
    """Q(F(t)) = t to the conditioning of the root: |Q(F(t)) - t| F'(t) <= a few eps (the rounding of p = F(t) itself)."""
    rng = np.random.default_rng(5)
    for n in (3, 64, 517):
        y, s = rng.standard_normal(n), rng.uniform(0.05, 0.5, n)
        for t in np.quantile(y, [0.02, 0.3, 0.5, 0.8, 0.99]):
            p = ref.cdf(y, s, t)
            back = ref.quantile_row(y, s, p)
            dens = math.fsum(np.exp(-0.5 * ((t - y) / s) ** 2) / (s * math.sqrt(2 * math.pi))) / n
            assert abs(back - t) * dens <= 8 * np.finfo(np.float64).eps * max(p, abs(t) * dens), (n, t, back)


def test_bracket_holds():
    rng = np.random.default_rng(6)
    for name, series, std2, _ in cases.crafted():
        s = np.sqrt(std2)
        for y in series:
            for p in PROBS:
                lo, hi = ref.bracket(y, s, p)
                # (F_ref is exact up to the element function: a few ulp of p)
                assert ref.cdf(y, s, lo) <= p * (1 + 1e-14) and ref.cdf(y, s, hi) >= p * (1 - 1e-14) - 1e-16, (name, p)
    y, s = rng.standard_normal(1), np.array([0.3])
    assert ref.bracket(y, s, 0.3)[0] == ref.bracket(y, s, 0.3)[1]


def test_quantile_is_monotone_in_p():
    probs = np.concatenate([[1e-6], np.linspace(0.01, 0.99, 23), [1 - 1e-6]])
    for name, series, std2, _ in cases.crafted():
        if series.shape[1] > 1100:
            continue  # (the small cases: brentq costs tens of evaluations each)
        q = ref.quantiles(series, std2, probs)
        assert np.all(np.diff(q, axis=0) >= 0), name


def test_non_finite_row_and_bad_std2():
    rng = np.random.default_rng(7)
    y, s2 = rng.standard_normal((3, 40)), rng.uniform(0.01, 0.1, 40)
    y[1, 7] = np.inf
    q = ref.quantiles(y, s2, (0.05, 0.5))
    assert np.isnan(q[:, 1]).all() and np.isfinite(q[:, [0, 2]]).all()
    y[1, 7] = np.nan
    assert np.isnan(ref.quantiles(y, s2, (0.05, 0.5))[:, 1]).all()
    y[1, 7] = 0.0
    for bad in (0.0, -1.0, np.inf, np.nan):
        b = s2.copy()
        b[11] = bad
        assert np.isnan(ref.quantiles(y, b, (0.05, 0.5))).all(), bad
    with pytest.raises(ValueError):
        ref.quantiles(y, s2, (0.0,))
    with pytest.raises(ValueError):
        ref.quantiles(y, s2, (float("nan"),))


def test_row_zero_is_an_ordinary_row():
    (series, std2, probs), = [(y, s2, p) for name, y, s2, p in cases.crafted() if name == "k0"]
    q = ref.quantiles(series[:, :300], std2[:300], (0.05, 0.5, 0.95))[:, 0]
    assert q[1] == 0.0 and q[0] < 0 < q[2] and abs(q[0] + q[2]) <= 1e-15 * q[2]


def test_scheme_sizes_the_pass_bounds():
    """The library's iteration in float64 NumPy on the crafted cases: its residual against F_ref and its passes are what
    predictive_noise_cases.py records; it agrees with the brentq root to the root's conditioning."""
    worst = 0.0
    for name, series, std2, probs in cases.crafted():
        s = np.sqrt(std2)
        most = 0
        for y in series:
            for p in probs:
                t, passes = ref.scheme(y, s, p)
                worst = max(worst, abs(ref.cdf(y, s, t) - p))
                most = max(most, passes)
        print(f"{name}: passes {most} (recorded {cases.SCHEME_PASSES[name]})")
        assert most <= cases.SCHEME_PASSES[name] <= ref.MAX_PASSES, name
    print(f"largest residual {worst:.3e} (recorded {cases.SCHEME_RESIDUAL:.3e})")
    assert worst <= cases.SCHEME_RESIDUAL <= cases.TOL_RESIDUAL / 100
    # n = 5: the scheme's t and brentq's agree where the root is well conditioned
    (series, std2), = [(y, s2) for name, y, s2, _ in cases.crafted() if name == "n5"]
    for p in (0.05, 0.5, 0.95):
        t, _ = ref.scheme(series[0], np.sqrt(std2), p)
        assert abs(t - ref.quantile_row(series[0], np.sqrt(std2), p)) <= 1e-13


def test_header_and_binding_declare_the_same_symbols(pkg):
    """include/rsf_predict_noise.h against _abi.PREDICT_NOISE_PROTOTYPES: names, argument counts and the pass cap; the header is
    included by rsf_predict.h and adds nothing to rsf_abi.h."""
    abi = pkg._abi
    text = open(os.path.join(ROOT, "include", "rsf_predict_noise.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsf_\w+)\s*\(([^)]*)\)\s*;", code)}
    assert set(decl) == set(abi.PREDICT_NOISE_PROTOTYPES) == {"rsf_predict_noise_quantiles"}
    for name, args in decl.items():
        assert len(args.split(",")) == len(abi.PREDICT_NOISE_PROTOTYPES[name][1]), name
    assert int(re.search(r"#define\s+RSF_PREDICT_NOISE_MAX_PASSES\s+(\d+)", code).group(1)) == abi.PREDICT_NOISE_MAX_PASSES == ref.MAX_PASSES
    assert '#include "rsf_predict_noise.h"' in open(os.path.join(ROOT, "include", "rsf_predict.h")).read()
    assert not set(abi.PREDICT_NOISE_PROTOTYPES) & set(abi.PROTOTYPES)
    assert "rsf_predict_noise" not in open(os.path.join(ROOT, "include", "rsf_abi.h")).read()
