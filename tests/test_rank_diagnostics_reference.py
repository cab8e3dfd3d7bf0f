"""
CPU tests that pin tests/rank_diagnostics_reference.py, the specification of the rank-normalised diagnostics: hand cases for
ranks, scores and the HDI, NumPy's order statistics, the exact invariance of rank statistics under a monotone map, the iid
limit, the middle row of an odd n, constant parameters, signed zeros and non-finite draws.
"""
import numpy as np
from scipy import special

import rank_diagnostics_reference as rref


def _ar1(n, C, phi, seed):
    rng = np.random.default_rng(seed)
    x = np.empty((n, C))
    cur = rng.standard_normal(C) / np.sqrt(1 - phi * phi)
    for i in range(n):
        x[i] = cur
        cur = phi * cur + rng.standard_normal(C)
    return x


def test_ranks_and_scores_hand_case():
    # split set of 8 draws: -1.0 ranks 1; three ties at 1.0 share rank 3, two at 2.5 share 5.5; then 7 and 8
    v = np.array([1.0, 2.5, 1.0, -1.0, 2.5, 1.0, 7.0, 9.0])
    want_r = np.array([3.0, 5.5, 3.0, 1.0, 5.5, 3.0, 7.0, 8.0])
    z = rref.normal_scores(v)
    assert np.array_equal(z, special.ndtri((want_r - 0.375) / 8.25))
    assert z[0] == z[2] == z[5] and z[1] == z[4]
    # the same draws as a trace of 4 rows and 2 chains: the series is z at each draw's place
    _, ser = rref.prepare(v.reshape(4, 2))
    assert np.array_equal(ser[0, :, :, 0], z.reshape(4, 2))


def test_median_and_quantiles_are_numpys():
    rng = np.random.default_rng(1)
    for shape in ((20, 7), (21, 7), (5, 1)):
        x = rng.standard_normal(shape).round(1)
        probs = (0.0, 0.025, 0.05, 1 / 3, 0.5, 0.95, 0.975, 1.0)
        st, _ = rref.prepare(x, probs)
        assert st[0, 0] == np.median(x)
        assert np.array_equal(st[0, 1:3], np.quantile(x, [0.05, 0.95]))
        assert np.array_equal(st[0, len(rref.STATS):], np.quantile(x, probs))


def test_hdi_hand_case():
    # A = 8, k = floor(0.5 * 8) = 4: widths 11, 11, 11, 20; the first narrowest window starts at 0
    v = np.array([12.0, 0.0, 30.0, 2.0, 11.0, 1.0, 13.0, 10.0])
    assert rref.hdi(v, 0.5) == (0.0, 11.0)
    assert rref.hdi(v, 0.3) == (0.0, 2.0)  # k = 2: widths 2, 10, 10, 2, 2, 19 -> i = 0
    st, _ = rref.prepare(v.reshape(4, 2), hdi_prob=0.5)
    assert tuple(st[0, 3:5]) == (0.0, 11.0)


def test_bulk_statistics_invariant_under_exp():
    x = _ar1(60, 40, 0.8, 2) * 0.5
    y = np.exp(x)
    assert np.unique(y).size == np.unique(x).size == x.size  # exp made no new ties
    a, b = rref.rank_diagnostics(x)[0], rref.rank_diagnostics(y)[0]
    assert a["rhat_bulk"] == b["rhat_bulk"] and a["ess_bulk"] == b["ess_bulk"]
    assert a["ess_tail"] == b["ess_tail"]  # the indicators only compare with quantiles, which exp keeps in order


def test_iid_cauchy_chains():
    x = np.random.default_rng(3).standard_cauchy((400, 8))
    r = rref.rank_diagnostics(x)[0]
    T = 400 * 8
    assert abs(r["rhat"] - 1) < 0.01
    assert 0.8 * T < r["ess_bulk"] < 1.25 * T
    assert 0.7 * T < r["ess_tail"] < 1.3 * T


def test_odd_n_leaves_middle_row_out():
    x = _ar1(41, 6, 0.5, 4)
    x[20] = 1e6  # the middle row: would take the top ranks if it counted
    _, ser = rref.prepare(x)
    _, even = rref.prepare(np.delete(x, 20, axis=0))
    assert np.all(ser[:, 20] == 0.0)
    assert np.array_equal(np.delete(ser, 20, axis=1)[0], even[0])  # bulk ranks; the folded series' median is the full set's
    assert ser[0].max() < 3  # z of T = 240 draws


def test_constant_parameter():
    x = np.stack([_ar1(30, 5, 0.3, 5), np.full((30, 5), 2.5)], axis=2)
    st, _ = rref.prepare(x)
    assert list(st[1, 6:10]) == [1.0, 1.0, 1.0, 1.0] and list(st[0, 6:10]) == [0.0, 0.0, 0.0, 0.0]
    r = rref.rank_diagnostics(x)
    assert r[1]["ess_bulk"] == 2 * 5 * 15 and r[1]["ess_tail"] == 2 * 5 * 15 and np.isnan(r[1]["rhat"])
    assert np.isfinite(r[0]["rhat"]) and r[0]["ess_bulk"] < 2 * 5 * 15


def test_signed_zeros_tie():
    v = np.array([-0.0, 1.0, 0.0, -1.0, 0.0, -0.0, 2.0, 3.0])
    z = rref.normal_scores(v)
    assert z[0] == z[2] == z[4] == z[5]  # four tied zeros share the average rank 3.5
    assert z[0] == special.ndtri((3.5 - 0.375) / 8.25)
    assert rref.hdi(v, 0.5)[1] - rref.hdi(v, 0.5)[0] == 1.0


def test_non_finite_draw_in_one_parameter_only():
    x = np.stack([_ar1(30, 5, 0.3, 6), _ar1(30, 5, 0.3, 7)], axis=2)
    x[4, 2, 1] = np.nan
    st, ser = rref.prepare(x, (0.5,))
    assert st[1, 5] == 1.0 and np.isnan(st[1, :5]).all() and np.isnan(st[1, -1]) and np.isnan(ser[..., 1]).all()
    assert st[0, 5] == 0.0 and np.isfinite(ser[..., 0]).all()
    r = rref.rank_diagnostics(x, (0.5,))
    assert all(np.isnan(r[1][k]) for k in rref.OUT[:-1]) and r[1]["lags_complete"]
    assert np.isfinite(r[0]["rhat"]) and np.isfinite(r[0]["ess_tail"])
