"""
CPU tests of the specification tests/joint_reference.py (include/rsf_joint.h) against independent witnesses — SciPy's
gaussian_kde, np.cov, np.corrcoef, np.histogram2d — and of the agreement of the C header with the ctypes table.

The 2-D KDE bound is rtol 1e-9 over points whose true density exceeds 1e-290; on these inputs SciPy itself sits up to 5.4e-12
from the extended-precision value, and the float64 restatement of the library's whitened scheme (whitened_float64), centred on
the mean, up to 9.2e-13 (both printed below).
"""
import os
import re

import numpy as np
import pytest
from scipy.stats import gaussian_kde

import joint_cases as cases
import joint_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def whitened_float64(x2, points, bw_factor=0.0):
    """The library's scheme in float64 NumPy: centre on the mean, W = L^-1 / sqrt 2, exponent -(du^2 + dv^2)."""
    n = x2.shape[0]
    c = x2.mean(0)
    f = bw_factor if bw_factor > 0 else n ** (-1.0 / 6.0)
    H = np.cov(x2.T) * f * f
    l00 = np.sqrt(H[0, 0]); l10 = H[0, 1] / l00; l11 = np.sqrt((H[0, 0] * H[1, 1] - H[0, 1] ** 2) / H[0, 0])
    r = np.sqrt(0.5)
    w00, w10, w11 = r / l00, -r * l10 / (l00 * l11), r / l11

    def white(a):
        da, db = a[:, 0] - c[0], a[:, 1] - c[1]
        return w00 * da, w10 * da + w11 * db

    (su, sv), (pu, pv) = white(x2), white(points)
    e = (pu[:, None] - su[None, :]) ** 2 + (pv[:, None] - sv[None, :]) ** 2
    return np.exp(-e).sum(axis=1) / (n * 2.0 * np.pi * l00 * l11)


@pytest.mark.parametrize("n", [5, 1037])
@pytest.mark.parametrize("pair", [(0, 1), (2, 0)])
def test_kde2d_against_scipy(n, pair):
    x = cases.synthetic(n, 3)
    x2 = np.ascontiguousarray(x[:, list(pair)])
    pts = np.vstack([cases.mesh(x2, 8.0, 9, 7), cases.scattered(x2, 50, n)])
    want = ref.kde2d(x2, pts)
    big = want > cases.KDE_FLOOR
    for bw in (0.0, 0.37):
        want = ref.kde2d(x2, pts, bw_factor=bw)
        big = want > cases.KDE_FLOOR
        sp = gaussian_kde(x2.T, bw_method=bw if bw > 0 else None).pdf(pts.T)
        rel = np.abs(sp[big] - want[big]) / want[big]
        own = np.abs(whitened_float64(x2, pts, bw)[big] - want[big]) / want[big]
        print(f"n={n} pair={pair} bw={bw}: SciPy against long double {float(rel.max()):.2e}, whitened float64 scheme {float(own.max()):.2e}")
        assert big.sum() >= 50 and rel.max() <= cases.RTOL_KDE and own.max() <= cases.RTOL_KDE


def test_kde2d_shards_add_and_collinear_raises():
    x2 = cases.synthetic(1037, 3)[:, :2]
    pts = cases.scattered(x2, 20, 3)
    cov = np.cov(x2.T)
    whole = ref.kde2d(x2, pts)
    parts = sum(ref.kde2d(s, pts, cov2=cov, n_total=1037) for s in (x2[:100], x2[100:611], x2[611:]))
    # cov in float64 is the long-double covariance rounded: 1e-16 relative in H, times an exponent of up to a few hundred
    assert np.all(np.abs(parts - whole) <= 1e-12 * whole)
    line = np.column_stack([x2[:, 0], 2.0 * x2[:, 0]])
    with pytest.raises(ValueError):
        ref.kde2d(line, pts)
    with pytest.raises(ValueError):
        ref.kde2d(x2[:2], pts)
    with pytest.raises(np.linalg.LinAlgError):
        gaussian_kde(line.T)


@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_moments_against_numpy(d):
    for n in (2, 5, 1037):
        x = cases.synthetic(n, d)
        for c in (x[0], cases.given_center(x) if n > 2 else x[1]):
            m = ref.moments(x, c)
            cov = np.atleast_2d(np.cov(x.T))
            sd = np.sqrt(np.diag(cov))
            assert m["n"] == n and m["nonfinite"] == 0
            # the witness is the weaker side here: np.mean sums the uncentred values pairwise, log2(n) roundings of |mean|
            assert np.all(np.abs(m["mean"].astype(np.float64) - x.mean(0)) <= 16 * np.spacing(np.abs(x.mean(0))) + 1e-13 * sd)
            assert np.all(np.abs(m["cov"].astype(np.float64) - cov) <= 1e-11 * np.outer(sd, sd))
            assert np.all(np.abs(m["corr"].astype(np.float64) - np.atleast_2d(np.corrcoef(x.T))) <= 1e-11)


def test_moments_edge_cases():
    x = cases.synthetic(40, 3)
    y = x.copy()
    y[3, 1], y[17, 0], y[30, 2] = np.nan, np.inf, -np.inf
    keep = np.isfinite(y).all(axis=1)
    m, want = ref.moments(y, x[0]), ref.moments(x[keep], x[0])
    assert m["nonfinite"] == 3 and m["n"] == 37
    assert np.array_equal(m["cov"], want["cov"]) and np.array_equal(m["mean"], want["mean"])
    one = ref.moments(x[:1], x[0])
    assert one["n"] == 1 and np.isnan(one["cov"]).all() and np.isnan(one["corr"]).all() and np.array_equal(one["mean"].astype(np.float64), x[0])
    z = x.copy()
    z[:, 1] = 0.011
    corr = ref.moments(z, z[0])["corr"]
    assert np.isnan(corr[1]).all() and np.isnan(corr[:, 1]).all() and abs(corr[0, 0] - 1) <= 1e-18 and np.isfinite(corr[0, 2])
    # shards about a common centre add
    a, b = ref.partials(x[:13], x[5]), ref.partials(x[13:], x[5])
    assert np.all(np.abs((a + b) - ref.partials(x, x[5])) <= 1e-17 * np.abs(ref.partials(x, x[5])) + 1e-30)


@pytest.mark.parametrize("nbins", [(1, 1), (20, 16), (126, 126)])
def test_hist2d_against_numpy(nbins):
    nbx, nby = nbins
    x, ((lo_a, hi_a), (lo_b, hi_b)) = cases.edge_block(1037, nbx, nby, 11)
    counts = ref.hist2d(x[:, 0], x[:, 2], nbx, nby, lo_a, hi_a, lo_b, hi_b)
    assert counts.shape == (nbx + 2, nby + 2) and counts.sum() == x.shape[0]
    fin = np.isfinite(x[:, 0]) & np.isfinite(x[:, 2])
    want = np.histogram2d(x[fin, 0], x[fin, 2], (nbx, nby), ((lo_a, hi_a), (lo_b, hi_b)))[0]
    assert np.array_equal(counts[1:-1, 1:-1], want)
    # the per-axis index is the 1-D histogram's: the marginal of the table is np.histogram's, with the out-of-range rows outside
    in_b = (x[:, 2] >= lo_b) & (x[:, 2] <= hi_b)
    assert np.array_equal(counts[1:-1, 1:-1].sum(axis=1), np.histogram(x[in_b & fin, 0], nbx, (lo_a, hi_a))[0])
    assert counts[0].sum() == (x[:, 0] < lo_a).sum() and counts[-1].sum() == (~(x[:, 0] <= hi_a)).sum()
    assert counts[:, 0].sum() == (x[:, 2] < lo_b).sum() and counts[:, -1].sum() == (~(x[:, 2] <= hi_b)).sum()
    assert (ref.axis_index(x[:, 0], nbx, lo_a, hi_a) == nbx).sum() >= (x[:, 0] == hi_a).sum() > 0 or nbx > 1


@pytest.mark.parametrize("name", sorted(cases.HPD_CASES))
def test_hpd_levels_hand_made(name):
    w, probs, want = cases.HPD_CASES[name]
    got = ref.hpd_levels(w, probs)
    assert np.array_equal(got, np.array(want)), (got, want)
    w = np.asarray(w)
    for p, lv in zip(probs, got):  # the definition itself
        assert w[w >= lv].sum() >= p * w.sum() and w[w > lv].sum() < p * w.sum()


def test_hpd_levels_refuses():
    for bad in ([1.0, -1.0], [np.nan, 1.0], [0.0, 0.0], [np.inf]):
        with pytest.raises(ValueError):
            ref.hpd_levels(bad, (0.5,))
    for p in (0.0, 1.0, np.nan):
        with pytest.raises(ValueError):
            ref.hpd_levels([1.0, 2.0], (p,))


def test_header_and_binding_declare_the_same_symbols(pkg):
    """include/rsf_joint.h against _abi.JOINT_PROTOTYPES: names, argument counts and the constants; nothing is added to rsf_abi.h."""
    abi = pkg._abi
    text = open(os.path.join(ROOT, "include", "rsf_joint.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = dict(re.findall(r"\bint\s+(rsf_\w+)\s*\(([^;]*)\)\s*;", code))
    names = {"rsf_pool_joint_partials", "rsf_pool_joint_finish", "rsf_pool_kde2d", "rsf_pool_histogram2d", "rsf_pool_hpd_levels"}
    assert set(decl) == set(abi.JOINT_PROTOTYPES) == names
    for name, args in decl.items():
        assert len(args.split(",")) == len(abi.JOINT_PROTOTYPES[name][1]), name
    const = {k: int(v) for k, v in re.findall(r"#define\s+(RSF_\w+)\s+(\d+)\b", code)}
    assert const["RSF_JOINT_HEAD"] == abi.JOINT_HEAD == ref.HEAD
    assert const["RSF_JOINT_MAX_PARAMS"] == abi.JOINT_MAX_PARAMS == ref.MAX_PARAMS
    assert const["RSF_HIST2D_MAX_CELLS"] == abi.HIST2D_MAX_CELLS == ref.HIST2D_MAX_CELLS
    assert abi.JOINT_OUT == ("mean", "cov", "corr")
    assert not set(abi.JOINT_PROTOTYPES) & set(abi.PROTOTYPES)
    assert "rsf_pool_joint" not in open(os.path.join(ROOT, "include", "rsf_abi.h")).read()
    from bayesian_markov_chain_monte_carlo_amd import dist as rdist

    assert rdist.allreduce_joint_partials.__doc__
