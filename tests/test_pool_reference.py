"""
CPU tests of the specification tests/pool_reference.py (rsf_pool_summary, rsf_pool_kde, rsf_pool_histogram of include/rsf_abi.h)
against independent witnesses — np.mean, np.var, SciPy's gaussian_kde, np.histogram — of the non-finite rule against the CPU
restatement, and of the bounds of tests/pool_cases.py: that a plain float64 sum of the library's form stays inside them.

The KDE bound is rtol 1e-9 over points whose true density exceeds 1e-290; on these inputs (n = 5000, 1000 grid points, both
bandwidths) SciPy itself sits up to 3.9e-12 from the long-double value, and the CPU restatement up to 2.0e-12 (both printed below).
"""
import numpy as np
import pytest
from scipy.stats import gaussian_kde

import pool_cases as cases
import pool_reference as ref

@pytest.mark.parametrize("col", cases.COLUMNS)
def test_summary_against_numpy(col):
    for n in (1, 2, 70, 256 * 3 + 5, 16421):
        _, _, x = cases.column(n, col)
        s = ref.summary(x)
        assert s["n"] == n and s["min"] == x.min() and s["max"] == x.max()
        sd = x.std()
        # the witness is the weaker side: np.mean sums the uncentred values pairwise, log2(n) roundings of |mean|
        assert abs(float(s["mean"]) - x.mean()) <= 16 * np.spacing(abs(x.mean())) + 1e-13 * sd
        if n > 1:
            assert abs(float(s["var"]) - x.var(ddof=1)) <= 1e-11 * x.var(ddof=1)
        else:
            assert s["var"] == 0


def test_kde_against_scipy(cpu_engine):
    x = cases.column(5000, 1)[2]
    for bw in (0.0, 0.3):
        grid = cases.kde_grid(x, 1000, ref.bandwidth(x, bw))
        want = ref.kde(x, grid, bw)
        big = want > cases.joint_cases.KDE_FLOOR
        assert want[0] > 1.0 and big.sum() >= 100 and (~big).sum() >= 20 and want[-1] < 1e-300, "the grid runs from the mode past underflow"
        sp = gaussian_kde(x, bw_method=bw if bw > 0 else None).pdf(grid)
        own = cpu_engine.pool_kde(x, grid, bw_factor=bw)
        rel = float((np.abs(sp[big] - want[big]) / want[big]).max())
        rel_own = float((np.abs(own[big] - want[big]) / want[big]).max())
        print(f"n=5000 bw={bw}: SciPy against long double {rel:.2e}, the CPU restatement {rel_own:.2e}")
        assert rel <= cases.joint_cases.RTOL_KDE and rel_own <= cases.joint_cases.RTOL_KDE
        assert np.all(np.abs(own[~big] - want[~big].astype(np.float64)) <= cases.joint_cases.ATOL_KDE)
    # the chunked sum is the plain one: a pool that spans three chunks against one pass
    y = cases.column(2 * ref.CHUNK + 77, "vector")[2]
    g = cases.kde_grid(y, 3, ref.bandwidth(y))
    c = ref.bandwidth(y)
    plain = np.array([np.exp(-(gj - y.astype(ref.LD)) ** 2 / (2 * c)).sum(dtype=ref.LD) for gj in g.astype(ref.LD)])
    plain /= ref.LD(y.size) * np.sqrt(2 * ref.LD(np.pi) * c)
    assert np.all(np.abs(ref.kde(y, g) - plain) <= 1e-17 * plain)


def test_kde_refuses():
    for bad in ([1.0], [2.0, 2.0, 2.0], [1.0, np.nan, 2.0], [1.0, np.inf, 2.0]):
        with pytest.raises(ValueError):
            ref.kde(bad, [1.0])


def test_histogram_against_numpy(cpu_engine):
    # the edge cases of tests/test_gpu_parity.py::test_pool_histogram: samples on the bin edges and one ulp either side
    for nbins, lo, hi in ((10, 0.0, 1.0), (100, 0.005, 0.02), (7, 0.008, 0.014), (1000, 900.0, 1100.0), (3, -1.0, 2.0), (1, 0.0, 1.0)):
        edges = np.linspace(lo, hi, nbins + 1)
        x = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [0.3, 0.7, lo + 0.3 * (hi - lo)],
                            [np.nan, np.inf, -np.inf, np.nan]])
        got = ref.histogram(x, nbins, lo, hi)
        assert got.shape == (nbins + 2,) and got.sum() == x.size
        assert np.array_equal(got[1:-1], np.histogram(x[np.isfinite(x)], nbins, (lo, hi))[0])
        assert got[0] == (x < lo).sum() and got[-1] == (x > hi).sum() + 2, "NaN goes to the upper border"
        assert np.array_equal(got, cpu_engine.pool_histogram(x, nbins, lo, hi))
    for col in (1, 2):
        b, p, x = cases.column(cases.HIST_SIZE, col)
        nbins, lo, hi = cases.hist_range(x)
        got = ref.histogram(x, nbins, lo, hi)
        assert got[0] > 0 and got[-1] > 0 and got.sum() == x.size
        assert np.array_equal(got, cpu_engine.pool_histogram(b, nbins, lo, hi, param=p))
    with pytest.raises(ValueError):
        ref.histogram([1.0], 4, 1.0, 1.0)


@pytest.mark.parametrize("name", [c[0] for c in cases.NONFINITE])
def test_non_finite_rule(cpu_engine, name):
    """The rule, case by case, in the specification and in the CPU restatement (oracle/rsf_oracle.c)."""
    (x, n, nan_moments, mn, mx), = [c[1:] for c in cases.NONFINITE if c[0] == name]
    for s in (ref.summary(x), cpu_engine.pool_summary(np.array(x))):
        assert s["n"] == n
        assert np.isnan(s["mean"]) and np.isnan(s["var"]) and nan_moments
        for got, want in ((s["min"], mn), (s["max"], mx)):
            assert (np.isnan(got) and np.isnan(want)) or got == want, (name, s)
    # a strided column whose neighbours are finite; and a finite column next to a non-finite one is untouched
    blk = np.column_stack([np.arange(len(x), dtype=np.float64), np.array(x), np.ones(len(x))])
    s = cpu_engine.pool_summary(blk, param=1)
    assert np.isnan(s["mean"]) and np.isnan(s["var"]) and s["n"] == n
    s0 = cpu_engine.pool_summary(blk, param=0)
    assert s0["mean"] == (n - 1) / 2 and s0["min"] == 0.0 and s0["max"] == n - 1


def test_non_finite_draws_refuse_the_kde(pkg, cpu_engine):
    for bad in ([1.0, np.nan, 2.0], [np.nan, 1.0, 2.0], [1.0, np.inf, 2.0], [-np.inf, 1.0, 2.0]):
        with pytest.raises(pkg.RsfError, match="rsf_pool_kde") as ei:
            cpu_engine.pool_kde(np.array(bad), np.array([1.0]))
        assert ei.value.code == -1
    for bad in ([1.0], [2.0, 2.0, 2.0]):
        with pytest.raises(pkg.RsfError, match="rsf_pool_kde"):
            cpu_engine.pool_kde(np.array(bad), np.array([1.0]))


@pytest.mark.parametrize("n", cases.FAR_SIZES)
def test_far_first_draw_bound_can_be_met(n):
    """A plain float64 one-pass shifted sum about x[0] (np.sum), x[0] k sd from the bulk, stays inside the scaled bounds."""
    for col in cases.FAR_COLUMNS:
        for k in cases.FAR_K:
            _, _, x = cases.far_first(n, col, k)
            want = ref.summary(x)
            z = abs(x[0] - x[1:].mean()) / x[1:].std()
            assert abs(z / k - 1) < 1e-6 and (want["max"] if col == "vector" else want["min"]) == x[0]
            with pytest.raises(AssertionError):
                cases.check_center(x)  # the benign condition does not hold: these legs have a bound of their own
            mean, var = cases.shifted_one_pass(x)
            got = {"n": n, "mean": mean, "var": var, "min": x.min(), "max": x.max()}
            cases.check_summary(got, want, f"float64 one-pass about x[0], n={n} column {col} k={k:g}", k=k)
    # ... and the benign bound holds for the same form when x[0] is a draw of the bulk
    _, _, x = cases.column(n, "vector")
    mean, var = cases.shifted_one_pass(x)
    cases.check_summary({"n": n, "mean": mean, "var": var, "min": x.min(), "max": x.max()}, ref.summary(x), f"float64 one-pass, benign n={n}")
