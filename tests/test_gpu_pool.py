"""
GPU tests of the one-column post-processing of the pooled draws (include/rsf_abi.h: rsf_pool_summary, rsf_pool_kde,
rsf_pool_histogram; Engine.pool_summary, pool_kde, pool_histogram) against the specification tests/pool_reference.py.
tests/pool_cases.py holds the sizes — past the caps of the grids: the second trip of pool_moments_kernel's grid-stride loop, the
multi-tile loop of pool_kde_kernel, its second pass over the grid points — the bounds and the conditions they rest on.

Every test prints its measured error over its bound (run with -s); DESIGN.md, "The one-column family past its grid caps".
"""
import numpy as np
import pytest

import pool_cases as cases
import pool_reference as ref

pytestmark = pytest.mark.gpu

_MEMO = {}


@pytest.fixture(scope="module")
def dev_engine(pkg):
    e = pkg.Engine(mem="device")
    yield e
    e.close()


def _dev(a):
    import torch

    return torch.tensor(np.asarray(a), device="cuda")  # a copy: the shared inputs are read-only


def _same(a, b):
    """Two summaries agree bit for bit (NaN equal to NaN)."""
    return all(np.array_equal(np.float64(a[k]), np.float64(b[k]), equal_nan=True) for k in ("n", "mean", "var", "min", "max"))


# ---- summary ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", cases.SUMMARY_SIZES)
def test_summary(gpu_engine, dev_engine, n):
    for col in cases.COLUMNS:
        samples, p, x = cases.column(n, col)
        cases.check_center(x)
        want = ref.summary(x)
        got = gpu_engine.pool_summary(samples, param=p)
        cases.check_summary(got, want, f"summary n={n} column {col}")
        if n == 1:
            assert got["var"] == 0.0 and got["mean"] == x[0]
        # device memory: the same kernel on the caller's own buffer, the same bits; and again
        assert _same(dev_engine.pool_summary(_dev(samples), param=p), got)
        assert _same(gpu_engine.pool_summary(samples, param=p), got)


@pytest.mark.parametrize("n", cases.FAR_SIZES)
def test_summary_far_first_draw(gpu_engine, dev_engine, n):
    """x[0], the shift of the one-pass sums, k sd from the bulk: the variance within 1e-11 (1 + k^2) / 101 (pool_cases.py)."""
    for col in cases.FAR_COLUMNS:
        for k in cases.FAR_K:
            samples, p, x = cases.far_first(n, col, k)
            got = gpu_engine.pool_summary(samples, param=p)
            cases.check_summary(got, ref.summary(x), f"summary far first draw n={n} column {col} k={k:g}", k=k)
            assert _same(dev_engine.pool_summary(_dev(samples), param=p), got)


@pytest.mark.parametrize("name", [c[0] for c in cases.NONFINITE])
def test_summary_non_finite_rule(gpu_engine, dev_engine, name):
    (x, n, _, mn, mx), = [c[1:] for c in cases.NONFINITE if c[0] == name]
    x = np.array(x)
    blk = np.column_stack([np.arange(n, dtype=np.float64), x, np.ones(n)])
    for s in (gpu_engine.pool_summary(x), dev_engine.pool_summary(_dev(x)), gpu_engine.pool_summary(blk, param=1)):
        assert s["n"] == n and np.isnan(s["mean"]) and np.isnan(s["var"]), (name, s)
        for got, want in ((s["min"], mn), (s["max"], mx)):
            assert (np.isnan(got) and np.isnan(want)) or got == want, (name, s)
    s0 = gpu_engine.pool_summary(blk, param=0)  # the finite column next to it
    assert s0["mean"] == (n - 1) / 2 and s0["min"] == 0.0 and s0["max"] == n - 1 and np.isfinite(s0["var"])


def test_summary_non_finite_in_a_capped_grid(gpu_engine):
    """+inf in the first trip of the grid-stride loop and NaN in the last, partial one; then the NaN alone."""
    n = 2 * cases.CAP + 77
    x = cases.nonfinite_large(n)
    want = ref.summary(x)
    got = gpu_engine.pool_summary(x)
    assert got["n"] == n and np.isnan(got["mean"]) and np.isnan(got["var"]) and got["min"] == want["min"] and got["max"] == np.inf
    x[5] = 1000.0
    want, got = ref.summary(x), gpu_engine.pool_summary(x)
    assert got["n"] == n and np.isnan(got["mean"]) and np.isnan(got["var"]) and got["min"] == want["min"] and got["max"] == want["max"]
    assert np.isfinite(got["max"])


# ---- KDE -------------------------------------------------------------------------------------------------------------

def _kde_case(n, m, col, bw):
    """(samples, param, x, grid, reference): the long-double reference computed once per case, shared, not changed."""
    key = (n, m, col, bw)
    if key not in _MEMO:
        samples, p, x = cases.column(n, col)
        grid = cases.kde_grid(x, m, ref.bandwidth(x, bw))
        want = ref.kde(x, grid, bw)
        want.setflags(write=False)
        _MEMO[key] = (samples, p, x, grid, want)
    return _MEMO[key]


@pytest.mark.parametrize("n,m,col,bw", cases.KDE_CASES)
def test_kde(gpu_engine, dev_engine, n, m, col, bw):
    samples, p, x, grid, want = _kde_case(n, m, col, bw)
    got = gpu_engine.pool_kde(samples, grid, param=p, bw_factor=bw)
    assert got.shape == (m,)
    cases.check_kde(got, want, f"kde n={n} m={m} column {col} bw_factor={bw}")
    if m > 1:
        assert want[0] > cases.joint_cases.KDE_FLOOR and want[-1] < 1e-300, "the grid runs from the mode past underflow"
    dens = dev_engine.pool_kde(_dev(samples), _dev(grid), param=p, bw_factor=bw)
    assert dens.is_cuda and np.array_equal(dens.cpu().numpy(), got)
    assert np.array_equal(gpu_engine.pool_kde(samples, grid, param=p, bw_factor=bw), got), "two calls differ"


@pytest.mark.parametrize("n", cases.KDE_SHARDED)
def test_kde_shards_add(gpu_engine, n):
    """Two uneven shards, each fed the pool's bandwidth through bw_factor and weighted n_s / n, against the one call: the
    multi-tile loop must count every sample once, whatever the split."""
    (m, col, bw), = [c[1:] for c in cases.KDE_LARGE if c[0] == n]
    samples, p, x, grid, want = _kde_case(n, m, col, bw)
    whole = gpu_engine.pool_kde(samples, grid, param=p, bw_factor=bw)
    f = bw if bw > 0 else float(n) ** (-1.0 / 5.0)
    c = gpu_engine.pool_summary(samples, param=p)["var"] * f * f
    cut = n // 3 + 11
    parts = np.zeros(m)
    for s in (samples[:cut], samples[cut:]):
        ns = s.shape[0]
        bw_s = float(np.sqrt(c / gpu_engine.pool_summary(s, param=p)["var"]))   # var_s bw_s^2 = c: the pool's bandwidth
        parts += gpu_engine.pool_kde(s, grid, param=p, bw_factor=bw_s) * (ns / n)
    big = whole > cases.joint_cases.KDE_FLOOR
    rel = np.abs(parts[big] - whole[big]) / whole[big]
    print(f"kde n={n}: two uneven shards against one call at {int(big.sum())} of {m} points, largest relative difference {rel.max():.3e}")
    assert big.sum() >= 2 and np.all(rel <= cases.joint_cases.RTOL_SHARDS)
    assert np.all(np.abs(parts[~big] - whole[~big]) <= cases.joint_cases.ATOL_KDE)
    cases.check_kde(parts, want, f"kde n={n}: sum of two shards")


def test_kde_refuses(pkg, gpu_engine, dev_engine):
    x = cases.column(1037, "vector")[0]
    grid = np.array([1000.0, 1001.0])
    bad = {"one draw": x[:1], "zero variance": np.full(1037, 1000.0)}
    for where in (0, 5, 1036):
        for v in (np.nan, np.inf, -np.inf):
            y = x.copy()
            y[where] = v
            bad[f"{v} at {where}"] = y
    for name, y in bad.items():
        for e, arr, g in ((gpu_engine, y, grid), (dev_engine, _dev(y), _dev(grid))):
            with pytest.raises(pkg.RsfError) as ei:
                e.pool_kde(arr, g)
            assert ei.value.code == -1, name
            assert "rsf_pool_kde" in e.lib.rsf_last_error().decode(), name
    with pytest.raises(pkg.RsfError, match="singular KDE"):
        gpu_engine.pool_kde(bad["zero variance"], grid)
    assert gpu_engine.pool_kde(x[:2], grid).shape == (2,)  # n = 2 is the smallest


# ---- histogram -------------------------------------------------------------------------------------------------------

def test_histogram_strided_columns_past_the_cap(gpu_engine, dev_engine):
    for col in (1, 2):
        b, p, x = cases.column(cases.HIST_SIZE, col)
        nbins, lo, hi = cases.hist_range(x)
        want = ref.histogram(x, nbins, lo, hi)
        got = gpu_engine.pool_histogram(b, nbins, lo, hi, param=p)
        assert np.array_equal(got, want) and got.sum() == cases.HIST_SIZE and got[0] > 0 and got[-1] > 0
        assert np.array_equal(dev_engine.pool_histogram(_dev(b), nbins, lo, hi, param=p).cpu().numpy(), want)
