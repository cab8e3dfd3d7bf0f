"""
Inputs and stated conditions shared by tests/test_joint_reference.py (CPU) and tests/test_gpu_joint.py.

Synthetic block: x = L z + (1000, 0.011, 0.006): Dc with standard deviation 5, a and b with standard deviations about 1e-4,
correlated (a and b trade off, Dc trades off with both) — the scales of a joint rate-and-state posterior, where centring before
scaling matters.  Columns 3..7 of the d = 8 block are further mixtures of the same z with an offset each.

Bounds of the GPU tests, from the issue that introduced the feature:
  moments   |mean_p - ref| <= 4 spacing(|ref|) + 1e-13 sd_p;   |cov_pq - ref_pq| <= 1e-11 sqrt(ref_pp ref_qq)
            under the condition that the centre lies within 10 sd of the mean in every column (check_center): sums about such a
            centre are at most (1 + 100) n sd^2, and their rounding at most about (1 + 100)(chain length + tree depth) 2^-53 of that,
            a few 1e-13 at these sizes.
  kde2d     rtol 1e-9 where the reference exceeds 1e-290 (the project's number for the 1-D KDE; SciPy itself sits up to 5.4e-12 from the
            extended-precision value on these inputs, tests/test_joint_reference.py), atol 1e-300 elsewhere; shards against one call rtol 1e-12 (only the order of
            summation differs: n terms of one sign, at most about log2(slices) + 2 roundings apart).
  hist2d    exact.
"""
import numpy as np

SIZES = (3, 5, 1037, 16421)   # 1037 crosses one 1024-sample tile; 16421 spans many slices and leaves an uneven tail
# past the cap of 1024 workgroups x 256 threads, where the grid-stride loops of pool_joint_moments_kernel and pool_hist2d_kernel take a
# second trip (in 257 threads only) and a third: kept out of SIZES, so that the parametrised matrix does not grow
SIZES_CAPPED = (262144 + 257, 2 * 262144 + 77)
# pool_kde2d_kernel past one 1024-sample tile a slice: m = 1 → 1024 slices of 1025 samples (a second tile of one sample; the last slice
# holds 2); m = 1031 → two chunks, 512 slices of 2049 samples, three tiles each
N_MULTI_TILE = (1 << 20) + 1
MEAN3 = np.array([1000.0, 0.011, 0.006])
TOL_MEAN_SD = 1e-13
TOL_COV = 1e-11
RTOL_KDE = 1e-9
KDE_FLOOR = 1e-290
ATOL_KDE = 1e-300
RTOL_SHARDS = 1e-12
PAIRS3 = ((0, 1), (0, 2), (1, 2), (2, 0))


def synthetic(n, d=3, seed=0):
    """(n, d) float64, d <= 8."""
    rng = np.random.default_rng(7000 + 13 * n + d + seed)
    z = rng.standard_normal((n, 3))
    L = np.array([[5.0, 0.0, 0.0], [-0.6e-4, 0.8e-4, 0.0], [0.5e-4, -0.7e-4, 0.5e-4]])
    x3 = z @ L.T + MEAN3
    if d <= 3:
        return np.ascontiguousarray(x3[:, :d])
    mix = np.random.default_rng(99).standard_normal((3, 5)) * np.array([2.0, 1e-3, 30.0, 0.5, 1e-5])
    extra = z @ mix + np.array([-40.0, 0.5, 2.0e4, 3.0, 1e-3])
    return np.ascontiguousarray(np.column_stack([x3, extra])[:, :d])


def given_center(x):
    """A centre that is not a draw: 3 sd above the mean in even columns, 3 sd below in odd ones."""
    x = x.reshape(-1, x.shape[-1])
    sign = np.where(np.arange(x.shape[1]) % 2 == 0, 3.0, -3.0)
    return x.mean(0) + sign * x.std(0)


def check_center(x, center):
    """The condition the moment bounds rest on: the centre within 10 sd of the mean in every column (finite rows only)."""
    x = x.reshape(-1, x.shape[-1])
    x = x[np.isfinite(x).all(axis=1)]
    if x.shape[0] >= 2:
        sd = x.std(0, ddof=1)
        assert np.all(np.abs(np.asarray(center) - x.mean(0)) <= 10.0 * sd), "centre further than 10 sd from the mean"


def check_moments(got, ref, label=""):
    """got: the library's dict, ref: joint_reference.moments → (largest mean error in sd, largest scaled cov error); asserts the bounds."""
    mean_r, cov_r = ref["mean"], ref["cov"]
    sd = np.sqrt(np.diag(cov_r)).astype(np.float64)
    em = np.abs(got["mean"].astype(np.longdouble) - mean_r).astype(np.float64)
    bound = 4 * np.spacing(np.abs(mean_r.astype(np.float64))) + TOL_MEAN_SD * sd
    scale = np.sqrt(np.outer(np.diag(cov_r), np.diag(cov_r))).astype(np.float64)
    ec = (np.abs(got["cov"].astype(np.longdouble) - cov_r).astype(np.float64)) / scale
    er = np.abs(got["corr"].astype(np.longdouble) - ref["corr"]).astype(np.float64)
    print(f"{label}: mean error / bound {np.max(em / bound):.3e}, cov error / sqrt(c_pp c_qq) {ec.max():.3e}, corr error {er.max():.3e}")
    assert np.all(em <= bound), (em, bound)
    assert np.all(ec <= TOL_COV), ec
    assert np.all(er <= 2 * TOL_COV + 4e-16), er  # corr = cov_pq / (sd_p sd_q): cov_pq within TOL_COV of its scale, sd_p sd_q within TOL_COV relative
    return float(np.max(em / bound)), float(ec.max())


def mesh(x2, k, nx, ny):
    """nx x ny points over mean +- k sd of the two columns → (nx * ny, 2)."""
    mu, sd = x2.mean(0), x2.std(0)
    ga, gb = (np.linspace(mu[i] - k * sd[i], mu[i] + k * sd[i], nn) for i, nn in ((0, nx), (1, ny)))
    return np.stack(np.meshgrid(ga, gb, indexing="ij"), axis=-1).reshape(-1, 2)


def scattered(x2, m, seed):
    """m points around the data: a draw each, moved by up to 1.5 sd."""
    rng = np.random.default_rng(seed)
    return x2[rng.integers(0, x2.shape[0], m)] + rng.uniform(-1.5, 1.5, (m, 2)) * x2.std(0)


def check_kde(got, ref, label=""):
    """got float64 (m,), ref long double (m,): rtol RTOL_KDE where ref > KDE_FLOOR, atol ATOL_KDE elsewhere → largest relative error."""
    got = np.asarray(got, dtype=np.float64)
    big = ref > KDE_FLOOR
    rel = (np.abs(got[big].astype(np.longdouble) - ref[big]) / ref[big]).astype(np.float64)
    worst = float(rel.max()) if rel.size else 0.0
    small = np.abs(got[~big].astype(np.longdouble) - ref[~big]).astype(np.float64)
    print(f"{label}: {int(big.sum())} of {ref.size} points above {KDE_FLOOR:g}, largest relative error {worst:.3e}; "
          f"elsewhere largest absolute error {float(small.max()) if small.size else 0.0:.3e}")
    assert np.isfinite(got).all() and np.all(got >= 0)
    assert worst <= RTOL_KDE
    assert np.all(small <= ATOL_KDE)
    return worst


def edge_block(n, nbx, nby, seed):
    """(n, 3) block for the 2-D histogram with ranges ((lo_a, hi_a), (lo_b, hi_b)) on columns (0, 2): values placed exactly on
    interior edges, on lo and on hi (columns rounded to the edges' own grid, as test_pool_histogram does), rows below and above
    the range on either axis, NaN in either column → (x, ranges)."""
    rng = np.random.default_rng(seed)
    lo_a, hi_a, lo_b, hi_b = 990.0, 1010.0, 0.0057, 0.0063
    ea, eb = np.linspace(lo_a, hi_a, nbx + 1), np.linspace(lo_b, hi_b, nby + 1)
    x = np.column_stack([rng.normal(1000.0, 5.0, n), rng.normal(0.011, 1e-4, n), rng.normal(0.006, 1e-4, n)])
    k = n // 4
    x[:k, 0] = ea[rng.integers(0, nbx + 1, k)]          # exactly on an edge of axis a (lo and hi included)
    x[k:2 * k, 2] = eb[rng.integers(0, nby + 1, k)]     # ... of axis b
    x[2 * k:2 * k + k // 2, 0] = ea[rng.integers(0, nbx + 1, k // 2)]
    x[2 * k:2 * k + k // 2, 2] = eb[rng.integers(0, nby + 1, k // 2)]   # on an edge of both
    tail = x[2 * k + k // 2:]
    if tail.shape[0] >= 8:
        tail[0, 0], tail[1, 0], tail[2, 2], tail[3, 2] = lo_a - 1.0, hi_a + 1.0, lo_b - 1e-3, hi_b + 1e-3
        tail[4, 0], tail[5, 2] = np.nan, np.nan
        tail[6] = (np.nan, 0.011, np.nan)
        tail[7, 0], tail[7, 2] = np.nextafter(lo_a, -np.inf), np.nextafter(hi_b, np.inf)
    return np.ascontiguousarray(x), ((lo_a, hi_a), (lo_b, hi_b))


# hand-made weights for the highest-density levels: (weights, probs, expected levels)
HPD_CASES = {
    # descending 8 4 4 2 1 1 (total 20), running mass 8 12 16 18 19 20
    "ties": ([1.0, 4.0, 8.0, 4.0, 2.0, 1.0], (0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.96),
             (8.0, 8.0, 4.0, 4.0, 4.0, 4.0, 2.0, 1.0, 1.0)),
    "all_equal": ([0.25] * 8, (0.01, 0.5, 0.99), (0.25, 0.25, 0.25)),
    "one": ([3.5], (0.1, 0.9), (3.5, 3.5)),
    "zeros_among": ([0.0, 2.0, 0.0, 6.0], (0.5, 0.75, 0.76), (6.0, 6.0, 2.0)),
}
