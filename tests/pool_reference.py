"""
Specification of rsf_pool_summary, rsf_pool_kde and rsf_pool_histogram (include/rsf_abi.h) in NumPy with np.longdouble
accumulation: the moments of one column of the pooled draws, its Gaussian KDE with Scott's bandwidth, and the fixed-bin histogram
with its two border counts.  Written from the formulas; nothing here calls the library.  np.mean / np.var, SciPy's gaussian_kde
and np.histogram enter the CPU tests (tests/test_pool_reference.py) as independent witnesses, and np.histogram here for the
interior of the histogram, which IS the definition.

Non-finite samples in summary (the same words stand next to rsf_pool_summary in include/rsf_abi.h):
    out[0] counts every sample;
    mean and variance are NaN as soon as one sample is NaN or infinite;
    min and max are those of the samples that are not NaN (an infinite sample is an extreme), and NaN only when every sample is NaN.
rsf_pool_kde refuses such a pool (RSF_ERR_INVALID); kde() raises ValueError.
"""
import numpy as np

LD = np.longdouble
CHUNK = 1 << 18  # samples per long-double temporary of kde(): 4 MiB each


def summary(x):
    """→ dict(n, mean, var (ddof = 1, two-pass about the long-double mean; 0 for n = 1), min, max); mean and var long double."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    if n < 1:
        raise ValueError("n >= 1")
    seen = x[~np.isnan(x)]
    mn, mx = (float(seen.min()), float(seen.max())) if seen.size else (np.nan, np.nan)
    if not np.isfinite(x).all():
        return {"n": n, "mean": LD(np.nan), "var": LD(np.nan), "min": mn, "max": mx}
    v = x.astype(LD)
    mean = v.sum(dtype=LD) / LD(n)
    dlt = v - mean
    var = (dlt * dlt).sum(dtype=LD) / LD(n - 1) if n > 1 else LD(0)
    return {"n": n, "mean": mean, "var": var, "min": mn, "max": mx}


def bandwidth(x, bw_factor=0.0):
    """c = var f^2 in long double, f = bw_factor if > 0 else n^(-1/5) (Scott, one dimension)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.size < 2:
        raise ValueError("n >= 2")
    if not np.isfinite(x).all():
        raise ValueError("a non-finite draw")
    f = LD(bw_factor) if bw_factor > 0 else LD(x.size) ** (-LD(1) / LD(5))
    c = summary(x)["var"] * f * f
    if not c > 0:
        raise ValueError("the samples have zero variance (singular KDE)")
    return c


def kde(x, grid, bw_factor=0.0):
    """density[j] = 1 / (n sqrt(2 pi c)) sum_i exp(-(grid[j] - x_i)^2 / (2 c)) in long double → (m,) long double (values below
    float64's range survive: long double reaches 1e-4932).  The samples pass in chunks of CHUNK, so that two million of them at a
    handful of grid points stay within a few seconds and a few tens of MB."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    g = np.asarray(grid, dtype=np.float64).reshape(-1).astype(LD)
    c = bandwidth(x, bw_factor)
    acc = np.zeros(g.size, dtype=LD)
    for i0 in range(0, x.size, CHUNK):
        v = x[i0:i0 + CHUNK].astype(LD)
        for j in range(g.size):
            dlt = g[j] - v
            acc[j] += np.exp(-(dlt * dlt) / (2 * c)).sum(dtype=LD)
    return acc / (LD(x.size) * np.sqrt(2 * LD(np.pi) * c))


def histogram(x, nbins, lo, hi):
    """counts (nbins + 2,) float64: [below lo, np.histogram(x, nbins, (lo, hi)), above hi or NaN]."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if not (nbins >= 1 and hi > lo and np.isfinite(hi - lo)):
        raise ValueError("nbins >= 1, finite lo < hi")
    with np.errstate(invalid="ignore"):
        below, inside = x < lo, (x >= lo) & (x <= hi)
    counts = np.empty(nbins + 2)
    counts[0] = below.sum()
    counts[1:-1] = np.histogram(x[inside], nbins, (lo, hi))[0]
    counts[-1] = x.size - below.sum() - inside.sum()
    return counts
