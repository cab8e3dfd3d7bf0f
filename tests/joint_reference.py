"""
Specification of include/rsf_joint.h in NumPy with np.longdouble accumulation: the joint moments of an (n, d) block, the 2-D
Gaussian KDE of two columns, the 2-D histogram with its out-of-range border, and the highest-density levels of a table of
weights.  Written from the formulas; SciPy and np.cov / np.histogram2d enter the CPU tests (tests/test_joint_reference.py) as
independent witnesses, and np.histogram2d here for the interior of the histogram, which IS the definition.
"""
import numpy as np

LD = np.longdouble
HEAD = 2              # n_finite, nonfinite
MAX_PARAMS = 8
HIST2D_MAX_CELLS = 16384
PD_TOL = 1e-12        # det H <= PD_TOL h00 h11: not positive definite in floating point (rsf_joint.h)


def n_partials(d):
    return HEAD + d + d * (d + 1) // 2


def partials(x, center):
    """[n_finite, nonfinite, sum (x_p - c_p), sum (x_p - c_p)(x_q - c_q) for p <= q] of the rows without a non-finite entry."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, 1) if x.ndim == 1 else x.reshape(-1, x.shape[-1])
    d = x.shape[1]
    ok = np.isfinite(x).all(axis=1)
    v = x[ok].astype(LD) - np.asarray(center, dtype=np.float64).astype(LD)
    out = [LD(ok.sum()), LD((~ok).sum())] + [v[:, p].sum(dtype=LD) for p in range(d)]
    out += [(v[:, p] * v[:, q]).sum(dtype=LD) for p in range(d) for q in range(p, d)]
    return np.array(out, dtype=LD)


def finish(part, center):
    """mean (d,), cov (d, d) with ddof = 1, corr (d, d) of summed partials, in long double."""
    c = np.asarray(center, dtype=np.float64).astype(LD).reshape(-1)
    d = c.size
    part = np.asarray(part, dtype=LD)
    n, s1, s2 = part[0], part[HEAD:HEAD + d], part[HEAD + d:]
    with np.errstate(all="ignore"):
        mean = c + s1 / n
        cov = np.full((d, d), np.nan, dtype=LD)
        e = 0
        for p in range(d):
            for q in range(p, d):
                if n >= 2:
                    cov[p, q] = cov[q, p] = (s2[e] - s1[p] * s1[q] / n) / (n - 1)
                e += 1
        sd = np.sqrt(np.where(np.diag(cov) > 0, np.diag(cov), np.nan))
        corr = cov / np.outer(sd, sd)
    return mean, cov, corr


def moments(x, center):
    """→ dict(n, nonfinite, mean, cov, corr) of the block about `center` (any centre gives the same values up to rounding)."""
    part = partials(x, center)
    mean, cov, corr = finish(part, center)
    return {"n": int(part[0]), "nonfinite": int(part[1]), "mean": mean, "cov": cov, "corr": corr}


def bandwidth(x2, bw_factor=0.0, cov2=None, n_total=None):
    """H (2, 2) in long double and n_total: H = cov f^2, f = bw_factor if > 0 else n_total^(-1/6) (Scott, two dimensions)."""
    x2 = np.asarray(x2, dtype=np.float64)
    nt = int(n_total) if n_total else x2.shape[0]
    cov = moments(x2, x2[0])["cov"] if cov2 is None else np.asarray(cov2, dtype=np.float64).astype(LD)
    f = LD(bw_factor) if bw_factor > 0 else LD(nt) ** (-LD(1) / LD(6))
    H = cov * f * f
    det = H[0, 0] * H[1, 1] - H[0, 1] * H[1, 0]
    if not (np.isfinite(H).all() and H[0, 0] > 0 and H[1, 1] > 0 and det > PD_TOL * H[0, 0] * H[1, 1]):
        raise ValueError("the covariance of the two columns is not finite or not positive definite (singular KDE)")
    return H, nt


def kde2d(x2, points, bw_factor=0.0, cov2=None, n_total=None):
    """density[j] = 1 / (n_total 2 pi sqrt(det H)) sum_i exp(-1/2 (p_j - x_i)^T H^-1 (p_j - x_i)) in long double, x2 (n, 2),
    points (m, 2) → (m,) long double (values below float64's range survive: long double reaches 1e-4932)."""
    x2 = np.asarray(x2, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    if x2.shape[0] < 3:
        raise ValueError("n >= 3")
    H, nt = bandwidth(x2, bw_factor, cov2, n_total)
    det = H[0, 0] * H[1, 1] - H[0, 1] * H[1, 0]
    i00, i01, i11 = H[1, 1] / det, -H[0, 1] / det, H[0, 0] / det
    xa, xb = x2[:, 0].astype(LD), x2[:, 1].astype(LD)
    out = np.empty(pts.shape[0], dtype=LD)
    for j, (pa, pb) in enumerate(pts):
        da, db = LD(pa) - xa, LD(pb) - xb
        out[j] = np.exp(-(i00 * da * da + 2 * i01 * da * db + i11 * db * db) / 2).sum(dtype=LD)
    return out / (LD(nt) * 2 * LD(np.pi) * np.sqrt(det))


def axis_index(v, nb, lo, hi):
    """rsf_pool_histogram's index of every value: 0 below lo, 1 + numpy's bin, nb + 1 above hi or NaN."""
    v = np.asarray(v, dtype=np.float64)
    edges = np.linspace(lo, hi, nb + 1)
    with np.errstate(invalid="ignore"):
        b = np.searchsorted(edges, v, side="right")          # numpy.histogramdd's own search
        b[v == edges[-1]] = nb                                # ... and its closing of the last bin
        idx = np.where(v < lo, 0, np.where(v <= hi, b, nb + 1))
    return np.where(np.isnan(v), nb + 1, idx).astype(np.int64)


def hist2d(xa, xb, nbx, nby, lo_a, hi_a, lo_b, hi_b):
    """counts (nbx + 2, nby + 2) float64: the interior is np.histogram2d's, the border (a row below or above the range on
    either axis, NaN counted as above) is counted directly from the per-axis index."""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    ia, ib = axis_index(xa, nbx, lo_a, hi_a), axis_index(xb, nby, lo_b, hi_b)
    counts = np.zeros((nbx + 2, nby + 2))
    border = (ia == 0) | (ia == nbx + 1) | (ib == 0) | (ib == nby + 1)
    np.add.at(counts, (ia[border], ib[border]), 1.0)
    fin = np.isfinite(xa) & np.isfinite(xb)
    counts[1:-1, 1:-1] = np.histogram2d(xa[fin], xb[fin], (nbx, nby), ((lo_a, hi_a), (lo_b, hi_b)))[0]
    return counts


def hpd_levels(weights, probs):
    """levels[k]: the largest weight w such that the sum of all weights >= w is >= probs[k] total.  Sort descending, cumulative sum."""
    w = np.sort(np.asarray(weights, dtype=np.float64).reshape(-1))[::-1]
    if w.size < 1 or not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError("weights are finite, non-negative and do not sum to 0")
    cum = np.cumsum(w.astype(LD), dtype=LD)
    out = []
    for p in np.atleast_1d(probs):
        if not 0.0 < p < 1.0:
            raise ValueError("a probability lies strictly inside (0, 1)")
        out.append(w[min(int(np.searchsorted(cum, LD(np.float64(p) * np.float64(cum[-1])), side="left")), w.size - 1)])
    return np.array(out)
