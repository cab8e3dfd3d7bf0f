"""
Inputs, sizes and bounds shared by tests/test_pool_reference.py (CPU) and tests/test_gpu_pool.py: rsf_pool_summary, rsf_pool_kde
and rsf_pool_histogram against tests/pool_reference.py.  Each size is the smallest at which the named path of
csrc/rsf_kernels_pool.h can go wrong.

Draws: the columns of joint_cases.synthetic(n, 3) — 1000 +- 5, 0.011 +- 1e-4, 0.006 +- 1e-4 — as a plain vector (column 0, copied
out) and as columns 1 and 2 of the (n, 3) block, stride 3.

summary   pool_moments_kernel runs min(1024, ceil(n / 256)) workgroups of 256 and walks the pool with a grid-stride loop:
              1                  var = 0
              2
              70                 a partial second wave
              256 * 3 + 5        four workgroups, the last nearly empty
              262 144            the cap reached, one row per thread
              262 144 + 257      the second trip of the loop, in 257 threads only
              2 * 262 144 + 77   three trips in 77 threads
kde       pool_kde_kernel gives a workgroup per = ceil(n / min(1024, ceil(n / 1024))) samples in tiles of 1024:
              2, 3
              1023, 1024, 1025   one workgroup, one full, two
              16 421             17 workgroups, the last one short
              2^20               1024 workgroups of one full tile
              2^20 + 1           per = 1025: a second tile of one sample; the last workgroup holds 2 samples
              2^21 + 1029        per = 2050: three tiles, the last of 2 samples, the last workgroup short
          grid sizes, the j0 loop over 256 points a pass:
              1, 255, 256
              257                a second pass with one live thread (the other 255 ride along through the barriers)
              1000
          The grid sizes go with n <= 16 421; the three large n take 5 points.  The grid runs from the mean to 40 bandwidths past the
          largest draw, where the density is below exp(-800): from the mode, through 1e-290, to 0 in float64.  Columns and
          bw_factor (0 = Scott, or given) rotate over the cases.

Bounds, the project's own:
  mean      |mean - ref| <= 4 spacing(|ref|) + 1e-13 sd                 } joint_cases.py's rule, under its condition that the centre
  variance  |var - ref| <= 1e-11 ref                                    } — here x[0] — lies within 10 sd of the mean (check_center)
  min, max  equal to the reference
  kde       rtol 1e-9 where the reference exceeds 1e-290, atol 1e-300 elsewhere (joint_cases.check_kde)
  shards    two uneven shards with the pool's bandwidth, weighted n_s / n, add to the one call within joint_cases.RTOL_SHARDS
  histogram equal to the reference
  host against device memory: equal bit for bit.

The first draw far from the bulk.  rsf_pool_summary sums about x[0].  With x[0] k sd from the bulk, sum (x - x[0])^2 is
(1 + k^2) n sd^2 and its rounding at most about (1 + k^2) (chain + tree length) 2^-53 of n sd^2 (joint_cases.py states this for
k <= 10, where 1 + k^2 <= 101 goes with 1e-11).  The bound scales by the same factor:
    |var - ref| <= 1e-11 (1 + k^2) / 101 ref            k = 1e2, 1e3, 1e4  →  9.9e-10, 9.9e-8, 9.9e-6
and the mean's, whose sum (x - x[0]) is (1 + k) n sd at most, by (1 + k) / 11:
    |mean - ref| <= 4 spacing(|ref|) + 1e-13 (1 + k) / 11 sd.
sd in both is the reference's, which includes the far draw.  tests/test_pool_reference.py shows that a plain float64 one-pass
shifted sum about x[0] stays inside on these inputs (the bound can be met); the GPU test prints the measured error over it.
"""
import numpy as np

import joint_cases

CAP = 1024 * 256                      # kPoolBlocks workgroups of kMaxBlock threads
KDE_TILE = 1024
SUMMARY_SIZES = (1, 2, 70, 256 * 3 + 5, CAP, CAP + 257, 2 * CAP + 77)
COLUMNS = ("vector", 1, 2)
TOL_MEAN_SD = joint_cases.TOL_MEAN_SD
TOL_VAR = joint_cases.TOL_COV
FAR_K = (1e2, 1e3, 1e4)
FAR_SIZES = (1037, 2 * CAP + 77)
FAR_COLUMNS = ("vector", 1)           # +k sd on the vector (x[0] is the maximum), -k sd on the strided column (the minimum)
HIST_SIZE = CAP + 257

KDE_SMALL_N = (2, 3, 1023, 1024, 1025, 16421)
KDE_M = (1, 255, 256, 257, 1000)
KDE_LARGE = ((1 << 20, 5, "vector", 0.0), ((1 << 20) + 1, 5, 1, 0.0), ((1 << 21) + 1029, 5, 2, 0.02))
KDE_SHARDED = ((1 << 20) + 1, (1 << 21) + 1029)
# (n, m, column, bw_factor)
KDE_CASES = tuple((n, m, COLUMNS[(i + j) % 3], 0.0 if (i + j) % 2 == 0 else 0.3)
                  for i, n in enumerate(KDE_SMALL_N) for j, m in enumerate(KDE_M)) + KDE_LARGE

_MEMO = {}


def block(n):
    """joint_cases.synthetic(n, 3): made once per size, shared, read-only."""
    if n not in _MEMO:
        x = joint_cases.synthetic(n, 3)
        x.setflags(write=False)
        _MEMO[n] = x
    return _MEMO[n]


def column(n, col):
    """→ (samples, param, x): what Engine.pool_* takes (a vector, or the block and a column index) and the same draws as a
    contiguous 1-D array for the reference."""
    b = block(n)
    if col == "vector":
        x = np.ascontiguousarray(b[:, 0])
        return x, 0, x
    return b, int(col), np.ascontiguousarray(b[:, int(col)])


def far_first(n, col, k):
    """column(n, col) with x[0] moved k sd of the bulk away from its mean: up on the vector, down on the strided column."""
    samples, param, x = column(n, col)
    samples = samples.copy()
    far = x[1:].mean() + (k if col == "vector" else -k) * x[1:].std()
    if col == "vector":
        samples[0] = far
        x = samples
    else:
        samples[0, param] = far
        x = np.ascontiguousarray(samples[:, param])
    return samples, param, x


def check_center(x):
    """The condition the benign bounds rest on: x[0] within 10 sd of the mean."""
    joint_cases.check_center(np.asarray(x).reshape(-1, 1), [x[0]])


def summary_bounds(ref, k=0.0):
    """(mean bound, variance bound) for a first draw k sd from the bulk; k <= 10 is the benign rule itself."""
    fm, fv = (1.0, 1.0) if k <= 10.0 else ((1.0 + k) / 11.0, (1.0 + k * k) / 101.0)
    sd = float(np.sqrt(ref["var"]))
    return 4 * np.spacing(abs(float(ref["mean"]))) + TOL_MEAN_SD * fm * sd, TOL_VAR * fv * float(ref["var"])


def check_summary(got, ref, label="", k=0.0):
    """got: the library's dict, ref: pool_reference.summary → (mean error / bound, variance error / bound); asserts the bounds."""
    bm, bv = summary_bounds(ref, k)
    em = float(abs(np.longdouble(got["mean"]) - ref["mean"]))
    ev = float(abs(np.longdouble(got["var"]) - ref["var"]))
    rm, rv = em / bm, (ev / bv if bv > 0 else ev)
    print(f"{label}: mean error / bound {rm:.3e}, variance error / bound {rv:.3e} (relative error {ev / float(ref['var']) if bv > 0 else 0.0:.3e})")
    assert got["n"] == ref["n"] and got["min"] == ref["min"] and got["max"] == ref["max"], (got, ref)
    assert em <= bm, (em, bm)
    assert ev <= bv, (ev, bv)
    return rm, rv


def shifted_one_pass(x):
    """The library's form in plain float64 NumPy: sums about x[0] in one pass (np.sum: pairwise) → (mean, var)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    d = x - x[0]
    s, ss = np.sum(d), np.sum(d * d)
    m = s / n
    return x[0] + m, (ss - n * m * m) / (n - 1)


def kde_grid(x, m, c):
    """m points from the mean to 40 bandwidths past the largest draw (one point: 0.3 sd above the mean)."""
    x = np.asarray(x, dtype=np.float64)
    if m == 1:
        return np.array([x.mean() + 0.3 * x.std()])
    return np.linspace(x.mean(), x.max() + 40.0 * float(np.sqrt(c)), m)


check_kde = joint_cases.check_kde


def hist_range(x):
    """(nbins, lo, hi) that leaves draws on either side outside: mean -+ 2.5 sd, rounded to the draws' own grid."""
    x = np.asarray(x, dtype=np.float64)
    return 40, float(np.float32(x.mean() - 2.5 * x.std())), float(np.float32(x.mean() + 2.5 * x.std()))


# the non-finite rule of pool_reference, case by case: (name, samples, n, mean and var are NaN, min, max)
NONFINITE = (
    ("nan_first", [np.nan, 2.0, -1.0, 5.0], 4, True, -1.0, 5.0),
    ("nan_later", [2.0, -1.0, np.nan, 5.0], 4, True, -1.0, 5.0),
    ("plus_inf", [2.0, np.inf, -1.0, 5.0], 4, True, -1.0, np.inf),
    ("minus_inf_first", [-np.inf, 2.0, -1.0], 3, True, -np.inf, 2.0),
    ("both_inf", [2.0, np.inf, -np.inf], 3, True, -np.inf, np.inf),
    ("one_inf", [np.inf], 1, True, np.inf, np.inf),
    ("nan_and_inf", [np.nan, np.inf, 1.0], 3, True, 1.0, np.inf),
    ("all_nan", [np.nan, np.nan, np.nan], 3, True, np.nan, np.nan),
    ("one_nan", [np.nan], 1, True, np.nan, np.nan),
)


def nonfinite_large(n):
    """A benign vector of n draws with a NaN in the last (partial) trip of the grid-stride loop and +inf in the first."""
    x = column(n, "vector")[0].copy()
    x[n - 3], x[5] = np.nan, np.inf
    return x
