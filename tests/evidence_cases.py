"""
Inputs shared by tests/test_evidence_reference.py (CPU) and tests/test_gpu_evidence.py, and the bounds of the GPU tests.

Bounds.  Each DIST_* is the distance between tests/evidence_reference.py evaluated in plain float64 NumPy and in long double on the
crafted inputs below (test_evidence_reference.py::test_float64_distance_sizes_the_bounds prints and re-checks them); the GPU
tolerance is 8 x that distance, as tests/psis_cases.py has it — the factor covers a sum of n terms taken in another order than
NumPy's pairwise one, and a library exponential and logarithm that are a few ulp, not half an ulp.
    DIST_THETA    9.04e-16  proposal draws, relative per coordinate (the logged ones go through exp: |phi| ulp)
    DIST_LOGG     5.52e-14  log g, over max(|log g|, 1) (d3_identity: the forward substitution cancels against a diagonal of 6e-5)
    DIST_PARTIAL  3.49e-16  the six sums of the partials, relative
The converged log_integral = log r + lstar differed by 0 in all three crafted cases, which is luck of the last rounding and sizes
nothing.  Its bound is reasoned instead: r is a ratio of two of the sums, each within TOL_PARTIAL, so log r moves by at most
2 TOL_PARTIAL, and the sum with lstar is rounded once, half an ulp of |log I| (|lstar| = 37.25: ulp 7.1e-15):
    TOL_LOGI = 2 TOL_PARTIAL + 7.1e-15.
The iteration contracts (3 to 5 iterations), so the library and the specification stop at the same iteration: asserted.
"""
import numpy as np

DIST_THETA = 9.1e-16
DIST_LOGG = 5.6e-14
DIST_PARTIAL = 3.5e-16
TOL_THETA, TOL_LOGG, TOL_PARTIAL = 8 * DIST_THETA, 8 * DIST_LOGG, 8 * DIST_PARTIAL
TOL_LOGI = 2 * TOL_PARTIAL + 7.1e-15

N2S = (1, 63, 257, 1037)  # a partial wave, one workgroup plus one, several workgroups
OFFSET = 100003

# (name, mean, chol, transform, lo, hi): the working coordinates are the logged ones where transform is 1
PROPOSALS = (
    ("d1_identity", [1000.0], [[35.0]], [0], [900.0], [1100.0]),
    ("d1_log", [np.log(1000.0)], [[0.04]], [1], [900.0], [1100.0]),
    ("d3_identity", [1000.0, 0.011, 0.015], [[40.0, 0, 0], [-3.5e-4, 6e-5, 0], [1e-5, -2e-5, 4e-4]], [0, 0, 0], [850.0, 0.009, 0.0145],
     [1150.0, 0.013, 0.0158]),
    ("d3_log", [np.log(1000.0), np.log(0.011), 0.015], [[0.04, 0, 0], [-0.035, 0.006, 0], [1e-5, -2e-5, 4e-4]], [1, 1, 0],
     [850.0, 0.009, 0.0145], [1150.0, 0.013, 0.0158]),
)

BRIDGE_SIZES = ((1, 1), (5, 3), (1037, 16421))
# past the cap of evidence_terms_kernel's grid (1024 workgroups x 256 threads): a second trip of the grid-stride loop in 257 threads
# only, and a third; each size once as the posterior draws' set and once as the proposal draws'
BRIDGE_SIZES_CAPPED = ((262144 + 257, 2 * 262144 + 77), (2 * 262144 + 77, 262144 + 257))


def crafted_l(n1, n2, seed=7):
    """(l1 (n1,), l2 (n2,), lstar): a bulk of width a few units about lstar, a tenth of each set spread to +-1e4 about it, and a
    tenth of l2 at -inf (at least one entry of l2 stays finite)."""
    rng = np.random.default_rng(seed + 1000 * n1 + n2)
    lstar = -37.25
    l1 = lstar + 1.5 * rng.standard_normal(n1) + 0.7
    l2 = lstar + 2.5 * rng.standard_normal(n2) - 1.1
    for l in (l1, l2):
        far = rng.uniform(size=l.size) < 0.1
        l[far] = lstar + rng.uniform(-1e4, 1e4, int(far.sum()))
    out = rng.uniform(size=n2) < 0.1
    if n2 > 1:
        out[0] = False
        l2[out] = -np.inf
    return l1, l2, lstar


def shards(n, parts=(0.23, 0.61)):
    """three uneven contiguous shards of range(n) (some may be empty for tiny n)"""
    a, b = int(parts[0] * n), int(parts[1] * n)
    return (slice(0, a), slice(a, b), slice(b, n))


# the closed forms of tests/posterior_reference.py (quadratic SSq, shape 12): log I by tensor Gauss-Legendre quadrature, at two
# orders that agree to 2e-14 (d = 1: 200 and 400 nodes) and 6e-8 (d = 3: 96^3 and 160^3 nodes)
CLOSED_TRUTH = {1: -1.33535090116, 3: -3.6247807}
CLOSED_N = 16384  # N1 = N2
CLOSED_RE_MAX = 0.01
