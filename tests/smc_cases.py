"""
Inputs shared by tests/test_smc_reference.py (CPU) and tests/test_gpu_smc.py, and the bounds of the GPU tests.

Bounds.  Each DIST_* is the distance between tests/smc_reference.py evaluated in plain float64 NumPy and in long double on the
crafted inputs below (test_smc_reference.py::test_float64_distance_sizes_the_bounds prints and re-checks them); the GPU tolerance
is 8 x that distance, as tests/psis_cases.py and tests/evidence_cases.py have it — the factor covers a sum of n terms taken in
another order than NumPy's, and a library exponential that is a few ulp, not half an ulp.
    DIST_INIT  the start, relative per coordinate (one rounding of lo + u (hi - lo) against two)
    DIST_INIT  2.22e-16
    DIST_SUMS  1.82e-16  sum w and sum w^2 of the crafted l at the steps DELTAS, relative (lmax is the far end of the spread: the
               sums are led by weights near 1, whose exponents are small)
    DIST_CUM   8.18e-15  the inclusive prefix sum, each entry above CUM_FLOOR relative to itself: the early entries are weights with
               an exponent delta (l - lmax) down to -700, rounded to float64 before the exponential — up to 700 x 1.1e-16 relative
"""
import numpy as np

DIST_INIT = 2.3e-16
DIST_SUMS = 1.9e-16
DIST_CUM = 8.2e-15
CUM_FLOOR = 1e-290  # prefix sums below it are subnormal weights, or a few ulp of one: no relative accuracy to speak of
TOL_INIT, TOL_SUMS, TOL_CUM = 8 * DIST_INIT, 8 * DIST_SUMS, 8 * DIST_CUM

# the chain of one run, GPU against specification with the same seeds (test_chain_logic_through_the_split_path): the two differ in
# the covariance of the resampled particles (pool_joint's fixed-order sums against np.cov: n eps = 2e-13 at n = 1037, times the
# condition of the 3 x 3 Cholesky factorisation, about 10) and in the library's normals (4 ulp); an error made at one stage is
# carried by the particles through the at most 40 x 3 steps that follow: 120 x 2e-12 = 2.4e-10, relative to the box's width for q
# and absolute, times shape, for l (l = -shape log SSq, and SSq moves by that relative amount)
TOL_CHAIN = 2.4e-10

NS = (1, 63, 257, 1037, 16421)      # a partial wave, a workgroup plus one, several tiles of the scan's 2048, a non-multiple of everything
DIST_NS = (1, 5, 1037, 16421)
DELTAS = (0.0, 1e-5, 1e-4, 1e-3, 0.01, 0.1, 0.5, 1.0)
OFFSET = 100003
BOXES = {1: ([0.0], [1.0e4]), 3: ([850.0, 0.009, 0.0145], [1150.0, 0.013, 0.0158])}


def crafted_l(n, seed=11):
    """l (n,): a bulk of width a few units about -37.25, a tenth spread to +-1e4 about it, a tenth at -inf (entry 0 stays finite)"""
    rng = np.random.default_rng(seed + 1000 * n)
    l = -37.25 + 2.5 * rng.standard_normal(n)
    far = rng.uniform(size=n) < 0.1
    l[far] = -37.25 + rng.uniform(-1e4, 1e4, int(far.sum()))
    out = rng.uniform(size=n) < 0.1
    out[0] = False
    l[out] = -np.inf
    return l


def exact_l(n, seed=5):
    """l in {0, -inf}: with lmax = 0 every weight is 1 or 0 at any step, so every prefix sum is an exact integer in float64 and the
    ancestors have one right answer.  About a third of the particles carry weight (entry n // 2 always does)."""
    rng = np.random.default_rng(seed + n)
    l = np.where(rng.uniform(size=n) < 1.0 / 3.0, 0.0, -np.inf)
    l[n // 2] = 0.0
    return l


# ---- measured constants -------------------------------------------------------------------------------------------------------
# SPEC_SD[d]: the standard deviation of log I over R = 32 replicate runs (seeds 0..31) of the long double specification at
# n = 4096, rho = 0.5, 3 steps on the closed forms of tests/posterior_reference.py (printed by
# test_smc_reference.py::test_exact_integral_and_final_sample)
SPEC_SD = {1: 0.0275, 3: 0.0748}
# SPEC_SD_REAL: the same for the real model's d = 1 problem of tests/test_gpu_smc.py::test_end_to_end_real_model (nsteps 500, data
# at 1 % noise, box (0, 1e4), n = 4096; the specification with the checker library's SSq, seeds 0..31: 6 to 7 stages each, mean log I
# 3172.129), measured once with tools/smc_bench.py --spec-sd (a minute of CPU, too long for the suite).  It is ten times the closed
# forms': the posterior is 1e-4 of the box wide, and the first stages' weights rest on the few particles that start near it
SPEC_SD_REAL = 0.261
R_SPEC, N_SPEC = 32, 4096
SD_RATIO_MAX = 3.2  # the 99.9 % point of an F(7, 31) variance ratio is 10.2 = 3.2^2: 8 GPU replicates against 32 of the specification
