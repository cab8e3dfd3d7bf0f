"""
Inputs shared by tests/test_predictive_noise_reference.py (CPU) and tests/test_gpu_predictive_noise.py: crafted rows, the
bound on the residual and the recorded pass counts.

The criterion of the GPU tests is the residual |F_ref(t) - p| <= TOL_RESIDUAL = 1e-12 of the library's t, F_ref of
tests/predictive_noise_reference.py (float64 elements, exact sum) evaluated once per (row, probability).  1e-12 is the project's
bound for scaled sums, and F is a mean of n terms in [0, 1].  The part of the floor that can be derived is the spacing of float64
t: one ulp moves F by at most ulp(t) max F' <= 1.1e-16 |t| phi(0) / min_i s_i, and every input here keeps
    max |y| / min_i s_i <= MAX_Y_OVER_S = 1000                                   (`check_condition` asserts it)
which puts that floor at 4.4e-14: the bound has a 20-fold margin over it.

Measured with predictive_noise_reference.scheme — the library's iteration in float64 NumPy, sums in 256 strided partials and a
tree — over every crafted case and its probabilities (test_predictive_noise_reference.py re-measures both):
    largest residual against F_ref:  SCHEME_RESIDUAL
    passes over a row, per case:     SCHEME_PASSES
The GPU tests bound the kernel's passes on every crafted case but `bimodal` by the scheme's count on the same input plus
PASS_MARGIN = 3: the kernel's erfc and exp round otherwise than SciPy's, so at the rounding floor rule (a) or (b) can fire one
pass earlier or later, and a step that was a Newton step can become a bisection; three passes cover one such change and what
follows from it.  (`bimodal` starts where F' = 0 and bisects into a mode; how many bisections that takes depends on the last bits
of F at points where it is flat, so only the cap holds for it.)
"""
import numpy as np

TOL_RESIDUAL = 1e-12
MAX_Y_OVER_S = 1000.0
PASS_MARGIN = 3

PROBS = (1e-6, 0.025, 0.05, 0.5, 0.95, 0.999)
REAL_PROBS = (0.025, 0.05, 0.5, 0.95, 0.975)

# measured: predictive_noise_reference.scheme on crafted(), the largest over rows and probabilities
SCHEME_RESIDUAL = 2.8e-15  # 2.776e-15, in `tight`, where one ulp of t moves F by 2.3e-15
SCHEME_PASSES = {"tight": 6, "wide": 13, "bimodal": 14, "k0": 7, "n1": 2, "n5": 10, "scales": 7, "extreme_p": 11}


def check_condition(series, std2):
    y, s = np.asarray(series, dtype=np.float64), np.sqrt(np.asarray(std2, dtype=np.float64))
    fin = np.isfinite(y)
    assert np.abs(y[fin]).max() / s.min() <= MAX_Y_OVER_S, (np.abs(y[fin]).max(), s.min())


def crafted():
    """[(name, series (rows, n), std2 (n,), probs)] — each named after the failure it can expose."""
    rng = np.random.default_rng(20251)
    cases = []
    # tight: the spread of y is 1e-3 of |y| and |y| / s = 100 — the bracket is narrow and F' is at its largest
    n = 4099
    y = np.vstack([1.0 + 1e-3 * rng.standard_normal(n), -1.0 - 1e-3 * rng.standard_normal(n)])
    cases.append(("tight", y, (0.01 * rng.uniform(0.9, 1.1, n)) ** 2, PROBS))
    # wide: the spread of y is 100 s — F is the empirical distribution smoothed a little, Newton sees a ragged F'
    cases.append(("wide", rng.standard_normal((2, n)), (0.02 * rng.uniform(0.5, 1.5, n)) ** 2, PROBS))
    # bimodal: +-1 with s = 0.01 — at the bracket's midpoint F' is 0 to rounding and Newton must give way to bisection
    m = 1000
    two = np.vstack([np.where(np.arange(m) % 2 == 0, -1.0, 1.0), np.where(np.arange(m) % 5 < 2, -1.0, 1.0)])
    cases.append(("bimodal", two, np.full(m, 0.01 ** 2), PROBS))
    # k0: every y = 0 (the series' first row) and lognormal s — a scale mixture at 0; at p = 1/2 the bracket is the point 0
    cases.append(("k0", np.zeros((1, n)), (0.01 * np.exp(0.5 * rng.standard_normal(n))) ** 2, PROBS))
    # n1, n5: fewer draws than a wave (n = 1: the bracket is the answer)
    cases.append(("n1", np.array([[0.7], [-0.2]]), np.array([0.05 ** 2]), PROBS))
    cases.append(("n5", rng.standard_normal((2, 5)), (0.05 * rng.uniform(0.5, 1.5, 5)) ** 2, PROBS))
    # scales: s over e^{+-3}: the components' widths differ 400-fold, the wide ones own the tails and the narrow ones the middle
    cases.append(("scales", 0.5 * rng.standard_normal((2, n)), (0.1 * np.exp(np.clip(rng.standard_normal(n), -3.0, 3.0))) ** 2, PROBS))
    # extreme p: 1e-6 and 1 - 1e-6 — the sum is taken in the smaller tail, or 1 - 1e-6 would be resolved to 1e-10 of its tail only
    cases.append(("extreme_p", rng.standard_normal((2, 517)), (0.05 * rng.uniform(0.5, 1.5, 517)) ** 2, (1e-6, 1.0 - 1e-6)))
    for _, series, std2, _ in cases:
        check_condition(series, std2)
    return cases
