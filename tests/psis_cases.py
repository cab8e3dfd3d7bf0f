"""
Inputs shared by tests/test_psis_reference.py (CPU) and tests/test_gpu_psis.py: crafted rows, and the bounds of the GPU test.

A row can be given any set of log-ratios through the one entry point: with data = 0 and std2 = 0.5 for every draw,
l = -1/2 log(pi) - y^2, so y_i = sqrt(target_i) makes x_i = -l_i = target_i + const.

Bounds (none can be derived: the fit multiplies rounding by N through L_j): the distance between tests/psis_reference.py evaluated in plain float64 NumPy and
in long double, over every crafted case below and the real-draw cases (d = 1 and 3, n = 1037 and 16 421, nsteps 500, the series
of the CPU restatement), times 8 — the factor covers the kernel summing n terms in another order than NumPy's pairwise sum.
Measured (test_psis_reference.py::test_float64_distance_sizes_the_bounds prints and re-checks them):
    elpd_loo_k over max(|elpd_loo_k|, 1):  1.449e-13 (real draws, d = 3, n = 16 421; the crafted rows: 1.2e-15)
    weight_ess_k, relative:                1.4572e-13, recorded as 1.458e-13 (real draws, d = 3, n = 1037; the crafted rows: 1.0e-14)
    pareto_k, absolute:                    1.736e-13 (real draws, d = 3, n = 16 421; the crafted rows: 6.6e-14)
    n_tail: equal in every row.
The scaled bound, for elpd_loo_k and weight_ess_k, is 8 x the larger of the first two; pareto_k has its own.
"""
import numpy as np

DIST_SCALED = 1.458e-13  # measured: float64 against long double, elpd_loo_k and weight_ess_k
DIST_K = 1.736e-13       # measured: float64 against long double, pareto_k (absolute)
TOL_SCALED = 8 * DIST_SCALED  # 1.1664e-12
TOL_K = 8 * DIST_K            # 1.3888e-12

STD2 = 0.5


def series_of(targets):
    """Rows of log-ratios (rows, n), each >= 0 → the series y = sqrt(target) that produces them with data = 0, std2 = 0.5."""
    return np.sqrt(np.asarray(targets, dtype=np.float64))


def crafted():
    """[(name, series (rows, n), r_eff)]; std2 = full(n, STD2), data = zeros(rows)."""
    rng = np.random.default_rng(20240)
    cases = []
    # heavy tails with known shape: ratios u^-k, log-ratios k * Exp(1); k = 0.2, 0.5, 0.9 and light (k -> 0: a normal's square)
    n = 4099
    e = rng.exponential(size=(3, n))
    cases.append(("heavy_tail", series_of(np.vstack([0.2 * e[0], 0.5 * e[1], 0.9 * e[2], rng.standard_normal(n) ** 2])), 1.0))
    # a pool with repeated draws: 300 values 14 times each; n = 4200, tail_len = 195, x_(4004) is the first of a group of 14, so
    # the 13 groups above it are the tail: n_tail = 182 < tail_len.  Second row: the same pool shuffled
    vals = np.sort(0.7 * rng.exponential(size=300))
    rep = np.repeat(vals, 14)
    cases.append(("repeats", series_of(np.vstack([rep, rng.permutation(rep)])), 1.0))
    for n in (1, 5, 25):
        cases.append((f"n{n}", series_of(0.5 * rng.exponential(size=(2, n))), 1.0))
    # an all-equal row, and one with a single different draw
    one = np.full(517, 0.3)
    other = one.copy()
    other[100] = 2.0
    cases.append(("all_equal", series_of(np.vstack([one, other])), 1.0))
    # a range of x beyond 708: 950 draws near 0, 50 near 1450; x_(904) - max is about -1500, so the cutoff clamps at log(DBL_MIN)
    wide = np.concatenate([rng.uniform(0.0, 1.0, 950), 1400.0 + 100.0 * rng.uniform(size=50) ** 3])
    cases.append(("clamped_cutoff", series_of(np.vstack([rng.permutation(wide), wide])), 1.0))
    # r_eff != 1: a longer tail (n = 4099, r_eff = 0.37: 316 against 193), and the longest the library takes in one workgroup's
    # LDS: n = 40 000, r_eff = 0.01 gives 6000
    cases.append(("r_eff", series_of(np.vstack([0.5 * e[1], 0.9 * e[2]])), 0.37))
    cases.append(("long_tail", series_of(0.4 * rng.exponential(size=(1, 40000))), 0.01))
    return cases


def real_draws(pkg, cpu, n, d, seed, nsteps=500):
    """Draws from the box of tests/test_gpu_predictive.py, noise variances and an observation for a model of nsteps output
    times (set on `cpu`, the CPU restatement) → (model, q (n, d), std2 (n,), data (nout,))."""
    model = pkg.RateStateModel(number_time_steps=nsteps)
    model.RadiationDamping = True
    cpu.set_model(model, 1)
    rng = np.random.default_rng(seed)
    q = np.ascontiguousarray(np.column_stack([rng.uniform(600.0, 1600.0, n), rng.uniform(0.009, 0.013, n), rng.uniform(0.013, 0.017, n)])[:, :d])
    truth = restatement_series(cpu, np.array([[1000.0, model.a, model.b]])[:, :d])[:, 0]
    amp = np.abs(truth).max()
    data = truth + 0.05 * amp * rng.standard_normal(truth.size)
    std2 = (rng.uniform(0.05, 0.3, n) * amp) ** 2
    return model, q, std2, data


def restatement_series(cpu, q):
    d = q.shape[1]
    _, acc = cpu.forward(q[:, 0], a=q[:, 1] if d == 3 else None, b=q[:, 2] if d == 3 else None)
    return np.asarray(acc)


REAL = ((1, 1037), (3, 1037), (1, 16421), (3, 16421))  # (d, n); seed 400 + d + n
