"""
CPU tests of the quadrature reference (tests/posterior_reference.py) and of the checker's sampler against it.

1. Closed forms: with SSq = S0 + (q - q0)^T K (q - q0) the marginal is a Student-t (d = 1) or multivariate t (d = 3) with
   nu = 2 shape - d; a d = 1 box that truncates is compared with scipy.integrate.quad.
2. Its own accuracy on the rate-and-state targets: halving every grid spacing moves no reported moment or quantile by more
   than 0.05 of the Monte-Carlo SE the GPU legs use, the mass outside the fine window is below 1e-9, and start draws pass
   the checks.
3. The checker's sampler (the C restatement) keeps the target: the chain logic alone on the closed forms, and mcmc_run on
   the rate-and-state model — the machinery is right before any GPU is involved.
4. The float32 target's drift from the float64 one, exactly.
"""
import numpy as np
import pytest
from scipy import integrate, stats

import posterior_reference as R
from conftest import synthetic_data

LO3, HI3 = [0.0, 0.005, 0.005], [1.0e4, 0.02, 0.03]
_CACHE = {}


def _rsf(pkg, cpu_engine, d, nsteps=500, precision="float64", n_scale=1):
    key = (d, nsteps, precision, n_scale)
    if key not in _CACHE:
        m = pkg.RateStateModel(number_time_steps=nsteps)
        cpu_engine.set_model(m, 1)
        data = synthetic_data(cpu_engine)
        m.precision = precision
        cpu_engine.set_model(m, 1)
        fn = R.checker_ssq(cpu_engine, data)
        if d == 1:
            ref = R.Posterior1(fn, 0.0, 1.0e4, 0.5 * data.size, n_fine=4000 * n_scale + 1, n_coarse=4000 * n_scale + 1)
        else:
            ref = R.Posterior3(fn, LO3, HI3, 0.5 * data.size, n_ab=32 * n_scale, n_pc=96 * n_scale + 1, n_fine=2000 * n_scale + 1)
        _CACHE[key] = (ref, data)
    return _CACHE[key]


# ---- 1. closed forms -----------------------------------------------------------------------------------------------------

def _nodes(mg, x):
    """the CDF's grid points nearest x (between them the CDF is interpolated linearly: ~1e-7, well inside what KS resolves)"""
    return mg.xs[np.abs(mg.xs[None, :] - np.asarray(x)[:, None]).argmin(axis=1)]


def test_one_parameter_student_t():
    S0, q0, k, shape = 2.0, 3.0, 5.0, 20.0
    nu = 2 * shape - 1
    t = stats.t(nu, loc=q0, scale=np.sqrt(S0 / (k * nu)))
    ref = R.Posterior1(R.quadratic_ssq(S0, [q0], [[k]]), -100.0, 100.0, shape)
    mg = ref.marg["Dc"]
    assert ref.outside < 1e-9
    assert abs(mg.mean - t.mean()) < 1e-8 * t.std()
    assert abs(mg.var / t.var() - 1) < 1e-8
    xs = _nodes(mg, t.ppf([0.001, 0.025, 0.3, 0.5, 0.8, 0.999]))
    np.testing.assert_allclose(mg.cdf(xs), t.cdf(xs), atol=1e-8)
    # sigma^2: E[sigma^2] = E[SSq] / (2 (shape - 1)), E[SSq] = S0 + k Var(q)
    assert abs(ref.marg["sigma2"].mean / ((S0 + k * t.var()) / (2 * (shape - 1))) - 1) < 1e-8


def test_one_parameter_truncated_by_the_box():
    S0, q0, k, shape, lo, hi = 1.0, 1.0, 4.0, 12.0, 0.0, 1.3
    f = lambda x: (S0 + k * (x - q0) ** 2) ** -shape  # noqa: E731
    Z = integrate.quad(f, lo, hi, epsabs=0, epsrel=1e-13)[0]
    m = integrate.quad(lambda x: x * f(x), lo, hi, epsabs=0, epsrel=1e-13)[0] / Z
    v = integrate.quad(lambda x: (x - m) ** 2 * f(x), lo, hi, epsabs=0, epsrel=1e-13)[0] / Z
    ref = R.Posterior1(R.quadratic_ssq(S0, [q0], [[k]]), lo, hi, shape)
    mg = ref.marg["Dc"]
    assert abs(mg.mean - m) < 1e-8 * np.sqrt(v) and abs(mg.var / v - 1) < 1e-8
    for x in _nodes(mg, [0.7, 0.95, 1.1, 1.25]):
        assert abs(mg.cdf(x) - integrate.quad(f, lo, x, epsabs=0, epsrel=1e-13)[0] / Z) < 1e-8


def test_three_parameter_multivariate_t():
    """(Dc, a, b) with a box of +-9 SD about q0 in every parameter: mean q0, covariance nu / (nu - 2) S0 K^-1 / nu."""
    S0, q0, shape = 1.0, np.array([1.0, 2.0, 3.0]), 30.0
    K = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, -0.8], [0.5, -0.8, 2.0]])
    nu = 2 * shape - 3
    cov = S0 * np.linalg.inv(K) / (nu - 2)
    sd = np.sqrt(np.diag(cov))
    ref = R.Posterior3(R.quadratic_ssq(S0, q0, K), q0 - 9 * sd, q0 + 9 * sd, shape, n_ab=64, n_pc=193, n_fine=4001)
    # the box's own truncation of a multivariate t at 9 SD (nu = 57): P(|T| > 9) ~ 1e-12 per parameter.  Measured: means within
    # 1.6e-8 SD, variances within 1e-8 relative (the p window's corners are cut by the Dc box here; the rate-and-state target's
    # are not); tolerance 1e-7
    tol = 1e-7
    for name, k in (("a", 1), ("b", 2)):
        mg = ref.marg[name]
        assert abs(mg.mean - q0[k]) < tol * sd[k], (name, mg.mean - q0[k])
        assert abs(mg.var / cov[k, k] - 1) < tol, (name, mg.var / cov[k, k] - 1)
    # Dc: integrated in p = Dc a, then transformed back
    mg = ref.marg["Dc"]
    assert abs(mg.mean - q0[0]) < tol * sd[0] and abs(mg.var / cov[0, 0] - 1) < tol, (mg.mean - q0[0], mg.var / cov[0, 0] - 1)
    t = stats.t(nu, loc=q0[1], scale=np.sqrt(cov[1, 1] * (nu - 2) / nu))
    xs = _nodes(ref.marg["a"], t.ppf([0.01, 0.3, 0.5, 0.9]))
    np.testing.assert_allclose(ref.marg["a"].cdf(xs), t.cdf(xs), atol=tol)


# ---- 2. the reference's own accuracy ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,C", [(1, 262144), (3, 65536)])
def test_grid_halving_moves_nothing_the_tests_could_see(pkg, cpu_engine, d, C):
    ref, _ = _rsf(pkg, cpu_engine, d)
    fine, _ = _rsf(pkg, cpu_engine, d, n_scale=2)
    assert ref.outside < 1e-9 and fine.outside < 1e-9
    shift = R.grid_shift_in_se(ref, fine, C)
    print(d, shift)
    assert max(shift.values()) < 0.05, shift


@pytest.mark.parametrize("d,C", [(1, 262144), (3, 65536)])
def test_start_draws_match_the_quadrature(pkg, cpu_engine, d, C):
    ref, data = _rsf(pkg, cpu_engine, d)
    rng = np.random.default_rng(31 + d)
    q = ref.draw(rng, C)
    fn = R.checker_ssq(cpu_engine, data)
    cpu_engine.set_model(pkg.RateStateModel(number_time_steps=500), 1)
    std2 = R.draw_std2(rng, fn(*q.T) if d == 3 else fn(q[:, 0]), ref.shape)
    fails = []
    R.check(f"draws d{d}", ref, q, std2, fails)
    assert not fails, fails


# ---- 3. the checker's sampler keeps the target -------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 3])
def test_checker_chain_logic_keeps_the_closed_form_target(cpu_engine, d):
    """rsf_mcmc_propose / rsf_mcmc_replay_ssq of the restatement, NumPy variates, a box that truncates."""
    ref, fn, c = R.closed_reference(d)
    fails = []
    R.run_injected(cpu_engine, ref, fn, c, 20000, (15, 30), 300 + d, f"checker injected d{d}", fails)
    assert not fails, fails


def test_checker_sampler_keeps_the_rate_and_state_target(pkg, cpu_engine, oracle_lib):
    """rsf_mcmc_run of the restatement (its own Philox variates), d = 1, 4096 chains x 100 iterations from the target."""
    ref, data = _rsf(pkg, cpu_engine, 1)
    C, rng = 4096, np.random.default_rng(41)
    e = pkg.Engine(lib=oracle_lib)
    try:
        e.set_model(pkg.RateStateModel(number_time_steps=500), 1)
        e.mcmc_init(ref.draw(rng, C), data, [0.0], [1.0e4], seed=41, n0=0.0, prior_len=3)
        _, ssq0, _, V = e.get_state()
        e.set_state(std2=R.draw_std2(rng, ssq0, ref.shape), V=np.ascontiguousarray(np.broadcast_to(V[:1], V.shape)))  # one V
        fails = []
        for n in (50, 50):
            e.mcmc_run(n, traces=False)
            q, _, std2, _ = e.get_state()
            R.check("checker mcmc_run d1", ref, q, std2, fails)
        assert 0.2 < e.stats()["accepted"] / (C * 100) < 0.95
    finally:
        e.close()
    assert not fails, fails


# ---- 4. the float32 target's drift ----------------------------------------------------------------------------------------

# Largest shift of a reported mean or quantile of the float32 target from the float64 one, in posterior SD of the quantity.
# Measured: d = 1, nsteps 500: 8.1e-6; nsteps 4000: 5.6e-5; d = 3, nsteps 500: 9.2e-6.  Bound 2e-4: 3.5x over the largest.
F32_DRIFT_MAX = 2e-4


@pytest.mark.parametrize("d,nsteps", [(1, 500), (1, 4000), (3, 500)])
def test_float32_target_drift_is_exact_and_small(pkg, cpu_engine, d, nsteps):
    r64, _ = _rsf(pkg, cpu_engine, d, nsteps)
    r32, _ = _rsf(pkg, cpu_engine, d, nsteps, precision="float32")
    worst = 0.0
    for name, m64 in r64.marg.items():
        if m64.xs.size <= 2:
            continue
        m32 = r32.marg[name]
        s = max(abs(m32.mean - m64.mean), np.abs(m32.quantiles() - m64.quantiles()).max()) / m64.sd
        print(f"d{d} n{nsteps} {name}: float32 drift {s:.2e} SD")
        worst = max(worst, s)
    print(f"d{d} n{nsteps}: largest float32 drift {worst:.2e} SD")
    assert worst < F32_DRIFT_MAX
