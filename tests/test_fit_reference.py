"""
CPU tests of the specification of the multi-start Levenberg-Marquardt fit (tests/fit_reference.py) — on closed-form residual
models, where the answer is known, and on the checker's forward solve, where it reproduces the figures the rule was chosen by —
and of rsf_fit_laplace (host arithmetic of librsf_hip.so, no GPU) against long double.
"""
import ctypes

import numpy as np
import pytest

import fit_reference as F
from duck_model import DecayModel

LD = np.longdouble


# ---- closed forms -------------------------------------------------------------------------------------------------------------------
def _linear(seed=5, N=40, d=3):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, d)) * np.array([1.0, 0.3, 3.0])[:d]
    truth = np.array([4.0, -2.0, 0.5])[:d]
    data = A @ truth + 0.05 * rng.standard_normal(N)
    return A, data, (lambda pts: A @ np.asarray(pts, dtype=np.float64).T)


def test_linear_model_one_undamped_step_is_exact():
    A, data, solve = _linear()
    want = np.linalg.lstsq(A, data, rcond=None)[0]
    lo, hi = np.full(3, -100.0), np.full(3, 100.0)
    q0 = np.array([[1.0, 1.0, 1.0], [7.0, -5.0, 2.0]])
    ssq, g, H = F.normal(solve, q0, data, 1e-6)
    # The forward difference of a linear model is its derivative — divided by (1 + fd), since the PERTURBED value is in the
    # denominator: X is 1e-6 small, X^T X 2e-6, and the undamped step (X^T X)^-1 X^T r 1e-6 long.  On top of that comes the
    # rounding of the difference, which 1 / fd amplifies to ~1e-9: a quarter of fd is allowed for it.
    fd = 1e-6
    np.testing.assert_allclose(H[0] * (1 + fd) ** 2, A.T @ A, rtol=0.25 * fd)
    np.testing.assert_allclose(g[0] * (1 + fd), A.T @ (A @ q0[0] - data), rtol=0.25 * fd, atol=1e-8)
    for i in range(2):
        ok, qt = F.trial(q0[i], g[i], H[i], 0.0, lo, hi)
        assert ok
        assert np.abs(qt - want).max() <= 1.25 * fd * np.abs(want - q0[i]).max()
    # the damped iteration gets there too, and says so (once at the minimum it still has to see a decrease below ftol, between
    # rejections in the rounding noise: the 40 iterations the real model is allowed)
    st = F.fit(lambda p: F.normal(solve, p, data, 1e-6), q0, lo, hi)
    assert (st["status"] == F.CONVERGED).all() and (st["iters"] <= 40).all()
    np.testing.assert_allclose(st["q"], np.tile(want, (2, 1)), rtol=1e-6)
    r = A @ want - data
    np.testing.assert_allclose(st["ssq"], float(r @ r), rtol=1e-12)


def test_box_clamp_failed_factor_and_failed_start():
    A, data, solve = _linear(d=1)
    lo, hi = np.array([0.0]), np.array([3.0])  # the minimum (near 4) lies outside: the iterates stop one ulp inside the edge
    st = F.fit(lambda p: F.normal(solve, p, data, 1e-6), [[1.0]], lo, hi, max_iter=40)
    assert st["q"][0, 0] == np.nextafter(3.0, 0.0) and st["status"][0] == F.STALLED  # at the edge nothing decreases any more
    ok, qt = F.trial(np.array([1.0]), np.array([1.0e3]), np.array([[1.0]]), 0.0, lo, hi)
    assert ok and qt[0] == np.nextafter(0.0, 3.0)
    # a factor that fails: no trial point, lam grows tenfold per iteration, STALLED once above 1e12
    for H in (np.array([[0.0]]), np.array([[-1.0]]), np.array([[np.nan]]), np.array([[np.inf]])):
        assert not F.trial(np.array([1.0]), np.array([1.0]), H, 1e-3, lo, hi)[0]
    st = F.new_state([[1.0]], [2.0], [[1.0]], [[[0.0]]])
    n = 0
    while st["status"][0] == F.RUNNING:
        ok, acc, _ = F.iterate(lambda p: (np.array([1.0]), np.array([[1.0]]), np.array([[[1.0]]])), st, lo, hi)
        assert not ok[0] and not acc[0]
        n += 1
    assert n == 16 and st["iters"][0] == 16 and st["status"][0] == F.STALLED and st["q"][0, 0] == 1.0
    # a start whose first sum is not finite never moves
    st = F.fit(lambda p: (np.array([np.nan]), np.array([[1.0]]), np.array([[[1.0]]])), [[1.0]], lo, hi)
    assert st["status"][0] == F.FAILED and st["iters"][0] == 0 and st["q"][0, 0] == 1.0
    # a non-finite trial sum is a rejection
    st = F.new_state([[1.0]], [2.0], [[1.0]], [[[1.0]]])
    _, acc, _ = F.iterate(lambda p: (np.array([np.inf]), np.array([[1.0]]), np.array([[[1.0]]])), st, lo, hi)
    assert not acc[0] and st["lam"][0] == 1e-2 and st["ssq"][0] == 2.0


def test_decay_model():
    m = DecayModel()
    rng = np.random.default_rng(8)

    def solve(pts):
        return np.stack([np.exp(-m.t / dc) * np.sin(3.0 * m.t) + 0.1 * np.log1p(dc) for dc in np.asarray(pts)[:, 0]], axis=1)

    data = solve(np.array([[4.0]]))[:, 0] + 0.02 * rng.standard_normal(m.t.size)
    lo, hi = np.array([0.1]), np.array([50.0])
    hist = []
    st = F.fit(lambda p: F.normal(solve, p, data, 1e-6), [[0.5], [2.0], [9.0], [30.0]], lo, hi, history=hist)
    assert (st["status"] == F.CONVERGED).all() and (st["iters"] <= 40).all()
    grid = np.linspace(3.6, 4.4, 4001)
    gmin = float(((solve(grid[:, None]) - data[:, None]) ** 2).sum(axis=0).min())
    assert (st["ssq"] <= gmin * (1 + 1e-9)).all() and np.ptp(st["q"]) <= 1e-6 * 4.0
    # an accepted step lowers ssq, a rejected one leaves it
    assert all((s[acc] < b[acc]).all() for _, acc, s, b in hist)


# ---- the checker's forward solve: the figures the rule was chosen by --------------------------------------------------------------
STARTS = (30.0, 300.0, 1000.0, 3000.0, 9000.0)


def checker_problem(pkg, eng, dc_true):
    """nsteps 500, noise 1 % of max|acc| (seed 3) -> (data, solve for fit_reference.normal at d = 1)"""
    model = pkg.RateStateModel(number_time_steps=500)
    model.RadiationDamping = True
    eng.set_model(model, 1)
    truth = np.asarray(eng.forward([dc_true])[1])[:, 0]
    data = truth + 0.01 * np.abs(truth).max() * np.random.default_rng(3).standard_normal(truth.size)
    return data, (lambda pts: np.asarray(eng.forward(np.ascontiguousarray(np.asarray(pts)[:, 0]))[1]))


@pytest.mark.parametrize("dc_true", [100.0, 1000.0, 5000.0])
def test_specification_on_the_checker(pkg, cpu_engine, dc_true):
    data, solve = checker_problem(pkg, cpu_engine, dc_true)
    st = F.fit(lambda p: F.normal(solve, p, data, 1e-6), np.array(STARTS)[:, None], [0.0], [1.0e4])
    grid = np.linspace(0.98 * dc_true, 1.02 * dc_true, 4001)
    gmin = float(np.asarray(cpu_engine.forward(grid, data=data, want_ssq=True, want_acc=False)[0]).min())
    print(f"Dc_true {dc_true}: iterations {st['iters'].tolist()}, ssq / grid minimum - 1 = {(st['ssq'] / gmin - 1).tolist()}, "
          f"spread of q {np.ptp(st['q']) / dc_true:.2e}, of ssq {np.ptp(st['ssq']) / gmin:.2e}")
    assert (st["status"] == F.CONVERGED).all()
    assert (st["iters"] <= 40).all()
    assert (st["ssq"] <= gmin * (1 + 1e-9)).all()


# ---- rsf_fit_laplace --------------------------------------------------------------------------------------------------------------
def _laplace(lib, d, n_obs, shape, ssq, jtj, lo, hi):
    out = np.empty(d * d + 2)
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rc = lib.rsf_fit_laplace(d, n_obs, shape, ssq, dp(jtj), dp(lo), dp(hi), dp(out))
    return rc, out


@pytest.mark.parametrize("d", [1, 2, 3])
def test_laplace_against_long_double(pkg, d):
    lib = pkg._abi.load()
    rng = np.random.default_rng(d)
    X = rng.standard_normal((50, d)) * np.array([2.0e-3, 40.0, 7.0])[:d]
    jtj = X.T @ X
    lo, hi = np.array([0.0, 1e-3, 1e-3])[:d], np.array([1.0e4, 0.1, 0.1])[:d]
    n_obs, shape, ssq = 500, 250.0, 3.7e-5
    rc, out = _laplace(lib, d, n_obs, shape, ssq, jtj, lo, hi)
    assert rc == 0, lib.rsf_last_error()
    cov, logi, ev = F.laplace(d, n_obs, shape, ssq, jtj, lo, hi)
    # a d x d factorisation of a matrix of condition number up to ~1e9 (the columns' scales squared): 1e-7 of sqrt(C_pp C_rr)
    sd = np.sqrt(np.diag(cov).astype(np.float64))
    assert np.abs((out[:d * d].reshape(d, d) - cov.astype(np.float64)) / np.outer(sd, sd)).max() <= 1e-7
    # log I ~ 2.5e3 is a sum of a few terms of that size: a few ulp of it
    assert abs(out[d * d] - float(logi)) <= 16 * np.spacing(abs(float(logi)))
    assert abs(out[d * d + 1] - float(ev)) <= 16 * np.spacing(abs(float(logi)))
    # the constant is rsf_smc_log_evidence's
    v = ctypes.c_double()
    dp = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.rsf_smc_log_evidence(out[d * d], shape, d, dp(lo), dp(hi), ctypes.byref(v)) == 0 and v.value == out[d * d + 1]


def test_laplace_errors(pkg):
    lib = pkg._abi.load()
    ok = dict(d=1, n_obs=500, shape=250.0, ssq=1.0, jtj=[[2.0]], lo=[0.0], hi=[1.0])
    assert _laplace(lib, **ok)[0] == 0
    for kw, code in ((dict(jtj=[[0.0]]), -6), (dict(jtj=[[-1.0]]), -6), (dict(jtj=[[np.nan]]), -6), (dict(d=0), -1), (dict(d=4), -1),
                     (dict(n_obs=1), -1), (dict(shape=0.0), -1), (dict(ssq=0.0), -1), (dict(ssq=np.inf), -1), (dict(lo=[1.0]), -1)):
        args = dict(ok)
        args.update(kw)
        assert _laplace(lib, **args)[0] == code, kw
    assert _laplace(lib, 2, 500, 250.0, 1.0, [[1.0, 2.0], [2.0, 1.0]], [0.0, 0.0], [1.0, 1.0])[0] == -6  # indefinite
    assert b"positive definite" in lib.rsf_last_error()
