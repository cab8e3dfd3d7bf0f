"""
GPU tests of the convergence diagnostics (include/rsf_diag.h): rsf_diag_partials against the long-double reference
(tests/diagnostics_reference.py) on synthetic and sampler-made traces, its determinism and additivity, the finished statistics,
argument validation through a real ctx, and the superchain start points of MCMC.sample_batched end to end.
"""
import ctypes

import numpy as np
import pytest

import diagnostics_reference as ref
from conftest import synthetic_data

pytestmark = pytest.mark.gpu

HEAD = ref.HEAD


def _scales(want):
    """Per-field scale of reference partials (d, HEAD + L): sums that may cancel are measured against what bounds them."""
    w = np.abs(np.asarray(want, dtype=np.float64))
    s = w.copy()
    s[:, 1] = np.sqrt(w[:, 0] * w[:, 2])
    s[:, 5] = np.sqrt(w[:, 4] * w[:, 6])
    s[:, HEAD:] = np.maximum(w[:, 3:4], w[:, HEAD:].max(axis=1, keepdims=True))
    return np.maximum(s, 1e-300)


def _check_partials(got, want, rtol=1e-12):
    want64 = np.asarray(want, dtype=np.float64)
    assert got.shape == want64.shape
    err = np.abs(got - want64) / _scales(want)
    assert err.max() <= rtol, f"max scaled error {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"


def _real_trace(engine, d, C, n, seed):
    import bayesian_markov_chain_monte_carlo_amd as pkg

    model = pkg.RateStateModel(number_time_steps=500)
    engine.set_model(model, 1)
    data = synthetic_data(engine)
    rng = np.random.default_rng(seed)
    q0 = np.column_stack([rng.uniform(600.0, 1600.0, C), rng.uniform(0.009, 0.013, C), rng.uniform(0.013, 0.017, C)])[:, :d]
    lo, hi = [0.0, 0.005, 0.005][:d], [1e4, 0.02, 0.03][:d]
    engine.mcmc_init(q0, data, lo, hi, seed=seed, prior_len=3 if d == 1 else 0, fd_rel_step=1e-6 if d == 1 else 1e-4)
    tq, _, _ = engine.mcmc_run(n, traces=("q",))
    return np.asarray(tq)


@pytest.fixture(scope="module")
def trace_d1():
    import bayesian_markov_chain_monte_carlo_amd as pkg

    with pkg.Engine(mem="host") as e:
        return _real_trace(e, 1, 65536, 100, 21)


@pytest.fixture(scope="module")
def trace_d3():
    import bayesian_markov_chain_monte_carlo_amd as pkg

    with pkg.Engine(mem="host") as e:
        return _real_trace(e, 3, 4096, 100, 22)


def test_partials_smallest_shape(gpu_engine):
    x = np.array([1.0, 3.0, 2.0, 4.0]).reshape(4, 1, 1)
    _check_partials(gpu_engine.diag_partials(x), ref.partials(x))
    _check_partials(gpu_engine.diag_partials(x, superchain_size=1), ref.partials(x, 1))


@pytest.mark.parametrize("S", [None, 17])
def test_partials_odd_length_ragged_block(gpu_engine, S):
    rng = np.random.default_rng(31)
    x = np.array([1000.0, 0.011, 0.014]) + np.cumsum(rng.standard_normal((101, 4097, 3)), axis=0) * [1.0, 1e-4, 1e-4]
    x[:, 5::7] = x[:1, 5::7]  # chains that never moved
    _check_partials(gpu_engine.diag_partials(x, S), ref.partials(x, S))


@pytest.mark.parametrize("S", [None, 1, 8, 65536])
def test_partials_real_trace_d1(gpu_engine, trace_d1, S):
    assert trace_d1.shape == (100, 65536, 1)
    _check_partials(gpu_engine.diag_partials(trace_d1, S), ref.partials(trace_d1, S))


def test_partials_real_trace_d3(gpu_engine, trace_d3):
    _check_partials(gpu_engine.diag_partials(trace_d3, 8), ref.partials(trace_d3, 8))
    _check_partials(gpu_engine.diag_partials(trace_d3, None, lag_begin=5, lag_end=37), ref.partials(trace_d3, None, None, 5, 37))


def test_partials_far_centre(gpu_engine, trace_d1):
    # c = 0 with Dc near 1000: sums of (xbar - c)^2 carry 1e6 where the spread is O(1e2)
    _check_partials(gpu_engine.diag_partials(trace_d1, 8, center=0.0), ref.partials(trace_d1, 8, 0.0))


def test_partials_deterministic_and_memory_space_independent(gpu_engine, trace_d1):
    import torch

    import bayesian_markov_chain_monte_carlo_amd as pkg

    a = gpu_engine.diag_partials(trace_d1, 8)
    b = gpu_engine.diag_partials(trace_d1, 8)
    assert a.tobytes() == b.tobytes()
    with pkg.Engine(mem="device") as dev:
        c = dev.diag_partials(torch.as_tensor(trace_d1, device="cuda"), 8)
    assert a.tobytes() == c.tobytes()


def test_partials_of_two_halves_add_up(gpu_engine, trace_d1):
    C = trace_d1.shape[1]
    c = ref.default_center(trace_d1)
    whole = gpu_engine.diag_partials(trace_d1, 8, c)
    parts = gpu_engine.diag_partials(trace_d1[:, : C // 2], 8, c) + gpu_engine.diag_partials(trace_d1[:, C // 2:], 8, c)
    n = trace_d1.shape[0]
    for a, b in zip(gpu_engine.diag_finish(n, parts, c, 8), gpu_engine.diag_finish(n, whole, c, 8)):
        for k in ref.OUT:
            assert a[k] == pytest.approx(b[k], rel=1e-12, abs=0) or (np.isnan(a[k]) and np.isnan(b[k])), k


def _alternatives(n, part, center, S):
    """The reference's finish, plus — for every Geyer pair sum within 1e-9 of zero — the finish with that pair's sign flipped:
    a near-tie may fall either way in float64."""
    part = np.asarray(part, dtype=ref.LD)
    out = [ref.finish(n, part, center, S)]
    for p, r in enumerate(out[0]):
        if not np.isfinite(r["W"]) or not r["W"] > 0:
            continue
        Mp, vp, W = part[p, 0], r["var_plus"], r["W"]
        rho = 1 - (W - part[p, HEAD:] / Mp) / vp
        for t in range(1, len(rho) - 2, 2):
            s = rho[t + 1] + rho[t + 2]
            if abs(s) < 1e-9:
                print(f"near-tie: parameter {p}, pair ({t + 1}, {t + 2}) sums to {float(s):.3e}")
                alt = part.copy()
                alt[p, HEAD + t + 1] -= 2 * s * vp * Mp + np.sign(s) * 1e-12 * vp * Mp
                out.append(ref.finish(n, alt, center, S))
    return out


def _check_stats(got, alternatives, rtol=1e-10):
    for p, g in enumerate(got):
        ok = False
        for alt in alternatives:
            w = alt[p]
            ok = ok or all((np.isnan(float(w[k])) and np.isnan(g[k])) or abs(g[k] - float(w[k])) <= rtol * abs(float(w[k]))
                           for k in ref.OUT)
        assert ok, (p, g, alternatives[0][p])


@pytest.mark.parametrize("S", [None, 8])
def test_finished_statistics_real_trace(gpu_engine, trace_d1, S):
    got = gpu_engine.diagnostics(trace_d1, superchain_size=S)
    tr = ref.Trace(trace_d1, S)
    n_lags = got[0]["n_lags"]
    _check_stats(got, _alternatives(100, tr.partials(0, n_lags), tr.center, S))
    assert got[0]["K"] == (65536 // S if S else 0)


def test_finished_statistics_d3_and_explicit_lags(gpu_engine, trace_d3):
    got = gpu_engine.diagnostics(trace_d3, superchain_size=8, n_lags=12)
    tr = ref.Trace(trace_d3, 8)
    _check_stats(got, _alternatives(100, tr.partials(0, 12), tr.center, 8))
    full = gpu_engine.diagnostics(trace_d3, superchain_size=8)
    assert all(r["lags_complete"] for r in full)


def test_argument_validation(gpu_engine):
    lib, ctx = gpu_engine.lib, gpu_engine._ctx
    x = np.zeros((8, 6, 1))
    c = np.zeros(3)
    out = np.empty((3, HEAD + 8))
    dbl = ctypes.POINTER(ctypes.c_double)
    X, Cp, O = x.ctypes.data, c.ctypes.data_as(dbl), out.ctypes.data_as(dbl)
    f = lib.rsf_diag_partials
    assert f(ctx, 8, 6, 1, X, 3, Cp, 0, 4, O) == 0
    bad = [(ctx, 3, 6, 1, X, 0, Cp, 0, 1, O), (ctx, 8, 0, 1, X, 0, Cp, 0, 4, O), (ctx, 8, 6, 0, X, 0, Cp, 0, 4, O),
           (ctx, 8, 2, 4, X, 0, Cp, 0, 4, O), (ctx, 8, 6, 1, X, 4, Cp, 0, 4, O), (ctx, 8, 6, 1, X, -1, Cp, 0, 4, O),
           (ctx, 8, 6, 1, X, 0, Cp, 2, 2, O), (ctx, 8, 6, 1, X, 0, Cp, 0, 5, O), (ctx, 8, 6, 1, X, 0, Cp, -1, 3, O),
           (None, 8, 6, 1, X, 0, Cp, 0, 4, O), (ctx, 8, 6, 1, None, 0, Cp, 0, 4, O), (ctx, 8, 6, 1, X, 0, None, 0, 4, O),
           (ctx, 8, 6, 1, X, 0, Cp, 0, 4, None)]
    for args in bad:
        assert f(*args) == -1, args
    c[0] = np.nan
    assert f(ctx, 8, 6, 1, X, 0, Cp, 0, 4, O) == -1


def _mcmc(pkg):
    model = pkg.RateStateModel(number_time_steps=500)
    with pkg.Engine(mem="host") as e:
        e.set_model(model, 1)
        data = synthetic_data(e)
    return pkg.MCMC(model, data, 1000.0, ["Uniform", 0.0, 10000.0], 1000.0, nsamples=80, lstm_model=None, verbose=False)


def test_sample_batched_superchains_end_to_end(pkg):
    mc = _mcmc(pkg)
    C, seed, jit = 512, 5, (500.0, 2000.0)
    pool = mc.sample_batched(C, seed=seed, jitter=jit, superchain_size=8, mem="host")
    # the same run from start points shared by each block of 8 chains, built by hand
    q0 = np.array([np.random.default_rng([seed, g // 8]).uniform(*jit) for g in range(C)])
    assert np.all(q0.reshape(-1, 8) == q0[::8, None]) and len(np.unique(q0)) == C // 8
    again = mc.sample_batched(C, seed=seed, q0=q0, mem="host")
    assert pool.samples.tobytes() == again.samples.tobytes()
    got = pool.diagnostics()
    assert got[0]["K"] == C // 8
    tr = ref.Trace(pool.samples, 8)
    _check_stats(got, _alternatives(pool.samples.shape[0], tr.partials(0, got[0]["n_lags"]), tr.center, 8))


def test_sample_batched_default_keying_unchanged(pkg):
    mc = _mcmc(pkg)
    C, seed, jit = 256, 6, (500.0, 2000.0)
    pool = mc.sample_batched(C, seed=seed, jitter=jit, mem="host")
    q0 = np.array([np.random.default_rng([seed, g]).uniform(*jit) for g in range(C)])
    again = mc.sample_batched(C, seed=seed, q0=q0, mem="host")
    assert pool.samples.tobytes() == again.samples.tobytes()
    assert np.isnan(pool.diagnostics()[0]["nested_rhat"])
