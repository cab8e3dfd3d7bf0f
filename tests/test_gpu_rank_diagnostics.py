"""
GPU tests of the rank-normalised diagnostics and order statistics (include/rsf_diag.h, rsf_diag_rank_*): the derived series,
median, quantiles and HDI against tests/rank_diagnostics_reference.py on synthetic and sampler-made traces, the finished
statistics, determinism across calls and memory spaces, argument checks through a real ctx, and PosteriorPool end to end.
"""
import ctypes

import numpy as np
import pytest

import rank_diagnostics_reference as rref
from conftest import synthetic_data

pytestmark = pytest.mark.gpu

NS = len(rref.STATS)


def ar1(n, C, d, seed, phi=0.9, frozen_every=0):
    """AR(1) chains around (1000, 0.011, 0.014); every `frozen_every`-th chain never leaves its start."""
    rng = np.random.default_rng(seed)
    z = np.empty((n, C, d))
    cur = rng.standard_normal((C, d)) / np.sqrt(1 - phi * phi)
    for i in range(n):
        z[i] = cur
        cur = phi * cur + rng.standard_normal((C, d))
    x = np.array([1000.0, 0.011, 0.014])[:d] + z * np.array([50.0, 1e-3, 1e-3])[:d]
    if frozen_every:
        x[:, 7::frozen_every] = x[:1, 7::frozen_every]
    return x


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_prepare(eng, x, probs=(0.025, 0.5, 0.975), hdi_prob=0.94):
    """Series and stats of rsf_diag_rank_prepare against the reference: z within 1e-14 max(1, |z|), everything else exact."""
    st, ser = eng.rank_prepare(x, probs, hdi_prob, series=True)
    eng.rank_release()
    ser = ser.cpu().numpy() if hasattr(ser, "cpu") else ser
    want_st, want_ser = rref.prepare(x, probs, hdi_prob)
    assert _same(st, want_st), (st, want_st)
    for q in (0, 1):
        g, w = ser[q], want_ser[q]
        assert np.array_equal(np.isnan(g), np.isnan(w))
        ok = np.isnan(w) | (np.abs(g - w) <= 1e-14 * np.maximum(1.0, np.abs(w)))
        assert ok.all(), f"series {rref.SERIES[q]}: {np.count_nonzero(~ok)} scores off, first at {np.argwhere(~ok)[0]}"
    assert _same(ser[2:], want_ser[2:])
    return st, ser


def check_stats(got, want, rtol=1e-10):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in rref.OUT[:-1]:
            a, b = g[k], float(w[k])
            assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= rtol * abs(b), (k, a, b)
        assert g["lags_complete"] == w["lags_complete"]
        assert _same(g["median"], w["median"]) and _same(g["hdi"], w["hdi"])
        assert _same(list(g["quantiles"].values()), list(w["quantiles"].values()))


def reference_stats(x, got, **kw):
    return rref.rank_diagnostics(x, n_lags=got[0]["n_lags"], **kw)


@pytest.mark.parametrize("d,n,C", [(1, 40, 3000), (1, 41, 3000), (2, 41, 1500), (3, 40, 1000), (3, 41, 1000)])
def test_ar1_series_order_stats_and_statistics(gpu_engine, d, n, C):
    x = ar1(n, C, d, seed=10 * d + n, frozen_every=100)
    check_prepare(gpu_engine, x)
    got = gpu_engine.rank_diagnostics(x)
    assert all(r["lags_complete"] for r in got)
    check_stats(got, reference_stats(x, got))


def _tie_heavy_trace(pkg, C=4096, n=120, seed=3):
    """The reference's main.py setting at Dc_true = 100: list prior on [0, 1e4], every chain started at 1000, no adaptation."""
    model = pkg.RateStateModel(number_time_steps=500)
    with pkg.Engine(mem="host") as e:
        e.set_model(model, 1)
        data = synthetic_data(e, dc_true=100.0)
        e.mcmc_init(np.full((C, 1), 1000.0), data, [0.0], [1.0e4], seed=seed, prior_len=3)
        tq, _, _ = e.mcmc_run(n, traces=("q",))
        stats = e.stats()
    return np.asarray(tq), stats


def test_sampler_tie_heavy_trace(gpu_engine, pkg):
    x, stats = _tie_heavy_trace(pkg)
    rate = stats["accepted"] / (x.shape[0] * x.shape[1])
    assert rate < 0.05, rate
    assert np.unique(x).size < x.size / 10  # mostly runs of repeated draws
    check_prepare(gpu_engine, x)
    got = gpu_engine.rank_diagnostics(x)
    check_stats(got, reference_stats(x, got))


def test_constant_parameter(gpu_engine):
    x = ar1(30, 500, 2, seed=4)
    x[:, :, 1] = 0.0125
    st, _ = check_prepare(gpu_engine, x)
    assert list(st[1, 6:10]) == [1.0, 1.0, 1.0, 1.0]
    got = gpu_engine.rank_diagnostics(x)
    T = 2 * 500 * 15
    assert got[1]["ess_bulk"] == T and got[1]["ess_tail"] == T and np.isnan(got[1]["rhat"])
    check_stats(got, reference_stats(x, got))


def test_one_non_finite_draw(gpu_engine):
    x = ar1(30, 700, 3, seed=5)
    x[17, 333, 1] = np.nan
    x[3, 5, 2] = np.inf
    st, _ = check_prepare(gpu_engine, x)
    assert list(st[:, 5]) == [0.0, 1.0, 1.0]
    got = gpu_engine.rank_diagnostics(x)
    assert np.isfinite(got[0]["rhat"]) and np.isnan(got[1]["ess_bulk"]) and np.isnan(got[2]["median"])
    check_stats(got, reference_stats(x, got))


def test_signed_zeros_tie(gpu_engine):
    rng = np.random.default_rng(6)
    x = rng.choice([-0.0, 0.0, -1.5, 2.0, 1e-300, -1e-300], size=(24, 300, 1))
    st, ser = check_prepare(gpu_engine, x)
    z = ser[0, :, :, 0]
    assert np.unique(z[x[:, :, 0] == 0.0]).size == 1  # -0.0 and +0.0 share one rank
    got = gpu_engine.rank_diagnostics(x)
    check_stats(got, reference_stats(x, got))


def test_many_workgroups_per_radix_pass(gpu_engine):
    # n*C > 2^24: every pass, scan and carry runs over thousands of tiles; odd n leaves out a middle row
    n, C = 65, 262144
    rng = np.random.default_rng(7)
    x = (1000.0 + 50.0 * rng.standard_normal((n, C, 1))).round(2)  # 2-decimal values: many ties spread over long runs
    assert n * C > 1 << 24
    check_prepare(gpu_engine, x, probs=(0.0, 0.1, 0.5, 1.0), hdi_prob=0.5)


def test_deterministic_and_memory_space_independent(gpu_engine, pkg):
    import torch

    x = ar1(50, 4000, 2, seed=8, frozen_every=50)
    a = gpu_engine.rank_prepare(x, (0.1, 0.9), 0.8, series=True)
    b = gpu_engine.rank_prepare(x, (0.1, 0.9), 0.8, series=True)
    pa = gpu_engine.rank_partials(0, 20)
    gpu_engine.rank_release()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    with pkg.Engine(mem="device") as dev:
        c = dev.rank_prepare(torch.as_tensor(x, device="cuda"), (0.1, 0.9), 0.8, series=True)
        pc = dev.rank_partials(0, 20)
        dev.rank_release()
    assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].cpu().numpy().tobytes()
    assert pa.tobytes() == pc.tobytes()
    r1 = gpu_engine.rank_diagnostics(x)
    r2 = gpu_engine.rank_diagnostics(x)
    assert repr(r1) == repr(r2)


def test_diag_partials_unchanged_by_rank_call(gpu_engine):
    x = ar1(40, 2048, 3, seed=9)
    before = gpu_engine.diag_partials(x, 8)
    gpu_engine.rank_prepare(x)
    gpu_engine.rank_partials(0, 10)
    after_prepare = gpu_engine.diag_partials(x, 8)
    gpu_engine.rank_release()
    gpu_engine.rank_diagnostics(x)
    after = gpu_engine.diag_partials(x, 8)
    assert before.tobytes() == after_prepare.tobytes() == after.tobytes()


def test_argument_validation(gpu_engine):
    lib, ctx = gpu_engine.lib, gpu_engine._ctx
    dbl = ctypes.POINTER(ctypes.c_double)
    x = np.zeros((8, 6, 1))
    pr = np.array([0.5])
    st = np.empty((3, NS + 1))
    X, P, S = x.ctypes.data, pr.ctypes.data_as(dbl), st.ctypes.data_as(dbl)
    part = np.empty((4, 3, 9 + 4))
    O = part.ctypes.data_as(dbl)
    f = lib.rsf_diag_rank_prepare
    assert lib.rsf_diag_rank_partials(ctx, 0, 2, O) == -1  # partials before prepare
    assert f(ctx, 8, 6, 1, X, 1, P, 0.5, S, None) == 0
    assert lib.rsf_diag_rank_partials(ctx, 0, 4, O) == 0
    bad = [(ctx, 3, 6, 1, X, 1, P, 0.5, S, None), (ctx, 8, 0, 1, X, 1, P, 0.5, S, None), (ctx, 8, 6, 0, X, 1, P, 0.5, S, None),
           (ctx, 8, 2, 4, X, 1, P, 0.5, S, None), (ctx, 8, 6, 1, X, -1, P, 0.5, S, None), (ctx, 8, 6, 1, X, 1, P, 0.0, S, None),
           (ctx, 8, 6, 1, X, 1, P, 1.0, S, None), (ctx, 8, 6, 1, X, 1, P, 0.01, S, None), (ctx, 8, 6, 1, X, 1, P, float("nan"), S, None),
           (ctx, 1 << 16, 1 << 16, 1, X, 1, P, 0.5, S, None), (None, 8, 6, 1, X, 1, P, 0.5, S, None),
           (ctx, 8, 6, 1, None, 1, P, 0.5, S, None), (ctx, 8, 6, 1, X, 1, None, 0.5, S, None), (ctx, 8, 6, 1, X, 1, P, 0.5, None, None)]
    for args in bad:
        assert f(*args) == -1, args
    for v in (-0.1, 1.1, float("nan")):
        pr[0] = v
        assert f(ctx, 8, 6, 1, X, 1, P, 0.5, S, None) == -1, v
    assert f(ctx, 8, 6, 1, X, 0, None, 0.5, S, None) == 0  # no quantiles asked: probs may be NULL
    for lb, le in ((-1, 2), (2, 2), (0, 5)):
        assert lib.rsf_diag_rank_partials(ctx, lb, le, O) == -1
    assert lib.rsf_diag_rank_partials(ctx, 0, 4, None) == -1
    assert lib.rsf_diag_rank_release(ctx) == 0
    assert lib.rsf_diag_rank_partials(ctx, 0, 4, O) == -1  # released
    assert lib.rsf_diag_rank_release(None) == -1
    out = np.empty((1, 8))
    fin = lib.rsf_diag_rank_finish
    assert fin(8, 1, S, 0, O, 4, out.ctypes.data_as(dbl)) == 0
    for args in ((3, 1, S, 0, O, 4), (8, 0, S, 0, O, 4), (8, 1, S, -1, O, 4), (8, 1, S, 0, O, 1), (8, 1, S, 0, O, 5),
                 (8, 1, None, 0, O, 4), (8, 1, S, 0, None, 4)):
        assert fin(*args, out.ctypes.data_as(dbl)) == -1, args
    with pytest.raises(ValueError):
        gpu_engine.rank_partials(0, 2)


def test_posterior_pool_rank_diagnostics(pkg):
    model = pkg.RateStateModel(number_time_steps=500)
    with pkg.Engine(mem="host") as e:
        e.set_model(model, 1)
        data = synthetic_data(e)
    mc = pkg.MCMC(model, data, 1000.0, ["Uniform", 0.0, 10000.0], 1000.0, nsamples=80, lstm_model=None, verbose=False)
    pool = mc.sample_batched(512, seed=5, jitter=(500.0, 2000.0), mem="host")
    got = pool.rank_diagnostics(probs=(0.05, 0.5, 0.95), hdi_prob=0.9)
    check_stats(got, reference_stats(pool.samples, got, probs=(0.05, 0.5, 0.95), hdi_prob=0.9))
