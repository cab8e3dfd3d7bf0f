"""
GPU tests of the caller's loading history and the state law (include/rsf_law.h: rsf_set_loading / rsf_get_loading /
rsf_loading_size / rsf_law_forward; Engine.set_loading / loading / law_forward; RateStateModel.loading / state_law;
MCMC.compare_laws and the slip-law paths):
  1. the round trip: the table read back and set again, and the built-in history restored, change no bit of any result;
  2. law_forward under the ageing law is rsf_forward_batch's solve;
  3. both laws against the long-double specification (tests/law_reference.py) under the step and the hold history;
  4. the existing tier kernels under a custom history: no kernel trusts the a-priori 1.2 V_ref bound;
  5. a non-finite lane, its wave neighbours, and the rows past n;
  6. end to end: compare_laws against the specification's quadrature, sample_dr and sample_smc under the slip law;
  7. the refusals.
"""
import ctypes

import numpy as np
import pytest

import law_cases as C
import law_reference as R
from conftest import synthetic_data

pytestmark = pytest.mark.gpu


def _model(pkg, nsteps=500, substeps=1, **attrs):
    m = pkg.RateStateModel(number_time_steps=nsteps)
    m.substeps = substeps
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _bits(x):
    return np.ascontiguousarray(np.asarray(x.cpu() if hasattr(x, "cpu") else x, dtype=np.float64)).view(np.int64)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- 1. the round trip ----------------------------------------------------------------------------------------------------------------
def test_round_trip_changes_no_bit(pkg, gpu_engine):
    eng = gpu_engine
    eng.set_model(_model(pkg), 1)
    dc = np.geomspace(3.0, 5000.0, 257)  # every a-priori tier, FULL to TIGHT
    data = synthetic_data(eng)
    before = eng.forward(dc, data=data, want_ssq=True, want_acc=True)
    table = eng.loading()
    assert table.shape == (eng.loading_size(),) == (2 * (eng.nout - 1) + 1,)
    # rsf_set_model's table is the formula at the stage times: libm's exp and sin against NumPy's, an ulp each
    assert np.allclose(table, R.table(C.spec(), "builtin"), rtol=0.0, atol=8 * 2.0 ** -52)
    eng.set_loading(table)
    assert _same(before, eng.forward(dc, data=data, want_ssq=True, want_acc=True))
    eng.set_loading(R.table(C.spec(), "step"))
    assert np.array_equal(eng.loading(), R.table(C.spec(), "step"))
    step = eng.forward(dc, data=data, want_ssq=True, want_acc=True)
    assert not np.array_equal(_bits(step[1]), _bits(before[1]))
    eng.set_loading(None)
    assert np.array_equal(_bits(eng.loading()), _bits(table))
    assert _same(before, eng.forward(dc, data=data, want_ssq=True, want_acc=True))
    eng.set_loading(R.step_history)  # a callable, then a new model: rsf_set_model resets the history
    eng.set_model(_model(pkg), 1)
    assert np.array_equal(_bits(eng.loading()), _bits(table))


def test_round_trip_of_the_sampler(pkg, gpu_engine):
    eng = gpu_engine
    eng.set_model(_model(pkg, nsteps=100), 1)
    data = synthetic_data(eng)
    q0 = np.random.default_rng(3).uniform(300.0, 3000.0, (130, 1))

    def run():
        eng.mcmc_init(q0, data, [0.0], [1.0e4], seed=11, prior_len=3)
        return eng.mcmc_run(4)

    before = run()
    eng.set_loading(eng.loading())
    assert eng.n_chains is None  # the chains are discarded, as rsf_set_model discards them
    assert eng.lib.rsf_mcmc_stats(eng._ctx, None, None, None, None) == -3  # RSF_ERR_STATE
    assert _same(before, run())
    eng.set_loading(R.hold_history)
    eng.set_loading(None)
    assert _same(before, run())


# ---- 2. the new kernel is the old solve -------------------------------------------------------------------------------------------------
SAME_SOLVE = {
    "n 1": dict(n=1), "n 63, (a, b)": dict(n=63, ab=True), "n 65": dict(n=65), "n 257, (a, b)": dict(n=257, ab=True),
    "n 65, k1 = 0, (a, b)": dict(n=65, k1=0.0, ab=True), "n 257, k1 = 0": dict(n=257, k1=0.0), "n 63, undamped": dict(n=63, RadiationDamping=False),
    "n 65, two chunks": dict(n=65, nsteps=900, substeps=4, chunks=2),
}


@pytest.mark.parametrize("name", list(SAME_SOLVE))
def test_ageing_law_is_the_forward_batch_solve(pkg, gpu_engine, name):
    """SSq and series within the project's Tier-1 bound, rtol 1e-9 (the series relative to the lane's max|acc|); the distance
    measured is printed (about 1e-12 when this was written)."""
    c = dict(SAME_SOLVE[name])
    n, ab, chunks = c.pop("n"), c.pop("ab", False), c.pop("chunks", 1)
    eng = gpu_engine
    nsteps, substeps = c.pop("nsteps", 500), c.pop("substeps", 1)
    eng.set_model(_model(pkg, nsteps, substeps, **c), substeps)
    # the table and the observation of the chunked case do not fit the 56 KiB LDS budget at once
    assert (2 * substeps * (eng.nout - 1) + 1 + eng.nout > 56 * 1024 // 8) == (chunks == 2)
    dc = np.geomspace(8.0, 5000.0, n) if n > 1 else np.array([700.0])
    rng = np.random.default_rng(n)
    kw = dict(a=rng.uniform(0.009, 0.013, n), b=rng.uniform(0.012, 0.016, n)) if ab else {}
    data = synthetic_data(eng)
    s0, a0 = eng.forward(dc, data=data, want_ssq=True, want_acc=True, **kw)
    s1, a1 = eng.law_forward("ageing", dc, data=data, want_ssq=True, want_acc=True, **kw)
    assert np.isfinite(a0).all() and np.isfinite(a1).all() and (a1[0] == 0.0).all()
    d_acc = (np.abs(a1 - a0).max(axis=0) / np.abs(a0).max(axis=0)).max()
    d_ssq = (np.abs(s1 - s0) / s0).max()
    print(f"{name}: series {d_acc:.2e}, SSq {d_ssq:.2e}")
    assert d_acc < C.CAP and d_ssq < C.CAP
    # each output alone is the same launch's: SSq without the series, the series without SSq
    assert np.array_equal(_bits(eng.law_forward(0, dc, data=data, want_ssq=True, want_acc=False, **kw)[0]), _bits(s1))
    assert np.array_equal(_bits(eng.law_forward(0, dc, **kw)[1]), _bits(a1))


# ---- 3. both laws against long double ------------------------------------------------------------------------------------------------------
def _gpu_error(s, acc):
    return R.rel_error(np.asarray(acc)[:, :s["dc"].size], s["ext"])


@pytest.mark.parametrize("history", ["step", "hold"])
@pytest.mark.parametrize("law", R.LAWS)
def test_both_laws_against_long_double(pkg, gpu_engine, history, law):
    """Per lane set the GPU's largest error against the long-double specification, relative to the lane's max|acc|, is at most
    4 x the float64 specification's own largest error on that set — two CPU arrangements of the same recurrence differed by up
    to 2.1 x, and the device adds FMA contraction and its own log / exp — and in any case below 1e-9."""
    s = C.precision_set(history, law)
    eng = gpu_engine
    eng.set_model(_model(pkg, loading=R.HISTORIES[history]), 1)
    assert np.array_equal(eng.loading(), s["vl"])
    _, acc = eng.law_forward(law, C.padded(s["dc"]))
    err = _gpu_error(s, acc)
    print(f"{history} {law}: GPU {err.max():.2e}, float64 specification {s['yardstick']:.2e}, ratio {err.max() / s['yardstick']:.2f}; "
          f"per lane {np.array2string(err / s['err'], precision=2)}")
    assert np.isfinite(np.asarray(acc)).all()
    assert err.max() < C.CAP
    assert err.max() <= 4.0 * s["yardstick"]


# ---- 4. the existing tiers under a custom history ------------------------------------------------------------------------------------------
def test_tier_kernels_under_the_step_history(pkg, gpu_engine):
    """rsf_forward_batch — the incremental tiers with their a-priori classes, which assume |V_l - v| <~ 1.2 V_ref, and their
    escalation — under V_l = 10 V_ref: against law_forward's plain solve (Tier-1 bound) and against the long-double
    specification by test 3's rule.  Dc = 2 and 3 run the full 500 steps at the stiff edge of what fixed-step RK4 integrates."""
    s = C.precision_set("step", "aging", low=True)
    eng = gpu_engine
    eng.set_model(_model(pkg, loading=s["vl"]), 1)
    dc = C.padded(s["dc"])
    _, tiers = eng.forward(dc)
    _, plain = eng.law_forward("aging", dc)
    e_t, e_p = _gpu_error(s, tiers), _gpu_error(s, plain)
    between = (np.abs(tiers - plain).max(axis=0) / np.abs(plain).max(axis=0)).max()
    print(f"tiers {e_t.max():.2e} (ratio {e_t.max() / s['yardstick']:.2f}), plain {e_p.max():.2e} (ratio {e_p.max() / s['yardstick']:.2f}), "
          f"float64 specification {s['yardstick']:.2e}; tiers against plain {between:.2e}")
    assert np.isfinite(tiers).all() and between < C.CAP
    for e in (e_t, e_p):
        assert e.max() < C.CAP and e.max() <= 4.0 * s["yardstick"]


def test_fused_dr_against_split_under_the_step_history(pkg):
    """one fused sampler family under the custom history: four iterations of rsf_dr_run against rsf_dr_propose / _ssq / _accept,
    bit for bit, 130 chains"""
    m, n, lo, hi, L, gamma, seed, offset = C.spec(), 130, 5.0, 200.0, [[3.0]], 0.3, 5, 900
    vl = R.table(m, "step")
    data = R.bf_data(m, vl, "aging")
    q0 = np.random.default_rng(7).uniform(10.0, 60.0, (n, 1))
    cnt = lambda: [np.zeros(n, dtype=np.int32) for _ in range(5)]
    with pkg.Engine(mem="host", block_threads=64) as eng:
        eng.set_model(_model(pkg, loading=vl), 1)
        shape = 0.5 * eng.nout
        l0 = -shape * np.log(np.asarray(eng.fit_normal(q0, data)[0]))
        fused, split = [dict(q=q0.copy(), l=l0.copy(), c=cnt()) for _ in range(2)]
        moved = 0
        for it in range(1, 5):
            eng.dr_run(fused["q"], fused["l"], data, lo, hi, L, 1, fused["c"], gamma=gamma, shape=shape, seed=seed, offset=offset, iter0=it)
            kw = dict(gamma=gamma, seed=seed, offset=offset, iteration=it)
            y, msk = eng.dr_propose(split["q"], split["l"], lo, hi, L, 1, **kw)
            l1, pend = eng.dr_accept(split["q"], split["l"], lo, hi, 1, y, msk, eng.dr_ssq(y, msk, data), split["c"], shape, **kw)
            y, msk = eng.dr_propose(split["q"], split["l"], lo, hi, L, 2, pending=pend, **kw)
            eng.dr_accept(split["q"], split["l"], lo, hi, 2, y, msk, eng.dr_ssq(y, msk, data), split["c"], shape, l1=l1, pending=pend, **kw)
            assert np.array_equal(_bits(fused["q"]), _bits(split["q"])) and np.array_equal(_bits(fused["l"]), _bits(split["l"])), it
            assert all(np.array_equal(a, b) for a, b in zip(fused["c"], split["c"]))
        moved = int(sum(c.sum() for c in fused["c"][:2]))
        # ... and the chains' l is the step history's: the plain solve's SSq at the final states, to the Tier-1 bound
        ssq = np.asarray(eng.law_forward("aging", fused["q"][:, 0], data=data, want_ssq=True, want_acc=False)[0])
        assert moved > 0 and np.allclose(fused["l"], -shape * np.log(ssq), rtol=0.0, atol=shape * 4 * C.CAP)


# ---- 5. non-finite paths -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", R.LAWS)
def test_non_finite_lane_and_rows_past_n(pkg, gpu_engine, law):
    eng = gpu_engine
    eng.set_model(_model(pkg, loading=R.step_history), 1)
    nout, n = eng.nout, 70  # two waves; the second holds six lanes of the batch
    data = R.bf_data(C.spec(), R.table(C.spec(), "step"), "aging")
    dc = np.concatenate([[0.5], np.geomspace(5.0, 5000.0, n - 1)])
    ssq, acc = eng.law_forward(law, dc, data=data, want_ssq=True, want_acc=True)
    assert not np.isfinite(ssq[0]) and np.isfinite(ssq[1:]).all() and np.isfinite(acc[:, 1:]).all()
    # its wave neighbours are unaffected: the same lanes beside a harmless lane 0
    calm = dc.copy()
    calm[0] = 1000.0
    ssq2, acc2 = eng.law_forward(law, calm, data=data, want_ssq=True, want_acc=True)
    assert np.array_equal(_bits(ssq[1:]), _bits(ssq2[1:])) and np.array_equal(_bits(acc[:, 1:]), _bits(acc2[:, 1:]))
    # a lane past n writes nothing: the series is time-major with stride n, so such a store would land in the rows past nout
    SENT = -7.25
    big_acc, big_ssq = np.full((nout + 2, n), SENT), np.full(n + 64, SENT)
    pkg._abi.check(eng.lib, eng.lib.rsf_law_forward(eng._ctx, pkg._abi.LAWS[law], n, dc.ctypes.data, None, None, data.ctypes.data, big_ssq.ctypes.data,
                                                    big_acc.ctypes.data))
    assert (big_acc[nout:] == SENT).all() and (big_ssq[n:] == SENT).all()
    assert np.array_equal(_bits(big_acc[:nout]), _bits(acc)) and np.array_equal(_bits(big_ssq[:n]), _bits(ssq))


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------------
def _sampler(pkg, truth, **attrs):
    p = C.bayes_factor_problem(truth)
    model = _model(pkg, loading=p["vl"], **attrs)
    return p, model, pkg.MCMC(model, p["data"], R.BF_TRUTH, ["Uniform", *R.BF_BOX], R.BF_TRUTH, nsamples=10, verbose=False)


@pytest.mark.parametrize("truth, sign", [("slip", +1), ("aging", -1)])
def test_compare_laws_names_the_true_law(pkg, truth, sign):
    """Each law's log evidence within 1e-6 of the specification's quadrature ON THE SAME NODES (a cap: the project's d = 1
    figure is 2.3e-13), the log Bayes factor on the CPU test's side and beyond 5."""
    p, model, mc = _sampler(pkg, truth)
    out = mc.compare_laws()
    try:
        assert model.state_law == "aging" and sorted(out) == ["aging", "log_bayes_factor", "slip"]
        for law in R.LAWS:
            g = out[law]
            ssq = R.forward(p["m"], g.x[0], p["vl"], law, data=p["data"])[1]
            want, _ = R.log_evidence_1d(g.x[0], g.w[0], ssq, g.shape, *R.BF_BOX)
            print(f"truth {truth}, {law}: log evidence {g.log_evidence:.9f}, specification on its nodes {want:.9f} ({g.log_evidence - want:+.2e}); "
                  f"on 4001 trapezoid nodes {p['log_evidence'][law]:.6f}; mean {g.mean[0]:.4f}, outside {g.outside:.1e}")
            assert abs(g.log_evidence - want) < 1e-6
        print(f"truth {truth}: log Bayes factor {out['log_bayes_factor']:+.4f} (specification {p['log_bayes_factor']:+.4f})")
        assert out["log_bayes_factor"] == out["slip"].log_evidence - out["aging"].log_evidence
        assert sign * out["log_bayes_factor"] > 5.0 and np.sign(out["log_bayes_factor"]) == np.sign(p["log_bayes_factor"])
    finally:
        for law in R.LAWS:
            out[law].engine.close()


def test_sample_dr_under_the_slip_law(pkg):
    """256 chains x 200 iterations started from the quadrature's own draws — so every chain is stationary from its first state and
    the chains are independent: the pooled mean is the mean of 256 independent chain means, its standard error their SD / 16, and it
    lies within 4.5 of them (tests/posterior_reference.py's Z_MAX) of the quadrature's mean, which has no Monte-Carlo error."""
    p, model, mc = _sampler(pkg, "slip", state_law="slip")
    grid = mc.quadrature(n_draws=256, seed=3)
    try:
        sd = float(np.sqrt(grid.cov[0, 0]))
        pool = mc.sample_dr(256, 200, nburn=0, start=grid.q, factor=[[2.38 * sd]], seed=9)
    finally:
        grid.engine.close()
    x = np.asarray(pool.samples)[:, :, 0]
    assert x.shape == (200, 256) and pool.stats["stuck"] == 0 and pool.stats["adapt"] is False
    means = x.mean(axis=0)
    se = means.std(ddof=1) / np.sqrt(means.size)
    z = (means.mean() - grid.mean[0]) / se
    print(f"pooled mean {means.mean():.4f}, quadrature {grid.mean[0]:.4f} (SD {sd:.4f}), SE {se:.2e}, z {z:+.2f}; accept rates {pool.stats['accept_rate1']:.2f} "
          f"{pool.stats['accept_rate2']:.2f}; the ageing law's posterior mean lies {abs(C.bayes_factor_problem('slip')['log_bayes_factor']):.1f} log units of evidence away")
    assert 0.05 < pool.accept_rate < 0.95
    assert abs(z) < 4.5
    # the chains' l is the slip law's, not the ageing law's: -N/2 log SSq of the plain solve at the final states
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        ssq = eng.law_ssq_fn("slip", p["data"])(x[-1].reshape(-1, 1))
        other = eng.law_ssq_fn("aging", p["data"])(x[-1].reshape(-1, 1))
    want = -0.5 * len(p["data"]) * np.log(ssq)
    assert np.allclose(pool.stats["l"][-1], want, rtol=1e-12, atol=0.0)
    assert np.abs(-0.5 * len(p["data"]) * np.log(other) - want).min() > 1e-3


def test_sample_smc_and_the_model_under_the_slip_law(pkg):
    p, model, mc = _sampler(pkg, "slip", state_law="slip")
    pool = mc.sample_smc(512, seed=2)
    q = np.asarray(pool.samples).transpose(1, 0, 2).reshape(-1, 1)
    assert ((q > R.BF_BOX[0]) & (q < R.BF_BOX[1])).all() and pool.stats["n_solves"] > 512
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        ssq = eng.law_ssq_fn("slip", p["data"])(q)
        g = eng.grid_posterior(None, *R.BF_BOX, ssq_fn=eng.law_ssq_fn("slip", p["data"]))
    assert np.allclose(pool.stats["l"], -0.5 * len(p["data"]) * np.log(ssq), rtol=1e-12, atol=0.0)
    print(f"SMC log evidence {pool.stats['log_evidence']:.3f}, quadrature {g.log_evidence:.3f}; particle mean {q.mean():.3f}, quadrature {g.mean[0]:.3f}")
    # the front end honours both options: evaluate and evaluate_batch are the specification's slip-law series under the step history
    model.Dc = R.BF_TRUTH
    want = R.forward(p["m"], [R.BF_TRUTH, 50.0], p["vl"], "slip", dtype=R.LD)[0]
    t, acc, _ = model.evaluate()
    batch = model.evaluate_batch([R.BF_TRUTH, 50.0])
    assert t.shape == acc.shape == (R.nout(p["m"]),)
    assert R.rel_error(acc[:, None], want[:, :1]).max() < C.CAP and R.rel_error(batch.T, want).max() < C.CAP
    # ... and the ageing law with the model's loading runs the existing kernels: the sampler's own SSq is the step history's
    model.state_law = "aging"
    got = mc.SSqcalc(np.array([[R.BF_TRUTH]]))[0, 0]
    want = float(R.forward(p["m"], [R.BF_TRUTH], p["vl"], "aging", data=p["data"], dtype=R.LD)[1][0])
    assert abs(got - want) < C.CAP * want
    pool = mc.sample_batched(64, seed=1, n_iters=20, mem="host")
    assert np.isfinite(np.asarray(pool.samples)).all()


# ---- 7. the refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    abi = pkg._abi
    with pkg.Engine(mem="host") as eng:
        lib, one = eng.lib, np.ones(8)
        n64 = ctypes.c_int64()
        assert lib.rsf_set_loading(eng._ctx, ctypes.cast(one.ctypes.data, abi._DP), 8) == -3  # RSF_ERR_STATE: no model
        assert lib.rsf_loading_size(eng._ctx, ctypes.byref(n64)) == -3
        for attrs in (dict(integrator="dop853"), dict(precision="float32")):
            eng.set_model(_model(pkg, nsteps=50, **attrs), 1)
            table = np.ones(2 * (eng.nout - 1) + 1)
            assert lib.rsf_set_loading(eng._ctx, ctypes.cast(table.ctypes.data, abi._DP), table.size) == -5, attrs  # RSF_ERR_UNSUPPORTED
            assert lib.rsf_set_loading(eng._ctx, None, 0) == -5
        dc, acc = np.array([100.0]), np.empty((eng.nout, 1))
        assert lib.rsf_law_forward(eng._ctx, 1, 1, dc.ctypes.data, None, None, None, None, acc.ctypes.data) == 0  # float32 flag: the float64 solve
        assert np.isfinite(acc).all()
        eng.set_model(_model(pkg, nsteps=50, integrator="dop853"), 1)
        assert lib.rsf_law_forward(eng._ctx, 0, 1, dc.ctypes.data, None, None, None, None, acc.ctypes.data) == -5
        eng.set_model(_model(pkg, nsteps=50), 1)
        table = np.ones(2 * (eng.nout - 1) + 1)
        assert lib.rsf_law_forward(eng._ctx, 7, 1, dc.ctypes.data, None, None, None, None, acc.ctypes.data) == -1  # RSF_ERR_INVALID
        assert b"law" in lib.rsf_last_error()
        assert lib.rsf_set_loading(eng._ctx, ctypes.cast(table.ctypes.data, abi._DP), table.size - 1) == -1
        table[5] = np.nan
        assert lib.rsf_set_loading(eng._ctx, ctypes.cast(table.ctypes.data, abi._DP), table.size) == -1
        assert lib.rsf_law_forward(eng._ctx, 1, 1, dc.ctypes.data, None, None, None, acc.ctypes.data, None) == -1  # ssq_out without data
        with pytest.raises(NotImplementedError, match="state_law='slip' with precision='float32'"):
            eng.set_model(_model(pkg, state_law="slip", precision="float32"), 1)
