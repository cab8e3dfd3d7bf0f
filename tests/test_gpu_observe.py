"""
GPU tests of the observable option (include/rsf_observe.h: rsf_law_observe; Engine.law_observe / law_ssq_fn(observable=);
RateStateModel.observable / trajectory; MCMC on friction data):
  1. law_observe(law, "acc") is law_forward(law), bit for bit;
  2. the velocity series is the V whose differences the acc series holds;
  3. mu, theta and velocity against the long-double specification (tests/observe_reference.py), relative to the excursion;
  4. the sum of squares is the returned series' own, and the long-double one;
  5. a non-finite lane, its neighbours, the rows past n and nout, n = 0, the C refusals;
  6. end to end on friction data: compare_laws, the posterior SD against acceleration data, sample_dr, sample_smc, the model.
Shapes: nsteps 500 x substeps 1 under the step history unless stated.
"""
import numpy as np
import pytest

import law_cases as C
import law_reference as R
import observe_cases as OC
import observe_reference as O

pytestmark = pytest.mark.gpu


def _model(pkg, nsteps=500, substeps=1, **attrs):
    m = pkg.RateStateModel(number_time_steps=nsteps)
    m.substeps = substeps
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def _noisy(series, seed):
    """a series plus 5 % of its excursion, N(0, 1)"""
    return series + 0.05 * np.abs(series - series[0]).max() * np.random.default_rng(seed).standard_normal(series.size)


# ---- 1. the new kernel is the old solve ---------------------------------------------------------------------------------------------
SAME_SOLVE = {
    "n 1": dict(n=1), "n 63, (a, b)": dict(n=63, ab=True), "n 65": dict(n=65), "n 257, (a, b)": dict(n=257, ab=True),
    "n 65, k1 = 0, (a, b)": dict(n=65, k1=0.0, ab=True), "n 257, k1 = 0": dict(n=257, k1=0.0), "n 63, undamped": dict(n=63, RadiationDamping=False),
    "n 65, undamped, (a, b)": dict(n=65, RadiationDamping=False, ab=True), "n 65, two chunks, (a, b)": dict(n=65, nsteps=900, substeps=4, chunks=2, ab=True),
}


@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("name", list(SAME_SOLVE))
def test_acc_is_law_forward_bit_for_bit(pkg, gpu_engine, name, law):
    c = dict(SAME_SOLVE[name])
    n, ab, chunks = c.pop("n"), c.pop("ab", False), c.pop("chunks", 1)
    nsteps, substeps = c.pop("nsteps", 500), c.pop("substeps", 1)
    eng = gpu_engine
    eng.set_model(_model(pkg, nsteps, substeps, loading=R.step_history, **c), substeps)
    # the table and the observation of the chunked case do not fit the 56 KiB LDS budget at once
    assert (2 * substeps * (eng.nout - 1) + 1 + eng.nout > 56 * 1024 // 8) == (chunks == 2)
    dc = np.geomspace(5.0, 5000.0, n) if n > 1 else np.array([20.0])
    rng = np.random.default_rng(n)
    kw = dict(a=rng.uniform(0.009, 0.013, n), b=rng.uniform(0.012, 0.016, n)) if ab else {}
    data = _noisy(np.asarray(eng.law_forward(law, [20.0])[1])[:, 0], 1)
    s0, a0 = eng.law_forward(law, dc, data=data, want_ssq=True, want_acc=True, **kw)
    s1, a1 = eng.law_observe(law, "acc", dc, data=data, want_ssq=True, want_series=True, **kw)
    assert np.isfinite(a0).all() and np.isfinite(s0).all() and np.abs(a0).max() > 0.0
    assert np.array_equal(_bits(s1), _bits(s0)) and np.array_equal(_bits(a1), _bits(a0))
    # each output alone is the same launch's
    assert np.array_equal(_bits(eng.law_observe(law, 0, dc, data=data, want_ssq=True, want_series=False, **kw)[0]), _bits(s0))
    assert np.array_equal(_bits(eng.law_observe(law, "acc", dc, **kw)[1]), _bits(a0))


# ---- 2. velocity is the V that acc differences --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("nsteps, substeps", [(500, 1), (900, 4)])
def test_velocity_is_the_series_acc_differences(pkg, gpu_engine, law, nsteps, substeps):
    eng = gpu_engine
    m = _model(pkg, nsteps, substeps, loading=R.step_history)
    eng.set_model(m, substeps)
    dc = C.padded(R.LANES)
    V = np.asarray(eng.law_observe(law, "velocity", dc)[1])
    acc = np.asarray(eng.law_observe(law, "acc", dc)[1])
    inv_dt = 1.0 / ((m.t_final - m.t_start) / nsteps)  # the host's K.inv_dt = 1.0 / c->delta_t
    assert (V[0] == m.V_ref).all() and (acc[0] == 0.0).all() and np.isfinite(V).all()
    assert np.array_equal(_bits((V[1:] - V[:-1]) * inv_dt), _bits(acc[1:]))
    assert np.array_equal(_bits(eng.law_observe(law, "V", dc)[1]), _bits(V))


# ---- 3. each observable against long double --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("history", ["step", "hold"])
@pytest.mark.parametrize("law", R.LAWS)
def test_observables_against_long_double(pkg, gpu_engine, history, law):
    """Per lane set and observable the GPU's largest error against the long-double specification, relative to the lane's
    EXCURSION max|s - s_0|, is at most 4 x the yardstick — the larger of the two CPU float64 arrangements' largest error on the
    same set; the factor is test_both_laws_against_long_double's — and in any case below law_cases.CAP.  The device differs
    from the second arrangement by FMA contraction and its own log, exp and reciprocal only.  Measured on an MI355X when this
    was written (GPU / yardstick, the largest per-lane ratio against the specification in brackets): see DESIGN.md 4o."""
    s = OC.precision_set(history, law)
    eng = gpu_engine
    eng.set_model(_model(pkg, loading=R.HISTORIES[history]), 1)
    assert np.array_equal(eng.loading(), s["vl"])
    n, worst = s["dc"].size, []
    for obs in OC.GATED:
        got = np.asarray(eng.law_observe(law, obs, C.padded(s["dc"]))[1])
        assert np.isfinite(got).all()
        err = O.range_error(got[:, :n], s["ext"][obs])
        print(f"{history} {law} {obs}: GPU {err.max():.2e}, yardstick {s['yardstick'][obs]:.2e} (specification {s['err_spec'][obs].max():.2e}, device "
              f"arrangement {s['err_lane'][obs].max():.2e}), ratio {err.max() / s['yardstick'][obs]:.2f}; per lane against the specification "
              f"{np.array2string(err / s['err_spec'][obs], precision=2)}")
        worst.append((obs, float(err.max()), s["yardstick"][obs]))
    for obs, err, yard in worst:
        assert err < C.CAP, obs
        assert err <= 4.0 * yard, obs


# ---- 4. SSq is the series' sum ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("obs", O.OBSERVABLES)
def test_ssq_is_the_returned_series_sum(pkg, gpu_engine, obs, law):
    """The returned SSq against the float64 sum of the RETURNED series' squared residuals: both are sums of nout non-negative
    terms of the same residuals, one a running fma and one NumPy's, so they agree within 4 nout 2^-53 relative; and against the
    long-double specification's SSq within 1e-9."""
    s = OC.precision_set("step", law)
    eng = gpu_engine
    eng.set_model(_model(pkg, loading=R.step_history), 1)
    n = s["dc"].size
    data = _noisy(O.forward(s["m"], [R.BF_TRUTH], s["vl"], law, obs)[0][:, 0], 4)
    ssq, series = eng.law_observe(law, obs, C.padded(s["dc"]), data=data, want_ssq=True, want_series=True)
    ssq, series = np.asarray(ssq), np.asarray(series)
    own = ((series - data[:, None]) ** 2).sum(axis=0)
    ext = (((s["ext"][obs] - data.astype(R.LD)[:, None]) ** 2).sum(axis=0)).astype(np.float64)
    print(f"{obs} {law}: SSq against its own series {np.abs(ssq / own - 1).max():.2e} (bound {4 * eng.nout * 2.0 ** -53:.2e}), against long double "
          f"{np.abs(ssq[:n] / ext - 1).max():.2e}")
    assert np.isfinite(ssq).all() and (ssq > 0).all()
    assert (np.abs(ssq - own) <= 4 * eng.nout * 2.0 ** -53 * own).all()
    assert (np.abs(ssq[:n] - ext) <= 1e-9 * ext).all()
    # SSq alone is the same launch's
    assert np.array_equal(_bits(eng.law_observe(law, obs, C.padded(s["dc"]), data=data, want_ssq=True, want_series=False)[0]), _bits(ssq))


# ---- 5. edges -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("obs", O.OBSERVABLES)
def test_non_finite_lane_and_rows_past_n(pkg, gpu_engine, obs, law):
    eng = gpu_engine
    eng.set_model(_model(pkg, loading=R.step_history), 1)
    nout, n = eng.nout, 70  # two waves; the second holds six lanes of the batch
    data = _noisy(O.forward(C.spec(), [R.BF_TRUTH], R.table(C.spec(), "step"), law, obs)[0][:, 0], 4)
    dc = np.concatenate([[0.5], np.geomspace(5.0, 5000.0, n - 1)])
    ssq, series = eng.law_observe(law, obs, dc, data=data, want_ssq=True, want_series=True)
    assert not np.isfinite(ssq[0]) and np.isfinite(ssq[1:]).all() and np.isfinite(series[:, 1:]).all()
    # its wave neighbours keep the bits they have beside a harmless lane 0
    calm = dc.copy()
    calm[0] = 1000.0
    ssq2, series2 = eng.law_observe(law, obs, calm, data=data, want_ssq=True, want_series=True)
    assert np.array_equal(_bits(ssq[1:]), _bits(ssq2[1:])) and np.array_equal(_bits(series[:, 1:]), _bits(series2[:, 1:]))
    # a lane past n writes nothing: the series is time-major with stride n, so such a store would land in the rows past nout
    SENT = -7.25
    big, big_ssq = np.full((nout + 2, n), SENT), np.full(n + 64, SENT)
    code = pkg._abi.OBSERVABLES[obs]
    pkg._abi.check(eng.lib, eng.lib.rsf_law_observe(eng._ctx, pkg._abi.LAWS[law], code, n, dc.ctypes.data, None, None, data.ctypes.data, big_ssq.ctypes.data,
                                                    big.ctypes.data))
    assert (big[nout:] == SENT).all() and (big_ssq[n:] == SENT).all()
    assert np.array_equal(_bits(big[:nout]), _bits(series)) and np.array_equal(_bits(big_ssq[:n]), _bits(ssq))
    # n = 0: RSF_OK, nothing touched
    assert eng.lib.rsf_law_observe(eng._ctx, pkg._abi.LAWS[law], code, 0, dc.ctypes.data, None, None, data.ctypes.data, big_ssq.ctypes.data, big.ctypes.data) == 0
    assert np.array_equal(_bits(big[:nout]), _bits(series)) and (big[nout:] == SENT).all() and np.array_equal(_bits(big_ssq[:n]), _bits(ssq))


def test_refusals(pkg):
    with pkg.Engine(mem="host") as eng:
        lib, dc = eng.lib, np.array([100.0])
        out, ssq, data = np.full((50, 1), -7.25), np.full(1, -7.25), np.zeros(50)
        assert lib.rsf_law_observe(eng._ctx, 0, 1, 1, dc.ctypes.data, None, None, None, None, out.ctypes.data) == -3  # RSF_ERR_STATE: no model
        eng.set_model(_model(pkg, nsteps=50), 1)
        assert out.shape == (eng.nout, 1)
        assert lib.rsf_law_observe(eng._ctx, 0, 4, 1, dc.ctypes.data, None, None, None, None, out.ctypes.data) == -1  # RSF_ERR_INVALID
        assert b"observable" in lib.rsf_last_error() and b"4" in lib.rsf_last_error()
        assert lib.rsf_law_observe(eng._ctx, 0, -1, 1, dc.ctypes.data, None, None, None, None, out.ctypes.data) == -1
        assert lib.rsf_law_observe(eng._ctx, 7, 1, 1, dc.ctypes.data, None, None, None, None, out.ctypes.data) == -1
        assert b"law" in lib.rsf_last_error()
        assert lib.rsf_law_observe(eng._ctx, 1, 1, 1, dc.ctypes.data, None, None, None, ssq.ctypes.data, None) == -1  # ssq_out without data
        assert lib.rsf_law_observe(eng._ctx, 1, 1, -1, dc.ctypes.data, None, None, None, None, out.ctypes.data) == -1
        assert lib.rsf_law_observe(eng._ctx, 1, 1, 1, None, None, None, None, None, out.ctypes.data) == -1
        assert (out == -7.25).all() and (ssq == -7.25).all()
        eng.set_model(_model(pkg, nsteps=50, integrator="dop853"), 1)
        assert lib.rsf_law_observe(eng._ctx, 0, 1, 1, dc.ctypes.data, None, None, None, None, out.ctypes.data) == -5  # RSF_ERR_UNSUPPORTED
        assert (out == -7.25).all()
        eng.set_model(_model(pkg, nsteps=50, precision="float32"), 1)  # the float32 flag: the float64 solve
        assert lib.rsf_law_observe(eng._ctx, 1, 1, 1, dc.ctypes.data, None, None, data.ctypes.data, ssq.ctypes.data, out.ctypes.data) == 0
        eng.set_model(_model(pkg, nsteps=50), 1)
        want = eng.law_observe("slip", "mu", dc, data=data, want_ssq=True)
        assert np.array_equal(_bits(out), _bits(want[1])) and np.array_equal(_bits(ssq), _bits(want[0]))
        with pytest.raises(NotImplementedError, match="observable='mu' with precision='float32'"):
            eng.set_model(_model(pkg, observable="mu", precision="float32"), 1)


# ---- 6. end to end on friction data ---------------------------------------------------------------------------------------------------------
def _sampler(pkg, truth, **attrs):
    p = OC.friction_problem(truth)
    model = _model(pkg, loading=p["vl"], observable="mu", **attrs)
    return p, model, pkg.MCMC(model, p["data"], R.BF_TRUTH, ["Uniform", *R.BF_BOX], R.BF_TRUTH, nsamples=10, verbose=False)


@pytest.mark.parametrize("truth, sign", [("slip", +1), ("aging", -1)])
def test_compare_laws_on_friction_data(pkg, truth, sign):
    """Each law's log evidence within 1e-6 of the specification's quadrature on the result's own nodes
    (test_compare_laws_names_the_true_law's cap and method); the log Bayes factor has the truth's sign and lies beyond 100; the
    posterior SD of Dc under the true law is below half of what the same problem gives on acceleration data."""
    p, model, mc = _sampler(pkg, truth)
    out = mc.compare_laws()
    try:
        assert model.state_law == "aging" and model.observable == "mu" and sorted(out) == ["aging", "log_bayes_factor", "slip"]
        for law in R.LAWS:
            g = out[law]
            ssq = O.forward(p["m"], g.x[0], p["vl"], law, "mu", data=p["data"])[1]
            want, _ = R.log_evidence_1d(g.x[0], g.w[0], ssq, g.shape, *R.BF_BOX)
            print(f"truth {truth}, {law}: log evidence {g.log_evidence:.9f}, specification on its nodes {want:.9f} ({g.log_evidence - want:+.2e}); "
                  f"on 4001 trapezoid nodes {p['log_evidence'][law]:.6f}; mean {g.mean[0]:.4f}, SD {np.sqrt(g.cov[0, 0]):.4f}, outside {g.outside:.1e}")
            assert abs(g.log_evidence - want) < 1e-6
        print(f"truth {truth}: log Bayes factor {out['log_bayes_factor']:+.4f} (specification {p['log_bayes_factor']:+.4f})")
        assert out["log_bayes_factor"] == out["slip"].log_evidence - out["aging"].log_evidence
        assert sign * out["log_bayes_factor"] > 100.0 and np.sign(out["log_bayes_factor"]) == np.sign(p["log_bayes_factor"])
        sd = float(np.sqrt(out[truth].cov[0, 0]))
    finally:
        for law in R.LAWS:
            out[law].engine.close()
    # the same problem on acceleration data (law_cases.bayes_factor_problem), by the same quadrature
    pa = C.bayes_factor_problem(truth)
    acc = pkg.MCMC(_model(pkg, loading=pa["vl"], state_law=truth), pa["data"], R.BF_TRUTH, ["Uniform", *R.BF_BOX], R.BF_TRUTH, nsamples=10, verbose=False).quadrature()
    acc.engine.close()
    sd_acc = float(np.sqrt(acc.cov[0, 0]))
    print(f"truth {truth}: SD of Dc {sd:.4f} on friction data (specification {p['sd'][truth]:.4f}), {sd_acc:.4f} on acceleration data (specification {OC.acc_sd(truth):.4f})")
    assert sd < 0.5 * sd_acc


@pytest.mark.parametrize("truth", R.LAWS)
def test_sample_dr_on_friction_data(pkg, truth):
    """test_sample_dr_under_the_slip_law's construction on friction data under the true law — under the ageing law too, which
    takes the split path for the observable's sake: 256 chains x 200 iterations started from the quadrature's own draws, the
    pooled mean within 4.5 standard errors of the quadrature's mean."""
    p, model, mc = _sampler(pkg, truth, state_law=truth)
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
    print(f"truth {truth}: pooled mean {means.mean():.4f}, quadrature {grid.mean[0]:.4f} (SD {sd:.4f}), SE {se:.2e}, z {z:+.2f}; accept rates "
          f"{pool.stats['accept_rate1']:.2f} {pool.stats['accept_rate2']:.2f}")
    assert 0.05 < pool.accept_rate < 0.95
    assert abs(z) < 4.5
    # the chains' l is the friction's: -N/2 log SSq of law_observe at the final states, not the acceleration's
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        ssq = eng.law_ssq_fn(truth, p["data"], observable="mu")(x[-1].reshape(-1, 1))
        other = eng.law_ssq_fn(truth, p["data"])(x[-1].reshape(-1, 1))
    want = -0.5 * len(p["data"]) * np.log(ssq)
    assert np.allclose(pool.stats["l"][-1], want, rtol=1e-12, atol=0.0)
    assert np.abs(-0.5 * len(p["data"]) * np.log(other) - want).min() > 1e-3


def test_sample_smc_and_the_model_on_friction_data(pkg):
    p, model, mc = _sampler(pkg, "aging")
    pool = mc.sample_smc(512, seed=2)
    q = np.asarray(pool.samples).transpose(1, 0, 2).reshape(-1, 1)
    assert ((q > R.BF_BOX[0]) & (q < R.BF_BOX[1])).all() and pool.stats["n_solves"] > 512
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        ssq = eng.law_ssq_fn("aging", p["data"], observable="friction")(q)
    assert np.allclose(pool.stats["l"], -0.5 * len(p["data"]) * np.log(ssq), rtol=1e-12, atol=0.0)
    assert abs(q.mean() - p["mean"]["aging"]) < 10.0 * p["sd"]["aging"]
    got = mc.SSqcalc(np.array([[R.BF_TRUTH]]))[0, 0]
    want = float(O.forward(p["m"], [R.BF_TRUTH], p["vl"], "aging", "mu", data=p["data"], dtype=R.LD)[1][0])
    assert abs(got - want) < C.CAP * want
    # what integrates with the tier kernels refuses, and names the observable
    for call in (lambda: mc.sample_smc(512, replicates=2), lambda: mc.sample_batched(64, n_iters=4, mem="host"), lambda: pool.predictive(model, p["data"]),
                 lambda: pool.loo(model, p["data"]), lambda: pool.evidence(model, p["data"], *R.BF_BOX)):
        with pytest.raises(NotImplementedError, match="observable(=| is )'mu'"):
            call()
    # the front end: evaluate, evaluate_batch and trajectory are the specification's series, within CAP of the excursion
    for law in R.LAWS:
        model.state_law = law
        model.Dc = R.BF_TRUTH
        ext = O.trajectory(p["m"], [R.BF_TRUTH, 50.0], p["vl"], law, dtype=R.LD)
        np.random.seed(1)
        state = np.random.get_state()[1].copy()
        t, mu, noisy = model.evaluate()
        assert np.array_equal(np.random.get_state()[1], state) and np.array_equal(mu, noisy)
        batch = model.evaluate_batch([R.BF_TRUTH, 50.0])
        assert t.shape == mu.shape == (R.nout(p["m"]),) and batch.shape == (2, t.size)
        assert O.range_error(mu[:, None], ext["mu"][:, :1]).max() < C.CAP and O.range_error(batch.T, ext["mu"]).max() < C.CAP
        one, two = model.trajectory(), model.trajectory([R.BF_TRUTH, 50.0])
        assert sorted(one) == sorted(two) == sorted(O.OBSERVABLES)
        for k in O.OBSERVABLES:
            assert one[k].shape == t.shape and two[k].shape == (2, t.size) and np.array_equal(_bits(one[k]), _bits(two[k][0]))
            assert O.range_error(two[k].T, ext[k]).max() < C.CAP, (law, k)
        assert np.array_equal(_bits(one["mu"]), _bits(mu))
