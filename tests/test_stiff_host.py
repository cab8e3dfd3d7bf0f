"""
Host logic of the stiffness independent of Dc (include/rsf_stiff.h; RateStateModel.stiffness, Engine.stiff_observe / stiff_dr_run /
stiff_dr_ssq and the routing of the law_* calls, MCMC): the prototype table against the header, the attribute and the model key,
check_law_options' refusals, the by-name refusal of every call whose kernel integrates k' = 0.1 / Dc, and the refusal on a
library without the symbols — on the checker engine, whose library exports nothing of rsf_stiff.h.  No GPU.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = r"rsf_stiff_(observe|dr_run|dr_ssq) is exported by librsf_hip.so only.*rsf_stiff\.h"
COUPLED = r"stiffness=0\.002.*integrates k' = 0\.1 / Dc"
K = 2e-3


def _model(pkg, **attrs):
    m = pkg.RateStateModel(number_time_steps=50)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _declared(name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsf_\w+)\s*\(([^;]*)\)\s*;", code)}


def _state(n, d=1):
    q = np.ascontiguousarray(np.tile([20.0, 0.011, 0.014][:d], (n, 1)))
    return q, np.zeros(n), [np.zeros(n, dtype=np.int32) for _ in range(5)]


def test_header_and_prototype_table_declare_the_same_symbols(pkg):
    abi = pkg._abi
    decl = _declared("rsf_stiff.h")
    assert sorted(decl) == sorted(abi.STIFF_PROTOTYPES) == ["rsf_stiff_dr_run", "rsf_stiff_dr_ssq", "rsf_stiff_observe"]
    names = lambda text: [a.split()[-1].lstrip("*") for a in text.split(",")]
    for name, header, base, table in (("rsf_stiff_observe", "rsf_observe.h", "rsf_law_observe", abi.OBSERVE_PROTOTYPES),
                                      ("rsf_stiff_dr_run", "rsf_law_dr.h", "rsf_law_dr_run", abi.LAW_DR_PROTOTYPES),
                                      ("rsf_stiff_dr_ssq", "rsf_law_dr.h", "rsf_law_dr_ssq", abi.LAW_DR_PROTOTYPES)):
        rt, args = abi.STIFF_PROTOTYPES[name]
        want = table[base][1]
        # the coupled call's arguments, in its order, with the stiffness behind (ctx, law, observable)
        assert rt is ctypes.c_int and args == want[:3] + [ctypes.c_double] + want[3:]
        other = names(_declared(header)[base])
        assert names(decl[name]) == other[:3] + ["stiffness"] + other[3:]
    assert not set(abi.STIFF_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.LAW_DR_PROTOTYPES) | set(abi.OBSERVE_PROTOTYPES))
    assert ctypes.sizeof(abi.Model) == 80  # the stiffness is an argument of the calls, not a field of rsf_model


def test_the_attribute_and_the_model_key(pkg):
    m = _model(pkg)
    assert m.stiffness is None
    key = m._model_key()
    m.stiffness = K
    assert m._model_key() != key and K in m._model_key()
    m.stiffness = None
    assert m._model_key() == key
    from bayesian_markov_chain_monte_carlo_amd.engine import stiffness_of

    assert stiffness_of(m) is None and stiffness_of(_model(pkg, stiffness=K)) == K and stiffness_of(object()) is None
    for bad in (0.0, -1e-3, float("inf"), float("nan"), "2e-3", True, [2e-3]):
        with pytest.raises(ValueError, match="stiffness is None"):
            stiffness_of(_model(pkg, stiffness=bad))


def test_check_law_options_refuses_the_other_solves(pkg):
    from bayesian_markov_chain_monte_carlo_amd.engine import check_law_options

    assert check_law_options(_model(pkg, stiffness=K)) == "aging"
    assert check_law_options(_model(pkg, stiffness=K, state_law="slip", observable="mu")) == "slip"
    with pytest.raises(NotImplementedError, match=r"stiffness=0\.002 with integrator='dop853'"):
        check_law_options(_model(pkg, stiffness=K, integrator="dop853"))
    with pytest.raises(NotImplementedError, match=r"stiffness=0\.002 with precision='float32'"):
        check_law_options(_model(pkg, stiffness=K, precision="float32"))


def test_set_model_records_the_stiffness(pkg, cpu_engine):
    eng = cpu_engine
    assert eng.stiffness is None
    eng.set_model(_model(pkg, stiffness=K), 1)
    assert eng.stiffness == K
    eng.set_model(_model(pkg), 1)
    assert eng.stiffness is None
    with pytest.raises(NotImplementedError, match="dop853"):
        eng.set_model(_model(pkg, stiffness=K, integrator="dop853"), 1)
    with pytest.raises(ValueError, match="stiffness is None"):
        eng.set_model(_model(pkg, stiffness=-1.0), 1)


def test_calls_that_integrate_the_coupled_spring_refuse_by_name(pkg, cpu_engine):
    """Nothing runs the reference's spring silently on a model with a stiffness: every Engine call whose kernel integrates
    k' = 0.1 / Dc raises before any library call."""
    eng = cpu_engine
    eng.set_model(_model(pkg, stiffness=K), 1)
    data = np.full(eng.nout, 0.6)
    q, l, cnt = _state(64)
    q3 = _state(64, 3)[0]
    ones, ints = np.ones(64), np.zeros(64, dtype=np.int32)
    grad, jtj = np.zeros((64, 1)), np.ones((64, 1, 1))
    calls = {
        # the tier kernels' methods
        "forward": lambda: eng.forward([20.0]),
        "mcmc_init": lambda: eng.mcmc_init(q, data, [5.0], [200.0]),
        "evidence_logtarget": lambda: eng.evidence_logtarget(q, data, [5.0], [200.0], ones),
        "evidence": lambda: eng.evidence(np.zeros((4, 64, 1)), data, [5.0], [200.0]),
        "smc_move": lambda: eng.smc_move(q, l, data, [5.0], [200.0], [[1.0]], 0.5),
        "smc": lambda: eng.smc(data, [5.0], [200.0], 64),
        "smc_batch_logtarget": lambda: eng.smc_batch_logtarget(q, data, [0], [5.0], [200.0]),
        "smc_batch_move": lambda: eng.smc_batch_move(q, l, data, [0], [5.0], [200.0], [[1.0]], [0.5], [1]),
        "smc_batch": lambda: eng.smc_batch(data, [5.0], [200.0], 64),
        "fit_normal": lambda: eng.fit_normal(q, data),
        "fit_run": lambda: eng.fit_run(q, data, [5.0], [200.0], ones, grad, jtj, ones, ints, ints, 1),
        "fit": lambda: eng.fit(q, data, [5.0], [200.0]),
        "mala_run": lambda: eng.mala_run(q, ones, grad, jtj, data, [5.0], [200.0], 1, ints, ints, ints),
        "mala": lambda: eng.mala(q, data, [5.0], [200.0], 4),
        "ensemble_run": lambda: eng.ensemble_run(q, l, data, [5.0], [200.0], 1, ints, ints, ints),
        "ensemble_ssq": lambda: eng.ensemble_ssq(q, np.ones(64, np.uint8), data, 0),
        "ensemble": lambda: eng.ensemble(q, data, [5.0], [200.0], 4),
        "dr_run": lambda: eng.dr_run(q, l, data, [5.0], [200.0], [[1.0]], 1, cnt),
        "dr_ssq": lambda: eng.dr_ssq(q, np.ones(64, np.uint8), data),
        "dr": lambda: eng.dr(q, data, [5.0], [200.0], [[1.0]], 4),
        "grid_logtarget": lambda: eng.grid_logtarget(np.linspace(5.0, 200.0, 9), data, [5.0], [200.0]),
        "grid_posterior": lambda: eng.grid_posterior(data, [5.0], [200.0]),
        "predictive_partials": lambda: eng.predictive_partials(q, ones, data, data, data),
        "predictive": lambda: eng.predictive(q, ones, data),
        # the state-law kernels without a stiffness
        "law_forward": lambda: eng.law_forward("slip", [20.0]),
        "law_fit_normal": lambda: eng.law_fit_normal("slip", "mu", q, data),
        "law_fit_run": lambda: eng.law_fit_run("slip", "mu", q, data, [5.0], [200.0], ones, grad, jtj, ones, ints, ints, 1),
        "law_fit": lambda: eng.law_fit("slip", "mu", q, data, [5.0], [200.0]),
        "law_logtarget": lambda: eng.law_logtarget("slip", "mu", data, [5.0], [200.0], theta=q),
        "law_grid_posterior": lambda: eng.law_grid_posterior("slip", "mu", data, [5.0], [200.0], [20.0], [[1.0]]),
        "law_evidence": lambda: eng.law_evidence("slip", "mu", np.zeros((4, 64, 1)), data, [5.0], [200.0]),
        "law_predictive_partials": lambda: eng.law_predictive_partials("slip", "mu", q, ones, data, data, data),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match=COUPLED):
            call()
    assert q3.shape == (64, 3)
    # without a stiffness the same engine runs them again: the first of them, on the checker
    eng.set_model(_model(pkg), 1)
    assert np.isfinite(np.asarray(eng.forward([20.0])[1])).all()


def test_mcmc_refusals_and_routes(pkg, cpu_engine, monkeypatch):
    eng = cpu_engine
    model = _model(pkg, stiffness=K, observable="mu")
    eng.set_model(model, 1)
    data = np.full(eng.nout, 0.6)
    mod = sys.modules[pkg.MCMC.__module__]
    monkeypatch.setattr(eng, "close", lambda: None)  # the methods make, enter and close an Engine of their own: here the checker's
    monkeypatch.setattr(mod, "Engine", lambda **kw: eng)
    mc = pkg.MCMC(model, data, 20.0, ["Uniform", 5.0, 200.0], 20.0, nsamples=10, verbose=False)
    assert mc._split() == "observable='mu'"
    plain = _model(pkg, stiffness=K)
    acc = pkg.MCMC(plain, data, 20.0, ["Uniform", 5.0, 200.0], 20.0, nsamples=10, verbose=False)
    assert acc._split() == "stiffness=0.002"
    # still refused, naming the stiffness
    for call in (lambda: mc.quadrature_law(), lambda: mc.bayes_factor_laws(), lambda: acc.fit(), lambda: acc.sample_batched(8, 4),
                 lambda: acc.sample_mala(8, 4), lambda: acc.sample_ensemble(8, 4), lambda: acc.sample_smc(64, replicates=2)):
        with pytest.raises(NotImplementedError, match=COUPLED):
            call()
    pool = pkg.MCMC.__globals__["PosteriorPool"] if hasattr(pkg.MCMC, "__globals__") else mod.PosteriorPool
    pool = pool(np.full((4, 8, 1), 20.0), np.ones((4, 8)), 0.5, {}, 0)
    with pytest.raises(NotImplementedError, match=COUPLED):
        pool.law_evidence(model, data, [5.0], [200.0], engine=eng)
    # the routes that run reach the library under the new names: the checker has none of them
    for call in (lambda: mc.SSqcalc(np.array([[20.0]])), lambda: acc.SSqcalc(np.array([[20.0]])), lambda: mc.sample_law(8, 4),
                 lambda: mc.sample_law(8, 4, factor=[[1.0]]), lambda: mc.sample_dr(8, 4, factor=[[1.0]]), lambda: acc.quadrature(),
                 lambda: mc.fit_law(n_starts=1), lambda: model.evaluate_batch([20.0]), lambda: model.trajectory(20.0)):
        model._engine, model._engine_key, plain._engine, plain._engine_key = eng, None, eng, None
        with pytest.raises(pkg.RsfError, match=MISSING) as ei:
            call()
        assert ei.value.code == -5
    model._engine = plain._engine = None
    # the predictive checks' split route asks for the series entry point first, which the checker lacks as well
    for call in (lambda: pool.law_predictive(model, data, engine=eng), lambda: pool.law_loo(model, data, engine=eng)):
        with pytest.raises(pkg.RsfError, match="rsf_predict_series_partials is exported by librsf_hip.so only"):
            call()


def test_checker_library_names_the_missing_symbol(pkg, cpu_engine):
    eng = cpu_engine
    eng.set_model(_model(pkg, observable="mu", state_law="slip"), 1)
    data = np.full(eng.nout, 0.6)
    q, l, cnt = _state(64)
    for call in (lambda: eng.stiff_observe("slip", "mu", K, [20.0]),
                 lambda: eng.law_observe("aging", "acc", [20.0], stiffness=K),
                 lambda: eng.stiff_dr_run("slip", "mu", K, q, l, data, 5.0, 200.0, [[1.0]], 1, cnt),
                 lambda: eng.law_dr_run(0, 3, q, l, data, 5.0, 200.0, [[1.0]], 1, cnt, trace=True, stiffness=K),
                 lambda: eng.stiff_dr_ssq("ageing", "friction", K, q, np.ones(64, np.uint8), data),
                 lambda: eng.law_dr_ssq("slip", "mu", q, np.ones(64, np.uint8), data, stiffness=K),
                 lambda: eng.law_ssq_fn("slip", data, "acc", stiffness=K)([[20.0]]),
                 lambda: eng.law_gn_factor("slip", "mu", [20.0], data, stiffness=K),
                 lambda: eng.law_dr("slip", "mu", q, data, 5.0, 200.0, [[1.0]], 4, stiffness=K)):
        with pytest.raises(pkg.RsfError, match=MISSING) as ei:
            call()
        assert ei.value.code == -5
    # the engine's model's stiffness is the default of every keyword
    eng.set_model(_model(pkg, stiffness=K), 1)
    for call in (lambda: eng.law_observe("aging", "acc", [20.0]), lambda: eng.law_dr_ssq("slip", "mu", q, np.ones(64, np.uint8), data),
                 lambda: eng.law_ssq_fn("aging", data)([[20.0]]), lambda: eng.law_dr("slip", "mu", q, data, 5.0, 200.0, [[1.0]], 4)):
        with pytest.raises(pkg.RsfError, match=MISSING):
            call()
