"""
Host logic of the observable option (include/rsf_observe.h; Engine.law_observe / law_ssq_fn(observable=), RateStateModel.observable /
noise_sd / trajectory, MCMC on a non-default observable): the prototype table against the header, and the argument checks and
refusals that run before any library call, on the checker engine — whose library exports nothing of rsf_observe.h.  No GPU.
"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(pkg, **attrs):
    m = pkg.RateStateModel(number_time_steps=50)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _declared(code):
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsf_\w+)\s*\(([^;]*)\)\s*;", code)}


def test_header_and_prototype_table_declare_the_same_symbols(pkg):
    abi = pkg._abi
    code = _header("rsf_observe.h")
    decl = _declared(code)
    assert sorted(decl) == sorted(abi.OBSERVE_PROTOTYPES) == ["rsf_law_observe"]
    for name, args in decl.items():
        assert len(args.split(",")) == len(abi.OBSERVE_PROTOTYPES[name][1]) == 10, name
    assert all(rt is ctypes.c_int for rt, _ in abi.OBSERVE_PROTOTYPES.values())
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RSF_OBS_\w+) (\d+)", code)}
    assert macros == {"RSF_OBS_ACC": abi.OBS_ACC, "RSF_OBS_MU": abi.OBS_MU, "RSF_OBS_THETA": abi.OBS_THETA, "RSF_OBS_VELOCITY": abi.OBS_VELOCITY}
    assert macros == {"RSF_OBS_ACC": 0, "RSF_OBS_MU": 1, "RSF_OBS_THETA": 2, "RSF_OBS_VELOCITY": 3}
    assert abi.OBSERVABLES == {"acc": 0, "mu": 1, "friction": 1, "theta": 2, "state": 2, "velocity": 3, "V": 3}
    # a table of its own: nothing of it in rsf_abi.h, which the checker library implements in full, or in rsf_law.h's table
    assert not set(abi.OBSERVE_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.LAW_PROTOTYPES))


def test_the_other_headers_are_untouched(pkg):
    law = open(os.path.join(ROOT, "include", "rsf_law.h")).read()
    assert sorted(_declared(_header("rsf_law.h"))) == ["rsf_get_loading", "rsf_law_forward", "rsf_loading_size", "rsf_set_loading"]
    assert sorted(pkg._abi.LAW_PROTOTYPES) == sorted(_declared(_header("rsf_law.h")))
    for text in (law, open(os.path.join(ROOT, "include", "rsf_abi.h")).read()):
        assert "rsf_law_observe" not in text and "rsf_observe" not in text and "RSF_OBS_" not in text


def test_the_model_struct_does_not_change(pkg):
    """the observable is a call argument: rsf_model keeps its 80 bytes and its flags"""
    eng = pkg.engine
    plain, opts = _model(pkg), _model(pkg, observable="mu", noise_sd=0.25)
    assert bytes(eng._model_struct(plain, 1)) == bytes(eng._model_struct(opts, 1)) and ctypes.sizeof(pkg._abi.Model) == 80


def test_model_key_follows_the_observable(pkg):
    m = _model(pkg)
    keys = [m._model_key()]
    for obs in ("mu", "theta", "velocity"):
        m.observable = obs
        keys.append(m._model_key())
    m.state_law = "slip"
    keys.append(m._model_key())
    assert len(set(keys)) == 5
    assert _model(pkg).observable == "acc" and _model(pkg).noise_sd == 0.0


def test_unknown_observable(pkg, cpu_engine):
    with pytest.raises(ValueError, match="observable is 'acc'"):
        cpu_engine.set_model(_model(pkg, observable="acceleration"), 1)
    m = _model(pkg, observable="slip rate")
    m.Dc = 100.0
    for call in (m.evaluate, lambda: m.evaluate_batch([100.0]), m.trajectory):
        with pytest.raises(ValueError, match="observable is 'acc'"):
            call()
    name = pkg.engine.observable_of
    assert name(_model(pkg)) == "acc" and name(_model(pkg, observable="friction")) == "mu" == name(_model(pkg, observable="mu"))
    assert name(_model(pkg, observable="state")) == "theta" and name(_model(pkg, observable="V")) == "velocity"
    cpu_engine.set_model(_model(pkg), 1)
    with pytest.raises(ValueError, match="observable is 'acc'"):
        cpu_engine.law_ssq_fn("aging", np.zeros(cpu_engine.nout), observable="stress")


def test_argument_errors_before_any_library_call(pkg, cpu_engine):
    eng = cpu_engine
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.law_observe("slip", "mu", [10.0])
    eng.set_model(_model(pkg), 1)
    with pytest.raises(ValueError, match="'aging'"):
        eng.law_observe("dieterich", "mu", [10.0])
    with pytest.raises(ValueError, match="observable is 'acc'"):
        eng.law_observe("slip", "shear", [10.0])
    with pytest.raises(ValueError, match="want_ssq needs data"):
        eng.law_observe("slip", "mu", [10.0], want_ssq=True)
    with pytest.raises(ValueError, match="the model produces"):
        eng.law_observe("slip", "mu", [10.0], data=np.zeros(7), want_ssq=True)


def test_checker_library_names_the_missing_symbol(pkg, cpu_engine):
    eng = cpu_engine
    eng.set_model(_model(pkg, observable="mu"), 1)
    assert eng.observable == "mu"
    data = np.zeros(eng.nout)
    m = _model(pkg, observable="friction")
    m.Dc = 100.0
    m._engine, m._engine_key = eng, None  # the model's own engine would be the product library's
    for call in (lambda: eng.law_observe("ageing", "acc", [10.0]), lambda: eng.law_observe(1, 3, [10.0]),
                 lambda: eng.law_ssq_fn("aging", data, observable="mu")([[10.0]]), m.evaluate, lambda: m.evaluate_batch([10.0, 20.0]), m.trajectory):
        with pytest.raises(pkg.RsfError, match=r"rsf_law_observe is exported by librsf_hip.so only.*rsf_observe\.h"):
            call()
    m._engine = None
    # with "acc" law_ssq_fn is what it was: it reaches rsf_law_forward
    with pytest.raises(pkg.RsfError, match="rsf_law_forward is exported by librsf_hip.so only"):
        eng.law_ssq_fn("aging", data)([[10.0]])
    with pytest.raises(pkg.RsfError, match="rsf_law_forward is exported by librsf_hip.so only"):
        eng.law_ssq_fn("aging", data, observable="acc")([[10.0]])


@pytest.mark.parametrize("observable", ["mu", "theta", "V"])
@pytest.mark.parametrize("solver", [{"integrator": "dop853"}, {"precision": "float32"}])
def test_refused_combinations_name_themselves(pkg, cpu_engine, observable, solver):
    m = _model(pkg, observable=observable, **solver)
    what = f"observable={pkg.engine.observable_name(observable)!r} with {next(iter(solver))}="
    with pytest.raises(NotImplementedError, match=what):
        cpu_engine.set_model(m, 1)
    m.Dc = 100.0
    for call in (m.evaluate, lambda: m.evaluate_batch([100.0]), m.trajectory):
        with pytest.raises(NotImplementedError, match=what):
            call()


def test_acceleration_kernels_refuse_another_observable(pkg, cpu_engine):
    """every Engine call that integrates with the tier kernels checks the observable the model was set with: none fits the
    acceleration silently"""
    eng = cpu_engine
    eng.set_model(_model(pkg, observable="friction"), 1)
    data = np.zeros(eng.nout)
    for call in (lambda: eng.forward([10.0]), lambda: eng.mcmc_init([[10.0]], data, [0.0], [100.0]), lambda: eng.smc(data, 1.0, 100.0, 64),
                 lambda: eng.grid_posterior(data, 1.0, 100.0), lambda: eng.dr([[10.0]], data, 1.0, 100.0, [[1.0]], 4),
                 lambda: eng.fit([[10.0]], data, 1.0, 100.0), lambda: eng.predictive([[10.0]], [1.0], data)):
        with pytest.raises(NotImplementedError, match="observable is 'mu'"):
            call()
    # under the slip law the slip law's message stays
    eng.set_model(_model(pkg, observable="mu", state_law="slip"), 1)
    with pytest.raises(NotImplementedError, match="state_law is 'slip'"):
        eng.forward([10.0])
    eng.set_model(_model(pkg), 1)  # and the default model runs as before
    assert eng.observable == "acc" and np.isfinite(eng.forward([10.0])[1]).all()


def test_mcmc_methods_name_the_observable(pkg):
    m = _model(pkg, observable="mu")
    mc = pkg.MCMC(m, np.full(50, 0.6), 20.0, ["Uniform", 5.0, 200.0], 20.0, nsamples=10, verbose=False)
    for call in (mc.sample, lambda: mc.sample_batched(4), lambda: mc.sample_mala(4, 4), lambda: mc.sample_ensemble(8, 4), mc.fit,
                 mc.compute_initial_covariance, lambda: mc.sample_dr(4, 4), lambda: mc.sample_dr(4, 4, factor=[[1.0]], start="fit"),
                 lambda: mc.sample_dr(4, 4, factor=[[1.0]], adapt=True)):
        with pytest.raises(NotImplementedError, match="observable(=| is )'mu'"):
            call()
    m.state_law = "slip"  # the slip law's wording stays
    for call in (mc.sample, lambda: mc.sample_dr(4, 4), lambda: mc.sample_dr(4, 4, factor=[[1.0]], adapt=True)):
        with pytest.raises(NotImplementedError, match="slip"):
            call()


def test_evaluate_noise_rule(pkg, monkeypatch):
    """another observable than "acc": series + noise_sd N(0, 1) from the global RNG, and no variate at noise_sd = 0; "acc": the
    reference's |acc| N(0, 1), one draw of nout variates, as before"""
    series = np.linspace(0.6, 0.61, 50)
    m = _model(pkg, observable="mu")
    m.Dc = 100.0
    monkeypatch.setattr(m, "_forward", lambda dc, a=None, b=None: (None, np.repeat(series[:, None], len(dc), axis=1)))
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    t, clean, noisy = m.evaluate()
    assert np.array_equal(clean, series) and np.array_equal(noisy, series) and noisy is not clean and t.shape == (50,)
    assert np.array_equal(np.random.get_state()[1], state)  # nothing was drawn
    m.noise_sd = 1e-3
    _, clean, noisy = m.evaluate()
    np.random.seed(5)
    assert np.array_equal(noisy, series + 1e-3 * np.random.randn(50))
    m.observable = "acc"
    np.random.seed(5)
    _, clean, noisy = m.evaluate()
    np.random.seed(5)
    assert np.array_equal(noisy, series + 1.0 * np.abs(series) * np.random.randn(50))
