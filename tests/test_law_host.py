"""
Host logic of the loading history and the state law (include/rsf_law.h; Engine.set_loading / loading / law_forward,
RateStateModel.loading / state_law, MCMC under the slip law): the prototype table against the header and the argument checks
that run before any library call, on the checker engine — whose library exports nothing of rsf_law.h.  No GPU.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import law_reference as R


def _model(pkg, **attrs):
    m = pkg.RateStateModel(number_time_steps=50)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_header_and_prototype_table_declare_the_same_symbols(pkg):
    abi = pkg._abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "rsf_law.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsf_\w+)\s*\(([^;]*)\)\s*;", code)}
    assert sorted(decl) == sorted(abi.LAW_PROTOTYPES) == ["rsf_get_loading", "rsf_law_forward", "rsf_loading_size", "rsf_set_loading"]
    for name, args in decl.items():
        assert len(args.split(",")) == len(abi.LAW_PROTOTYPES[name][1]), name
    assert all(rt is ctypes.c_int for rt, _ in abi.LAW_PROTOTYPES.values())
    for macro, value in (("RSF_LAW_AGEING", abi.LAW_AGEING), ("RSF_LAW_SLIP", abi.LAW_SLIP)):
        assert int(re.search(rf"#define {macro} (\d+)", code).group(1)) == value
    assert abi.LAWS == {"aging": 0, "ageing": 0, "slip": 1}
    # none of it is part of rsf_abi.h, which the checker library implements in full
    assert not set(abi.LAW_PROTOTYPES) & set(abi.PROTOTYPES)
    abi_header = open(os.path.join(root, "include", "rsf_abi.h")).read()
    assert "rsf_set_loading" not in abi_header and "rsf_law_forward" not in abi_header


def test_the_model_struct_does_not_change(pkg):
    """the law is a call argument and the loading a table: rsf_model keeps its size and its flags"""
    eng = pkg.engine
    plain, opts = _model(pkg), _model(pkg, state_law="slip", loading=lambda t: 1.0 + 0.0 * t)
    a, b = eng._model_struct(plain, 1), eng._model_struct(opts, 1)
    assert bytes(a) == bytes(b) and ctypes.sizeof(pkg._abi.Model) == 80


def test_loading_times_are_the_specifications(pkg, cpu_engine):
    for n, S in ((50, 1), (37, 3)):
        m = pkg.RateStateModel(number_time_steps=n)
        cpu_engine.set_model(m, S)
        spec = R.Spec(n, 0.0, 50.0, S)
        assert np.array_equal(cpu_engine.loading_times(), R.stage_times(spec))
        assert cpu_engine.loading_times().size == R.table_size(spec) == 2 * S * (cpu_engine.nout - 1) + 1


def test_argument_errors_before_any_library_call(pkg, cpu_engine):
    eng = cpu_engine
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.set_loading(np.ones(3))
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.law_forward("slip", [10.0])
    eng.set_model(_model(pkg), 1)
    t = eng.loading_times()
    with pytest.raises(ValueError, match="one value per RK4 stage time"):
        eng.set_loading(np.ones(t.size - 1))
    with pytest.raises(ValueError, match="one value per RK4 stage time"):
        eng.set_loading(lambda t: 1.0)  # a callable that is not vectorised over the stage times
    bad = np.ones(t.size)
    bad[7] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        eng.set_loading(bad)
    with pytest.raises(ValueError, match="not finite"):
        eng.set_loading(lambda t: np.where(t > 1.0, np.nan, 1.0))
    with pytest.raises(ValueError, match="'aging'"):
        eng.law_forward("dieterich", [10.0])
    with pytest.raises(ValueError, match="want_ssq needs data"):
        eng.law_forward("slip", [10.0], want_ssq=True)
    with pytest.raises(ValueError, match="the model produces"):
        eng.law_forward("slip", [10.0], data=np.zeros(7), want_ssq=True)


def test_checker_library_names_the_missing_symbol(pkg, cpu_engine):
    eng = cpu_engine
    eng.set_model(_model(pkg), 1)
    for name, call in (("rsf_set_loading", lambda: eng.set_loading(np.ones(eng.loading_times().size))),
                       ("rsf_set_loading", lambda: eng.set_loading(None)),
                       ("rsf_loading_size", eng.loading),
                       ("rsf_law_forward", lambda: eng.law_forward("ageing", [10.0]))):
        with pytest.raises(pkg.RsfError, match=f"{name} is exported by librsf_hip.so only"):
            call()
    # a model that carries a loading history reaches rsf_set_loading through set_model
    with pytest.raises(pkg.RsfError, match="rsf_set_loading is exported by librsf_hip.so only"):
        eng.set_model(_model(pkg, loading=R.step_history), 1)
    # ... and a set_model whose loading failed leaves no model behind, rather than this one under the built-in history
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.forward([10.0])
    with pytest.raises(ValueError, match="one value per RK4 stage time"):
        eng.set_model(_model(pkg, loading=np.ones(5)), 1)
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.forward([10.0])


@pytest.mark.parametrize("option", [{"state_law": "slip"}, {"loading": R.step_history}])
@pytest.mark.parametrize("solver", [{"integrator": "dop853"}, {"precision": "float32"}])
def test_refused_combinations_name_themselves(pkg, cpu_engine, option, solver):
    m = _model(pkg, **option, **solver)
    what = "state_law='slip'" if "state_law" in option else "a custom loading history"
    with pytest.raises(NotImplementedError, match=f"{what} with {next(iter(solver))}="):
        cpu_engine.set_model(m, 1)
    m.Dc = 100.0
    with pytest.raises(NotImplementedError, match=what):
        m.evaluate()
    with pytest.raises(NotImplementedError, match=what):
        m.evaluate_batch([100.0])


def test_unknown_state_law(pkg, cpu_engine):
    m = _model(pkg, state_law="ruina")
    with pytest.raises(ValueError, match="state_law is 'aging'"):
        cpu_engine.set_model(m, 1)
    assert pkg.engine.state_law_of(_model(pkg, state_law="ageing")) == "aging" == pkg.engine.state_law_of(_model(pkg))
    assert pkg.engine.state_law_of(_model(pkg, state_law="slip")) == "slip"


def test_model_key_follows_the_options(pkg):
    m = _model(pkg)
    k0 = m._model_key()
    m.state_law = "slip"
    k1 = m._model_key()
    v = np.ones(99)
    m.loading = v
    k2 = m._model_key()
    v[3] = 2.0  # the array's values, not its identity
    k3 = m._model_key()
    m.loading = R.step_history
    assert len({k0, k1, k2, k3, m._model_key()}) == 5


def test_ageing_kernels_refuse_a_slip_model(pkg, cpu_engine):
    """every Engine call that integrates on the device checks the law the model was set with: none runs the ageing law silently"""
    eng = cpu_engine
    eng.set_model(_model(pkg, state_law="slip"), 1)
    data = np.zeros(eng.nout)
    for call in (lambda: eng.forward([10.0]), lambda: eng.mcmc_init([[10.0]], data, [0.0], [100.0]), lambda: eng.smc(data, 1.0, 100.0, 64),
                 lambda: eng.grid_posterior(data, 1.0, 100.0), lambda: eng.dr([[10.0]], data, 1.0, 100.0, [[1.0]], 4),
                 lambda: eng.fit([[10.0]], data, 1.0, 100.0), lambda: eng.predictive([[10.0]], [1.0], data)):
        with pytest.raises(NotImplementedError, match="state_law is 'slip'"):
            call()
    eng.set_model(_model(pkg), 1)  # and the default model runs as before
    assert np.isfinite(eng.forward([10.0])[1]).all()


def test_mcmc_methods_name_the_law(pkg):
    m = _model(pkg, state_law="slip")
    mc = pkg.MCMC(m, np.zeros(50), 20.0, ["Uniform", 5.0, 200.0], 20.0, nsamples=10, verbose=False)
    for call in (mc.sample, lambda: mc.sample_batched(4), lambda: mc.sample_mala(4, 4), lambda: mc.sample_ensemble(8, 4), mc.fit,
                 mc.compute_initial_covariance, lambda: mc.sample_dr(4, 4), lambda: mc.sample_dr(4, 4, factor=[[1.0]], start="fit"),
                 lambda: mc.sample_dr(4, 4, factor=[[1.0]], adapt=True)):
        with pytest.raises(NotImplementedError, match="slip"):
            call()
    with pytest.raises(ValueError, match="once each"):
        mc.compare_laws(laws=("slip", "slip"))
    with pytest.raises(ValueError, match="state_law is"):
        mc.compare_laws(laws=("aging", "ruina"))
    assert m.state_law == "slip"
    m3 = pkg.MCMC(_model(pkg), np.zeros(50), 20.0, [["Uniform", 5.0, 200.0], ["Uniform", 0.005, 0.02], ["Uniform", 0.005, 0.02]],
                  [20.0, 0.011, 0.014], nsamples=10, verbose=False)
    with pytest.raises(NotImplementedError, match="one-parameter"):
        m3.compare_laws()
