"""
Host logic of the exact posterior of a state-law model on a grid in the coordinates of a fit (include/rsf_law_grid.h;
Engine.law_logtarget / law_grid_moments / law_grid_posterior / law_evidence, MCMC.quadrature_law / bayes_factor_laws,
PosteriorPool.law_evidence): the prototype table against the header, the refusal on a library without the symbols, the argument
checks that run before any call of that family — on the checker engine, whose library exports nothing of rsf_law_grid.h, so that a
check which came too late would show as the missing symbol's error instead of its own — the refusals that stay, and the model's
state_law after an exception in bayes_factor_laws.  No GPU.
"""
import contextlib
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = r"rsf_law_(logtarget|grid_moments) is exported by librsf_hip.so only.*rsf_law_grid\.h"
LO3, HI3 = np.array([8.0, 0.009, 0.012]), np.array([60.0, 0.013, 0.016])
POINT = np.array([20.0, 0.011, 0.014])
FACTOR = np.diag([0.25, 1.1e-4, 9.4e-5])
PRIORS3 = [["Uniform", float(LO3[k]), float(HI3[k])] for k in range(3)]


def _model(pkg, **attrs):
    m = pkg.RateStateModel(number_time_steps=50)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _declared(name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsf_\w+)\s*\(([^;]*)\)\s*;", code)}


def test_header_and_prototype_table_declare_the_same_symbols(pkg):
    abi = pkg._abi
    decl = _declared("rsf_law_grid.h")
    assert sorted(decl) == sorted(abi.LAW_GRID_PROTOTYPES) == ["rsf_law_grid_moments", "rsf_law_logtarget"]
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for name, (rt, args) in abi.LAW_GRID_PROTOTYPES.items():
        texts = decl[name].split(",")
        assert rt is ctypes.c_int and len(texts) == len(args) and args[0] is ctypes.c_void_p
        for text, want in zip(texts[1:], args[1:]):
            if "*" not in text:
                assert ctype[text.split()[-2]] is want, (name, text)
            else:
                assert want in (abi._P, abi._DP, abi._I32P), (name, text)
                assert (want is abi._I32P) == ("int32_t" in text), (name, text)
    # law and observable in front of the arguments, as in rsf_law_observe
    assert [a.split()[-1].lstrip("*") for a in decl["rsf_law_logtarget"].split(",")][:3] == ["ctx", "law", "observable"]
    header = open(os.path.join(ROOT, "include", "rsf_law_grid.h")).read()
    assert abi.LAW_GRID_MAX_PARAMS == int(re.search(r"#define RSF_LAW_GRID_MAX_PARAMS (\d+)", header).group(1))
    assert len(abi.LAW_GRID_FIELDS) == int(re.search(r"#define RSF_LAW_GRID_FIELDS (\d+)", header).group(1))
    assert {"LawGridPosterior"} <= set(pkg.__all__)


def test_checker_library_names_the_missing_symbol(pkg, cpu_engine, monkeypatch):
    eng = cpu_engine
    eng.set_model(_model(pkg, observable="mu", state_law="slip"), 1)
    data = np.full(eng.nout, 0.6)
    z = [np.linspace(-1, 1, 5)] * 3
    w = [np.ones(5)] * 3
    for call in (lambda: eng.law_logtarget("slip", "mu", data, LO3, HI3, z=z, m=POINT, L=FACTOR),
                 lambda: eng.law_logtarget(0, 3, data, 8.0, 60.0, theta=[20.0, 30.0]),
                 lambda: eng.law_grid_moments(z, w, POINT, FACTOR, None, None, np.zeros(125), np.ones(125), 0.0, POINT),
                 lambda: eng.law_grid_posterior("slip", "mu", data, LO3, HI3, POINT, FACTOR, n=(5, 3, 3)),
                 lambda: eng.law_grid_posterior("aging", "acc", data, 8.0, 60.0, 20.0, [[0.25]], log_coords=("Dc",))):
        with pytest.raises(pkg.RsfError, match=MISSING) as ei:
            call()
        assert ei.value.code == -5


def test_argument_errors_before_any_library_call(pkg, cpu_engine):
    eng = cpu_engine
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.law_logtarget("slip", "mu", np.zeros(50), LO3, HI3, theta=POINT[None, :])
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.law_grid_posterior("slip", "mu", np.zeros(50), LO3, HI3, POINT, FACTOR)
    eng.set_model(_model(pkg), 1)
    data = np.zeros(eng.nout)
    z = [np.linspace(-1, 1, 5)] * 3
    target = lambda **kw: eng.law_logtarget(kw.pop("law", "slip"), kw.pop("observable", "mu"), kw.pop("data", data), kw.pop("lo", LO3), kw.pop("hi", HI3), **kw)
    with pytest.raises(ValueError, match="law is 'aging'"):
        target(law="ruina", theta=POINT[None, :])
    with pytest.raises(ValueError, match="observable is 'acc'"):
        target(observable="shear", theta=POINT[None, :])
    with pytest.raises(ValueError, match="data has shape"):
        target(data=np.zeros(7), theta=POINT[None, :])
    for kw in (dict(), dict(z=z, m=POINT, L=FACTOR, theta=POINT[None, :])):
        with pytest.raises(ValueError, match="either the nodes of the axes z or theta"):
            target(**kw)
    with pytest.raises(ValueError, match="a grid needs the map"):
        target(z=z)
    with pytest.raises(ValueError, match="logg goes with theta"):
        target(z=z, m=POINT, L=FACTOR, logg=np.zeros(125))
    with pytest.raises(ValueError, match="logg holds 3 values, theta 1 points"):
        target(theta=POINT[None, :], logg=np.zeros(3))
    with pytest.raises(ValueError, match="d = 1 .Dc. or 3"):
        target(theta=np.ones((4, 2)), lo=LO3[:2], hi=HI3[:2])
    upper = FACTOR.copy()
    upper[0, 1] = 1e-3
    for kw, msg in ((dict(L=upper), "lower-triangular"), (dict(m=POINT[:2]), "the map is m"), (dict(perm=[0, 0, 1]), "perm is a permutation"),
                    (dict(tr=[1, 0]), "tr holds 3 flags")):
        with pytest.raises(ValueError, match=msg):
            target(**{**dict(z=z, m=POINT, L=FACTOR), **kw})
    with pytest.raises(ValueError, match="one value per node"):
        eng.law_grid_moments(z, [np.ones(5)] * 3, POINT, FACTOR, None, None, np.zeros(7), np.zeros(7), 0.0, POINT)
    post = lambda **kw: eng.law_grid_posterior(kw.pop("law", "slip"), kw.pop("observable", "mu"), data, kw.pop("lo", LO3), kw.pop("hi", HI3),
                                               kw.pop("center", POINT), kw.pop("factor", FACTOR), **kw)
    for kw, msg in ((dict(first="c"), "first and log_coords name"), (dict(first=3), "first and log_coords name"), (dict(log_coords=("Dc", "x")), "first and log_coords name"),
                    (dict(n=(5, 4, 3)), "odd node counts"), (dict(n=(5, 3)), "odd node counts"), (dict(window_sd=0.0), "window_sd"),
                    (dict(center=[70.0, 0.011, 0.014]), "center lies outside the box"), (dict(factor=np.eye(2)), "factor is a finite"),
                    (dict(lo=[0.0, 0.009, 0.012], log_coords=("Dc",)), "a logged parameter needs lo > 0"),
                    (dict(lo=[8.0, 0.009], hi=[60.0, 0.013], center=POINT[:2], factor=np.eye(2)), "d = 1 .Dc. or 3")):
        with pytest.raises(ValueError, match=msg):
            post(**kw)
    with pytest.raises(pkg.RsfError, match="not positive definite") as ei:
        post(factor=np.zeros((3, 3)))
    assert ei.value.code == pkg._abi.ERR_NOT_POSDEF


def test_front_end_argument_errors(pkg):
    data = np.zeros(50)
    mc = pkg.MCMC(_model(pkg, observable="mu", state_law="slip"), data, 20.0, PRIORS3, POINT, nsamples=10, verbose=False)
    for marg in ((), ("Dc", "Dc"), ("c",), "x"):
        with pytest.raises(ValueError, match="marginals names parameters"):
            mc.quadrature_law(marginals=marg)
    with pytest.raises(ValueError, match="laws names the ageing and the slip law once each"):
        mc.bayes_factor_laws(laws=("aging", "aging"))

    class Duck:
        Dc = 1.0

        def evaluate(self):
            return None, data

    with pytest.raises(TypeError, match="quadrature_law integrates the model on the device"):
        pkg.MCMC(Duck(), data, 20.0, ["Uniform", 5.0, 200.0], 20.0, nsamples=10, verbose=False).quadrature_law()


def test_refusals_that_stay(pkg, cpu_engine):
    data = np.zeros(50)
    mc = pkg.MCMC(_model(pkg, observable="mu", state_law="slip"), data, 20.0, PRIORS3, POINT, nsamples=10, verbose=False)
    with pytest.raises(NotImplementedError, match=r"compare_laws is one-parameter \(Dc\)"):
        mc.compare_laws()
    cpu_engine.set_model(_model(pkg), 1)
    with pytest.raises(NotImplementedError, match=r"grid_posterior takes an ssq_fn at d = 1 only"):
        cpu_engine.grid_posterior(np.zeros(cpu_engine.nout), LO3, HI3, ssq_fn=lambda q: np.ones(len(q)))
    # the calls of the ageing-only kernels still refuse a law model by name: PosteriorPool.evidence runs Engine.evidence
    cpu_engine.set_model(_model(pkg, state_law="slip"), 1)
    with pytest.raises(NotImplementedError, match="this call integrates the ageing law only"):
        cpu_engine.evidence(np.tile(POINT, (32, 1)), np.zeros(cpu_engine.nout), LO3, HI3)
    cpu_engine.set_model(_model(pkg, observable="mu"), 1)
    with pytest.raises(NotImplementedError, match="this call fits the acceleration only"):
        cpu_engine.evidence(np.tile(POINT, (32, 1)), np.zeros(cpu_engine.nout), LO3, HI3)


def test_state_law_is_restored_after_an_exception(pkg, monkeypatch):
    model = _model(pkg, observable="mu", state_law="slip")
    mc = pkg.MCMC(model, np.zeros(50), 20.0, PRIORS3, POINT, nsamples=10, verbose=False)
    seen, closed = [], []

    class Eng:
        def __init__(self, law):
            self.law = law

        def close(self):
            closed.append(self.law)

    def boom(**kw):
        seen.append(model.state_law)
        if len(seen) == 2:
            raise RuntimeError("the second law's quadrature fails")
        return type("Res", (), {"log_evidence": 0.0, "engine": Eng(model.state_law)})()

    monkeypatch.setattr(mc, "quadrature_law", boom)
    with pytest.raises(RuntimeError, match="second law"):
        mc.bayes_factor_laws(laws=("ageing", "slip"), n=(5, 3, 3))
    assert seen == ["ageing", "slip"] and model.state_law == "slip"
    assert closed == ["ageing"]  # the first law's result held an engine that nobody else can release
    model.state_law = "aging"
    seen.clear()
    with pytest.raises(RuntimeError):
        mc.bayes_factor_laws()
    assert model.state_law == "aging"


def test_law_evidence_runs_the_shared_driver(pkg, cpu_engine, monkeypatch):
    """Engine.law_evidence is Engine.evidence's driver with law_logtarget on points as its target: the driver's own argument check
    answers, and the target is asked with the draws, their log g and the transform's flags"""
    eng = cpu_engine
    eng.set_model(_model(pkg, observable="mu", state_law="slip"), 1)
    data = np.zeros(eng.nout)
    with pytest.raises(ValueError, match="fit_fraction"):
        eng.law_evidence("slip", "mu", np.tile(POINT, (64, 1)), data, LO3, HI3, fit_fraction=1.5)
    calls = []

    def driver(samples, ltarget, lo, hi, shape, n_data, transform, n_proposal, fit_fraction, seed, ess_factor):
        calls.append((shape, n_data, transform))
        return ltarget(np.tile(POINT, (2, 1)), np.zeros(2))

    def target(law, observable, obs, lo, hi, theta=None, logg=None, tr=None, shape=None, **kw):
        calls.append((law, observable, tuple(tr), shape, len(theta), len(logg)))
        return "l", "ssq"

    monkeypatch.setattr(eng, "_evidence", driver)
    monkeypatch.setattr(eng, "law_logtarget", target)
    assert eng.law_evidence("slip", "mu", np.tile(POINT, (64, 1)), data, LO3, HI3, transform=("log", "identity", "identity")) == "l"
    assert calls == [(0.5 * eng.nout, eng.nout, ("log", "identity", "identity")), ("slip", "mu", (1, 0, 0), 0.5 * eng.nout, 2, 2)]
