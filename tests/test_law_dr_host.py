"""
Host logic of the delayed-rejection sampler under a state law (include/rsf_law_dr.h; Engine.law_dr_run / law_dr_ssq / law_gn_factor /
law_dr, MCMC.sample_law): the prototype table against the header, the refusal on a library without the symbols, and the argument
checks that run before any library call, on the checker engine — whose library exports nothing of rsf_law_dr.h.  No GPU.
"""
import contextlib
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = r"rsf_law_dr_(run|ssq) is exported by librsf_hip.so only.*rsf_law_dr\.h"


def _model(pkg, **attrs):
    m = pkg.RateStateModel(number_time_steps=50)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _declared(code):
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsf_\w+)\s*\(([^;]*)\)\s*;", code)}


def _state(n, d=1):
    q = np.ascontiguousarray(np.tile([20.0, 0.011, 0.014][:d], (n, 1)))
    return q, np.zeros(n), [np.zeros(n, dtype=np.int32) for _ in range(5)]


def test_header_and_prototype_table_declare_the_same_symbols(pkg):
    abi = pkg._abi
    decl, dr = _declared(_header("rsf_law_dr.h")), _declared(_header("rsf_dr.h"))
    assert sorted(decl) == sorted(abi.LAW_DR_PROTOTYPES) == ["rsf_law_dr_run", "rsf_law_dr_ssq"]
    for name, base in (("rsf_law_dr_run", "rsf_dr_run"), ("rsf_law_dr_ssq", "rsf_dr_ssq")):
        rt, args = abi.LAW_DR_PROTOTYPES[name]
        assert rt is ctypes.c_int and len(decl[name].split(",")) == len(args) == len(abi.DR_PROTOTYPES[base][1]) + 2
        # rsf_dr_*'s arguments, in its order, behind (ctx, law, observable)
        assert args[:3] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] and args[3:] == abi.DR_PROTOTYPES[base][1][1:]
        names = lambda text: [a.split()[-1].lstrip("*") for a in text.split(",")]
        assert names(decl[name]) == ["ctx", "law", "observable"] + names(dr[base])[1:]
    # a table of its own: nothing of it in the other headers or their tables, and rsf_model keeps its size
    assert not set(abi.LAW_DR_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.DR_PROTOTYPES) | set(abi.LAW_PROTOTYPES) | set(abi.OBSERVE_PROTOTYPES))
    for other in ("rsf_abi.h", "rsf_dr.h", "rsf_law.h", "rsf_observe.h"):
        assert "rsf_law_dr" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert ctypes.sizeof(abi.Model) == 80


def test_checker_library_names_the_missing_symbol(pkg, cpu_engine, monkeypatch):
    eng = cpu_engine
    eng.set_model(_model(pkg, observable="mu", state_law="slip"), 1)
    data = np.full(eng.nout, 0.6)
    q, l, cnt = _state(64)
    for call in (lambda: eng.law_dr_run("slip", "mu", q, l, data, 5.0, 200.0, [[1.0]], 1, cnt),
                 lambda: eng.law_dr_run(0, 3, q, l, data, 5.0, 200.0, [[1.0]], 1, cnt, trace=True),
                 lambda: eng.law_dr_ssq("ageing", "friction", q, np.ones(64, np.uint8), data),
                 lambda: eng.law_gn_factor("slip", "mu", [20.0], data),
                 lambda: eng.law_gn_factor("aging", "acc", [20.0, 0.011, 0.014], data),
                 lambda: eng.law_dr("slip", "mu", q, data, 5.0, 200.0, [[1.0]], 4),
                 lambda: eng.law_dr(1, 1, q, data, 5.0, 200.0, [[1.0]], 4, l0=l)):
        with pytest.raises(pkg.RsfError, match=MISSING) as ei:
            call()
        assert ei.value.code == -5
    # MCMC.sample_law on this engine: the method makes its own Engine, which here is the checker's
    mod = sys.modules[pkg.MCMC.__module__]

    def checker(**kw):
        return contextlib.nullcontext(eng)

    monkeypatch.setattr(mod, "Engine", checker)
    mc = pkg.MCMC(_model(pkg, observable="mu", state_law="slip"), data, 20.0, ["Uniform", 5.0, 200.0], 20.0, nsamples=10, verbose=False)
    for kw in (dict(), dict(factor=[[1.0]]), dict(start=np.full((8, 1), 20.0), adapt=False)):
        with pytest.raises(pkg.RsfError, match=MISSING):
            mc.sample_law(8, 4, **kw)


def test_argument_errors_before_any_library_call(pkg, cpu_engine):
    eng = cpu_engine
    q, l, cnt = _state(64)
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.law_dr("slip", "mu", q, np.zeros(50), 5.0, 200.0, [[1.0]], 4)
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.law_gn_factor("slip", "mu", [20.0], np.zeros(50))
    eng.set_model(_model(pkg), 1)
    data = np.zeros(eng.nout)
    run = lambda **kw: eng.law_dr(kw.pop("law", "slip"), kw.pop("observable", "mu"), kw.pop("q0", q), kw.pop("data", data), kw.pop("lo", 5.0),
                                  kw.pop("hi", 200.0), kw.pop("chol", [[1.0]]), kw.pop("n_iter", 4), **kw)
    # the names
    for call in (lambda: run(law="dieterich"), lambda: eng.law_dr_run("ruina", "mu", q, l, data, 5.0, 200.0, [[1.0]], 1, cnt),
                 lambda: eng.law_dr_ssq("Slip", "mu", q, np.ones(64, np.uint8), data), lambda: eng.law_gn_factor("aging ", "mu", [20.0], data)):
        with pytest.raises(ValueError, match="law is 'aging'"):
            call()
    for call in (lambda: run(observable="shear"), lambda: eng.law_dr_run("slip", "stress", q, l, data, 5.0, 200.0, [[1.0]], 1, cnt),
                 lambda: eng.law_dr_ssq("slip", "MU", q, np.ones(64, np.uint8), data), lambda: eng.law_gn_factor("slip", "tau", [20.0], data)):
        with pytest.raises(ValueError, match="observable is 'acc'"):
            call()
    with pytest.raises(ValueError, match="observable is one of"):
        run(observable=7)
    # Engine.dr's checks, through the shared driver
    with pytest.raises(ValueError, match="q0 has shape"):
        run(q0=np.full((64, 2), 20.0), lo=[5.0, 5.0], hi=[200.0, 200.0], chol=np.eye(2))
    with pytest.raises(ValueError, match="finite lo < hi"):
        run(lo=200.0, hi=5.0)
    with pytest.raises(ValueError, match="finite lo < hi"):
        run(hi=np.inf)
    with pytest.raises(ValueError, match="stuck start"):
        run(q0=np.full(64, 5.0))  # on the edge: not strictly inside
    with pytest.raises(ValueError, match="stuck start"):
        run(q0=np.full(64, 300.0))
    with pytest.raises(ValueError, match="data has shape"):
        run(data=np.zeros(eng.nout + 1))
    with pytest.raises(ValueError, match="data has shape"):
        run(data=np.zeros((65, eng.nout)))
    with pytest.raises(ValueError, match="whole workgroups of 256"):
        run(q0=np.full(384, 20.0), data=np.zeros((2, eng.nout)))
    with pytest.raises(ValueError, match="chol"):
        run(chol=[[-1.0]])
    with pytest.raises(ValueError, match="holds 3 factors for 2 groups"):
        run(q0=np.full(512, 20.0), data=np.zeros((2, eng.nout)), chol=np.ones((3, 1, 1)))
    for kw in (dict(gamma=0.0), dict(gamma=1.5), dict(stages=3), dict(shape=0.0), dict(n_iter=0), dict(iters_per_launch=65), dict(keep=5), dict(thin=0),
               dict(seed=-1), dict(offset=-1), dict(adapt_launches=-1), dict(iter0=0), dict(iter0=2 ** 32)):
        with pytest.raises(ValueError):
            run(**kw)
    # the low-level calls: dr_run's and dr_ssq's checks
    with pytest.raises(ValueError, match="C-contiguous float64 array of shape"):
        eng.law_dr_run("slip", "mu", q, l[:3], data, 5.0, 200.0, [[1.0]], 1, cnt)
    with pytest.raises(ValueError, match="the counters are"):
        eng.law_dr_run("slip", "mu", q, l, data, 5.0, 200.0, [[1.0]], 1, cnt[:4])
    with pytest.raises(ValueError, match="chol has shape"):
        eng.law_dr_run("slip", "mu", q, l, data, 5.0, 200.0, np.eye(2), 1, cnt)
    with pytest.raises(ValueError, match=r"y is \(n, d\)"):
        eng.law_dr_ssq("slip", "mu", q, np.ones(3, np.uint8), data)
    # law_gn_factor's
    for bad in ([20.0, 0.011], [np.nan], [0.0], [20.0, 0.0, 0.014]):
        with pytest.raises(ValueError, match="q has shape"):
            eng.law_gn_factor("slip", "mu", bad, data)
    with pytest.raises(ValueError, match="rel_step"):
        eng.law_gn_factor("slip", "mu", [20.0], data, rel_step=0.0)
    with pytest.raises(ValueError, match="the model produces"):
        eng.law_gn_factor("slip", "mu", [20.0], np.zeros(7))


def test_sample_law_argument_errors(pkg):
    data = np.full(50, 0.6)
    mc = pkg.MCMC(_model(pkg, observable="mu", state_law="slip"), data, 20.0, ["Uniform", 5.0, 200.0], 20.0, nsamples=10, verbose=False)
    for factor in ("init", "fit", "GN"):
        with pytest.raises(ValueError, match="factor is 'gn'"):
            mc.sample_law(8, 4, factor=factor)
    for start in ("fit", "prior"):
        with pytest.raises(ValueError, match="start is 'qstart'"):
            mc.sample_law(8, 4, start=start)
    for kw in (dict(nburn=4), dict(nburn=-1), dict(thin=0), dict(iters_per_launch=0)):
        with pytest.raises(ValueError, match="n_chains >= 1"):
            mc.sample_law(8, 4, **kw)
    with pytest.raises(ValueError, match="n_chains >= 1"):
        mc.sample_law(0, 4)

    class Other:  # the reference's contract: .Dc and .evaluate(), integrated on the host
        Dc = 20.0

        def evaluate(self):
            return None, data, data

    with pytest.raises(TypeError, match="sample_law integrates the model on the device"):
        pkg.MCMC(Other(), data, 20.0, ["Uniform", 5.0, 200.0], 20.0, nsamples=10, verbose=False).sample_law(8, 4)
    # the existing methods keep their refusals
    with pytest.raises(NotImplementedError, match="slip"):
        mc.sample_dr(4, 4, factor=[[1.0]], adapt=True)
    with pytest.raises(NotImplementedError, match="slip"):
        mc.sample_dr(4, 4)


def test_refused_solvers_never_reach_the_kernel(pkg, cpu_engine):
    """integrator='dop853' or precision='float32' with the slip law, a custom loading or another observable: refused at set_model"""
    for attrs in (dict(state_law="slip", integrator="dop853"), dict(observable="mu", precision="float32"), dict(loading=lambda t: 1.0 + 0.0 * t, integrator="dop853")):
        with pytest.raises(NotImplementedError):
            cpu_engine.set_model(_model(pkg, **attrs), 1)
