"""
Host logic of the Levenberg-Marquardt fit under a state law (include/rsf_law_fit.h; Engine.law_fit_normal / law_fit_run / law_fit,
MCMC.fit_law): the prototype table against the header, the refusal on a library without the symbols, and the argument checks that
run before any call of that family, on the checker engine — whose library exports nothing of rsf_law_fit.h, so that a check which
came too late would show as the missing symbol's error instead of its own.  No GPU.
"""
import contextlib
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = r"rsf_law_fit_(normal|run) is exported by librsf_hip.so only.*rsf_law_fit\.h"


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
    return dict(q=q, ssq=np.ones(n), grad=np.zeros((n, d)), jtj=np.tile(np.eye(d), (n, 1, 1)), lam=np.full(n, 1e-3), status=np.zeros(n, np.int32),
                iters=np.zeros(n, np.int32))


def _run(eng, st, data, law="slip", observable="mu", lo=5.0, hi=200.0, n_iter=1, **kw):
    return eng.law_fit_run(law, observable, st["q"], data, lo, hi, st["ssq"], st["grad"], st["jtj"], st["lam"], st["status"], st["iters"], n_iter, **kw)


def test_header_and_prototype_table_declare_the_same_symbols(pkg):
    abi = pkg._abi
    decl, fit = _declared(_header("rsf_law_fit.h")), _declared(_header("rsf_fit.h"))
    assert sorted(decl) == sorted(abi.LAW_FIT_PROTOTYPES) == ["rsf_law_fit_normal", "rsf_law_fit_run"]
    for name, base in (("rsf_law_fit_normal", "rsf_fit_normal"), ("rsf_law_fit_run", "rsf_fit_run")):
        rt, args = abi.LAW_FIT_PROTOTYPES[name]
        assert rt is ctypes.c_int and len(decl[name].split(",")) == len(args) == len(abi.FIT_PROTOTYPES[base][1]) + 2
        # rsf_fit_*'s arguments, in its order, behind (ctx, law, observable)
        assert args[:3] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] and args[3:] == abi.FIT_PROTOTYPES[base][1][1:]
        names = lambda text: [a.split()[-1].lstrip("*") for a in text.split(",")]
        assert names(decl[name]) == ["ctx", "law", "observable"] + names(fit[base])[1:]
        # the C types of the header, argument by argument, against the table
        ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
        for text, want in zip(decl[name].split(",")[1:], args[1:]):
            if "*" not in text:
                assert ctype[text.split()[-2]] is want, (name, text)
            else:
                assert want in (abi._P, abi._DP), (name, text)
    # a table of its own: nothing of it in the other headers or their tables, and rsf_model keeps its size
    assert not set(abi.LAW_FIT_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.FIT_PROTOTYPES) | set(abi.LAW_PROTOTYPES) | set(abi.OBSERVE_PROTOTYPES)
                                             | set(abi.LAW_DR_PROTOTYPES) | set(abi.LAW_PREDICT_PROTOTYPES))
    for other in ("rsf_abi.h", "rsf_fit.h", "rsf_law.h", "rsf_observe.h", "rsf_law_dr.h", "rsf_law_predict.h"):
        assert "rsf_law_fit" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert ctypes.sizeof(abi.Model) == 80


def test_checker_library_names_the_missing_symbol(pkg, cpu_engine, monkeypatch):
    eng = cpu_engine
    eng.set_model(_model(pkg, observable="mu", state_law="slip"), 1)
    data = np.full(eng.nout, 0.6)
    st = _state(64)
    for call in (lambda: eng.law_fit_normal("slip", "mu", st["q"], data),
                 lambda: eng.law_fit_normal(0, 3, st["q"][:, 0], data, 1e-5),
                 lambda: _run(eng, st, data),
                 lambda: _run(eng, _state(8, 3), data, "ageing", "friction", [5.0, 0.009, 0.012], [200.0, 0.013, 0.016], 4),
                 lambda: eng.law_fit("slip", "mu", st["q"], data, 5.0, 200.0),
                 lambda: eng.law_fit(1, 1, [20.0, 30.0], data, 5.0, 200.0, max_iter=3)):
        with pytest.raises(pkg.RsfError, match=MISSING) as ei:
            call()
        assert ei.value.code == -5
    # MCMC.fit_law on this engine: the method makes its own Engine, which here is the checker's
    mod = sys.modules[pkg.MCMC.__module__]
    monkeypatch.setattr(mod, "Engine", lambda **kw: contextlib.nullcontext(eng))
    for model in (_model(pkg, observable="mu", state_law="slip"), _model(pkg)):  # any device model, the default one included
        mc = pkg.MCMC(model, data, 20.0, ["Uniform", 5.0, 200.0], 20.0, nsamples=10, verbose=False)
        for kw in (dict(), dict(seed=3, max_iter=5)):  # one start: the others are rsf_smc_init's, which the checker's library lacks too
            with pytest.raises(pkg.RsfError, match=MISSING):
                mc.fit_law(n_starts=1, **kw)


def test_argument_errors_before_any_library_call(pkg, cpu_engine):
    eng = cpu_engine
    st = _state(64)
    for call in (lambda: eng.law_fit("slip", "mu", st["q"], np.zeros(50), 5.0, 200.0), lambda: eng.law_fit_normal("slip", "mu", st["q"], np.zeros(50)),
                 lambda: _run(eng, st, np.zeros(50))):
        with pytest.raises(pkg.RsfError, match="set_model"):
            call()
    eng.set_model(_model(pkg), 1)
    data = np.zeros(eng.nout)
    fit = lambda **kw: eng.law_fit(kw.pop("law", "slip"), kw.pop("observable", "mu"), kw.pop("q0", st["q"]), kw.pop("data", data), kw.pop("lo", 5.0),
                                   kw.pop("hi", 200.0), **kw)
    # the names
    for call in (lambda: fit(law="dieterich"), lambda: eng.law_fit_normal("ruina", "mu", st["q"], data), lambda: _run(eng, st, data, law="Slip")):
        with pytest.raises(ValueError, match="law is 'aging'"):
            call()
    for call in (lambda: fit(observable="shear"), lambda: eng.law_fit_normal("slip", "stress", st["q"], data), lambda: _run(eng, st, data, observable="MU")):
        with pytest.raises(ValueError, match="observable is 'acc'"):
            call()
    with pytest.raises(ValueError, match="observable is one of"):
        fit(observable=7)
    with pytest.raises(ValueError, match="law is 0 or 1"):
        fit(law=2)
    # Engine.fit's checks, through the shared driver
    with pytest.raises(ValueError, match="q0 has shape"):
        fit(q0=np.full((64, 2), 20.0), lo=[5.0, 5.0], hi=[200.0, 200.0])
    with pytest.raises(ValueError, match="q0 has shape"):
        fit(q0=np.zeros((0, 1)))
    with pytest.raises(ValueError, match="finite lo < hi"):
        fit(lo=200.0, hi=5.0)
    with pytest.raises(ValueError, match="finite lo < hi"):
        fit(hi=np.inf)
    with pytest.raises(ValueError, match="data has shape"):
        fit(data=np.zeros(eng.nout + 1))
    with pytest.raises(ValueError, match="data has shape"):
        fit(data=np.zeros((2, 2, eng.nout)))
    with pytest.raises(ValueError, match="cannot be split evenly"):
        fit(q0=np.full(63, 20.0), data=np.zeros((2, eng.nout)))
    for kw in (dict(fd_rel_step=0.0), dict(fd_rel_step=np.nan), dict(ftol=-1.0), dict(ftol=np.inf), dict(max_iter=0), dict(iters_per_launch=0),
               dict(iters_per_launch=65)):
        with pytest.raises(ValueError, match="fd_rel_step is finite"):
            fit(**kw)
    # the low-level calls: fit_normal's and fit_run's checks
    with pytest.raises(ValueError, match="q has shape"):
        eng.law_fit_normal("slip", "mu", np.zeros((2, 2, 2)), data)
    with pytest.raises(ValueError, match="data has shape"):
        eng.law_fit_normal("slip", "mu", st["q"], np.zeros(7))
    with pytest.raises(ValueError, match="data has shape"):
        _run(eng, st, np.zeros(7))
    for key, bad in (("lam", st["lam"][:3]), ("status", st["status"].astype(np.int64)), ("grad", np.zeros((64, 2))), ("jtj", np.zeros((64, 1))),
                     ("ssq", np.ones(64, np.float32)), ("iters", st["iters"][::2]), ("q", np.full((64, 2), 20.0)[:, :1])):
        with pytest.raises(ValueError, match=f"{key} must be a C-contiguous"):
            _run(eng, dict(st, **{key: bad}), data)
    with pytest.raises(ValueError, match=r"q is \(n, d\)"):
        _run(eng, dict(st, q=st["q"][:, 0]), data)
    with pytest.raises(ValueError, match="lo"):
        _run(eng, st, data, lo=[5.0, 6.0])


def test_fit_law_argument_errors(pkg, cpu_engine, monkeypatch):
    data = np.full(50, 0.6)
    mod = sys.modules[pkg.MCMC.__module__]
    monkeypatch.setattr(mod, "Engine", lambda **kw: contextlib.nullcontext(cpu_engine))
    mc = pkg.MCMC(_model(pkg, observable="mu", state_law="slip"), data, 20.0, ["Uniform", 5.0, 200.0], 20.0, nsamples=10, verbose=False)
    with pytest.raises(ValueError, match="n_starts must be >= 1"):
        mc.fit_law(n_starts=0)
    for kw in (dict(ftol=-1.0), dict(max_iter=0), dict(iters_per_launch=65), dict(fd_rel_step=0.0)):
        with pytest.raises(ValueError, match="fd_rel_step is finite"):
            mc.fit_law(n_starts=1, **kw)
    with pytest.raises(TypeError):
        mc.fit_law(n_starts=1, eps=1.0)  # not an argument of Engine.law_fit

    class Other:  # the reference's contract: .Dc and .evaluate(), integrated on the host
        Dc = 20.0

        def evaluate(self):
            return None, data, data

    with pytest.raises(TypeError, match="fit_law integrates the model on the device"):
        pkg.MCMC(Other(), data, 20.0, ["Uniform", 5.0, 200.0], 20.0, nsamples=10, verbose=False).fit_law()
    # the existing methods keep their refusals, by name
    with pytest.raises(NotImplementedError, match="fit integrates the ageing law only"):
        mc.fit()
    with pytest.raises(NotImplementedError, match="start is|takes factor as"):
        mc.sample_dr(4, 4, start="fit", factor=[[1.0]])
    for kw in (dict(start="fit"), dict(factor="fit")):
        with pytest.raises(ValueError):
            mc.sample_law(8, 4, **kw)
    cpu_engine.set_model(_model(pkg, observable="mu", state_law="slip"), 1)
    with pytest.raises(NotImplementedError, match="ageing law only"):
        cpu_engine.fit([20.0], data, 5.0, 200.0)
    cpu_engine.set_model(_model(pkg, observable="mu"), 1)
    with pytest.raises(NotImplementedError, match="fits the acceleration only"):
        cpu_engine.fit([20.0], data, 5.0, 200.0)
