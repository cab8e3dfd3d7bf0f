"""
Host logic of the posterior predictive checks under a state law (include/rsf_law_predict.h; Engine.law_predictive_partials /
series_partials / law_predictive, PosteriorPool.law_predictive / law_loo): the prototype table against the header, the refusal
on a library without the symbols, and the argument checks that run before any library call, on the checker engine — whose
library exports nothing of rsf_law_predict.h.  No GPU.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = r"rsf_(law_predict_partials|predict_series_partials) is exported by librsf_hip.so only.*rsf_law_predict\.h"


def _model(pkg, **attrs):
    m = pkg.RateStateModel(number_time_steps=50)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _declared(code):
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsf_\w+)\s*\(([^;]*)\)\s*;", code)}


def _names(text):
    return [a.split()[-1].lstrip("*") for a in text.split(",")]


def test_header_and_prototype_table_declare_the_same_symbols(pkg):
    abi = pkg._abi
    decl, base = _declared(_header("rsf_law_predict.h")), _declared(_header("rsf_predict.h"))
    assert sorted(decl) == sorted(abi.LAW_PREDICT_PROTOTYPES) == ["rsf_law_predict_partials", "rsf_predict_series_partials"]
    # rsf_predict_partials' arguments, in its order, behind (ctx, law, observable)
    rt, args = abi.LAW_PREDICT_PROTOTYPES["rsf_law_predict_partials"]
    assert rt is ctypes.c_int and len(decl["rsf_law_predict_partials"].split(",")) == len(args) == len(abi.PREDICT_PROTOTYPES["rsf_predict_partials"][1]) + 2
    assert args[:3] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] and args[3:] == abi.PREDICT_PROTOTYPES["rsf_predict_partials"][1][1:]
    assert _names(decl["rsf_law_predict_partials"]) == ["ctx", "law", "observable"] + _names(base["rsf_predict_partials"])[1:]
    # the series entry: the series in the solve's place, no series out
    rt, args = abi.LAW_PREDICT_PROTOTYPES["rsf_predict_series_partials"]
    assert rt is ctypes.c_int and args[:3] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] and len(args) == 9
    assert _names(decl["rsf_predict_series_partials"]) == ["ctx", "n", "nout", "series", "std2", "data", "center_y", "center_l", "partials"]
    # a table of its own: nothing of it in the other headers or their tables, and rsf_model keeps its size
    others = (abi.PROTOTYPES, abi.PREDICT_PROTOTYPES, abi.PSIS_PROTOTYPES, abi.PREDICT_NOISE_PROTOTYPES, abi.LAW_PROTOTYPES, abi.OBSERVE_PROTOTYPES,
              abi.LAW_DR_PROTOTYPES)
    assert not any(set(abi.LAW_PREDICT_PROTOTYPES) & set(t) for t in others)
    for other in ("rsf_abi.h", "rsf_predict.h", "rsf_psis.h", "rsf_predict_noise.h", "rsf_law.h", "rsf_observe.h", "rsf_law_dr.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "rsf_law_predict" not in text and "rsf_predict_series_partials" not in text, other
    assert ctypes.sizeof(abi.Model) == 80
    # the partials are rsf_predict.h's: the new header defines no layout constant of its own
    assert "#define RSF_" not in _header("rsf_law_predict.h").replace("#define RSF_LAW_PREDICT_H", "")


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rsf_law_predict.h"\nint main(void) { return RSF_PREDICT_FIELDS == 7 && RSF_OBS_MU == 1 && RSF_LAW_SLIP == 1 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_product_library_exports_the_family(pkg):
    lib = pkg._abi.load()  # loads without a GPU
    for name, (rt, args) in pkg._abi.LAW_PREDICT_PROTOTYPES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is rt, name
    # the entry checks that run before the device is touched: a NULL ctx is refused under the function's name
    x = np.zeros(8)
    p = x.ctypes.data
    dp = x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.rsf_law_predict_partials(None, 0, 0, 1, 1, p, p, p, dp, dp, dp, None) == -1 and b"rsf_law_predict_partials" in lib.rsf_last_error()
    assert lib.rsf_predict_series_partials(None, 1, 1, p, p, p, dp, dp, dp) == -1 and b"rsf_predict_series_partials" in lib.rsf_last_error()


def _pool(pkg, n_keep=3, C=4, d=1):
    q = np.tile([20.0, 0.011, 0.014][:d], (n_keep, C, 1)) + 0.01 * np.arange(n_keep * C).reshape(n_keep, C, 1)
    return pkg.PosteriorPool(q, np.full((n_keep, C), 1e-6), 0.3, {}, 0)


def test_checker_library_names_the_missing_symbol(pkg, cpu_engine):
    eng = cpu_engine
    model = _model(pkg, observable="mu", state_law="slip")
    eng.set_model(model, 1)
    data, q, s2 = np.full(eng.nout, 0.6), np.full((8, 1), 20.0), np.full(8, 1e-6)
    c = np.zeros(eng.nout)
    for call in (lambda: eng.law_predictive_partials("slip", "mu", q, s2, data, c, c),
                 lambda: eng.law_predictive_partials(0, 3, np.full((8, 3), 1.0), s2, data, c, c, return_series=True),
                 lambda: eng.series_partials(np.zeros((eng.nout, 8)), s2, data, c, c),
                 lambda: eng.law_predictive("slip", "mu", q, s2, data),
                 lambda: eng.law_predictive("ageing", "friction", q, s2, data, center=(c, c), loo=True, noise_probs=(0.05, 0.95)),
                 lambda: _pool(pkg).law_predictive(model, data, engine=eng),
                 lambda: _pool(pkg, d=3).law_loo(model, data, engine=eng, max_draws=5)):
        with pytest.raises(pkg.RsfError, match=MISSING) as ei:
            call()
        assert ei.value.code == -5
    # the existing entries keep their refusals, which now name the way out
    for call in (lambda: eng.predictive(q, s2, data), lambda: eng.predictive_partials(q, s2, data, c, c), lambda: _pool(pkg).predictive(model, data, engine=eng),
                 lambda: _pool(pkg).loo(model, data, engine=eng)):
        with pytest.raises(NotImplementedError, match="state_law is 'slip'.*law_predictive"):
            call()
    eng.set_model(_model(pkg, observable="mu"), 1)
    with pytest.raises(NotImplementedError, match="observable is 'mu'.*law_predictive"):
        eng.predictive(q, s2, data)


def test_argument_errors_before_any_library_call(pkg, cpu_engine):
    eng = cpu_engine
    q, s2 = np.full((8, 1), 20.0), np.full(8, 1e-6)
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.law_predictive("slip", "mu", q, s2, np.zeros(50))
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.law_predictive_partials("slip", "mu", q, s2, np.zeros(50), np.zeros(50), np.zeros(50))
    eng.set_model(_model(pkg), 1)
    data, c = np.zeros(eng.nout), np.zeros(eng.nout)
    part = lambda **kw: eng.law_predictive_partials(kw.pop("law", "slip"), kw.pop("observable", "mu"), kw.pop("q", q), kw.pop("std2", s2),
                                                    kw.pop("data", data), kw.pop("cy", c), kw.pop("cl", c), **kw)
    full = lambda **kw: eng.law_predictive(kw.pop("law", "slip"), kw.pop("observable", "mu"), kw.pop("q", q), kw.pop("std2", s2), kw.pop("data", data), **kw)
    for call in (part, full):
        # the names: law_observe's checks
        for law in ("dieterich", "Slip", "aging "):
            with pytest.raises(ValueError, match="law is 'aging'"):
                call(law=law)
        for obs in ("shear", "MU", "tau"):
            with pytest.raises(ValueError, match="observable is 'acc'"):
                call(observable=obs)
        # predictive's checks
        with pytest.raises(ValueError, match=r"draws are \(n,\) or \(n, d\)"):
            call(q=np.full((8, 2), 20.0))
        with pytest.raises(ValueError, match="no draws"):
            call(q=np.zeros((0, 1)), std2=np.zeros(0))
        with pytest.raises(ValueError, match="std2 has shape"):
            call(std2=s2[:5])
        with pytest.raises(ValueError, match="data has shape"):
            call(data=np.zeros(eng.nout + 1))
    with pytest.raises(ValueError, match="a centre has shape"):
        part(cy=np.zeros(eng.nout - 1))
    with pytest.raises(ValueError, match="a centre has shape"):
        full(center=(c, np.zeros(3)))
    with pytest.raises(ValueError, match="probabilities lie"):
        full(probs=(1.5,), center=(c, c))
    with pytest.raises(ValueError, match="strictly inside"):
        full(noise_probs=(0.0,), center=(c, c))
    # the series entry needs no model, and checks the shapes against the series
    y = np.zeros((7, 8))
    for kw, what in ((dict(series=np.zeros(7)), r"a series is \(nout, n\)"), (dict(series=np.zeros((7, 0))), r"a series is \(nout, n\)"),
                     (dict(std2=s2[:5]), "std2 has shape"), (dict(data=np.zeros(6)), "data has shape"), (dict(cy=np.zeros(6)), "the series has 7 rows"),
                     (dict(cl=np.zeros(8)), "the series has 7 rows")):
        a = dict(series=y, std2=s2, data=np.zeros(7), cy=np.zeros(7), cl=np.zeros(7))
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            eng.series_partials(a["series"], a["std2"], a["data"], a["cy"], a["cl"])


def test_pool_wrappers_take_the_law_the_observable_and_the_loading_from_the_model(pkg):
    """PosteriorPool.law_predictive flattens the draws as predictive does, sets the model on the engine it is given and hands its
    law and observable on (here: an engine object that records, no GPU); law_loo is law_predictive without a band, with loo."""
    seen = {}

    class Fake:
        def set_model(self, model, substeps):
            seen.update(model=model, substeps=substeps)

        def law_predictive(self, law, observable, q, std2, data, **kw):
            seen.update(law=law, observable=observable, q=q, std2=std2, kw=kw)
            return {"mean": 1}

    samples = np.arange(5 * 4 * 3, dtype=np.float64).reshape(5, 4, 3)
    pool = pkg.PosteriorPool(samples, np.arange(20.0).reshape(5, 4), 0.3, {}, 0)
    model = _model(pkg, observable="friction", state_law="slip", loading=lambda t: 1.0 + 0.0 * t)
    model.substeps = 2
    res = pool.law_predictive(model, np.zeros(3), max_draws=5, engine=Fake())
    assert res == {"mean": 1, "law": "slip", "observable": "mu"}
    assert (seen["law"], seen["observable"], seen["substeps"], seen["model"]) == ("slip", "mu", 2, model)
    np.testing.assert_array_equal(seen["std2"], [0.0, 4.0, 8.0, 12.0, 16.0])
    np.testing.assert_array_equal(seen["q"], samples.reshape(20, 3)[[0, 4, 8, 12, 16]])
    assert tuple(seen["kw"]["probs"]) == (0.05, 0.5, 0.95) and "loo" not in seen["kw"] and "noise_probs" not in seen["kw"]
    res = pool.law_loo(_model(pkg), np.zeros(3), engine=Fake(), substeps=1, r_eff=0.5)
    assert (res["law"], res["observable"], seen["substeps"]) == ("aging", "acc", 1)
    assert seen["q"].shape == (20, 3) and seen["kw"] == dict(probs=(), loo=True, r_eff=0.5)
    pool.law_predictive(model, np.zeros(3), engine=Fake(), noise_probs=(0.05, 0.95), loo=True)
    assert seen["kw"]["noise_probs"] == (0.05, 0.95) and seen["kw"]["loo"] is True
    with pytest.raises(ValueError, match="max_draws"):
        pool.law_predictive(model, np.zeros(3), max_draws=0, engine=Fake())
    with pytest.raises(ValueError):
        pool.law_predictive(_model(pkg, state_law="dieterich"), np.zeros(3), engine=Fake())
