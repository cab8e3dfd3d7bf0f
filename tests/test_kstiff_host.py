"""
Host logic of the sampler with the stiffness among the parameters (include/rsf_kstiff.h; Engine.kstiff_*, MCMC.sample_stiffness):
the prototype table against the header, the refusals of MCMC.sample_stiffness and of the Engine calls that are made before any
library call, and the refusal on a library without the symbols — on the checker engine, whose library exports nothing of
rsf_kstiff.h.  No GPU.
"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = r"rsf_kstiff_(observe|dr_run|dr_ssq|dr_propose|dr_accept) is exported by librsf_hip.so only.*rsf_kstiff\.h"
K = 2e-3
NAMES = ["rsf_kstiff_dr_accept", "rsf_kstiff_dr_propose", "rsf_kstiff_dr_run", "rsf_kstiff_dr_ssq", "rsf_kstiff_observe"]


def _model(pkg, **attrs):
    m = pkg.RateStateModel(number_time_steps=50)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _declared(name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsf_\w+)\s*\(([^;]*)\)\s*;", code)}


def _state(n, d):
    q = np.ascontiguousarray(np.tile([20.0, 0.011, 0.014, K] if d == 4 else [20.0, K], (n, 1)))
    return q, np.zeros(n), [np.zeros(n, dtype=np.int32) for _ in range(5)]


def test_header_and_prototype_table_declare_the_same_symbols(pkg):
    abi = pkg._abi
    decl = _declared("rsf_kstiff.h")
    assert sorted(decl) == sorted(abi.KSTIFF_PROTOTYPES) == NAMES
    names = lambda text: [a.split()[-1].lstrip("*") for a in text.split(",")]
    stiff = _declared("rsf_stiff.h")
    # rsf_stiff_dr_run's and rsf_stiff_dr_ssq's argument lists without the scalar stiffness
    for name, base in (("rsf_kstiff_dr_run", "rsf_stiff_dr_run"), ("rsf_kstiff_dr_ssq", "rsf_stiff_dr_ssq")):
        other = names(stiff[base])
        assert other[3] == "stiffness" and names(decl[name]) == other[:3] + other[4:]
        rt, args = abi.KSTIFF_PROTOTYPES[name]
        want = abi.STIFF_PROTOTYPES[base][1]
        assert rt is ctypes.c_int and args == want[:3] + want[4:] and want[3] is ctypes.c_double
    # rsf_stiff_observe's with the stiffness an array of n behind b
    other = names(stiff["rsf_stiff_observe"])
    assert names(decl["rsf_kstiff_observe"]) == other[:3] + other[4:8] + ["k"] + other[8:]
    want = abi.STIFF_PROTOTYPES["rsf_stiff_observe"][1]
    assert abi.KSTIFF_PROTOTYPES["rsf_kstiff_observe"] == (ctypes.c_int, want[:3] + want[4:8] + [ctypes.c_void_p] + want[8:])
    # rsf_dr_propose's and rsf_dr_accept's argument lists
    dr = _declared("rsf_dr.h")
    for name, base in (("rsf_kstiff_dr_propose", "rsf_dr_propose"), ("rsf_kstiff_dr_accept", "rsf_dr_accept")):
        assert names(decl[name]) == names(dr[base])
        assert abi.KSTIFF_PROTOTYPES[name] == abi.DR_PROTOTYPES[base]
    tables = [getattr(abi, t) for t in dir(abi) if t.endswith("PROTOTYPES") and t != "KSTIFF_PROTOTYPES"]
    assert len(tables) >= 20 and not any(set(abi.KSTIFF_PROTOTYPES) & set(t) for t in tables)
    assert abi.KSTIFF_MAX_PARAMS == 4 and "#define RSF_KSTIFF_MAX_PARAMS 4" in open(os.path.join(ROOT, "include", "rsf_kstiff.h")).read()
    assert abi.DR_MAX_PARAMS == 3  # rsf_dr.h's own stays


def test_the_parent_header_keeps_its_three_symbols(pkg):
    assert sorted(_declared("rsf_stiff.h")) == ["rsf_stiff_dr_run", "rsf_stiff_dr_ssq", "rsf_stiff_observe"]
    assert sorted(pkg._abi.STIFF_PROTOTYPES) == ["rsf_stiff_dr_run", "rsf_stiff_dr_ssq", "rsf_stiff_observe"]


def test_sample_stiffness_refusals(pkg):
    data = np.full(50, 0.6)
    prior = ["Uniform", 5.0, 200.0]
    mc = pkg.MCMC(_model(pkg, stiffness=K, observable="mu"), data, 20.0, prior, 20.0, nsamples=10, verbose=False)
    assert mc.n_params == 1
    # a model without a stiffness: the start needs one
    none = pkg.MCMC(_model(pkg, observable="mu"), data, 20.0, prior, 20.0, nsamples=10, verbose=False)
    with pytest.raises(ValueError, match="model.stiffness"):
        none.sample_stiffness(8, 4, (1e-3, 4e-3))
    # the prior: 0 < klo < model.stiffness < khi
    for bad in ((0.0, 4e-3), (-1e-3, 4e-3), (2e-3, 4e-3), (1e-3, 2e-3), (3e-3, 4e-3), (1e-3, 1.5e-3), (1e-3, float("inf")), (float("nan"), 4e-3),
                (4e-3, 1e-3)):
        with pytest.raises(ValueError, match="0 < klo < model.stiffness < khi"):
            mc.sample_stiffness(8, 4, bad)
    # a non-device model

    class Other:
        Dc, stiffness = 20.0, K

        def evaluate(self):
            return None, data, data

    with pytest.raises(TypeError, match="sample_stiffness integrates the model on the device"):
        pkg.MCMC(Other(), data, 20.0, prior, 20.0, nsamples=10, verbose=False).sample_stiffness(8, 4, (1e-3, 4e-3))
    # the other solves, as check_law_options refuses them
    for attrs, what in ((dict(integrator="dop853"), r"stiffness=0\.002 with integrator='dop853'"),
                        (dict(precision="float32"), r"stiffness=0\.002 with precision='float32'")):
        m = pkg.MCMC(_model(pkg, stiffness=K, **attrs), data, 20.0, prior, 20.0, nsamples=10, verbose=False)
        with pytest.raises(NotImplementedError, match=what):
            m.sample_stiffness(8, 4, (1e-3, 4e-3))
    # sample_law's own argument checks
    for kw, what in ((dict(start="fit"), "start is 'qstart'"), (dict(factor="init"), "factor is 'gn'"), (dict(nburn=4), "0 <= nburn < n_iter")):
        with pytest.raises(ValueError, match=what):
            mc.sample_stiffness(8, 4, (1e-3, 4e-3), **kw)
    with pytest.raises(ValueError, match="start holds 3 chains"):
        mc.sample_stiffness(8, 4, (1e-3, 4e-3), start=np.tile([20.0, K], (3, 1)))
    assert "hold" in pkg.MCMC.sample_stiffness.__doc__.lower() and "101 %" in pkg.MCMC.sample_stiffness.__doc__ and "160" in pkg.MCMC.sample_stiffness.__doc__


def test_engine_refusals_before_any_library_call(pkg, cpu_engine):
    eng = cpu_engine
    eng.set_model(_model(pkg, observable="mu"), 1)
    data = np.full(eng.nout, 0.6)
    with pytest.raises(ValueError, match=r"\(m, 2\) of \(Dc, k\) or \(m, 4\)"):
        eng.kstiff_ssq_fn("aging", data, "mu")(np.zeros((4, 3)))
    with pytest.raises(ValueError, match=r"k has shape \(3,\)"):
        eng.kstiff_observe("aging", "mu", [20.0, 30.0], [K, K, K])
    with pytest.raises(ValueError, match=r"a finite point \(Dc, k\) or \(Dc, a, b, k\)"):
        eng.kstiff_gn_factor("aging", "mu", [20.0, 0.011, K], data)
    q, l, cnt = _state(64, 2)
    with pytest.raises(ValueError, match="d one of \\(2, 4\\)"):
        eng.kstiff_dr("aging", "mu", np.full((64, 3), 1.0), data, [0.5] * 3, [2.0] * 3, np.eye(3), 4)
    with pytest.raises(ValueError, match="lies in k > 0"):
        eng.kstiff_dr("aging", "mu", q, data, [5.0, 0.0], [200.0, 8e-3], np.diag([1.0, 1e-4]), 4)
    # the parent's driver keeps its dimensions
    with pytest.raises(ValueError, match="d one of \\(1, 3\\)"):
        eng.law_dr("aging", "mu", q, data, [5.0, 5e-4], [200.0, 8e-3], np.diag([1.0, 1e-4]), 4, stiffness=K)


@pytest.mark.parametrize("d", [2, 4])
def test_checker_library_names_the_missing_symbol(pkg, cpu_engine, d):
    eng = cpu_engine
    box = ([5.0, 5e-4], [200.0, 8e-3]) if d == 2 else ([5.0, 0.005, 0.008, 5e-4], [200.0, 0.02, 0.025, 8e-3])
    L = np.diag([1.0, 1e-5] if d == 2 else [1.0, 1e-4, 1e-4, 1e-5])
    # whatever the model's stiffness is: these calls take k from the points
    for stiffness in (None, K):
        eng.set_model(_model(pkg, observable="mu", state_law="slip", stiffness=stiffness), 1)
        data = np.full(eng.nout, 0.6)
        q, l, cnt = _state(64, d)
        ones = np.ones(64, np.uint8)
        for call in (lambda: eng.kstiff_observe("slip", "mu", q[:, 0].copy(), q[:, -1].copy()),
                     lambda: eng.kstiff_ssq_fn("slip", data, "mu")(q),
                     lambda: eng.kstiff_dr_run("slip", "mu", q, l, data, *box, L, 1, cnt),
                     lambda: eng.kstiff_dr_ssq("ageing", "friction", q, ones, data),
                     lambda: eng.kstiff_dr_propose(q, l, *box, L, 1),
                     lambda: eng.kstiff_dr_accept(q, l, *box, 1, q, ones, np.ones(64), cnt, 25.0),
                     lambda: eng.kstiff_gn_factor("slip", "mu", q[0], data),
                     lambda: eng.kstiff_dr("slip", "mu", q, data, *box, L, 4)):
            with pytest.raises(pkg.RsfError, match=MISSING) as ei:
                call()
            assert ei.value.code == -5
