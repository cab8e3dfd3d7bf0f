"""
CPU tests of the Python layer of the least-squares fit (Engine.fit, Engine.fit_from_residuals, FitResult, MCMC.fit): the argument
errors raised before any device call, and the launch loop — how many iterations each rsf_fit_run gets, when the loop stops, the
padding of observation groups to whole workgroups — driven through a STUB library: the checker's library for everything else, and
rsf_fit_normal / rsf_fit_run / rsf_fit_trial / rsf_fit_decide written in Python from the specification (tests/fit_reference.py) on a
closed-form model, series_k(q) = exp(-t_k / q_0) (+ q_1 t_k + q_2 at d = 3).
"""
import ctypes

import numpy as np
import pytest

import fit_reference as F


def _view(addr, shape, dtype=np.float64):
    n = int(np.prod(shape))
    ct = {np.float64: ctypes.c_double, np.int32: ctypes.c_int32, np.uint8: ctypes.c_uint8}[dtype]
    return np.ctypeslib.as_array((ct * n).from_address(int(addr))).reshape(shape)


class StubLib:
    """the checker's library plus the rsf_fit_* calls in Python; `calls` records (name, n, n_groups, n_iter)"""

    def __init__(self, oracle_lib, nout, pkg):
        self._lib, self.nout, self.calls = oracle_lib, nout, []
        self.t = np.linspace(0.0, 5.0, nout)
        self._hip = pkg._abi.load()  # rsf_fit_laplace is host arithmetic: the product library's own, no GPU

    def __getattr__(self, name):
        return getattr(self._hip if name == "rsf_fit_laplace" else self._lib, name)

    def series(self, pts):
        pts = np.asarray(pts, dtype=np.float64)
        s = np.exp(-self.t[:, None] / pts[None, :, 0])
        return s if pts.shape[1] == 1 else s + pts[None, :, 1] * self.t[:, None] + pts[None, :, 2]

    def rsf_fit_normal(self, ctx, n, d, q, data, G, fd, ssq, grad, jtj):
        self.calls.append(("normal", n, G, 0))
        s, g, H = F.normal(self.series, _view(q, (n, d)), _view(data, (G, self.nout)), fd)
        _view(ssq, (n,))[:], _view(grad, (n, d))[:], _view(jtj, (n, d, d))[:] = s, g, H
        return 0

    def rsf_fit_run(self, ctx, n, d, q, data, G, lo, hi, fd, ftol, n_iter, ssq, grad, jtj, lam, status, iters):
        self.calls.append(("run", n, G, n_iter))
        st = {"q": _view(q, (n, d)), "ssq": _view(ssq, (n,)), "g": _view(grad, (n, d)), "H": _view(jtj, (n, d, d)), "lam": _view(lam, (n,)),
              "status": _view(status, (n,), np.int32), "iters": _view(iters, (n,), np.int32)}
        obs = _view(data, (G, self.nout))
        blo, bhi = np.array(lo[:d]), np.array(hi[:d])
        for _ in range(n_iter):
            F.iterate(lambda p: F.normal(self.series, p, obs, fd), st, blo, bhi, ftol)
        return 0

    def rsf_fit_trial(self, ctx, n, d, q, grad, jtj, lam, lo, hi, status, q_trial, ok):
        self.calls.append(("trial", n, 1, 1))
        st = {"q": _view(q, (n, d)), "g": _view(grad, (n, d)), "H": _view(jtj, (n, d, d)), "lam": _view(lam, (n,)), "status": _view(status, (n,), np.int32)}
        _view(q_trial, (n, d))[:], _view(ok, (n,), np.uint8)[:] = F.trials(st, np.array(lo[:d]), np.array(hi[:d]))
        return 0

    def rsf_fit_decide(self, ctx, n, d, q, ssq, grad, jtj, lam, status, iters, q_trial, ok, ssq_new, grad_new, jtj_new, ftol):
        self.calls.append(("decide", n, 1, 1))
        st = {"q": _view(q, (n, d)), "ssq": _view(ssq, (n,)), "g": _view(grad, (n, d)), "H": _view(jtj, (n, d, d)), "lam": _view(lam, (n,)),
              "status": _view(status, (n,), np.int32), "iters": _view(iters, (n,), np.int32)}
        F.decide(st, _view(q_trial, (n, d)).copy(), _view(ok, (n,), np.uint8).astype(bool), _view(ssq_new, (n,)).copy(),
                 _view(grad_new, (n, d)).copy(), _view(jtj_new, (n, d, d)).copy(), ftol)
        return 0


@pytest.fixture()
def stub_engine(pkg, oracle_lib):
    eng = pkg.Engine(lib=StubLib(oracle_lib, 50, pkg))
    eng.set_model(pkg.RateStateModel(number_time_steps=50), 1)
    assert eng.nout == 50
    yield eng
    eng.close()


def _data(stub, truths, seed=4):
    rng = np.random.default_rng(seed)
    return np.stack([stub.series(np.array([[t]]))[:, 0] + 1e-3 * rng.standard_normal(stub.nout) for t in truths])


def test_launch_loop(pkg, stub_engine):
    eng, stub = stub_engine, stub_engine.lib
    data = _data(stub, [2.0])[0]
    q0 = [0.7, 1.5, 6.0]
    res = eng.fit(q0, data, 0.1, 50.0, max_iter=100, iters_per_launch=8)
    want = F.fit(lambda p: F.normal(stub.series, p, data, 1e-6), np.array(q0)[:, None], [0.1], [50.0])
    np.testing.assert_array_equal(res.q, want["q"])
    np.testing.assert_array_equal(res.status, want["status"])
    np.testing.assert_array_equal(res.iters, want["iters"])
    assert (res.status == pkg._abi.FIT_CONVERGED).all() and res.n_groups == 1 and res.n_obs == 50
    # one normal call, then launches of 8 until no start is RUNNING: ceil(max iters / 8) of them, none after
    runs = [c for c in stub.calls if c[0] == "run"]
    assert stub.calls[0] == ("normal", 3, 1, 0) and len(runs) == -(-int(want["iters"].max()) // 8) and all(c == ("run", 3, 1, 8) for c in runs)
    # max_iter cuts the last launch short; a start still RUNNING is reported as such
    stub.calls.clear()
    res = eng.fit(q0, data, 0.1, 50.0, max_iter=5, iters_per_launch=3)
    assert [c[3] for c in stub.calls if c[0] == "run"] == [3, 2] and (res.iters <= 5).all() and (res.status == pkg._abi.FIT_RUNNING).any()
    # the caller's start array is not written
    q0a = np.array(q0)
    eng.fit(q0a, data, 0.1, 50.0)
    np.testing.assert_array_equal(q0a, q0)
    # a first sum that is not finite: FAILED, never launched
    stub.calls.clear()
    bad = data.copy()
    bad[3] = np.nan
    res = eng.fit([1.0], bad, 0.1, 50.0)
    assert res.status[0] == pkg._abi.FIT_FAILED and res.iters[0] == 0 and res.q[0, 0] == 1.0 and [c[0] for c in stub.calls] == ["normal"]
    with pytest.raises(pkg.RsfError, match="finite"):
        res.best()


def test_groups_are_padded_to_whole_workgroups(pkg, stub_engine):
    eng, stub = stub_engine, stub_engine.lib
    data = _data(stub, [2.0, 9.0])
    q0 = np.array([0.7, 1.5, 6.0, 0.8, 3.0, 20.0])
    res = eng.fit(q0, data, 0.1, 50.0)
    assert stub.calls[0] == ("normal", 2 * pkg._abi.MAX_BLOCK, 2, 0) and res.q.shape == (6, 1) and res.n_groups == 2
    for g in range(2):
        want = F.fit(lambda p: F.normal(stub.series, p, data[g], 1e-6), q0[3 * g:3 * g + 3, None], [0.1], [50.0])
        np.testing.assert_array_equal(res.q[3 * g:3 * g + 3], want["q"])
        np.testing.assert_array_equal(res.iters[3 * g:3 * g + 3], want["iters"])
        i = res.best(g)
        assert 3 * g <= i < 3 * g + 3 and res.ssq[i] == res.ssq[3 * g:3 * g + 3].min()
    assert res.best() in (res.best(0), res.best(1))
    assert abs(res.q[res.best(0), 0] - 2.0) < 0.05 and abs(res.q[res.best(1), 0] - 9.0) < 0.5
    # covariance and the Laplace figure: the library's arithmetic on this start's ssq and jtj
    i = res.best(0)
    cov = res.covariance(i)
    assert cov.shape == (1, 1) and cov[0, 0] == pytest.approx(res.ssq[i] / (50 - 1) / res.jtj[i, 0, 0], rel=1e-14)
    lap = res.laplace(None, 0.1, 50.0, i)
    want = F.laplace(1, 50, 25.0, res.ssq[i], res.jtj[i], [0.1], [50.0])
    assert lap["shape"] == 25.0 and lap["log_integral"] == pytest.approx(float(want[1]), rel=1e-13) and lap["log_evidence"] == pytest.approx(float(want[2]), rel=1e-13)
    assert lap["stderr"][0] == pytest.approx(np.sqrt(cov[0, 0]))
    with pytest.raises(ValueError, match="group"):
        res.best(2)
    # an engine with smaller workgroups pads to its own
    with pkg.Engine(lib=stub, block_threads=64) as small:
        small.set_model(pkg.RateStateModel(number_time_steps=50), 1)
        stub.calls.clear()
        small.fit(q0, data, 0.1, 50.0, max_iter=1)
        assert stub.calls[0] == ("normal", 128, 2, 0)


def test_fit_from_residuals(pkg, stub_engine):
    eng, stub = stub_engine, stub_engine.lib
    truth = np.array([[3.0, 0.02, 0.5]])
    data = stub.series(truth)[:, 0] + 1e-3 * np.random.default_rng(6).standard_normal(stub.nout)
    lo, hi = [0.1, -1.0, -5.0], [50.0, 1.0, 5.0]
    q0 = np.array([[2.0, 0.01, 0.3], [5.0, 0.05, 1.0]])  # (no coordinate at 0: the forward-difference step is relative)
    calls = []

    def res_fn(pts):
        calls.append(pts.shape)
        return (stub.series(pts) - data[:, None]).T

    res = eng.fit_from_residuals(res_fn, q0, lo, hi)
    # (CONVERGED, or STALLED at the minimum: there a start waits for one more decrease, which the rounding noise may not give)
    assert np.isin(res.status, (pkg._abi.FIT_CONVERGED, pkg._abi.FIT_STALLED)).all() and res.n_obs == 50 and all(s == (8, 3) for s in calls)
    np.testing.assert_allclose(res.q, np.tile(truth, (2, 1)), rtol=0.05, atol=0.01)
    # one residual call for the starts and one per iteration, a trial and a decision each
    names = [c[0] for c in stub.calls]
    assert names.count("trial") == names.count("decide") == len(calls) - 1 == int(res.iters.max())
    with pytest.raises(ValueError, match="residuals"):
        eng.fit_from_residuals(lambda p: np.zeros(3), q0, lo, hi)


def test_argument_errors_before_any_device_call(pkg, cpu_engine):
    """On the checker engine, whose library has no rsf_fit_* at all: each of these is refused in Python."""
    eng = cpu_engine
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.fit([1000.0], np.zeros(50), 0.0, 1e4)
    eng.set_model(pkg.RateStateModel(number_time_steps=50), 1)
    data = np.zeros(eng.nout)
    ok = dict(q0=[1000.0, 2000.0], data=data, lo=0.0, hi=1e4)
    for kw in (dict(q0=np.zeros((2, 2))),                    # d = 2 has no solve
               dict(q0=np.zeros((0, 1))), dict(q0=np.zeros((2, 1, 1))),
               dict(lo=[0.0, 0.0]),                          # two bounds for one parameter
               dict(lo=1e4, hi=0.0), dict(hi=np.inf),
               dict(fd_rel_step=0.0), dict(fd_rel_step=np.nan), dict(ftol=-1.0), dict(max_iter=0),
               dict(iters_per_launch=0), dict(iters_per_launch=65),
               dict(data=np.zeros(eng.nout + 1)), dict(data=np.zeros((2, 2, eng.nout))),
               dict(q0=[1.0, 2.0, 3.0], data=np.zeros((2, eng.nout)))):  # three starts over two series
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.fit(**args)
    for kw in (dict(q0=np.zeros((2, 4))), dict(lo=1.0, hi=1.0), dict(max_iter=0), dict(ftol=np.inf)):
        args = dict(res_fn=lambda p: np.zeros((p.shape[0], 5)), q0=[1.0], lo=0.0, hi=2.0)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.fit_from_residuals(**args)
    # the sampler's front end
    model = pkg.RateStateModel(number_time_steps=50)
    with pytest.raises(ValueError, match="n_starts"):
        mc = pkg.MCMC(model, data, 1000.0, ["Uniform", 0.0, 1e4], 1000.0)
        mc._fit_starts(eng, 0, 0)
    from duck_model import DecayModel

    with pytest.raises(TypeError, match="RateStateModel"):
        pkg.MCMC(DecayModel(), data, 4.0, ["Uniform", 0.0, 10.0], 1.0).fit()


def test_low_level_calls_check_the_layout_of_a_state(pkg, stub_engine):
    """The low-level calls hand raw addresses to the library: a state array that is not C-contiguous, or of another type or shape,
    is refused; the arrays rsf_fit_decide only reads are copied into the right layout."""
    eng = stub_engine
    n, d = 3, 2
    st = dict(q=np.ones((n, d)), ssq=np.full(n, 2.0), grad=np.ones((n, d)), jtj=np.tile(np.eye(d), (n, 1, 1)), lam=np.full(n, 1e-3),
              status=np.zeros(n, dtype=np.int32), iters=np.zeros(n, dtype=np.int32))
    qt, ok = eng.fit_trial(st["q"], st["grad"], st["jtj"], st["lam"], st["status"], [-5.0] * d, [5.0] * d)
    assert ok.all()
    new = dict(ssq_new=np.array([1.0, 3.0, 1.5]), grad_new=np.arange(6.0).reshape(n, d), jtj_new=np.arange(12.0).reshape(n, d, d))
    want = {k: v.copy() for k, v in st.items()}
    eng.fit_decide(*(want[k] for k in ("q", "ssq", "grad", "jtj", "lam", "status", "iters")), qt, ok, **new)
    # the same inputs in Fortran order and as a list: the same result
    odd = dict(ssq_new=list(new["ssq_new"]), grad_new=np.asfortranarray(new["grad_new"]), jtj_new=np.ascontiguousarray(new["jtj_new"].transpose(2, 1, 0)).transpose(2, 1, 0))
    assert not odd["grad_new"].flags["C_CONTIGUOUS"] and not odd["jtj_new"].flags["C_CONTIGUOUS"]
    got = {k: v.copy() for k, v in st.items()}
    eng.fit_decide(*(got[k] for k in ("q", "ssq", "grad", "jtj", "lam", "status", "iters")), np.asfortranarray(qt), ok, **odd)
    for k in st:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got["grad"][0], new["grad_new"][0])
    np.testing.assert_array_equal(got["grad"][1], st["grad"][1])  # 3.0 > 2.0: rejected
    for k, bad in (("grad", np.asfortranarray(st["grad"])), ("jtj", st["jtj"].transpose(0, 2, 1)), ("lam", st["lam"].astype(np.float32)),
                   ("status", st["status"].astype(np.int64)), ("ssq", np.zeros(n + 1)), ("q", [[1.0, 1.0]] * n)):
        args = dict(st)
        args[k] = bad
        with pytest.raises(ValueError, match=k):
            eng.fit_decide(*(args[j] for j in ("q", "ssq", "grad", "jtj", "lam", "status", "iters")), qt, ok, **new)
        if k != "ssq":
            with pytest.raises(ValueError, match=k):
                eng.fit_trial(args["q"], args["grad"], args["jtj"], args["lam"], args["status"], [-5.0] * d, [5.0] * d)
    with pytest.raises(ValueError, match="q_trial"):
        eng.fit_decide(*(st[j] for j in ("q", "ssq", "grad", "jtj", "lam", "status", "iters")), qt[:2], ok, **new)
