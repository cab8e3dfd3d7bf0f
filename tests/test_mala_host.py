"""
CPU tests of the Python layer of the Gauss-Newton manifold MALA sampler (Engine.mala, Engine.mala_from_residuals, MalaResult,
MCMC.sample_mala, RSF.inference_mala): the prototype table, the argument errors raised before any library call, and the launch
loop — the iterations and the Philox iteration each rsf_mala_run gets, which launches are traced, the rows keep and thin select,
the padding of observation groups — driven through a STUB library: test_fit_host's (the checker's library and rsf_fit_normal on a
closed-form model) plus rsf_mala_run / _propose / _accept written in Python from the specification (tests/mala_reference.py).
"""
import ctypes

import numpy as np
import pytest

import fit_reference as F
import mala_reference as M
import smc_reference as S
from test_fit_host import StubLib, _view


class MalaStub(StubLib):
    """... `calls` records ("mala_run", n, n_groups, n_iter, iter0, traced), ("propose", n, iteration) and ("accept", n, iteration)"""

    @staticmethod
    def _draws(seed, offset, n, it, d):
        ids = offset + np.arange(n, dtype=np.uint64)
        return S.normals(seed, ids, it, d), S.accept_uniforms(seed, ids, it)

    def rsf_mala_run(self, ctx, n, d, q, ssq, grad, jtj, data, G, lo, hi, fd, eps, lam, shape, seed, offset, iter0, n_iter, accepted, outbox, stuck,
                     tq, ts):
        self.calls.append(("mala_run", n, G, n_iter, iter0, tq is not None))
        st = {"q": _view(q, (n, d)), "ssq": _view(ssq, (n,)), "g": _view(grad, (n, d)), "H": _view(jtj, (n, d, d)),
              "accepted": _view(accepted, (n,), np.int32), "outbox": _view(outbox, (n,), np.int32), "stuck": _view(stuck, (n,), np.int32)}
        obs = _view(data, (G, self.nout))
        for k in range(n_iter):
            z, u = self._draws(seed, offset, n, iter0 + k, d)
            M.iterate(lambda p: F.normal(self.series, p, obs, fd), st, z, u, np.array(lo[:d]), np.array(hi[:d]), eps, lam, shape)
            if tq is not None:
                _view(tq, (n_iter, n, d))[k], _view(ts, (n_iter, n))[k] = st["q"], st["ssq"]
        return 0

    def rsf_mala_propose(self, ctx, n, d, q, ssq, grad, jtj, lo, hi, eps, lam, shape, seed, offset, it, q_new, inbox, stuck):
        self.calls.append(("propose", n, it))
        z, _ = self._draws(seed, offset, n, it, d)
        qn, inb, stk, _ = M.propose(_view(q, (n, d)), _view(ssq, (n,)), _view(grad, (n, d)), _view(jtj, (n, d, d)), z, np.array(lo[:d]), np.array(hi[:d]),
                                    eps, lam, shape)
        _view(q_new, (n, d))[:], _view(inbox, (n,), np.uint8)[:], _view(stuck, (n,), np.uint8)[:] = qn, inb, stk
        return 0

    def rsf_mala_accept(self, ctx, n, d, q, ssq, grad, jtj, lo, hi, eps, lam, shape, seed, offset, it, q_new, inbox, ssq_new, grad_new, jtj_new,
                        accepted, outbox, stuck):
        self.calls.append(("accept", n, it))
        st = {"q": _view(q, (n, d)), "ssq": _view(ssq, (n,)), "g": _view(grad, (n, d)), "H": _view(jtj, (n, d, d)),
              "accepted": _view(accepted, (n,), np.int32), "outbox": _view(outbox, (n,), np.int32), "stuck": _view(stuck, (n,), np.int32)}
        z, u = self._draws(seed, offset, n, it, d)
        new = (_view(ssq_new, (n,)).copy(), _view(grad_new, (n, d)).copy(), _view(jtj_new, (n, d, d)).copy())
        out = M.iterate(lambda p: new, st, z, u, np.array(lo[:d]), np.array(hi[:d]), eps, lam, shape)
        assert np.array_equal(out["qn"], _view(q_new, (n, d))) and np.array_equal(out["inbox"], _view(inbox, (n,), np.uint8).astype(bool))
        return 0


@pytest.fixture()
def stub_engine(pkg, oracle_lib):
    eng = pkg.Engine(lib=MalaStub(oracle_lib, 50, pkg))
    eng.set_model(pkg.RateStateModel(number_time_steps=50), 1)
    yield eng
    eng.close()


def _data(stub, truths, seed=4):
    rng = np.random.default_rng(seed)
    return np.stack([stub.series(np.array([[t]]))[:, 0] + 1e-2 * rng.standard_normal(stub.nout) for t in truths])


def _spec_run(stub, q0, data, lo, hi, n_iter, seed=0, offset=0, eps=1.0, lam=1e-3, shape=25.0, fd=1e-6):
    """the specification with the stub's variates -> (final state, the state after every iteration)"""
    q0 = np.asarray(q0, dtype=np.float64).reshape(len(q0), -1)
    normal = lambda p: F.normal(stub.series, p, data, fd)
    st, rows = M.new_state(q0, *normal(q0)), []
    for it in range(1, n_iter + 1):
        z, u = MalaStub._draws(seed, offset, q0.shape[0], it, q0.shape[1])
        M.iterate(normal, st, z, u, np.atleast_1d(lo), np.atleast_1d(hi), eps, lam, shape)
        rows.append((st["q"].copy(), st["ssq"].copy()))
    return st, rows


def test_prototype_table(pkg):
    abi = pkg._abi
    assert sorted(abi.MALA_PROTOTYPES) == ["rsf_mala_accept", "rsf_mala_propose", "rsf_mala_run"]
    assert len(abi.MALA_PROTOTYPES["rsf_mala_run"][1]) == 24 and len(abi.MALA_PROTOTYPES["rsf_mala_propose"][1]) == 18
    assert len(abi.MALA_PROTOTYPES["rsf_mala_accept"][1]) == 23
    assert all(rt is ctypes.c_int for rt, _ in abi.MALA_PROTOTYPES.values())
    assert abi.MALA_MAX_ITER == 64 and abi.MALA_MAX_PARAMS == 3
    lib = abi.load()  # the product library exports them, typed by the table
    for name, (_, argtypes) in abi.MALA_PROTOTYPES.items():
        assert list(getattr(lib, name).argtypes) == argtypes, name


def test_launch_loop_keep_and_thin(pkg, stub_engine):
    eng, stub = stub_engine, stub_engine.lib
    data = _data(stub, [2.0])[0]
    q0 = [1.5, 2.0, 2.6]
    res = eng.mala(q0, data, 0.1, 50.0, 11, seed=5, offset=3, iters_per_launch=4, keep=6, thin=2)
    want, rows = _spec_run(stub, q0, data, 0.1, 50.0, 11, seed=5, offset=3)
    # one normal call, launches of 4, 4 and 3 at Philox iterations 1, 5 and 9; the launches that reach the last 6 iterations are traced
    assert stub.calls == [("normal", 3, 1, 0), ("mala_run", 3, 1, 4, 1, False), ("mala_run", 3, 1, 4, 5, True), ("mala_run", 3, 1, 3, 9, True)]
    for k, w in (("q", "q"), ("ssq", "ssq"), ("grad", "g"), ("jtj", "H"), ("accepted", "accepted"), ("outbox", "outbox"), ("stuck", "stuck")):
        np.testing.assert_array_equal(getattr(res, k), want[w], err_msg=k)
    assert res.n_iter == 11 and res.shape == 25.0 and res.accept_rate == want["accepted"].sum() / 33 and 0 < res.accept_rate
    # keep = 6, thin = 2: the states after iterations 6, 8 and 10
    assert res.iterations.tolist() == [6, 8, 10] and res.samples.shape == (3, 3, 1) and res.ssq_trace.shape == (3, 3)
    for r, it in enumerate(res.iterations):
        np.testing.assert_array_equal(res.samples[r], rows[it - 1][0])
        np.testing.assert_array_equal(res.ssq_trace[r], rows[it - 1][1])
    # keep = n_iter keeps every iteration and ends at the final state; keep = 0 keeps none and traces nothing
    res = eng.mala(q0, data, 0.1, 50.0, 5, seed=5, offset=3, keep=5)
    assert res.iterations.tolist() == [1, 2, 3, 4, 5]
    np.testing.assert_array_equal(res.samples[-1], res.q)
    stub.calls.clear()
    res = eng.mala(q0, data, 0.1, 50.0, 5)
    assert res.samples.shape == (0, 3, 1) and res.ssq_trace.shape == (0, 3) and not any(c[-1] for c in stub.calls if c[0] == "mala_run")
    # the caller's start array is not written
    q0a = np.array(q0)
    eng.mala(q0a, data, 0.1, 50.0, 2)
    np.testing.assert_array_equal(q0a, q0)


def test_groups_are_padded_to_whole_workgroups(pkg, stub_engine):
    eng, stub = stub_engine, stub_engine.lib
    data = _data(stub, [2.0, 9.0])
    q0 = np.array([1.5, 2.0, 2.6, 7.0, 9.0, 12.0])
    B = pkg._abi.MAX_BLOCK
    res = eng.mala(q0, data, 0.1, 50.0, 3, seed=2, keep=1)
    assert stub.calls[0] == ("normal", 2 * B, 2, 0) and stub.calls[1] == ("mala_run", 2 * B, 2, 3, 1, True)
    assert res.q.shape == (6, 1) and res.samples.shape == (1, 6, 1) and res.accepted.shape == (6,)
    for g in range(2):  # chain j of series g has the stream offset + g (n / G + pad) + j
        want, _ = _spec_run(stub, q0[3 * g:3 * g + 3], data[g], 0.1, 50.0, 3, seed=2, offset=g * B)
        np.testing.assert_array_equal(res.q[3 * g:3 * g + 3], want["q"])
        np.testing.assert_array_equal(res.accepted[3 * g:3 * g + 3], want["accepted"])


def test_mala_from_residuals(pkg, stub_engine):
    eng, stub = stub_engine, stub_engine.lib
    truth = np.array([[3.0, 0.02, 0.5]])
    data = stub.series(truth)[:, 0] + 1e-2 * np.random.default_rng(6).standard_normal(stub.nout)
    lo, hi = [0.1, -1.0, -5.0], [50.0, 1.0, 5.0]
    q0 = np.array([[3.0, 0.02, 0.5], [3.1, 0.03, 0.45]])
    calls = []

    def res_fn(pts):
        calls.append(pts.shape)
        return (stub.series(pts) - data[:, None]).T

    res = eng.mala_from_residuals(res_fn, q0, lo, hi, 6, 25.0, seed=7, keep=2)
    # one residual call for the starts and one per iteration, a proposal and a decision each, at Philox iterations 1..6
    assert all(s == (8, 3) for s in calls) and len(calls) == 7
    assert [c for c in stub.calls if c[0] == "propose"] == [("propose", 2, it) for it in range(1, 7)]
    assert [c for c in stub.calls if c[0] == "accept"] == [("accept", 2, it) for it in range(1, 7)]
    assert res.iterations.tolist() == [5, 6] and res.samples.shape == (2, 2, 3) and (res.accepted + res.outbox + res.stuck <= 6).all()
    np.testing.assert_array_equal(res.samples[-1], res.q)
    np.testing.assert_array_equal(res.ssq_trace[-1], res.ssq)
    assert res.accepted.sum() > 0 and np.isfinite(res.q).all()
    # the caller's normal equations instead of residuals
    K = np.array([[4.0]])
    fn = lambda p: (1.0 + 4.0 * (p[:, 0] - 1.0) ** 2, (p - 1.0) @ K.T, np.tile(K, (p.shape[0], 1, 1)))
    res = eng.mala_from_residuals(None, [0.9, 1.1], 0.0, 1.3, 3, 12.0, normal_fn=fn)
    np.testing.assert_array_equal(res.ssq, fn(res.q)[0])
    with pytest.raises(ValueError, match="residuals"):
        eng.mala_from_residuals(lambda p: np.zeros(3), q0, lo, hi, 2, 25.0)
    with pytest.raises(ValueError, match="normal_fn"):
        eng.mala_from_residuals(None, [0.9, 1.1], 0.0, 1.3, 3, 12.0, normal_fn=lambda p: (np.zeros(3), np.zeros((2, 1)), np.zeros((2, 1, 1))))
    with pytest.raises(ValueError, match="one of"):
        eng.mala_from_residuals(res_fn, [0.9, 1.1], 0.0, 1.3, 3, 12.0, normal_fn=fn)


def test_argument_errors_before_any_library_call(pkg, cpu_engine):
    """On the checker engine, whose library has no rsf_fit_* or rsf_mala_* at all: each of these is refused in Python."""
    eng = cpu_engine
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.mala([1000.0], np.zeros(50), 0.0, 1e4, 4)
    eng.set_model(pkg.RateStateModel(number_time_steps=50), 1)
    data = np.zeros(eng.nout)
    ok = dict(q0=[1000.0, 2000.0], data=data, lo=0.0, hi=1e4, n_iter=4)
    for kw in (dict(q0=np.full((2, 2), 5.0)),                  # d = 2 has no solve
               dict(q0=np.zeros((0, 1))), dict(q0=np.full((2, 1, 1), 5.0)),
               dict(q0=[0.0, 5.0]), dict(q0=[5.0, 1e4]), dict(q0=[5.0, np.nan]),  # a start on or outside the box
               dict(lo=[0.0, 0.0]), dict(lo=1e4, hi=0.0), dict(hi=np.inf),
               dict(fd_rel_step=0.0), dict(fd_rel_step=np.nan), dict(eps=0.0), dict(eps=np.inf), dict(lam=-1e-3), dict(lam=np.nan),
               dict(shape=0.0), dict(shape=np.inf), dict(n_iter=0), dict(seed=-1), dict(offset=-1),
               dict(iters_per_launch=0), dict(iters_per_launch=65), dict(keep=-1), dict(keep=5), dict(thin=0),
               dict(data=np.zeros(eng.nout + 1)), dict(data=np.zeros((2, 2, eng.nout))),
               dict(q0=[1.0, 2.0, 3.0], data=np.zeros((2, eng.nout)))):  # three chains over two series
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.mala(**args)
    for kw in (dict(q0=np.full((2, 4), 1.0)), dict(lo=1.0, hi=1.0), dict(n_iter=0), dict(shape=None), dict(shape=-1.0), dict(eps=-1.0), dict(keep=3),
               dict(q0=[2.0])):
        args = dict(res_fn=lambda p: np.zeros((p.shape[0], 5)), q0=[1.0], lo=0.0, hi=2.0, n_iter=2, shape=2.5)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.mala_from_residuals(**args)
    # the sampler's front ends
    mc = pkg.MCMC(pkg.RateStateModel(number_time_steps=50), data, 1000.0, ["Uniform", 0.0, 1e4], 1000.0)
    for kw in (dict(n_chains=0), dict(n_iter=0), dict(nburn=4), dict(nburn=-1), dict(thin=0), dict(start="prior")):
        args = dict(n_chains=8, n_iter=4)
        args.update(kw)
        with pytest.raises(ValueError):
            mc.sample_mala(**args)
    from duck_model import DecayModel

    with pytest.raises(TypeError, match="RateStateModel"):
        pkg.MCMC(DecayModel(), data, 4.0, ["Uniform", 0.0, 10.0], 1.0).sample_mala(8, 4, start="qstart")
    problem = pkg.RSF(number_slip_values=2, lowest_slip_value=100.0, largest_slip_value=5000.0, qstart=1000.0, plotfigs=False)
    for kw in (dict(n_chains=0), dict(n_iter=0), dict(nburn=200), dict(thin=0), dict(start="prior")):
        with pytest.raises(ValueError):
            problem.inference_mala(**kw)


def test_low_level_calls_check_the_layout_of_a_state(pkg, stub_engine):
    eng = stub_engine
    n, d = 3, 2
    st = dict(q=np.ones((n, d)), ssq=np.full(n, 2.0), grad=np.full((n, d), 0.1), jtj=np.tile(np.eye(d), (n, 1, 1)))
    cnt = [np.zeros(n, dtype=np.int32) for _ in range(3)]
    box = ([-5.0] * d, [5.0] * d)
    qn, inb, stk = eng.mala_propose(st["q"], st["ssq"], st["grad"], st["jtj"], *box, 12.0)
    assert inb.all() and not stk.any()
    new = dict(ssq_new=np.full(n, 2.0), grad_new=np.arange(6.0).reshape(n, d) * 0.01, jtj_new=np.tile(2.0 * np.eye(d), (n, 1, 1)))
    want = {k: v.copy() for k, v in st.items()}
    eng.mala_accept(*(want[k] for k in ("q", "ssq", "grad", "jtj")), *box, qn, inb, *new.values(), *cnt, 12.0)
    got, cnt2 = {k: v.copy() for k, v in st.items()}, [np.zeros(n, dtype=np.int32) for _ in range(3)]
    eng.mala_accept(*(got[k] for k in ("q", "ssq", "grad", "jtj")), *box, np.asfortranarray(qn), list(inb), list(new["ssq_new"]),
                    np.asfortranarray(new["grad_new"]), new["jtj_new"], *cnt2, 12.0)
    for k in st:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k, bad in (("grad", np.asfortranarray(st["grad"])), ("jtj", st["jtj"][:, :, ::-1]), ("ssq", np.zeros(n + 1)), ("q", [[1.0, 1.0]] * n)):
        args = dict(st)
        args[k] = bad
        with pytest.raises(ValueError, match=k):
            eng.mala_propose(args["q"], args["ssq"], args["grad"], args["jtj"], *box, 12.0)
        with pytest.raises(ValueError, match=k):
            eng.mala_accept(args["q"], args["ssq"], args["grad"], args["jtj"], *box, qn, inb, *new.values(), *cnt, 12.0)
    with pytest.raises(ValueError, match="accepted"):
        eng.mala_accept(*(st[k] for k in ("q", "ssq", "grad", "jtj")), *box, qn, inb, *new.values(), cnt[0].astype(np.int64), cnt[1], cnt[2], 12.0)
    with pytest.raises(ValueError, match="q_new"):
        eng.mala_accept(*(st[k] for k in ("q", "ssq", "grad", "jtj")), *box, qn[:2], inb, *new.values(), *cnt, 12.0)
