"""
CPU tests of the Python layer of the delayed-rejection sampler (Engine.dr, Engine.dr_from_ssq, DrResult, MCMC.sample_dr,
RSF.inference_dr): the prototype table against the header, the argument errors raised before any library call, the stuck start
refused, the launch loop — the iterations and the Philox iteration each rsf_dr_run gets, which launches are traced, the rows keep
and thin select, the observation groups and their factors — the adaptation formula against NumPy on a recorded trace, and the
n_solves bookkeeping, driven through a STUB library: test_fit_host's (the checker's library and a closed-form model) plus
rsf_evidence_logtarget, rsf_smc_std2, rsf_pool_joint_partials and rsf_dr_run / _propose / _accept written in Python from the
specification (tests/dr_reference.py).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import dr_reference as dr
import joint_reference as J
from test_fit_host import StubLib, _view

B = 64  # the stub engine's workgroup size
NAMES = ("accepted1", "accepted2", "outbox1", "outbox2", "stuck")


class DrStub(StubLib):
    """... `calls` records ("logtarget", n), ("dr_run", n, n_groups, n_iter, iter0, traced, the factors), ("propose", n, iteration,
    stage) and ("accept", n, iteration, stage)"""

    def __getattr__(self, name):
        return getattr(self._hip if name in ("rsf_fit_laplace", "rsf_pool_joint_finish") else self._lib, name)

    def ssq(self, pts, obs):
        return ((self.series(pts) - np.asarray(obs)[:, None]) ** 2).sum(axis=0)

    def rsf_evidence_logtarget(self, ctx, n, d, theta, data, shape, lo, hi, tr, logg, l):
        self.calls.append(("logtarget", n))
        _view(l, (n,))[:] = dr.start_l(_view(theta, (n, d)), lambda p: self.ssq(p, _view(data, (self.nout,))), shape) - _view(logg, (n,))
        return 0

    def rsf_smc_std2(self, ctx, n, l, shape, seed, offset, it, out):
        self.calls.append(("std2", n, it))
        _view(out, (n,))[:] = 0.5 * np.exp(-_view(l, (n,)) / shape) / shape
        return 0

    def rsf_pool_joint_partials(self, ctx, n, d, x, center, out):
        for k, v in enumerate(J.partials(_view(x, (n, d)), np.array(center[:d]))):
            out[k] = float(v)
        return 0

    def rsf_dr_run(self, ctx, n, d, q, l, data, G, lo, hi, chol, gamma, stages, shape, seed, offset, iter0, n_iter, a1, a2, o1, o2, stuck, tq, tl):
        ne = d * (d + 1) // 2
        Ls = [dr.unpack(chol[g * ne:(g + 1) * ne], d) for g in range(G)]
        self.calls.append(("dr_run", n, G, n_iter, iter0, tq is not None, np.array(Ls)))
        qv, lv = _view(q, (n, d)), _view(l, (n,))
        cnt = dict(zip(NAMES, (_view(c, (n,), np.int32) for c in (a1, a2, o1, o2, stuck))))
        obs, per = _view(data, (G, self.nout)), n // G
        blo, bhi = np.array(lo[:d]), np.array(hi[:d])
        for k in range(n_iter):
            for g in range(G):
                s = slice(g * per, (g + 1) * per)
                sub = {key: v[s] for key, v in cnt.items()}
                qs, ls = qv[s], lv[s]
                dr.step(qs, ls, lambda p: self.ssq(p, obs[g]), blo, bhi, Ls[g], gamma, stages, shape, seed, offset + g * per, iter0 + k, sub)
            if tq is not None:
                _view(tq, (n_iter, n, d))[k], _view(tl, (n_iter, n))[k] = qv, lv
        return 0

    def rsf_dr_propose(self, ctx, n, d, q, l, G, lo, hi, chol, gamma, stage, seed, offset, it, pending, y, mask):
        self.calls.append(("propose", n, it, stage))
        assert G == 1
        qv, lv, L = _view(q, (n, d)), _view(l, (n,)), dr.unpack(chol[:d * (d + 1) // 2], d)
        if stage == 1:
            # the specification's whole iteration on a copy, with every SSq 1: its first stage's proposals do not depend on them
            self._st = dr.step(qv.copy(), lv.copy(), lambda p: np.ones(len(p)), np.array(lo[:d]), np.array(hi[:d]), L, gamma, 2, 1.0, seed, offset, it,
                               dr.new_counters(n))
            _view(y, (n, d))[:], _view(mask, (n,), np.uint8)[:] = self._st["y1"], self._st["in1"]
        else:
            pend = _view(pending, (n,), np.uint8).astype(bool)
            ids = (offset + np.arange(n)).astype(np.uint64)
            y2 = dr.stage2_point(qv, L, dr.normals2(seed, ids, it, d), gamma)
            y2[~pend] = qv[~pend]
            _view(y, (n, d))[:] = y2
            _view(mask, (n,), np.uint8)[:] = pend & dr.smc.inbox(y2, np.array(lo[:d]), np.array(hi[:d]))
        return 0

    def rsf_dr_accept(self, ctx, n, d, q, l, lo, hi, gamma, stage, shape, seed, offset, it, y, mask, ssq, l1, pending, a1, a2, o1, o2, stuck):
        self.calls.append(("accept", n, it, stage))
        qv, lv, yv = _view(q, (n, d)), _view(l, (n,)), _view(y, (n, d))
        m, s = _view(mask, (n,), np.uint8).astype(bool), _view(ssq, (n,))
        ids = (offset + np.arange(n)).astype(np.uint64)
        u1, u2 = dr.uniforms(seed, ids, it)
        ln = np.where(m, dr.smc.log_target(np.where(m, s, 1.0), shape, np.float64), -np.inf)
        if stage == 1:
            ok = dr.smc.inbox(qv, np.array(lo[:d]), np.array(hi[:d])) & np.isfinite(lv)
            with np.errstate(invalid="ignore"):
                acc = m & dr.accept_test(np.where(m, ln - lv, -np.inf), np.log(u1))
            _view(l1, (n,))[:], _view(pending, (n,), np.uint8)[:] = ln, ok & ~acc
            _view(a1, (n,), np.int32)[acc] += 1
            _view(stuck, (n,), np.int32)[~ok] += 1
            _view(o1, (n,), np.int32)[ok & ~m] += 1
        else:
            pend = _view(pending, (n,), np.uint8).astype(bool)
            lq = dr.log_q(dr.smc.normals(seed, ids, it, d), dr.normals2(seed, ids, it, d), gamma)
            la, out = dr.log_alpha2(lv, _view(l1, (n,)), ln, lq)
            acc = m & ~out & dr.accept_test(la, np.log(u2))
            _view(a2, (n,), np.int32)[acc] += 1
            _view(o2, (n,), np.int32)[pend & ~m] += 1
        qv[acc], lv[acc] = yv[acc], ln[acc]
        return 0


@pytest.fixture()
def stub_engine(pkg, oracle_lib):
    eng = pkg.Engine(lib=DrStub(oracle_lib, 50, pkg), block_threads=B)
    eng.set_model(pkg.RateStateModel(number_time_steps=50), 1)
    yield eng
    eng.close()


def _data(stub, truths, seed=4):
    rng = np.random.default_rng(seed)
    return np.stack([stub.series(np.array([[t]]))[:, 0] + 1e-2 * rng.standard_normal(stub.nout) for t in truths])


def _starts(n, seed=1):
    return np.random.default_rng(seed).uniform(1.5, 2.5, (n, 1))


def test_header_and_prototype_table_declare_the_same_symbols(pkg):
    abi = pkg._abi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rsf_dr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(rsf_dr_\w+)\s*\(([^;]*)\)\s*;", code)}
    assert sorted(decl) == sorted(abi.DR_PROTOTYPES) == ["rsf_dr_accept", "rsf_dr_propose", "rsf_dr_run", "rsf_dr_ssq"]
    for name, args in decl.items():
        assert len(args.split(",")) == len(abi.DR_PROTOTYPES[name][1]), name
    assert len(abi.DR_PROTOTYPES["rsf_dr_run"][1]) == 24 and len(abi.DR_PROTOTYPES["rsf_dr_propose"][1]) == 17
    assert len(abi.DR_PROTOTYPES["rsf_dr_accept"][1]) == 23 and len(abi.DR_PROTOTYPES["rsf_dr_ssq"][1]) == 8
    assert all(rt is ctypes.c_int for rt, _ in abi.DR_PROTOTYPES.values())
    for macro, value in (("RSF_DR_MAX_ITER", abi.DR_MAX_ITER), ("RSF_DR_MAX_GROUPS", abi.DR_MAX_GROUPS), ("RSF_DR_MAX_PARAMS", abi.DR_MAX_PARAMS)):
        assert int(re.search(rf"#define {macro} (\d+)", code).group(1)) == value
    assert abi.DR_MAX_ITER == 64 and abi.DR_MAX_GROUPS == 64
    lib = abi.load()  # the product library exports them, typed by the table
    for name, (_, argtypes) in abi.DR_PROTOTYPES.items():
        assert list(getattr(lib, name).argtypes) == argtypes, name
    assert {"DrResult"} <= set(pkg.__all__)


def test_launch_loop_keep_and_thin(pkg, stub_engine):
    eng, stub = stub_engine, stub_engine.lib
    data = _data(stub, [2.0])[0]
    q0 = _starts(100)  # one group: any number of chains
    res = eng.dr(q0, data, 0.1, 50.0, 0.4, 11, gamma=0.3, seed=5, offset=3, iters_per_launch=4, keep=6, thin=2)
    want = dr.run(lambda p: stub.ssq(p, data), q0, [0.1], [50.0], [[0.4]], 11, 25.0, gamma=0.3, seed=5, offset=3, checkpoints=range(1, 12))
    runs = [c[:6] for c in stub.calls if c[0] == "dr_run"]
    # the start's l in one call, launches of 4, 4 and 3 at Philox iterations 1, 5 and 9; the launches that reach the last 6 iterations are traced
    assert stub.calls[0] == ("logtarget", 100) and runs == [("dr_run", 100, 1, 4, 1, False), ("dr_run", 100, 1, 4, 5, True), ("dr_run", 100, 1, 3, 9, True)]
    for k in ("q", "l") + NAMES:
        np.testing.assert_array_equal(getattr(res, k), want[k], err_msg=k)
    assert res.n_iter == 11 and res.shape == 25.0 and res.gamma == 0.3 and res.stages == 2 and res.chol.shape == (1, 1, 1) and res.chol[0, 0, 0] == 0.4
    assert res.accepted1.sum() > 0 and res.accepted2.sum() > 0 and res.stuck.sum() == 0
    assert res.accept_rate == (want["accepted1"].sum() + want["accepted2"].sum()) / (11 * 100)
    assert res.iterations.tolist() == [6, 8, 10] and res.trace_q.shape == (3, 100, 1) and res.trace_l.shape == (3, 100)
    for r, it in enumerate(res.iterations):
        np.testing.assert_array_equal(res.trace_q[r], want["at"][it][0])
        np.testing.assert_array_equal(res.trace_l[r], want["at"][it][1])
    stub.calls.clear()
    assert res.std2(engine=eng).shape == (100,) and res.std2(engine=eng, kept=True).shape == (3, 100)
    assert [c[2] for c in stub.calls if c[0] == "std2"] == [11, 6, 8, 10]  # sigma^2 at each state's own Philox iteration
    # n_solves: the counter identity, and the solves the specification made
    solves = []
    dr.run(lambda p: (solves.append(len(p)), stub.ssq(p, data))[1], q0, [0.1], [50.0], [[0.4]], 11, 25.0, gamma=0.3, seed=5, offset=3)
    c = {k: getattr(res, k).astype(np.int64) for k in NAMES}
    assert res.n_solves == sum(solves[1:]) == int((11 - c["stuck"] - c["outbox1"]).sum() + (11 - c["stuck"] - c["accepted1"] - c["outbox2"]).sum())
    one = eng.dr(q0, data, 0.1, 50.0, 0.4, 11, gamma=0.3, stages=1, seed=5, offset=3)
    assert one.accepted2.sum() == 0 and one.n_solves == int((11 - one.outbox1.astype(np.int64)).sum()) and one.accept_rates[1] == 0.0
    # a continuation: the state, the factor and the next Philox iteration give the rows of the whole run
    head = eng.dr(q0, data, 0.1, 50.0, 0.4, 7, gamma=0.3, seed=5, offset=3)
    stub.calls.clear()
    tail = eng.dr(head.q, data, 0.1, 50.0, head.chol, 4, gamma=0.3, seed=5, offset=3, iter0=8, l0=head.l)
    assert not any(c[0] == "logtarget" for c in stub.calls) and tail.iterations.tolist() == [8, 9, 10, 11]
    np.testing.assert_array_equal(tail.q, want["q"])
    np.testing.assert_array_equal(tail.trace_q[2], want["at"][10][0])
    # keep = 0 keeps none and traces nothing; the caller's start array is not written
    stub.calls.clear()
    q0a = q0.copy()
    res = eng.dr(q0a, data, 0.1, 50.0, 0.4, 5, keep=0)
    assert res.trace_q.shape == (0, 100, 1) and not any(c[5] for c in stub.calls if c[0] == "dr_run")
    np.testing.assert_array_equal(q0a, q0)


def test_observation_groups_have_their_own_factors(pkg, stub_engine):
    eng, stub = stub_engine, stub_engine.lib
    data = _data(stub, [2.0, 9.0])
    q0 = np.concatenate([_starts(B, 1), 4.5 * _starts(B, 2)])
    L = np.array([[[0.4]], [[1.5]]])
    res = eng.dr(q0, data, 0.1, 50.0, L, 3, seed=2, keep=1)
    assert [c[:6] for c in stub.calls] == [("logtarget", B), ("logtarget", B), ("dr_run", 2 * B, 2, 3, 1, True)]
    np.testing.assert_array_equal(stub.calls[-1][6], L)
    for g in range(2):  # chain j of series g has the stream offset + g n / G + j and the factor g
        s = slice(g * B, (g + 1) * B)
        want = dr.run(lambda p: stub.ssq(p, data[g]), q0[s], [0.1], [50.0], L[g], 3, 25.0, seed=2, offset=g * B)
        np.testing.assert_array_equal(res.q[s], want["q"])
        np.testing.assert_array_equal(res.accepted2[s], want["accepted2"])
    one = eng.dr(q0, data, 0.1, 50.0, 0.4, 3, seed=2)  # one factor for every group
    np.testing.assert_array_equal(one.chol, np.full((2, 1, 1), 0.4))
    with pytest.raises(ValueError, match="whole workgroups"):
        eng.dr(q0[:B + 10], data, 0.1, 50.0, L, 3)
    with pytest.raises(ValueError, match="factors"):
        eng.dr(q0, data[0], 0.1, 50.0, L, 3)


def test_adaptation_formula_on_a_recorded_trace(pkg, stub_engine):
    eng, stub = stub_engine, stub_engine.lib
    data = _data(stub, [2.0, 9.0])
    q0 = np.concatenate([_starts(B, 1), 4.5 * _starts(B, 2)])
    L0 = np.array([[[0.4]], [[1.5]]])
    res = eng.dr(q0, data, 0.1, 50.0, L0, 14, seed=2, iters_per_launch=4, adapt_launches=2)
    factors = [c[6] for c in stub.calls if c[0] == "dr_run"]
    traced = [c[5] for c in stub.calls if c[0] == "dr_run"]
    assert traced == [True] * 4 and len(factors) == 4
    np.testing.assert_array_equal(factors[0], L0)
    # after launch k the factor of group g is the formula on every state traced so far in that group, pooled over chains and iterations
    for k in (1, 2):
        for g in range(2):
            states = res.trace_q[:4 * k, g * B:(g + 1) * B].reshape(-1, 1)
            want = dr.adapted_factor(states, [0.1], [50.0], L0[g])
            np.testing.assert_allclose(factors[k][g], want, rtol=1e-12)
            np.testing.assert_allclose(want[0, 0] ** 2, 2.38 ** 2 * states.var(ddof=1) + (1e-6 * 49.9) ** 2, rtol=1e-12)
    # then frozen
    np.testing.assert_array_equal(factors[3], factors[2])
    np.testing.assert_array_equal(res.chol, factors[2])
    assert not np.array_equal(factors[1], factors[0]) and not np.array_equal(factors[2], factors[1])
    # the old factor is kept when the matrix has no Cholesky factor
    old = np.array([[2.0, 0.0], [0.5, 1.0]])
    bad = np.column_stack([np.linspace(0.0, 1.0, 50), np.full(50, np.nan)])
    np.testing.assert_array_equal(eng.dr_adapted_factor(bad, [0.0, 0.0], [1.0, 1.0], old), old)
    x = np.random.default_rng(3).standard_normal((500, 2)) @ np.array([[1.0, 0.3], [0.0, 0.2]])
    np.testing.assert_allclose(eng.dr_adapted_factor(x, [-5.0, -5.0], [5.0, 5.0], old), dr.adapted_factor(x, [-5.0, -5.0], [5.0, 5.0], old), rtol=1e-10)


def test_dr_from_ssq(pkg, stub_engine):
    eng, stub = stub_engine, stub_engine.lib
    lo, hi = [0.1, 0.2, 0.0], [4.0, 3.0, 1.0]
    rng = np.random.default_rng(8)
    q0 = rng.uniform(lo, hi, (150, 3))
    L = np.array([[0.8, 0.0, 0.0], [-0.3, 0.5, 0.0], [0.1, 0.05, 0.3]])
    calls = []

    def ssq_fn(pts):
        calls.append(pts.shape)
        return 1.0 + 30.0 * (pts[:, 0] * pts[:, 1] - 1.0) ** 2 + (pts[:, 2] - 0.5) ** 2

    res = eng.dr_from_ssq(ssq_fn, q0, lo, hi, L, 4, 12.0, gamma=0.25, seed=7, keep=2)
    solves = sum(c[0] for c in calls[1:])
    assert calls[0] == (150, 3) and len(calls) <= 9 and all(s[0] <= 150 and s[1] == 3 for s in calls[1:])
    assert [c for c in stub.calls if c[0] == "propose"] == [("propose", 150, it, st) for it in range(1, 5) for st in (1, 2)]
    assert [c for c in stub.calls if c[0] == "accept"] == [("accept", 150, it, st) for it in range(1, 5) for st in (1, 2)]
    want = dr.run(ssq_fn, q0, lo, hi, L, 4, 12.0, gamma=0.25, seed=7, checkpoints=(3, 4))
    for k in ("q", "l") + NAMES:
        np.testing.assert_array_equal(getattr(res, k), want[k], err_msg=k)
    assert res.iterations.tolist() == [3, 4] and res.trace_q.shape == (2, 150, 3)
    np.testing.assert_array_equal(res.trace_q[0], want["at"][3][0])
    assert res.accepted1.sum() > 0 and res.accepted2.sum() > 0 and res.outbox1.sum() > 0 and res.n_solves == solves
    stub.calls.clear()
    one = eng.dr_from_ssq(ssq_fn, q0, lo, hi, L, 2, 12.0, stages=1)
    assert [c[3] for c in stub.calls if c[0] == "propose"] == [1, 1] and one.accepted2.sum() == 0
    with pytest.raises(ValueError, match="returned"):
        eng.dr_from_ssq(lambda p: np.zeros(3), q0, lo, hi, L, 2, 12.0)
    with pytest.raises(ValueError, match="shape"):
        eng.dr_from_ssq(ssq_fn, q0, lo, hi, L, 2, None)
    with pytest.raises(ValueError, match="stuck start: 1 walkers"):
        eng.dr_from_ssq(lambda p: np.where(np.arange(p.shape[0]) == 5, np.inf, 1.0), q0, lo, hi, L, 2, 12.0)


def test_the_stuck_start_is_refused(pkg, stub_engine):
    eng, stub = stub_engine, stub_engine.lib
    data = _data(stub, [2.0])[0]
    q0 = _starts(70)
    bad = q0.copy()
    bad[17] = 60.0  # outside the box: refused before any library call
    with pytest.raises(ValueError, match="stuck start"):
        eng.dr(bad, data, 0.1, 50.0, 0.4, 3)
    assert stub.calls == []
    nodata = data.copy()
    nodata[3] = np.nan  # inside the box but without a finite target value: refused after the start's l, before any move
    with pytest.raises(ValueError, match="stuck start"):
        eng.dr(q0, nodata, 0.1, 50.0, 0.4, 3)
    assert stub.calls == [("logtarget", 70)]


def test_argument_errors_before_any_library_call(pkg, cpu_engine):
    """On the checker engine, whose library has no rsf_dr_* at all: each of these is refused in Python."""
    eng = cpu_engine
    n = 300
    with pytest.raises(pkg.RsfError, match="set_model"):
        eng.dr(np.full(n, 1000.0), np.zeros(50), 0.0, 1e4, 30.0, 4)
    eng.set_model(pkg.RateStateModel(number_time_steps=50), 1)
    data = np.zeros(eng.nout)
    q0 = np.linspace(900.0, 1100.0, n)
    ok = dict(q0=q0, data=data, lo=0.0, hi=1e4, chol=30.0, n_iter=4)
    edge = q0.copy()
    edge[3] = 1e4
    for kw in (dict(q0=np.full((n, 2), 5.0), chol=np.eye(2)),  # d = 2 has no solve
               dict(q0=np.zeros((0, 1))), dict(q0=np.full((n, 1, 1), 5.0)),
               dict(q0=edge), dict(q0=np.where(np.arange(n) == 0, np.nan, q0)),  # a chain on or outside the box
               dict(lo=[0.0, 0.0]), dict(lo=1e4, hi=0.0), dict(hi=np.inf),
               dict(gamma=0.0), dict(gamma=1.01), dict(gamma=-0.5), dict(gamma=np.nan), dict(gamma=np.inf),
               dict(stages=0), dict(stages=3),
               dict(chol=0.0), dict(chol=-1.0), dict(chol=np.inf), dict(chol=np.nan), dict(chol=np.eye(2)), dict(chol=np.ones((2, 1, 1))),
               dict(shape=0.0), dict(shape=np.inf), dict(n_iter=0), dict(seed=-1), dict(offset=-1), dict(iter0=0), dict(iter0=2 ** 32),
               dict(iters_per_launch=0), dict(iters_per_launch=65), dict(keep=-1), dict(keep=5), dict(thin=0), dict(adapt_launches=-1),
               dict(l0=np.zeros(n - 1)),
               dict(data=np.zeros(eng.nout + 1)), dict(data=np.zeros((2, 2, eng.nout))), dict(data=np.zeros((65, eng.nout))),
               dict(data=np.zeros((2, eng.nout)))):           # 150 chains per series: not whole workgroups
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.dr(**args)
    q3 = np.tile([1000.0, 0.01, 0.015], (n, 1))
    for chol in (np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), np.diag([1.0, 0.0, 1.0]), np.eye(2), 1.0):
        with pytest.raises(ValueError, match="chol"):
            eng.dr(q3, data, [0.0, 0.005, 0.005], [1e4, 0.02, 0.03], chol, 4)
    for kw in (dict(q0=np.full((n, 4), 1.0), chol=np.eye(4)), dict(lo=1.0, hi=1.0), dict(n_iter=0), dict(shape=None), dict(shape=-1.0), dict(gamma=0.0),
               dict(stages=3), dict(keep=3), dict(chol=np.ones((2, 1, 1))), dict(chol=-1.0)):
        args = dict(ssq_fn=lambda p: np.ones(p.shape[0]), q0=np.full(n, 1.0), lo=0.0, hi=2.0, chol=0.5, n_iter=2, shape=2.5)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.dr_from_ssq(**args)
    # the sampler's front ends
    mc = pkg.MCMC(pkg.RateStateModel(number_time_steps=50), data, 1000.0, ["Uniform", 0.0, 1e4], 1000.0)
    for kw in (dict(n_chains=0), dict(n_iter=0), dict(nburn=4), dict(nburn=-1), dict(thin=0), dict(start="prior"), dict(factor="am"), dict(iters_per_launch=0)):
        args = dict(n_chains=8, n_iter=4)
        args.update(kw)
        with pytest.raises(ValueError):
            mc.sample_dr(**args)
    from duck_model import DecayModel

    with pytest.raises(TypeError, match="RateStateModel"):
        pkg.MCMC(DecayModel(), data, 4.0, ["Uniform", 0.0, 10.0], 1.0).sample_dr(8, 4)
    problem = pkg.RSF(number_slip_values=2, lowest_slip_value=100.0, largest_slip_value=5000.0, qstart=1000.0, plotfigs=False)
    for kw in (dict(n_chains=0), dict(n_iter=0), dict(nburn=200), dict(thin=0), dict(start="prior"), dict(factor="am")):
        with pytest.raises(ValueError):
            problem.inference_dr(**kw)


def test_low_level_calls_check_the_layout_of_a_state(pkg, stub_engine):
    eng = stub_engine
    n, d = 70, 2
    rng = np.random.default_rng(2)
    st = dict(q=rng.uniform(1.0, 2.0, (n, d)), l=np.zeros(n))
    cnt = [np.zeros(n, dtype=np.int32) for _ in range(5)]
    box, L = ([0.5] * d, [5.0] * d), np.array([[0.5, 0.0], [0.1, 0.4]])
    y, m = eng.dr_propose(st["q"], st["l"], *box, L, 1)
    assert y.shape == (n, d) and m.any()
    l1, pend = eng.dr_accept(st["q"], st["l"], *box, 1, y, m, np.ones(n), cnt, 12.0)
    assert l1.shape == (n,) and pend.shape == (n,) and pend.dtype == np.uint8
    with pytest.raises(ValueError, match="l1 and pending"):
        eng.dr_accept(st["q"], st["l"], *box, 2, y, m, np.ones(n), cnt, 12.0)
    for k, bad in (("q", np.asfortranarray(st["q"])), ("l", np.zeros(n + 1)), ("q", [[1.0, 1.0]] * n)):
        args = dict(st)
        args[k] = bad
        with pytest.raises(ValueError, match=k):
            eng.dr_propose(args["q"], args["l"], *box, L, 1)
        with pytest.raises(ValueError, match=k):
            eng.dr_accept(args["q"], args["l"], *box, 1, y, m, np.ones(n), cnt, 12.0)
    with pytest.raises(ValueError, match="accepted1"):
        eng.dr_accept(st["q"], st["l"], *box, 1, y, m, np.ones(n), [cnt[0].astype(np.int64)] + cnt[1:], 12.0)
    with pytest.raises(ValueError, match="counters"):
        eng.dr_accept(st["q"], st["l"], *box, 1, y, m, np.ones(n), cnt[:3], 12.0)
    with pytest.raises(ValueError, match="y is"):
        eng.dr_accept(st["q"], st["l"], *box, 1, y[:2], m, np.ones(n), cnt, 12.0)
