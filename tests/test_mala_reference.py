"""
CPU tests of the specification of the Gauss-Newton manifold MALA sampler (tests/mala_reference.py): it keeps the closed-form
targets of tests/posterior_reference.py under a metric that depends on the position, it keeps the real model's d = 1 target on the
checker's solve, and a chain that cannot propose keeps its bits.  Every test prints what it measured before it asserts.
"""
import numpy as np
import pytest

import fit_reference as F
import mala_reference as M
import posterior_reference as R
from test_fit_reference import checker_problem

_REFS = {}


def closed(d):
    if d not in _REFS:
        _REFS[d] = R.closed_reference(d)
    return _REFS[d]


def closed_normal(c, fn, position_dependent):
    """the normal equations of a closed form: ssq its quadratic, g = K (q - q0), H = K, or K (1 + 0.5 sin 3 q_0)^2 — a metric that
    depends on the position (any deterministic symmetric positive definite function of q is a valid one)"""
    K, q0 = np.asarray(c["K"], dtype=np.float64), np.asarray(c["q0"], dtype=np.float64)

    def normal(q):
        q = np.asarray(q, dtype=np.float64)
        f = (1.0 + 0.5 * np.sin(3.0 * q[:, 0])) ** 2 if position_dependent else np.ones(q.shape[0])
        return fn(*q.T), (q - q0) @ K.T, K[None] * f[:, None, None]

    return normal


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("eps", [0.5, 1.0])
@pytest.mark.parametrize("lam,position_dependent", [(0.0, False), (1e-3, True)])
def test_specification_keeps_the_closed_form_targets(d, eps, lam, position_dependent):
    ref, fn, c = closed(d)
    C, shape = 65536, c["shape"]
    rng = np.random.default_rng([41, d, int(10 * eps), int(position_dependent)])
    fails = []
    tag = f"closed d {d} eps {eps} lam {lam}"

    def at(it, st):
        R.check(f"{tag} it {it}", ref, st["q"], R.draw_std2(rng, st["ssq"], shape), fails)

    st = M.run(closed_normal(c, fn, position_dependent), ref.draw(rng, C), c["lo"], c["hi"], 8, eps, lam, shape, rng, (4, 8), at)
    print(f"{tag}: accepted {st['accepted'].sum() / (8 * C):.3f}, outside the box {st['outbox'].sum() / (8 * C):.3f}, stuck {int(st['stuck'].sum())}")
    assert st["stuck"].sum() == 0 and (st["accepted"] + st["outbox"] <= 8).all()
    assert not fails, fails


def test_specification_keeps_the_real_model_target_on_the_checker(pkg, cpu_engine):
    data, solve = checker_problem(pkg, cpu_engine, 1000.0)
    shape, lo, hi, C = 0.5 * data.size, [0.0], [1.0e4], 4096
    ref = R.Posterior1(R.checker_ssq(cpu_engine, data), lo[0], hi[0], shape)
    assert ref.outside < 1e-9, ref.outside
    rng = np.random.default_rng(43)
    fails = []

    def at(it, st):
        R.check(f"checker d 1 it {it}", ref, st["q"], R.draw_std2(rng, st["ssq"], shape), fails)

    st = M.run(lambda p: F.normal(solve, p, data, 1e-6), ref.draw(rng, C), lo, hi, 8, 1.0, 1e-3, shape, rng, (4, 8), at)
    print(f"checker d 1: accepted {st['accepted'].sum() / (8 * C):.3f}, outside the box {int(st['outbox'].sum())}, stuck {int(st['stuck'].sum())}")
    assert st["stuck"].sum() == 0
    assert not fails, fails


def test_a_chain_that_cannot_propose_keeps_its_bits():
    # chains 0-3: a metric that does not factor (a diagonal that is zero, negative, NaN, infinite); 4: an ssq that is not finite;
    # 5: an ssq of zero; 6: an ordinary chain, whose proposal's sums are not finite (rejected); 7: the same chain, whose trial
    # metric does not factor (rejected)
    n = 8
    q = np.full((n, 1), 0.7)
    ssq = np.array([1.0, 1.0, 1.0, 1.0, np.inf, 0.0, 1.0, 1.0])
    g = np.full((n, 1), 0.25)
    H = np.array([0.0, -1.0, np.nan, np.inf, 4.0, 4.0, 4.0, 4.0]).reshape(n, 1, 1)
    st = M.new_state(q, ssq, g, H)
    before = {k: v.copy() for k, v in st.items()}
    rng = np.random.default_rng(3)

    def normal(p):
        return np.array([1.0] * 6 + [np.nan, 1.0]), np.full((n, 1), 0.1), np.array([4.0] * 7 + [-4.0]).reshape(n, 1, 1)

    for it in range(5):
        out = M.iterate(normal, st, rng.standard_normal((n, 1)), 1.0 - rng.uniform(size=n), [0.0], [1.3], 0.05, 1e-3, 12.0)
        assert out["stuck"].tolist() == [True] * 6 + [False] * 2 and not out["accepted"].any()
        assert np.array_equal(out["qn"][:6], q[:6])  # a chain without a proposal announces its own point
    for k in ("q", "ssq", "g", "H"):
        assert st[k].tobytes() == before[k].tobytes(), k
    assert st["stuck"].tolist() == [5] * 6 + [0] * 2 and st["accepted"].sum() == 0
    assert (st["outbox"][:6] == 0).all() and (st["outbox"][6:] <= 5).all()


def test_the_proposal_is_the_stated_gaussian():
    # the mean is q + (eps^2 / 2) delta and the covariance eps^2 (ssq / 2 shape) A^-1: 200 000 draws at one state
    rng = np.random.default_rng(9)
    C, d, eps, lam, shape = 200000, 3, 0.8, 1e-3, 12.0
    K = np.asarray(R.CLOSED[3]["K"], dtype=np.float64)
    q, g = np.array([1.2, 2.1, 2.9]), np.array([0.3, -0.2, 0.1])
    qn, inbox, stuck, _ = M.propose(np.tile(q, (C, 1)), np.full(C, 1.7), np.tile(g, (C, 1)), np.tile(K, (C, 1, 1)), rng.standard_normal((C, d)),
                                    [-1e9] * 3, [1e9] * 3, eps, lam, shape)
    A = K + lam * np.diag(np.diag(K))
    mean, cov = q - 0.5 * eps ** 2 * np.linalg.solve(A, g), eps ** 2 * 1.7 / (2 * shape) * np.linalg.inv(A)
    zm = np.abs(qn.mean(axis=0) - mean) / np.sqrt(np.diag(cov) / C)
    sd = np.sqrt(np.diag(cov))
    rc = (np.abs(np.cov(qn.T) - cov) / np.outer(sd, sd)).max()
    print(f"proposal: mean z {zm.tolist()}, covariance error over sqrt(c_pp c_rr) {rc:.2e}")
    # a sample covariance entry has variance (c_pp c_rr + c_pr^2) / C <= 2 c_pp c_rr / C
    assert inbox.all() and not stuck.any() and zm.max() < R.Z_MAX and rc < R.Z_MAX * np.sqrt(2.0 / C)
