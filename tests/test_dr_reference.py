"""
CPU tests of the delayed-rejection sampler's specification (tests/dr_reference.py; no GPU): that the two-stage rule keeps its
target — on the closed forms from independent draws of pi, held to the quadrature by posterior_reference.check — that the test
has the power to catch a wrong second-stage rule, that one stage is smc_reference.move_step at beta = 1, and the real d = 1 target on
the checker's solve.
"""
import numpy as np
import pytest

import dr_cases as cases
import dr_reference as dr
import posterior_reference as R
import smc_reference as smc
from test_fit_reference import checker_problem


def _leg(d, scale, gamma, mutant=None, use_rng=False):
    """the specification on a closed form from draws of pi → (fails, largest |z|, largest sqrt(C) D, the run)"""
    ref, fn, c = cases.closed_reference(d)
    rng = np.random.default_rng([cases.SEED, d, int(10 * scale)])
    q0 = ref.draw(rng, cases.C_TARGET)
    out = dr.run(cases.rows_fn(fn, d), q0, c["lo"], c["hi"], cases.closed_factor(c, scale), max(cases.CHECKPOINTS), c["shape"], gamma=gamma,
                 seed=cases.SEED, checkpoints=cases.CHECKPOINTS, mutant=mutant, rng=rng if use_rng else None)
    fails, zmax, kmax = [], 0.0, 0.0
    tag = f"closed d {d} scale {scale} gamma {gamma} {mutant or 'the rule'}"
    for it, (q, l) in sorted(out["at"].items()):
        assert smc.inbox(q, c["lo"], c["hi"]).all()
        z, k = R.check(f"{tag} it {it}", ref, q, R.draw_std2(rng, np.exp(-l / c["shape"]), c["shape"]), fails)
        zmax, kmax = max(zmax, z), max(kmax, k)
    n = 8.0 * cases.C_TARGET
    pend = n - out["accepted1"].sum()
    print(f"{tag}: largest |z| {zmax:.2f}, sqrt(C) D {kmax:.2f}; stage 1 accepted {out['accepted1'].sum() / n:.3f}, outside {out['outbox1'].sum() / n:.3f}; "
          f"stage 2 accepted {out['accepted2'].sum() / pend:.3f} of its proposals, outside {out['outbox2'].sum() / pend:.3f}")
    return fails, zmax, kmax, out


@pytest.mark.parametrize("d,scale,gamma", cases.LEGS)
def test_the_rule_keeps_its_target(d, scale, gamma):
    fails, _, _, out = _leg(d, scale, gamma)
    assert out["stuck"].sum() == 0 and out["accepted1"].sum() > 0 and out["accepted2"].sum() > 0
    if (d, scale) == (3, 3.0):
        assert out["outbox1"].sum() > 0.5 * 8 * cases.C_TARGET  # the leg where most first proposals leave the box
    assert not fails, fails


@pytest.mark.parametrize("d,scale,gamma", cases.MUTANT_LEGS)
@pytest.mark.parametrize("mutant", ["no_reject_terms", "no_logq"])
def test_the_target_test_has_power(d, scale, gamma, mutant):
    """the same run with a wrong second-stage rule must FAIL check()"""
    fails, zmax, kmax, _ = _leg(d, scale, gamma, mutant)
    assert fails, f"{mutant} passes at d {d}: largest |z| {zmax:.2f}, sqrt(C) D {kmax:.2f}"


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_one_stage_is_the_smc_move_step(d, dtype):
    c = R.CLOSED[3]
    lo, hi = np.array(c["lo"][:d]), np.array(c["hi"][:d])
    K, q0 = np.asarray(c["K"])[:d, :d], np.asarray(c["q0"])[:d]
    ssq_fn = cases.rows_fn(R.quadratic_ssq(c["S0"], q0, K), d)
    rng = np.random.default_rng(d)
    q = rng.uniform(lo, hi, (1037, d))
    L = 0.5 * np.linalg.cholesky(np.linalg.inv(K) / 20.0)
    qa, qb = q.copy(), q.copy()
    la, lb = dr.start_l(qa, ssq_fn, c["shape"], dtype), smc.log_target(ssq_fn(qb), c["shape"], dtype)
    cnt, moved = dr.new_counters(q.shape[0]), np.zeros(q.shape[0], np.int64)
    for it in (1, 2, 3):
        dr.step(qa, la, ssq_fn, lo, hi, L, 0.2, 1, c["shape"], 11, 5, it, cnt, dtype)
        moved += smc.move_step(qb, lb, ssq_fn, lo, hi, L, 1.0, c["shape"], 11, 5, it, dtype)
        np.testing.assert_array_equal(qa, qb)
        np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(cnt["accepted1"], moved)
    assert moved.sum() > 0 and cnt["outbox1"].sum() > 0 and cnt["accepted2"].sum() == 0 and cnt["outbox2"].sum() == 0 and cnt["stuck"].sum() == 0
    assert dr.n_solves(3, cnt, stages=1) == 3 * q.shape[0] - cnt["outbox1"].sum()


def test_counters_and_stuck_chains():
    """per iteration a chain is stuck, or ends at stage 1 (accepted1), or goes on to stage 2; a stuck chain keeps its bits"""
    d, c = 3, R.CLOSED[3]
    ssq_fn = cases.rows_fn(R.quadratic_ssq(c["S0"], c["q0"], c["K"]), d)
    rng = np.random.default_rng(5)
    q = rng.uniform(c["lo"], c["hi"], (300, d))
    q[3] = [20.0, 2.0, 3.0]
    l = dr.start_l(q, ssq_fn, c["shape"])
    l[70] = -np.inf
    q0, cnt = q.copy(), dr.new_counters(300)
    for it in (1, 2, 3, 4):
        st = dr.step(q, l, ssq_fn, c["lo"], c["hi"], cases.closed_factor(c, 3.0), 0.3, 2, c["shape"], 9, 0, it, cnt)
        assert not (st["acc1"] & st["acc2"]).any() and not (st["pending"] & (st["acc1"] | st["stuck"])).any()
        assert (st["l1"][~st["in1"]] == -np.inf).all()
    assert cnt["stuck"][3] == 4 and cnt["stuck"][70] == 4 and cnt["stuck"].sum() == 8
    np.testing.assert_array_equal(q[[3, 70]], q0[[3, 70]])
    assert ((cnt["accepted1"] + cnt["accepted2"] + cnt["stuck"]) <= 4).all() and ((cnt["outbox2"] + cnt["accepted2"] + cnt["accepted1"] + cnt["stuck"]) <= 4).all()
    assert ((q != q0).any(axis=1) <= (cnt["accepted1"] + cnt["accepted2"] > 0)).all() and cnt["outbox1"].sum() > 0 and cnt["outbox2"].sum() > 0
    solves = []
    dr.run(lambda p: (solves.append(len(p)), ssq_fn(p))[1], q0, c["lo"], c["hi"], cases.closed_factor(c, 3.0), 4, c["shape"], gamma=0.3, seed=9)
    cnt0 = dr.run(ssq_fn, q0, c["lo"], c["hi"], cases.closed_factor(c, 3.0), 4, c["shape"], gamma=0.3, seed=9)
    assert sum(solves[1:]) == dr.n_solves(4, cnt0)  # the first call is the start's


def test_log_q_is_the_gaussian_ratio():
    """log q = log N(y1; y2, L L^T) - log N(y1; q, L L^T), against the densities themselves"""
    rng = np.random.default_rng(2)
    d, n, gamma = 3, 200, 0.3
    A = rng.standard_normal((d, d))
    L = np.linalg.cholesky(A @ A.T + np.eye(d))
    q, z1, z2 = rng.standard_normal((n, d)), rng.standard_normal((n, d)), rng.standard_normal((n, d))
    y1, y2 = smc.propose(q, L, z1, np.float64), dr.stage2_point(q, L, z2, gamma)
    P = np.linalg.inv(L @ L.T)
    quad = lambda a, b: np.einsum("ni,ij,nj->n", a - b, P, a - b)
    np.testing.assert_allclose(dr.log_q(z1, z2, gamma), -0.5 * (quad(y1, y2) - quad(y1, q)), rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(dr.unpack(dr.pack(L), d), L)


def test_specification_keeps_the_real_model_target_on_the_checker(pkg, cpu_engine):
    data, _ = checker_problem(pkg, cpu_engine, 1000.0)
    shape, lo, hi, C = 0.5 * data.size, [0.0], [1.0e4], 4096
    fn = R.checker_ssq(cpu_engine, data)
    ref = R.Posterior1(fn, lo[0], hi[0], shape)
    assert ref.outside < 1e-9, ref.outside
    rng = np.random.default_rng(47)
    fails = []
    L = np.array([[3.0 * ref.marg["Dc"].sd]])  # a deliberately wide factor
    out = dr.run(lambda p: fn(p[:, 0]), ref.draw(rng, C), lo, hi, L, 8, shape, gamma=0.3, seed=47, checkpoints=(4, 8))
    for it, (q, l) in sorted(out["at"].items()):
        R.check(f"checker d 1 it {it}", ref, q, R.draw_std2(rng, np.exp(-l / shape), shape), fails)
    print(f"checker d 1: stage 1 accepted {out['accepted1'].sum() / (8 * C):.3f}, stage 2 accepted {out['accepted2'].sum() / (8 * C):.3f}")
    assert out["stuck"].sum() == 0 and out["accepted2"].sum() > 0
    assert not fails, fails


@pytest.mark.parametrize("d", [1, 2, 3])
def test_the_crafted_rows_of_the_split_path_meet_every_ending(d):
    """tests/test_gpu_dr.py's split-path problem on the specification alone: every crafted ending occurs, and no crafted row decides
    within the tie band"""
    prob = cases.split_problem(d)
    q = prob["q0"].copy()
    l = dr.start_l(q, prob["fn"], prob["shape"])
    for r, v in prob["bad_l"].items():
        l[r] = v
    cnt, steps = dr.new_counters(q.shape[0]), []
    crafted = np.arange(cases.SPLIT_N, q.shape[0])
    for it in range(1, cases.SPLIT_ITERS + 1):
        st = dr.step(q, l, prob["fn"], prob["lo"], prob["hi"], prob["L"], cases.SPLIT_GAMMA, 2, prob["shape"], cases.SPLIT_SEED, cases.SPLIT_OFFSET, it, cnt,
                     fix=prob["fix"])
        steps.append(st)
        m1 = np.abs(st["margin1"][crafted][st["in1"][crafted]])
        m2 = np.abs(st["margin2"][crafted][st["in2"][crafted] & ~st["rejected2"][crafted]])
        assert not (m1 <= 1e-9).any() and not (m2 <= 1e-9).any()
    assert cases.split_coverage(d, steps, prob) == []
    assert cnt["accepted1"][:cases.SPLIT_N].sum() > 0 and cnt["accepted2"][:cases.SPLIT_N].sum() > 0
