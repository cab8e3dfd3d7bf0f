"""
CPU tests of the ensemble sampler's specification (tests/ensemble_reference.py; no GPU): the stretch variate, the partner index and
— what makes the rule a sampler — that a half-step keeps its target, on the closed forms and on a thin curved ridge cut off by its
box, with and without log coordinates.  The runs start from independent draws of pi, so every later state is a draw of pi too if the
rule is right; the island-level statistic (ensemble_reference.island_z) holds them to the quadrature of posterior_reference.
"""
import numpy as np
import pytest

import ensemble_cases as cases
import ensemble_reference as ens
import posterior_reference as R
import smc_reference as smc

_RUNS = {}


def _spec_run(name, mask, size):
    """the specification on target `name` from draws of pi, once per (target, mask, size) → (ref, c, island, {iteration: (q, l, std2)})"""
    key = (name, mask, size)
    if key not in _RUNS:
        islands, island, cps = size
        mk, d, _ = cases.TARGETS[name]
        ref, fn, c = mk()
        rng = np.random.default_rng(cases.SEED)
        q0 = ref.draw(rng, islands * island)
        out = ens.run(cases.rows_fn(fn, d), q0, c["lo"], c["hi"], island // 2, max(cps), c["shape"], logmask=mask, seed=cases.SEED, checkpoints=cps)
        assert (out["stuck"] == 0).all() and 0 < out["accepted"].sum()
        at = {it: (q, l, R.draw_std2(rng, np.exp(-l / c["shape"]), c["shape"])) for it, (q, l) in out["at"].items()}
        _RUNS[key] = (ref, c, island, at)
    return _RUNS[key]


def test_stretch_variate():
    """z = ((a - 1) U + 1)^2 / a on the Philox uniforms: inside [1/a, a], E z = (a^2 + a + 1) / (3 a) (g(z) ~ z^-1/2)"""
    n = 1 << 16
    for a in (2.0, 1.5, 3.0):
        us, ua, _ = ens.draws(7, np.arange(n, dtype=np.uint64), 1, 64)
        z = ens.stretch(us, a)
        assert z.min() > 1.0 / a and z.max() <= a
        mean = (a * a + a + 1.0) / (3.0 * a)
        var = (a ** 4 + a ** 3 + a ** 2 + a + 1.0) / (5.0 * a * a) - mean ** 2
        assert abs(z.mean() - mean) < R.Z_MAX * np.sqrt(var / n)
        # the two uniforms of the accept slot are different words: uncorrelated
        assert abs(np.corrcoef(us, ua)[0, 1]) < R.Z_MAX / np.sqrt(n)
        np.testing.assert_array_equal(ua, smc.accept_uniforms(7, np.arange(n, dtype=np.uint64), 1))


@pytest.mark.parametrize("B", [64, 128, 256])
def test_partner_index(B):
    """always in the other half of the mover's own island, and uniform over its B walkers (chi^2 over B bins)"""
    n = 2 * B * 64
    q, l = np.full((n, 1), 0.5), np.zeros(n)
    counts = np.zeros(B)
    for half in (0, 1):
        for it in (1, 2, 3, 4):
            pr = ens.propose(q, l, [0.0], [1.0], B, 2.0, 0, 3, 1000, it, half, exact=False)
            rows, partner = pr["rows"], pr["partner"]
            assert rows.size == n // 2 and np.unique(rows).size == rows.size
            assert ((rows // B) % 2 == half).all() and ((partner // B) % 2 == 1 - half).all()
            assert (rows // (2 * B) == partner // (2 * B)).all()
            counts += np.bincount(partner % B, minlength=B)
    e = counts.sum() / B
    chi2 = ((counts - e) ** 2 / e).sum()
    # chi^2 with B - 1 degrees of freedom: mean B - 1, variance 2 (B - 1)
    assert abs(chi2 - (B - 1)) < R.Z_MAX * np.sqrt(2.0 * (B - 1)), chi2


def test_exact_fma_is_one_rounding():
    rng = np.random.default_rng(0)
    x, y, z = rng.standard_normal(200), rng.standard_normal(200), rng.standard_normal(200) * 1e-8
    got = ens.fma(x, y, z, True)
    want = np.array([float(np.longdouble(a) * np.longdouble(b) + np.longdouble(c)) for a, b, c in zip(x, y, z)])
    assert (np.abs(got - want) <= np.spacing(np.abs(want))).all()  # long double rounds twice: within one ulp
    assert (got != x * y + z).any()  # and it is not the two-rounding float64 expression


def test_counters_and_stuck_walkers():
    """per half-step exactly one of accepted / outbox / stuck / 'rejected inside' happens to a mover; a stuck walker never moves"""
    B, d = 64, 3
    c = R.CLOSED[3]  # the SSq alone: no quadrature is needed here
    fn = R.quadratic_ssq(c["S0"], c["q0"], c["K"])
    rng = np.random.default_rng(5)
    q = rng.uniform(c["lo"], c["hi"], (4 * B, d))
    q[3] = [20.0, 2.0, 3.0]  # outside the box
    l = ens.start_l(q, cases.rows_fn(fn, d), c["shape"])
    l[70] = -np.inf  # no target value
    q0, cnt = q.copy(), ens.new_counters(q.shape[0])
    for it in (1, 2, 3):
        for half in (0, 1):
            ens.half_step(q, l, cases.rows_fn(fn, d), c["lo"], c["hi"], B, 2.0, 0, c["shape"], 9, 0, it, half, cnt)
    total = cnt["accepted"] + cnt["outbox"] + cnt["stuck"]
    assert (total <= 3).all() and cnt["stuck"][3] == 3 and cnt["stuck"][70] == 3 and cnt["stuck"].sum() == 6
    np.testing.assert_array_equal(q[[3, 70]], q0[[3, 70]])
    moved = (q != q0).any(axis=1)
    assert (moved == (cnt["accepted"] > 0)).all() and cnt["outbox"].sum() > 0


@pytest.mark.parametrize("name,mask", [(n, m) for n, (_, _, masks) in cases.TARGETS.items() for m in masks])
def test_the_rule_keeps_its_target(name, mask):
    ref, c, island, at = _spec_run(name, mask, cases.CPU_SIZE)
    fails = []
    for it, (q, l, std2) in sorted(at.items()):
        assert smc.inbox(q, c["lo"], c["hi"]).all()
        ens.island_check(f"{name} mask {mask:#05b} iteration {it}", ref, R.quantities(q, std2), island, fails, cases.Z_ISLAND)
        R.check(f"pooled {name} mask {mask:#05b} iteration {it}", ref, q, std2, [])  # reported, not asserted at this size
    assert not fails, fails


def test_what_the_gpu_tests_may_assert_of_the_pooled_check():
    """ensemble_cases.POOLED_ASSERTED, re-derived: the specification at the GPU tests' sizes passes check() on the closed forms,
    and on the ridge the reference's own draws already miss its Dc marginal's CDF."""
    for name in ("closed1", "closed3"):
        ref, c, island, at = _spec_run(name, 0, cases.GPU_SSQ_SIZE)
        fails = []
        for it, (q, l, std2) in sorted(at.items()):
            ens.island_check(f"{name} iteration {it}", ref, R.quantities(q, std2), island, fails, cases.Z_ISLAND)
            R.check(f"pooled {name} iteration {it}", ref, q, std2, fails)
        assert (not fails) == cases.POOLED_ASSERTED[name], fails
    ref, fn, c = cases.ridge_reference()
    rng = np.random.default_rng(1)
    islands, island, _ = cases.GPU_SSQ_SIZE
    q = ref.draw(rng, islands * island)
    fails = []
    R.check("the ridge reference's own draws", ref, q, R.draw_std2(rng, fn(*q.T), c["shape"]), fails)
    assert bool(fails) and not cases.POOLED_ASSERTED["ridge"]
