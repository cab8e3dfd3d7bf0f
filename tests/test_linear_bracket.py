"""
The rho^2 term that the in-step TIGHT step's stage brackets leave out (csrc/rsf_device.h: tight_incr_scaled, tight_rho_limit),
measured on the extended-precision RK4 of tests/rk4_extended.py for the lanes the GPU tests run.  No GPU.

For every lane of tests/test_gpu_linear_bracket.py's cases (accuracy, decisions with each of the three lanes beyond their limit,
paths, the lanes the bound frees, the lane it holds) and of tests/test_gpu_series_scale.py's cases (accuracy, decisions, paths) —
every set is built in tests/linear_bracket.py, where the GPU tests take theirs from:
  the term    |bh| rho^2 |d1'| of each of the three stages whose bracket takes rho, largest over the series, is at most
              2^-47 V_ref wherever the lane is inside its limit (its largest |rho| and |c1| of the series below the lane's
              thresholds) — the limit is cbrt(2^-47 V_ref / |bh|) for that purpose.  (The limit alone proves 2^-47 V_ref for the
              half-step stages and 7 x that for the full-step stage, whose own d1' it holds only through the step's end; the
              measured term is what is asserted, for all three.)  Nothing is claimed of a lane beyond its limit: the guard
              removes it;
  the limit   the restated limit never exceeds 2^-20, and is 2^-20 exactly where |bh| <= 8192 V_ref;
  the lanes   test_gpu_series_scale's lanes, placed against the constant thresholds, lie below 0.95 of the per-lane ones as well:
              their decisions are what they were.
"""
import numpy as np
import pytest

import linear_bracket as LB
import test_gpu_series_scale as S


def _check(tag, m, dc, a, b, steps, d):
    r = S._scan(m, dc, a, b, steps, d)
    lim = LB.lim_rho(m, dc, b)
    bhl = LB.bh(m, dc, b)
    assert (lim <= LB.R20).all() and (lim[np.abs(bhl) <= 8192.0 * m.V_ref] == LB.R20).all() and (lim[np.abs(bhl) > 8193.0 * m.V_ref] < LB.R20).all()
    inside = (r["rho"].max(axis=0) < lim) & (r["c1"].max(axis=0) < 0.5 * lim)
    kw = {} if d == 1 else {"a": a, "b": b}
    term = LB.dropped_term(m, dc, steps, vl=S._table(m, steps), **kw)
    rel = term / (LB.EPS * m.V_ref)
    print(f"{tag}: {int(inside.sum())} of {dc.size} lanes inside their limit; bh {bhl.min():.3g} .. {bhl.max():.3g}; the dropped term over 2^-47 V_ref: "
          f"{rel[inside].max():.3g} at most inside (median {np.median(rel[inside]):.2g}), {rel.max():.3g} over all lanes")
    assert inside.any() and (rel[inside] <= 1.0).all(), rel[inside].max()
    return r, inside


@pytest.mark.parametrize("steps,h,damping,d,kind", LB.ACCURACY)
def test_dropped_term_on_the_accuracy_lanes(oracle_mod, steps, h, damping, d, kind):
    m, dc, a, b, _ = LB.accuracy_lanes(oracle_mod, steps, h, damping, d, kind)
    _, inside = _check(f"{kind} steps {steps} h {h} damping {damping} d {d}", m, dc, a, b, steps, d)
    assert inside.all()


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("h", [0.025, 0.1])
def test_dropped_term_on_the_decision_lanes(oracle_mod, h, damping):
    """the lanes of test_guard_on_the_lanes_limit: those that stay, then with lane 7 at 1.07, 1.15 and 1.35 x its limit"""
    steps = 200
    m, a, b, dc, overs = LB.decision_lanes(oracle_mod, h, damping, steps)
    _, inside = _check(f"decisions h {h} damping {damping} inside", m, dc, a, b, steps, 1)
    assert inside.all()
    for over, (dco, _) in overs.items():
        _, inside = _check(f"decisions h {h} damping {damping} lane 7 at {over}", m, dco, a, b, steps, 1)
        assert not inside[7] and np.delete(inside, 7).all()


@pytest.mark.parametrize("steps,h,damping,d", LB.PATHS)
def test_dropped_term_on_the_paths_lanes(oracle_mod, steps, h, damping, d):
    """the lanes of test_paths_with_the_lanes_bound_bit_for_bit: the ones that run unguarded under the lane's Bmax, and the held one"""
    m, dc, a, b = LB.paths_lanes(oracle_mod, steps, h, damping, d)
    _, inside = _check(f"paths steps {steps} h {h} damping {damping} d {d}", m, dc, a, b, steps, d)
    assert inside.all() and (LB.bh(m, dc, b)[:LB.C // 2] > 8192.0).sum() >= LB.C // 4


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("steps,h", LB.FREE)
def test_dropped_term_on_the_freed_and_held_lanes(oracle_mod, steps, h, damping):
    """the lanes of test_bound_frees_lanes_inside_their_own_limit and of test_lanes_bound_keeps_the_guard (its lane 7 beyond its limit)"""
    m, dc, a, b = LB.free_lanes(oracle_mod, steps, h, damping)
    _, inside = _check(f"freed steps {steps} h {h} damping {damping}", m, dc, a, b, steps, 1)
    assert inside.all()
    m, dc, a, b = LB.held_lanes(oracle_mod, steps, h, damping)
    _, inside = _check(f"held steps {steps} h {h} damping {damping}", m, dc, a, b, steps, 1)
    assert not inside[7] and np.delete(inside, 7).all()


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("kind", ["rho", "dlt"])
def test_dropped_term_on_series_scale_decision_lanes(oracle_mod, kind, damping):
    """test_gpu_series_scale.test_guard_on_the_rescaled_increments: the lanes that stay, then lane 7 beyond a CONSTANT threshold"""
    m, a, b, sets = LB.series_scale_decision_lanes(oracle_mod, kind, damping)
    for i, dc in enumerate(sets):
        r, inside = _check(f"series_scale decisions {kind} damping {damping} set {i}", m, dc, a, b, 200, 1)
        others = np.delete(np.arange(LB.C), 7) if i else np.arange(LB.C)
        # these lanes have small Dc: the lane's limit is the constant one, their decisions are what they were
        assert inside[others].all() and (LB.lim_rho(m, dc, b) == LB.R20).all()
        assert np.array_equal(LB.largest(r, m, dc, b), S._largest(r))


@pytest.mark.parametrize("steps,h,damping,d", LB.PATHS)
def test_dropped_term_on_series_scale_paths_lanes(oracle_mod, steps, h, damping, d):
    """test_gpu_series_scale.test_guarded_and_unguarded_trips_bit_for_bit: Dc up to 2e4, bh up to 7e4 — placed against the constant
    thresholds, they stay below 0.7 of the lane's own, and the bound with the lane's Bmax decides what the constant one decided"""
    m, dc, a, b = LB.series_scale_paths_lanes(oracle_mod, steps, h, damping, d)
    r, inside = _check(f"series_scale paths steps {steps} h {h} damping {damping} d {d}", m, dc, a, b, steps, d)
    p = LB.predicate(r, m, dc, b)
    print(f"  bh up to {LB.bh(m, dc, b).max():.3g}; largest increment over the lane's thresholds {LB.largest(r, m, dc, b).max():.3f}; rb over the lane's Bmax, wave 0: {p['rb'][:, :LB.C // 2].max():.3f}")
    assert inside.all() and LB.largest(r, m, dc, b).max() < 0.7 and LB.clear(p) and np.array_equal(p["need"], r["need"])


@pytest.mark.parametrize("steps,h,damping,d", S.CASES)
def test_series_scale_lanes_keep_their_decisions(oracle_mod, steps, h, damping, d):
    m, dc, a, b = LB.series_scale_lanes(oracle_mod, steps, h, damping, d)
    r, inside = _check(f"series_scale steps {steps} h {h} damping {damping} d {d}", m, dc, a, b, steps, d)
    new, old = LB.largest(r, m, dc, b).max(axis=0), S._largest(r).max(axis=0)
    print(f"  largest increment over the lane's thresholds {new.max():.3f}, over the constant ones {old.max():.3f}; {int((new > old * (1 + 1e-12)).sum())} lanes nearer to theirs")
    assert inside.all() and new.max() < 0.95
    # wave 1, the lanes at 0.5 .. 0.9 of a constant threshold: small Dc, the limit is the constant one
    assert (LB.lim_rho(m, dc, b)[LB.C // 2:] == LB.R20).all() and np.array_equal(new[LB.C // 2:], old[LB.C // 2:])
