"""
The float64 sampler's in-step TIGHT step with one log1p bracket for its two half-step stages (csrc/rsf_device.h: rk4_tight INSTEP,
tight_incr_scaled, tight_bracket) and the per-lane limit on rho that holds what that leaves out to 2^-43 (tight_pb_limit, through
Series::lim_rho / lim_c1 / bmax), on the CPU: the restatement of tests/shared_bracket.py against the extended-precision RK4.  No GPU.

Accuracy  the six series of tests/test_ms_free.py (2000 steps at h = 0.025, 4000 at h = 0.0125, 500 at h = 0.1, damping on and off) x
          its two lane sets (64 lanes with the model's (a, b), 64 with per-lane (a, b), Dc 300 .. 5000): every lane's error of w, of Rh
          and of the sum of squares against the extended-precision walk is at most MARGIN x the largest error of the PARENT's form
          (ms_free.walk, carry=False: every stage its own bracket) on that set.  MARGIN 2, test_ms_free's rule.  Measured: the
          largest ratio is 1.16 (the sum of squares at h = 0.1, per-lane (a, b): 1.07e-14 -> 1.23e-14); w and Rh do not move in three
          digits (the figures are printed).
The limit the lane sets of test_gpu_series_scale, test_gpu_linear_bracket, test_gpu_ms_free and test_gpu_unguarded_trip, through
          their own helpers (tests/linear_bracket.py builds the first two's):
          placed    every lane those tests expect to stay in TIGHT has its largest |rho| and |c1| of the series below 0.95 of the
                    NEW thresholds as well (lim_pb formed from the largest Rh of the series, the strictest a loop entry could
                    see), and every lane they send out is beyond 1.05 of the threshold they placed it against, as before: no
                    decision of the guard moves.  lim_pb is at or above the limit the lane was placed against on every lane but the
                    one pinned in BINDS (asserted): one lane of test_gpu_series_scale's (h = 0.1, d = 3, Dc 534, b/a 1.38: lim_pb 0.945 x 2^-20,
                    its |rho| at 0.63 of that; |dlt| is what binds there).  With 2^-44 in place of 2^-43 — the figure first meant
                    for the limit — this check fails: test_gpu_series_scale's lanes at 0.9 of 2^-20 (h = 0.025, Dc 228 .. 254) have
                    lim_pb at 0.88 .. 0.97 of 2^-20 then, their |rho| at up to 1.03 of it (profiles/shared_bracket/README.md);
          gate      tight_needs_guard restated with the new bmax frees exactly the trips it frees with the parent's;
          term      on the extended-precision trajectory the term that the shared bracket leaves out of the second half-step stage's
                    dlt, (b/2a) |rho_b| |rho_b - rho_a|, is at most 2^-43 on every lane inside its limit (measured: 0.22 of it at
                    most, on the raised model's lanes; 0.05 on test_gpu_series_scale's), and at most the derivation's own bound on it.
          The full-step stage keeps its own bracket.  Had it taken the shared one (rho_s = 2 c1', twice a half-step stage's) the
          term there, (b/2a) |2 c1| |2 c1 - a1|, would reach 2.3e-13 = 2.1 x 2^-43 on test_gpu_series_scale's lanes at 0.9 of the
          rho threshold, inside every limit: asserted below as the reason it does not (test_full_step_stage_cannot_share).
lim_pb    rounded down against 2^-43 / ((b/2a)(2^-10 + 2^-20) 2 |Rh|) in long double over b/a in [0.3, 6] and Rh in [1e-8, 1e-3], both
          signs; never more than 2^-28 below it; NaN for a zero, infinite or NaN input, which the lane's limit ignores (fmin).
"""
import numpy as np
import pytest

import linear_bracket as LB
import ms_free as M
import rk4_extended as X
import shared_bracket as SB
import test_gpu_ms_free as GM
import test_gpu_series_scale as S
import test_gpu_unguarded_trip as U
import test_ms_free as TM
import tight_bound as T

MARGIN = 2.0
IN, OUT = 0.95, 1.05


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("steps,h", TM.SERIES)
def test_shared_bracket_no_worse_than_the_parents_step(oracle_mod, steps, h, damping):
    m, dc, a, b, vl, data, ext, _ = TM._problem(oracle_mod, steps, h, damping)
    parent = M.walk(m, dc, a, b, vl, data, steps, carry=False)
    same = SB.walk(m, dc, a, b, vl, data, steps, share="none")
    assert all(np.array_equal(parent[k], same[k]) for k in parent)  # the restatement here is ms_free's but for the bracket
    old = M.errors(parent, ext)
    new = M.errors(SB.walk(m, dc, a, b, vl, data, steps, share="half"), ext)
    missed = []
    for k in ("w", "Rh", "ssq"):
        for name, sl in TM.SETS.items():
            n, o = new[k][sl], old[k][sl]
            print(f"steps {steps} h {h} damping {damping} {k:3s} {name}: parent max {o.max():.2e} med {np.median(o):.2e}; shared max {n.max():.2e} "
                  f"med {np.median(n):.2e}; shared / parent {n.max() / o.max():.3f}")
            if not (n <= MARGIN * o.max()).all():
                missed.append((k, name))
    assert not missed, missed


# --- the limit on the lanes of the GPU tests ---------------------------------------------------------------------------------

# The lanes of the existing tests' sets on which lim_pb is below the limit they were placed against, by the tag's prefix: one, recorded
# in profiles/shared_bracket/README.md (h = 0.1, d = 3, Dc 534, b/a 1.378: lim_pb at 0.945 of 2^-20, its |rho| at 0.63 of that).
# Everywhere else lim_pb is above that limit: idle.
BINDS = {"series_scale steps 35 h 0.1 damping True d 3": [120], "series_scale steps 530 h 0.1 damping True d 3": [120]}


def _check(tag, m, dc, a, b, steps, d, vl=None, out=()):
    """out: the lanes the GPU test sends out of TIGHT.  -> (scan, the dropped terms, the lanes inside their limit)"""
    kw = {} if d == 1 else {"a": a, "b": b}
    r = T.scan(m, dc, steps, vl=vl, **kw)
    stay = np.setdiff1d(np.arange(dc.size), np.asarray(out, dtype=int))
    rh_max = SB.rh_entry(m, dc, r["theta"]).max(axis=0)  # the strictest limit a loop entry of the series could form
    old, new, pb = LB.lim_rho(m, dc, b), SB.lim_rho(m, dc, a, b, rh_max), SB.lim_pb(b / a, rh_max)
    rho, c1 = r["rho"].max(axis=0), r["c1"].max(axis=0)
    big_old = np.maximum(rho / old, c1 / (0.5 * old))
    big_new = np.maximum(rho / new, c1 / (0.5 * new))
    binds = pb < old
    print(f"{tag}: Dc {dc.min():.0f} .. {dc.max():.0f}, lim_pb / the lane's limit {(pb / old).min():.3g} .. {(pb / old).max():.3g} ({int(binds.sum())} lanes below 1); "
          f"largest |rho|, |c1| over the limit: parent's {big_old[stay].max():.3f}, new {big_new[stay].max():.3f}")
    for i in np.flatnonzero(binds):
        print(f"    lane {i}: Dc {dc[i]:.1f} b/a {b[i] / a[i]:.3f} Rh {rh_max[i]:.3g} lim_pb {pb[i] / LB.R20:.3f} x 2^-20, its |rho| at {big_new[i]:.3f} of the new limit")
    # idle: lim_pb is at or above the limit the lanes were placed against, but for the recorded lane (and there by 6 % at the most)
    assert list(np.flatnonzero(binds)) == BINDS.get(tag, []) and (pb >= 0.94 * old).all(), (tag, np.flatnonzero(binds), (pb / old).min())
    # placed: the lanes that stay are inside the new thresholds with the margin the tests ask of the old ones; the ones sent out are out
    assert (big_new[stay] < IN).all(), (tag, big_new[stay].max())
    for k in out:
        assert LB.largest(r, m, dc, b)[:, k].max() > OUT or S._largest(r)[:, k].max() > OUT, (tag, k)
    # gate: the restated bound with the new bmax frees the trips it freed
    p_old, p_new = LB.predicate(r, m, dc, b), SB.predicate(r, m, dc, a, b)
    moved = p_old["need"] != p_new["need"]
    assert not moved.any(), (tag, np.argwhere(moved)[:8], p_old["rb"][moved][:8], p_new["rb"][moved][:8])
    # term: what the shared bracket leaves out, on the lanes inside their limit
    t = SB.dropped_term(m, dc, steps, vl=vl, **kw)
    inside = (t["rho"] < new) & (t["c1"] < 0.5 * new)
    assert inside[stay].all()
    rel = t["half"] / SB.EPS
    print(f"    the dropped term over 2^-43: {rel[inside].max():.3g} at most inside the limit (median {np.median(rel[inside]):.2g}); over its own bound "
          f"{(t['half'] / t['bound'])[inside].max():.3f}; the full-step stage's, had it shared: {(t['full'] / SB.EPS)[inside].max():.3g}")
    assert (rel[inside] <= 1.0).all() and (t["half"][inside] <= 1.02 * t["bound"][inside]).all(), (tag, rel[inside].max())
    return r, t, inside


@pytest.mark.parametrize("steps,h,damping,d", S.CASES)
def test_limit_on_series_scale_accuracy_lanes(oracle_mod, steps, h, damping, d):
    m, dc, a, b = LB.series_scale_lanes(oracle_mod, steps, h, damping, d)
    _check(f"series_scale steps {steps} h {h} damping {damping} d {d}", m, dc, a, b, steps, d)


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("kind", ["rho", "dlt"])
def test_limit_on_series_scale_decision_lanes(oracle_mod, kind, damping):
    m, a, b, sets = LB.series_scale_decision_lanes(oracle_mod, kind, damping)
    for i, dc in enumerate(sets):
        _check(f"series_scale decisions {kind} damping {damping} set {i}", m, dc, a, b, 200, 1, vl=S._table(m, 200), out=(7,) if i else ())


@pytest.mark.parametrize("steps,h,damping,d", LB.PATHS)
def test_limit_on_paths_lanes(oracle_mod, steps, h, damping, d):
    for name, lanes in (("series_scale", LB.series_scale_paths_lanes), ("linear_bracket", LB.paths_lanes)):
        m, dc, a, b = lanes(oracle_mod, steps, h, damping, d)
        _check(f"{name} paths steps {steps} h {h} damping {damping} d {d}", m, dc, a, b, steps, d)


@pytest.mark.parametrize("steps,h,damping,d,kind", LB.ACCURACY)
def test_limit_on_linear_bracket_accuracy_lanes(oracle_mod, steps, h, damping, d, kind):
    m, dc, a, b, _ = LB.accuracy_lanes(oracle_mod, steps, h, damping, d, kind)
    _check(f"linear_bracket {kind} steps {steps} h {h} damping {damping} d {d}", m, dc, a, b, steps, d)


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("h", [0.025, 0.1])
def test_limit_on_linear_bracket_decision_free_and_held_lanes(oracle_mod, h, damping):
    steps = 200
    m, a, b, dc, overs = LB.decision_lanes(oracle_mod, h, damping, steps)
    _check(f"linear_bracket decisions h {h} damping {damping} inside", m, dc, a, b, steps, 1)
    for over, (dco, _) in overs.items():
        _check(f"linear_bracket decisions h {h} damping {damping} lane 7 at {over}", m, dco, a, b, steps, 1, out=(7,))
    for fsteps, fh in LB.FREE:
        if fh == h:
            mf, dcf, af, bf = LB.free_lanes(oracle_mod, fsteps, fh, damping)
            _check(f"linear_bracket freed steps {fsteps} h {fh} damping {damping}", mf, dcf, af, bf, fsteps, 1)
            mf, dcf, af, bf = LB.held_lanes(oracle_mod, fsteps, fh, damping)
            _check(f"linear_bracket held steps {fsteps} h {fh} damping {damping}", mf, dcf, af, bf, fsteps, 1, out=(7,))


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("which", ["tight", "bump"])
def test_limit_on_ms_free_lanes(oracle_mod, which, damping, d):
    """test_gpu_ms_free's tight and bump sets (its full set leaves TIGHT for the wider tiers by design: nothing there is expected to
    stay), on the steps they were placed on"""
    dc, a, b = GM._lanes(oracle_mod, which, damping, d)
    steps = GM.FREE if which == "tight" else GM.PLACED
    m = GM._model(oracle_mod, which, steps, damping)
    _check(f"ms_free {which} damping {damping} d {d}", m, dc, a, b, steps, d, vl=S._table(m, steps), out=(7,) if which == "bump" else ())


@pytest.mark.parametrize("damping", [True, False])
def test_limit_on_unguarded_trip_lanes(oracle_mod, damping):
    steps = 530
    m = U._model(oracle_mod, steps, damping)
    dca = U._lanes(600.0, 2000.0, 21)
    dcb = dca.copy()
    dcb[::X.WAVE] = 300.0
    one = np.ones(U.C)
    for tag, dc in (("A", dca), ("B", dcb)):
        _check(f"unguarded_trip {tag} damping {damping}", m, dc, m.a * one, m.b * one, steps, 1)
    mt = U._model(oracle_mod, steps, damping, U._ends_table)
    vl = U._ends_table(np.arange(2 * steps + 1, dtype=np.float64) * (0.5 * float(mt.delta_t)))
    dcu = U._lanes(1350.0, 3000.0, 23)
    dcg = dcu.copy()
    dcg[::X.WAVE] = 1000.0
    for tag, dc in (("table", dcu), ("table guarded", dcg)):
        _check(f"unguarded_trip {tag} damping {damping}", mt, dc, mt.a * one, mt.b * one, steps, 1, vl=vl)


@pytest.mark.parametrize("damping", [True, False])
def test_full_step_stage_cannot_share(oracle_mod, damping):
    """The reason the full-step stage keeps its own bracket: on test_gpu_series_scale's rho-bound decision lanes (0.3 .. 0.9 of 2^-20,
    every one inside every limit) the term a shared bracket would leave out of THAT stage's dlt passes 2^-43 (and 4 x the 2^-44 first
    meant), where the half-step stage's stays under a twentieth of it."""
    m, a, b, sets = LB.series_scale_decision_lanes(oracle_mod, "rho", damping)
    dc = sets[0]
    t = SB.dropped_term(m, dc, 200)
    lim = SB.lim_rho(m, dc, a, b, SB.rh_entry(m, dc))
    assert ((t["rho"] < lim) & (t["c1"] < 0.5 * lim)).all()
    print(f"damping {damping}: full-step stage {(t['full'] / SB.EPS).max():.3g} x 2^-43 = {t['full'].max():.3g}; half-step stage {(t['half'] / SB.EPS).max():.3g} x 2^-43")
    assert t["full"].max() > 1.5 * SB.EPS and t["half"].max() < 0.1 * SB.EPS


def test_lim_pb_rounded_down():
    rng = np.random.default_rng(5)
    n = 200000
    boa = np.concatenate([rng.uniform(0.3, 6.0, n), [0.3, 6.0]]) * rng.choice([-1.0, 1.0], n + 2)
    Rh = np.concatenate([np.exp(rng.uniform(np.log(1e-8), np.log(1e-3), n)), [1e-8, 1e-3]]) * rng.choice([-1.0, 1.0], n + 2)
    got, ext = SB.lim_pb(boa, Rh), SB.lim_pb_ext(boa, Rh)
    rel = ((ext - X._w(got)) / ext).astype(np.float64)
    print(f"lim_pb below the exact quotient by {rel.min():.3g} .. {rel.max():.3g} of it")
    assert (rel > 0.0).all() and rel.max() < 2.0 ** -28
    # the kernel's reciprocal may be an ulp off NumPy's: the factor 1 - 2^-30 covers that four million times over
    assert rel.min() > 2.0 ** -31
    # zero and NaN: no limit of its own — the lane's limit is tight_rho_limit's
    with np.errstate(all="ignore"):
        bad = SB.lim_pb(np.array([0.0, 1.2, np.nan, 1.2, -0.0]), np.array([1e-5, 0.0, 1e-5, np.nan, -0.0]))
    assert np.isnan(bad).all()
    assert (np.fmin(LB.R20, bad) == LB.R20).all()
    assert np.isnan(SB.lim_pb(1.2, np.inf)) and np.isnan(SB.lim_pb(np.inf, 1e-5))  # an infinite factor: the kernel's reciprocal gives NaN too


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("damping", [True, False])
def test_term_where_the_limit_binds(oracle_mod, damping, d):
    """test_gpu_shared_bracket's lanes on the model where lim_pb is the limit that decides (shared_bracket.binding_model): the term on
    every lane inside its limit, lane 7 at 0.9 of it included; at 1.15 that lane is outside and nothing is claimed of it."""
    import test_gpu_shared_bracket as G

    steps, k = 200, 7
    m, a, b, sets = G.binding_lanes(oracle_mod, steps, damping, d)
    for target, dc in sets.items():
        t = SB.dropped_term(m, dc, steps, a=a, b=b, vl=S._table(m, steps))
        lim = SB.lim_rho(m, dc, a, b, SB.rh_entry(m, dc))
        inside = (t["rho"] < lim) & (t["c1"] < 0.5 * lim)
        rel = t["half"] / SB.EPS
        print(f"damping {damping} d {d} lane {k} at {target}: lim_pb / 2^-20 {(lim / LB.R20).min():.3f} .. {(lim / LB.R20).max():.3f}; the dropped term over 2^-43: "
              f"{rel[inside].max():.3g} at most inside the limit, lane {k} {rel[k]:.3g}; over its own bound {(t['half'] / t['bound'])[inside].max():.3f}")
        assert inside[np.arange(dc.size) != k].all() and inside[k] == (target < 1.0)
        assert (rel[inside] <= 1.0).all() and (t["half"][inside] <= 1.02 * t["bound"][inside]).all()
