"""
GPU tests: the float64 sampler's in-step TIGHT step with its stage brackets to first order in rho (csrc/rsf_device.h:
tight_incr_scaled, rk4_tight — brx = bh (1 - rho), no rho^2) and the per-lane limit on rho that holds the dropped term to
2^-47 V_ref (tight_rho_limit, Series::lim_rho / lim_c1 / bmax), restated in tests/linear_bracket.py.

One replayed iteration that proposes the start point itself (test_gpu_series_scale._sampler), 128 chains = two waves, delta_t =
0.025 and 0.1, damping on and off, step counts that walk the trip structure (35, 200, 530), one parameter and three.  Two models:
  builtin  mu_t_zero = mu_ref.  Wave 0 headline-like (Dc 300 .. 5000), wave 1 at 0.5 .. 0.9 of the threshold that binds for the
           lane — small Dc, bh < 8192: the thresholds there are what they were
  raised   mu_t_zero raised so that the slip rate starts at 1.2 V_ref: |rho| ~ (h / 2 Dc) 0.2 for the whole series, which sits
           between the lane's new limit and 2^-20 at Dc of 1e4 .. 1e5, where bh is 1e5 .. 1e7 and no increment of mu is near its
           threshold: the NEW limit is what binds, for every lane (asserted)
Accuracy   the sampler's SSq against the extended-precision RK4: per wave, max and median of its error within FACTOR (4) x the
           CPU restatement's — a plain float64 RK4 — on the same lanes (x SSQ_FLOOR where that is at rounding level itself),
           the max under SSQ_CAP: test_gpu_rk4_extended's yardstick, as test_gpu_series_scale uses it.
Decisions  raised model: lanes below 0.95 x every threshold stay in TIGHT — nothing redone, every step a TIGHT step; a lane at
           1.07, 1.15, 1.35 x its new limit, yet below 0.95 x 2^-20 and 2^-21, leaves it — its trip is redone and its wave goes on
           in NARROW.  No lane lies between 0.95 and 1.05 of any threshold in the extended-precision maxima.
Paths      builtin model: wave 0 inside tight_needs_guard's bound with the lane's own limit (lanes with bh > 8192 among them),
           wave 1 the same Dc but for one lane that keeps it under the guard at every trip: the 63 common lanes agree bit for
           bit, and steps_unguarded is what the restated predicate says (every decision 10 % or more from its edge).  Raised
           model: both waves at 0.3 .. 0.75 of the new limit, where the bound with the lane's limit still frees every trip; and
           a wave with one lane beyond its own Bmax but inside the constant one, which must not run a single trip unguarded.
Every lane set is built in tests/linear_bracket.py, where tests/test_linear_bracket.py measures the dropped term on it.
"""
import numpy as np
import pytest

import linear_bracket as LB
import rk4_extended as X
import test_gpu_rk4_extended as R
import test_gpu_series_scale as S
import tight_bound as T

pytestmark = pytest.mark.gpu

C = LB.C
FACTOR = S.FACTOR
_REF = {}


def _reference(cpu_engine, oracle_mod, steps, h, damping, d, kind):
    """model, lanes, observation, the trips' extended-precision maxima, extended SSq and the restatement's SSq errors (computed once)"""
    key = (steps, h, damping, d, kind)
    if key not in _REF:
        m, dc, a, b, want = LB.accuracy_lanes(oracle_mod, steps, h, damping, d, kind)
        data = S._data(oracle_mod, steps, h)
        r = S._scan(m, dc, a, b, steps, d)
        kw = {} if d == 1 else {"a": a, "b": b}
        _, ssq_ext = X.forward_ext(m, dc, data=data, **kw)
        assert cpu_engine.set_model(m, 1) == data.size
        s_cpu, _ = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=False, **kw)
        o = (np.abs(X._w(s_cpu) - ssq_ext) / ssq_ext).astype(np.float64)
        _REF[key] = (m, dc, a, b, data, r, want, ssq_ext, o)
    return _REF[key]


@pytest.mark.parametrize("steps,h,damping,d,kind", LB.ACCURACY)
def test_linear_bracket_within_float64_rounding(gpu_engine, cpu_engine, oracle_mod, steps, h, damping, d, kind):
    m, dc, a, b, data, r, want, ssq_ext, o = _reference(cpu_engine, oracle_mod, steps, h, damping, d, kind)
    tag = f"{kind} steps {steps} h {h} damping {damping} d {d}"
    top = LB.largest(r, m, dc, b).max(axis=0)
    bind, bhl = LB.binding(r, m, dc, b), LB.bh(m, dc, b)
    print(f"{tag}: wave 0 Dc {dc[:X.WAVE].min():.0f} .. {dc[:X.WAVE].max():.0f}, largest increment {top[:X.WAVE].max():.3f} of its threshold; "
          f"wave 1 Dc {dc[X.WAVE:].min():.0f} .. {dc[X.WAVE:].max():.0f}, {top[X.WAVE:].min():.3f} .. {top[X.WAVE:].max():.3f}; bh {bhl.min():.3g} .. "
          f"{bhl.max():.3g}, lim_rho / 2^-20 {(LB.lim_rho(m, dc, b) / LB.R20).min():.3f} .. {(LB.lim_rho(m, dc, b) / LB.R20).max():.3f}, binding {sorted(set(bind))}")
    # the lanes are where they were meant to be: wave 1 at its targets, every lane below 0.95 of every threshold
    assert np.allclose(top[X.WAVE:], want, rtol=1e-2) and want.min() >= 0.49 and want.max() > 0.75, (top[X.WAVE:], want)
    assert top.max() < 0.95
    if kind == "raised":  # the new limit binds, for every lane; |dlt| is nowhere near
        assert (bhl > 8192.0).all() and np.isin(bind, ("rho", "c1")).all() and (LB.lim_rho(m, dc, b) < 0.5 * LB.R20).all()
        assert max((r[k] / T.GUARDS[k]).max() for k in ("dlt", "dlt_h")) < 0.1
    ssq, acc, cnt = S._sampler(gpu_engine, m, dc, a, b, data, d)
    print(f"{tag}: counters {cnt}")
    assert acc.all(), f"{tag}: {int((~acc).sum())} chains did not accept"
    assert S._all_tight(cnt, steps), cnt
    g = (np.abs(X._w(ssq) - ssq_ext) / ssq_ext).astype(np.float64)
    fails = []
    for w in range(2):
        sl = slice(X.WAVE * w, X.WAVE * (w + 1))
        R._check(f"{tag} wave {w}", g[sl], o[sl], FACTOR, R.SSQ_FLOOR, R.SSQ_CAP, fails)
    assert not fails, fails


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("h", [0.025, 0.1])
def test_guard_on_the_lanes_limit(gpu_engine, oracle_mod, h, damping):
    steps = 200
    # the lanes that stay: both waves at 0.3 .. 0.9 of the new limit
    m, a, b, dc, overs = LB.decision_lanes(oracle_mod, h, damping, steps)
    data = S._data(oracle_mod, steps, h)
    r = S._scan(m, dc, a, b, steps, 1)
    big, old = LB.largest(r, m, dc, b), S._largest(r)
    print(f"h {h} damping {damping}: Dc {dc.min():.0f} .. {dc.max():.0f}, largest increments {big.max(axis=0).min():.3f} .. {big.max():.3f} of the lane's "
          f"thresholds, {old.max():.3f} of 2^-20 / 2^-21; lim_rho / 2^-20 {(LB.lim_rho(m, dc, b) / LB.R20).min():.3f} .. {(LB.lim_rho(m, dc, b) / LB.R20).max():.3f}")
    assert big.max() < 0.95 and big.max() > 0.85 and np.isin(LB.binding(r, m, dc, b), ("rho", "c1")).all() and (LB.bh(m, dc, b) > 8192.0).all()
    _, acc, cnt = S._sampler(gpu_engine, m, dc, a, b, data, 1)
    print(f"h {h} damping {damping} inside: {cnt}")
    assert acc.all() and S._all_tight(cnt, steps), cnt
    # the lanes that leave: one at a time in place of lane 7 of wave 0, beyond its own limit and inside 2^-20 / 2^-21
    for over in LB.OVERS:
        k = 7
        dco, got = overs[over]
        ro = S._scan(m, dco, a, b, steps, 1)
        bo, oo = LB.largest(ro, m, dco, b), S._largest(ro)
        assert got == over and abs(bo[:, k].max() / over - 1.0) < 1e-2, (bo[:, k].max(), got, over)
        assert oo.max() < 0.95, oo.max()  # the constant thresholds alone would have kept the lane
        band = (bo > 0.95) & (bo < 1.05)
        first = int(np.argmax(bo[:, k] > 1.05))
        assert not band[:first + 1].any() and (np.delete(bo, k, axis=1) < 0.95).all()
        _, acc_o, cnt_o = S._sampler(gpu_engine, m, dco, a, b, data, 1)
        print(f"h {h} damping {damping} lane at {over} (Dc {dco[k]:.0f}, {oo[:, k].max():.3f} of the constant threshold): first trip over its limit {first}, {cnt_o}")
        assert acc_o.all()
        # wave 1 as before; wave 0: TIGHT up to and with that trip, the trip redone, NARROW from there on
        assert cnt_o["steps_redone"] >= T.TRIP and cnt_o["steps_narrow"] > 0 and cnt_o["steps_full"] == 0, cnt_o
        assert cnt_o["steps_tight"] >= (steps - steps % 2) + T.TRIP * (first + 1), cnt_o
        assert cnt_o["steps_tight"] + cnt_o["steps_narrow"] + cnt_o["steps_wide"] == 2 * steps, cnt_o


@pytest.mark.parametrize("steps,h,damping,d", LB.PATHS)
def test_paths_with_the_lanes_bound_bit_for_bit(gpu_engine, oracle_mod, steps, h, damping, d):
    # increments at 0.02 .. 0.1 of the lane's thresholds: far inside the a-priori bound as well, and Dc large enough for bh > 8192
    m, dc, a, b = LB.paths_lanes(oracle_mod, steps, h, damping, d)
    data, trips, free = S._data(oracle_mod, steps, h), steps // T.TRIP, dc[:X.WAVE]
    r = S._scan(m, dc, a, b, steps, d)
    p = LB.predicate(r, m, dc, b)
    assert LB.clear(p), (p["D"].max(axis=0), p["rb"].max(axis=0))
    need, bhl = p["need"], LB.bh(m, dc, b)
    assert need[:, X.WAVE].all() and not np.delete(need, X.WAVE, axis=1).any() and LB.largest(r, m, dc, b).max() < 0.7
    assert (bhl[:X.WAVE] > 8192.0).sum() >= X.WAVE // 2, bhl[:X.WAVE]  # the lane's own Bmax decides for half the wave or more
    ssq, acc, cnt = S._sampler(gpu_engine, m, dc, a, b, data, d)
    print(f"steps {steps} h {h} damping {damping} d {d}: Dc {free.min():.0f} .. {free.max():.0f} and {dc[X.WAVE]:.0f}; bh > 8192 in {int((bhl[:X.WAVE] > 8192.0).sum())} "
          f"lanes, rb {p['rb'][:, :X.WAVE].max():.3f} of the lane's limit; {cnt}")
    assert acc.all() and S._all_tight(cnt, steps), cnt
    assert cnt["steps_unguarded"] == T.predicted_unguarded(need[:, :X.WAVE]) + T.predicted_unguarded(need[:, X.WAVE:]) == T.TRIP * trips, cnt
    assert np.isfinite(ssq).all() and np.array_equal(ssq[1:X.WAVE], ssq[X.WAVE + 1:])


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("steps,h", LB.FREE)
def test_bound_frees_lanes_inside_their_own_limit(gpu_engine, oracle_mod, steps, h, damping):
    m, dc, a, b = LB.free_lanes(oracle_mod, steps, h, damping)
    data = S._data(oracle_mod, steps, h)
    r = S._scan(m, dc, a, b, steps, 1)
    p = LB.predicate(r, m, dc, b)
    print(f"steps {steps} h {h} damping {damping}: Dc {dc.min():.0f} .. {dc.max():.0f}, rb {p['rb'].max(axis=0).min():.3f} .. {p['rb'].max():.3f} of the lane's limit, "
          f"lim_rho / 2^-20 {(LB.lim_rho(m, dc, b) / LB.R20).min():.3f} .. {(LB.lim_rho(m, dc, b) / LB.R20).max():.3f}")
    assert LB.clear(p) and not p["need"].any() and (LB.bh(m, dc, b) > 8192.0).all() and p["rb"].max() > 0.8
    _, acc, cnt = S._sampler(gpu_engine, m, dc, a, b, data, 1)
    print(f"steps {steps} h {h} damping {damping}: {cnt}")
    assert acc.all() and S._all_tight(cnt, steps), cnt
    assert cnt["steps_unguarded"] == 2 * T.TRIP * (steps // T.TRIP), cnt


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("steps,h", LB.FREE)
def test_lanes_bound_keeps_the_guard(gpu_engine, oracle_mod, steps, h, damping):
    """A Bmax too lax for a lane with bh > 8192 shows here: lane 7 of wave 0 is beyond its own limit on rho (1.35 x) and inside the
    constant 2^-20 / 2^-21, its bound rb beyond 1.1 x the lane's Bmax and below 0.9 x the constant 0.9 * 2^-21 at every trip.  With
    the lane's Bmax no trip of wave 0 may run without the guard (the guard trips, the wave alternates with NARROW, and whenever it
    is back in TIGHT the bound asks for the guard again); with the constant every such trip would — unmeasured, beyond the limit.
    Wave 1, the same lanes without that one, runs every whole trip without the guard."""
    m, dc, a, b = LB.held_lanes(oracle_mod, steps, h, damping)
    data, k = S._data(oracle_mod, steps, h), 7
    r = S._scan(m, dc, a, b, steps, 1)
    p = LB.predicate(r, m, dc, b)
    big = LB.largest(r, m, dc, b)
    print(f"steps {steps} h {h} damping {damping}: lane {k} Dc {dc[k]:.0f}, bh {LB.bh(m, dc, b)[k]:.3g}, {big[:, k].max():.3f} of its limit, rb {p['rb'][:, k].min():.3f} .. "
          f"{p['rb'][:, k].max():.3f} of the lane's Bmax, {r['rb'][:, k].max():.3f} of the constant; the others' rb at most {np.delete(p['rb'], k, axis=1).max():.3f}")
    assert LB.clear(p) and (LB.bh(m, dc, b) > 8192.0).all()
    assert (p["rb"][:, k] > 1.1).all() and (r["rb"][:, k] < 0.9).all() and (r["D"][:, k] < 0.9).all() and not r["never"][k]  # the constant would free it
    assert p["need"][:, k].all() and not np.delete(p["need"], k, axis=1).any()
    assert big[:, k].min() > 1.05 and np.delete(big, k, axis=1).max() < 0.95 and S._largest(r).max() < 0.95
    _, acc, cnt = S._sampler(gpu_engine, m, dc, a, b, data, 1)
    print(f"steps {steps} h {h} damping {damping}: {cnt}")
    assert acc.all() and cnt["steps_redone"] >= T.TRIP and cnt["steps_narrow"] > 0 and cnt["steps_full"] == 0, cnt
    # wave 1 alone: T.predicted_unguarded of wave 0 is 0
    assert T.predicted_unguarded(p["need"][:, :X.WAVE]) == 0
    assert cnt["steps_unguarded"] == T.predicted_unguarded(p["need"][:, X.WAVE:]) == T.TRIP * (steps // T.TRIP), cnt
