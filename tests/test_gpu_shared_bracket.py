"""
GPU tests: the float64 sampler's in-step TIGHT step with one log1p bracket for its two half-step stages (csrc/rsf_device.h:
rk4_tight INSTEP, tight_incr_scaled, tight_bracket) and the per-lane limit on rho that goes with it (tight_pb_limit, through
Series::lim_rho / lim_c1 / bmax), restated in tests/shared_bracket.py.

One replayed iteration that proposes the start point itself (test_gpu_series_scale._sampler), 128 chains = two waves, delta_t = 0.025
and 0.1, damping on and off, one parameter and three (per-lane a in [0.009, 0.013], b - a in [-0.003, 0.006]), step counts 35, 530
and 1100.  Lanes (placed once per (delta_t, damping, d) on the first PLACED steps, where the loading is largest, and checked on the
whole series):
  wave 0   headline-like: Dc log-uniform from 300 (or 1 % above TIGHT's a-priori edge, where that is higher) to 5000
  wave 1   every lane at a chosen 0.5 .. 0.9 of the guard threshold that binds for it, the new limit among them
SSq       against the extended-precision RK4, at test_gpu_rk4_extended's tolerance (R._check with its FACTOR_SSQ, SSQ_FLOOR, SSQ_CAP):
          per wave, max and median within FACTOR_SSQ x a plain float64 RK4's — the CPU restatement — on the same lanes.
counters  steps per tier, steps redone, steps without the guard and early rejections equal to PARENT: what the build of the parent
          commit (every stage its own bracket, no tight_pb_limit) gave on the same inputs, recorded from a run of that build on an
          MI355X (profiles/shared_bracket/parent_and_new_cases.log).  No decision may move.
paths     twin waves, one free of the guard at every trip and one held under it by a single lane (tests/linear_bracket.py's
          paths_lanes, the restated predicate with the new bmax): the 63 common lanes agree bit for bit.
"""
import numpy as np
import pytest

import linear_bracket as LB
import rk4_extended as X
import shared_bracket as SB
import test_gpu_rk4_extended as R
import test_gpu_series_scale as S
import tight_bound as T

pytestmark = pytest.mark.gpu

C = 2 * X.WAVE
STEPS = [35, 530, 1100]
PLACED = 200
CASES = [(steps, h, damping, d) for steps in STEPS for h in (0.025, 0.1) for damping in (True, False) for d in (1, 3)]
_REF = {}


def _place(m, a, b, steps, d, target):
    """linear_bracket.place against the thresholds with the new limit"""
    lo = 1.005 * S._edge(m, a) * np.ones(np.shape(target))

    def top(dc):
        return SB.largest(S._scan(m, dc, a, b, steps, d), m, dc, a, b).max(axis=0)

    target = np.minimum(target, 0.98 * top(lo))
    hi = 1.0e5 * lo
    for _ in range(13):
        mid = np.sqrt(lo * hi)
        above = top(mid) > target
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    return np.sqrt(lo * hi), target


def lanes(oracle_mod, h, damping, d):
    key = ("lanes", h, damping, d)
    if key not in _REF:
        m = S._model(oracle_mod, PLACED, h, damping)
        a, b = S._ab(m, d, C, 31)
        dc = np.empty(C)
        dc[:X.WAVE] = S._headline_wave(m, a[:X.WAVE], 32)
        dc[X.WAVE:], want = _place(m, a[X.WAVE:], b[X.WAVE:], PLACED, d, np.linspace(0.5, 0.9, X.WAVE))
        _REF[key] = (dc, a, b, want)
    return _REF[key]


def _reference(cpu_engine, oracle_mod, steps, h, damping, d):
    """model, lanes, observation, the trips' extended-precision maxima, extended SSq and the restatement's SSq errors (computed once)"""
    key = (steps, h, damping, d)
    if key not in _REF:
        m, data = S._model(oracle_mod, steps, h, damping), S._data(oracle_mod, steps, h)
        dc, a, b, want = lanes(oracle_mod, h, damping, d)
        r = S._scan(m, dc, a, b, steps, d)
        kw = {} if d == 1 else {"a": a, "b": b}
        _, ssq_ext = X.forward_ext(m, dc, data=data, **kw)
        assert cpu_engine.set_model(m, 1) == data.size
        s_cpu, _ = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=False, **kw)
        o = (np.abs(X._w(s_cpu) - ssq_ext) / ssq_ext).astype(np.float64)
        _REF[key] = (m, dc, a, b, data, r, want, ssq_ext, o)
    return _REF[key]


def run_case(gpu_engine, cpu_engine, oracle_mod, steps, h, damping, d):
    """-> (SSq errors of the sampler, of the plain float64 RK4, accept flags, counter deltas)"""
    m, dc, a, b, data, _, _, ssq_ext, o = _reference(cpu_engine, oracle_mod, steps, h, damping, d)
    ssq, acc, cnt = S._sampler(gpu_engine, m, dc, a, b, data, d)
    g = (np.abs(X._w(ssq) - ssq_ext) / ssq_ext).astype(np.float64)
    return g, o, acc, {k: int(v) for k, v in cnt.items()}


def case_id(steps, h, damping, d):
    return f"{steps}-{h}-{'damp' if damping else 'nodamp'}-d{d}"


def _cnt(tight, narrow, wide, full, redone, unguarded, early_rejected):
    return {"steps_tight": tight, "steps_narrow": narrow, "steps_wide": wide, "steps_full": full, "steps_redone": redone,
            "steps_unguarded": unguarded, "early_rejected": early_rejected}


# The counters of the parent commit's build on these inputs (see the module's docstring), by case_id:
# wave-steps tight, narrow, wide, full, redone, without the guard; early rejections.
PARENT = {
    "35-0.025-damp-d1": _cnt(68, 0, 2, 0, 0, 0, 0),
    "35-0.025-damp-d3": _cnt(68, 0, 2, 0, 0, 0, 0),
    "35-0.025-nodamp-d1": _cnt(68, 0, 2, 0, 0, 0, 0),
    "35-0.025-nodamp-d3": _cnt(68, 0, 2, 0, 0, 0, 0),
    "35-0.1-damp-d1": _cnt(68, 0, 2, 0, 0, 0, 0),
    "35-0.1-damp-d3": _cnt(68, 0, 2, 0, 0, 0, 0),
    "35-0.1-nodamp-d1": _cnt(68, 0, 2, 0, 0, 0, 0),
    "35-0.1-nodamp-d3": _cnt(68, 0, 2, 0, 0, 0, 0),
    "530-0.025-damp-d1": _cnt(1060, 0, 0, 0, 0, 0, 0),
    "530-0.025-damp-d3": _cnt(1060, 0, 0, 0, 0, 0, 0),
    "530-0.025-nodamp-d1": _cnt(1060, 0, 0, 0, 0, 0, 0),
    "530-0.025-nodamp-d3": _cnt(1060, 0, 0, 0, 0, 0, 0),
    "530-0.1-damp-d1": _cnt(1060, 0, 0, 0, 0, 0, 0),
    "530-0.1-damp-d3": _cnt(1060, 0, 0, 0, 0, 0, 0),
    "530-0.1-nodamp-d1": _cnt(1060, 0, 0, 0, 0, 0, 0),
    "530-0.1-nodamp-d3": _cnt(1060, 0, 0, 0, 0, 0, 0),
    "1100-0.025-damp-d1": _cnt(2200, 0, 0, 0, 0, 0, 0),
    "1100-0.025-damp-d3": _cnt(2200, 0, 0, 0, 0, 0, 0),
    "1100-0.025-nodamp-d1": _cnt(2200, 0, 0, 0, 0, 0, 0),
    "1100-0.025-nodamp-d3": _cnt(2200, 0, 0, 0, 0, 0, 0),
    "1100-0.1-damp-d1": _cnt(2200, 0, 0, 0, 0, 0, 0),
    "1100-0.1-damp-d3": _cnt(2200, 0, 0, 0, 0, 0, 0),
    "1100-0.1-nodamp-d1": _cnt(2200, 0, 0, 0, 0, 0, 0),
    "1100-0.1-nodamp-d3": _cnt(2200, 0, 0, 0, 0, 0, 0),
}


@pytest.mark.parametrize("steps,h,damping,d", CASES, ids=[case_id(*c) for c in CASES])
def test_shared_bracket_within_float64_rounding(gpu_engine, cpu_engine, oracle_mod, steps, h, damping, d):
    m, dc, a, b, data, r, want, ssq_ext, o = _reference(cpu_engine, oracle_mod, steps, h, damping, d)
    tag = case_id(steps, h, damping, d)
    top = SB.largest(r, m, dc, a, b).max(axis=0)
    bind = SB.binding(r, m, dc, a, b)
    print(f"{tag}: wave 0 Dc {dc[:X.WAVE].min():.0f} .. {dc[:X.WAVE].max():.0f}, largest increment {top[:X.WAVE].max():.3f} of its threshold; wave 1 Dc "
          f"{dc[X.WAVE:].min():.0f} .. {dc[X.WAVE:].max():.0f}, {top[X.WAVE:].min():.3f} .. {top[X.WAVE:].max():.3f}; binding {sorted(set(bind[X.WAVE:]))}")
    # the lanes are where they were meant to be: wave 1 at its targets on the steps it was placed on, and nowhere beyond them later
    assert want.min() >= 0.49 and want.max() > 0.75 and top.max() < 0.95, (top.max(), want)
    if steps >= PLACED:
        assert (top[X.WAVE:] > (1.0 - 1e-2) * want).all(), (top[X.WAVE:], want)
    g, o, acc, cnt = run_case(gpu_engine, cpu_engine, oracle_mod, steps, h, damping, d)
    print(f"{tag}: counters {cnt}")
    assert acc.all(), f"{tag}: {int((~acc).sum())} chains did not accept"
    assert S._all_tight(cnt, steps), cnt  # every lane below 0.95 of every threshold: nothing redone, every step a TIGHT step
    fails = []
    for w in range(2):
        sl = slice(X.WAVE * w, X.WAVE * (w + 1))
        R._check(f"{tag} wave {w}", g[sl], o[sl], R.FACTOR_SSQ, R.SSQ_FLOOR, R.SSQ_CAP, fails)
    assert not fails, fails
    assert cnt == PARENT[tag], (cnt, PARENT[tag])


PATHS = [(35, 0.025, True, 1), (530, 0.025, False, 1), (530, 0.1, True, 1), (200, 0.025, True, 3), (530, 0.1, True, 3)]


@pytest.mark.parametrize("steps,h,damping,d", PATHS)
def test_guarded_and_unguarded_trips_bit_for_bit(gpu_engine, oracle_mod, steps, h, damping, d):
    m, dc, a, b = LB.paths_lanes(oracle_mod, steps, h, damping, d)
    data, trips = S._data(oracle_mod, steps, h), steps // T.TRIP
    r = S._scan(m, dc, a, b, steps, d)
    p = SB.predicate(r, m, dc, a, b)
    assert LB.clear(p), (p["D"].max(axis=0), p["rb"].max(axis=0))
    need = p["need"]
    assert need[:, X.WAVE].all() and not np.delete(need, X.WAVE, axis=1).any() and SB.largest(r, m, dc, a, b).max() < 0.7
    ssq, acc, cnt = S._sampler(gpu_engine, m, dc, a, b, data, d)
    print(f"steps {steps} h {h} damping {damping} d {d}: Dc {dc[:X.WAVE].min():.0f} .. {dc[:X.WAVE].max():.0f} and {dc[X.WAVE]:.0f}; "
          f"rb {p['rb'][:, :X.WAVE].max():.3f} of the lane's limit; {cnt}")
    assert acc.all() and S._all_tight(cnt, steps), cnt
    assert cnt["steps_unguarded"] == T.TRIP * trips, cnt  # wave 0: every whole trip without the guard; wave 1: none
    assert np.isfinite(ssq).all() and np.array_equal(ssq[1:X.WAVE], ssq[X.WAVE + 1:])


# --- the new limit decides -----------------------------------------------------------------------------------------------------------

def _scan_new(m, dc, a, b, steps, d):
    r = S._scan(m, dc, a, b, steps, d)
    return r, SB.largest(r, m, dc, a, b), SB.predicate(r, m, dc, a, b)


def binding_lanes(oracle_mod, steps, damping, d, k=7):
    """shared_bracket.binding_model: both waves the same 64 lanes at 0.27 .. 0.45 of the new limit — free under the lane's bmax —, then
    lane k of wave 0 at 0.9 and at 1.15 of it.  -> (m, a, b, {target: dc})"""
    key = ("binding", steps, damping, d)
    if key not in _REF:
        m = SB.binding_model(lambda *args: S._model(oracle_mod, *args), steps, damping)
        a1, _ = S._ab(m, d, X.WAVE, 31)
        a = np.tile(a1, 2)
        b = SB.BOA * a
        free, _ = _place(m, a1, b[:X.WAVE], steps, d, np.linspace(0.27, 0.45, X.WAVE))
        sets = {}
        for target in (0.9, 1.15):
            dc = np.tile(free, 2)
            dck, got = _place(m, a[k:k + 1], b[k:k + 1], steps, d, np.array([target]))
            assert got[0] == target
            dc[k] = dck[0]
            sets[target] = dc
        _REF[key] = (m, a, b, sets)
    return _REF[key]


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("damping", [True, False])
def test_the_shared_brackets_limit_decides(gpu_engine, oracle_mod, damping, d):
    steps, k = 200, 7
    trips = steps // T.TRIP
    m, a, b, sets = binding_lanes(oracle_mod, steps, damping, d)
    data = S._data(oracle_mod, steps, SB.H_BIND)
    others = np.delete(np.arange(C), k)
    for target, dc in sets.items():
        r, big, p = _scan_new(m, dc, a, b, steps, d)
        old = LB.largest(r, m, dc, b)
        rh = SB.rh_entry(m, dc, r["theta"])
        print(f"damping {damping} d {d} lane {k} at {target}: Dc {dc[k]:.0f} (the others {dc[others].min():.0f} .. {dc[others].max():.0f}), {big[:, k].max():.3f} of its limit in trip "
              f"{int(np.argmax(big[:, k]))}, {old[:, k].max():.3f} of the parent's; lim_pb / the parent's limit {(SB.thresholds(m, dc, a, b)['rho'] / LB.lim_rho(m, dc, b)).max():.3f} at most; "
              f"rb of the lane {p['rb'][:, k].min():.3f} .. {p['rb'][:, k].max():.3f}, of the others {p['rb'][:, others].max():.3f} at most; Rh moves by {(rh.max(axis=0) / rh.min(axis=0)).max() - 1:.1e}")
        # the new limit is what binds, for lane k and most of the others (all of them with the model's a); the parent's thresholds are
        # nowhere near — that build keeps lane k either way
        bind = SB.binding(r, m, dc, a, b)
        assert bind[k] == "pb" and (bind == "pb").sum() >= (C if d == 1 else C // 2) and old.max() < 0.6, (bind, old.max())
        assert abs(big[:, k].max() / target - 1.0) < 1e-2 and big[0, k] == big[:, k].max() and big[:, others].max() < 0.5
        assert (rh.max(axis=0) / rh.min(axis=0)).max() < 1.01  # the limit a later loop entry forms is the first one's to 1 %
        # the a-priori bound: lane k needs the guard at every trip, no other lane at any — every decision 10 % from its edge
        assert LB.clear(p) and p["need"][:, k].all() and not p["need"][:, others].any(), (p["rb"][:, k], p["rb"][:, others].max())
        _, acc, cnt = S._sampler(gpu_engine, m, dc, a, b, data, d)
        print(f"damping {damping} d {d} lane {k} at {target}: {cnt}")
        assert acc.all()
        # wave 1, the twin without that lane: every whole trip without the guard; wave 0: none
        assert cnt["steps_unguarded"] == T.TRIP * trips, cnt
        if target < 1.0:
            assert S._all_tight(cnt, steps), cnt  # stays: nothing redone, every step a TIGHT step
        else:  # leaves in its first trip: that trip redone, the wave on in NARROW
            assert cnt["steps_redone"] >= T.TRIP and cnt["steps_narrow"] > 0 and cnt["steps_full"] == 0, cnt
            assert cnt["steps_tight"] >= (steps - steps % 2) + T.TRIP and cnt["steps_narrow"] >= T.TRIP, cnt
            assert cnt["steps_tight"] + cnt["steps_narrow"] + cnt["steps_wide"] == 2 * steps, cnt
