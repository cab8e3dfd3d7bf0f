"""
GPU tests: the float64 sampler's in-step TIGHT step with the stage stiffness folded into the series constants
(csrc/rsf_device.h: struct Series, tight_incr_scaled) — the increments are carried as del = dlt / k, the series' coefficients
hold the powers of k, and the guard compares |del| with per-lane thresholds.

One replayed iteration that proposes the start point itself (as test_gpu_step_forms._sampler does), 128 chains = two waves,
delta_t = 0.025 and 0.1, damping on and off, step counts that walk the trip structure (35: two 16-step trips, a pair, the
odd step; 200: twelve trips and four pairs; 530: the resync at step 512 inside a run of trips), one parameter and three
(per-lane a in [0.009, 0.013], b - a in [-0.003, 0.006]).  Lanes:
  wave 0   headline-like: Dc log-uniform from 300 (or 1 % above TIGHT's a-priori edge, where that is higher) to 5000
  wave 1   every lane's Dc found on the CPU (bisection on tight_bound.scan, the extended-precision trajectory) so that its
           largest increment sits at a chosen 0.5 .. 0.9 of the guard threshold that binds for it (|rho| and |c1| at
           delta_t = 0.025, |dlt| of the half-step and full-step stages at 0.1; up to 0.98 of what the a-priori edge allows)
Accuracy   the sampler's SSq against the extended-precision RK4: per wave, max and median of its error within FACTOR (4) x the
           CPU restatement's — a plain float64 RK4 — on the same lanes (x test_gpu_rk4_extended's SSQ_FLOOR where that is at
           rounding level itself), and the max under its SSQ_CAP.
Guard      what the guard should have done, from the extended-precision maxima of every trip (tight_bound.scan): lanes below
           0.95 x every threshold stay in TIGHT — nothing redone, every step a TIGHT step; a lane above 1.05 x some threshold
           leaves it — its trip is redone and its wave goes on in NARROW.  Over-lanes by |rho| (delta_t = 0.025, the built-in
           loading) and by |dlt| (delta_t = 0.1 and a caller's loading of amplitude 1.8 V_ref: the a-priori edge knows 1.2),
           the second kind being what the per-lane thresholds on del decide.  No lane lies between 0.95 and 1.05.
Paths      wave 0 far enough inside the a-priori bound of tight_needs_guard to run without the guard; wave 1 the same Dc, but
           for one lane that keeps it under the guard at every trip: the 63 common lanes agree bit for bit.
"""
import numpy as np
import pytest

import rk4_extended as X
import test_gpu_rk4_extended as R
import tight_bound as T

pytestmark = pytest.mark.gpu

C = 2 * X.WAVE
FACTOR = 4.0
STEPS = [35, 200, 530]
_REF = {}


def _model(oracle_mod, steps, h, damping, loading=None):
    n = steps + 1
    m = oracle_mod.ModelSpec(n, 0.0, h * n, 1)
    m.RadiationDamping = damping
    assert m.nout == n and abs(m.delta_t - h) < 1e-15
    if loading is not None:
        m.loading = loading
    return m


def _ab(m, d, lanes, seed):
    """per-lane (a, b): the model's for one parameter, off the defaults for three"""
    if d == 1:
        return np.full(lanes, float(m.a)), np.full(lanes, float(m.b))
    a = np.random.default_rng(seed).uniform(0.009, 0.013, lanes)
    return a, X.lane_b(a, lanes, seed)


def _edge(m, a):
    return X.tier_edges(m, a)[0]


def _table(m, steps):
    if getattr(m, "loading", None) is None:
        return None
    t = float(m.t_start) + np.arange(2 * steps + 1, dtype=np.float64) * (0.5 * float(m.delta_t))
    return m.loading(t)


def _scan(m, dc, a, b, steps, d):
    kw = {} if d == 1 else {"a": a, "b": b}
    return T.scan(m, dc, steps, vl=_table(m, steps), **kw)


def _largest(r):
    """(trips, lanes): the trip's largest increment over its own threshold"""
    return np.maximum.reduce([r[k] / thr for k, thr in T.GUARDS.items()])


def _place(m, a, b, steps, d, target, lo_factor=1.005):
    """Dc per lane, above lo_factor x TIGHT's a-priori edge, at which the lane's largest increment of the whole series is `target`
    x its threshold (log-bisection: the figure falls monotonically with Dc) — or 0.98 of what the edge allows, if that is less"""
    lo = lo_factor * _edge(m, a)
    top = _largest(_scan(m, lo, a, b, steps, d)).max(axis=0)
    target = np.minimum(target, 0.98 * top)
    hi = 200.0 * lo
    for _ in range(11):  # (Dc to 0.3 %, the figure to 0.6 %)
        mid = np.sqrt(lo * hi)
        above = _largest(_scan(m, mid, a, b, steps, d)).max(axis=0) > target
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    return np.sqrt(lo * hi), target


def _headline_wave(m, a, seed):
    lo = np.maximum(300.0, 1.01 * _edge(m, a))
    return np.exp(np.random.default_rng(seed).uniform(np.log(lo), np.log(5000.0)))


def _data(oracle_mod, steps, h):
    """an observation: the built-in model's extended solve at Dc = 1000 plus |acc| N(0, 1) (the bench's recipe)"""
    key = ("data", steps, h)
    if key not in _REF:
        acc, _ = X.forward_ext(_model(oracle_mod, steps, h, True), np.array([1000.0]))
        acc = acc[:, 0].astype(np.float64)
        _REF[key] = acc + np.abs(acc) * np.random.default_rng(steps).standard_normal(acc.size)
    return _REF[key]


def _reference(cpu_engine, oracle_mod, steps, h, damping, d):
    """model, lanes, observation, the trips' extended-precision maxima, extended SSq and the restatement's SSq errors (computed once)"""
    key = (steps, h, damping, d)
    if key not in _REF:
        m, data = _model(oracle_mod, steps, h, damping), _data(oracle_mod, steps, h)
        a, b = _ab(m, d, C, 31)
        dc = np.empty(C)
        dc[:X.WAVE] = _headline_wave(m, a[:X.WAVE], 32)
        want = np.linspace(0.5, 0.9, X.WAVE)
        dc[X.WAVE:], want = _place(m, a[X.WAVE:], b[X.WAVE:], steps, d, want)
        r = _scan(m, dc, a, b, steps, d)
        kw = {} if d == 1 else {"a": a, "b": b}
        _, ssq_ext = X.forward_ext(m, dc, data=data, **kw)
        assert cpu_engine.set_model(m, 1) == data.size
        s_cpu, _ = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=False, **kw)
        o = (np.abs(X._w(s_cpu) - ssq_ext) / ssq_ext).astype(np.float64)
        _REF[key] = (m, dc, a, b, data, r, want, ssq_ext, o)
    return _REF[key]


def _sampler(engine, m, dc, a, b, data, d):
    """one replayed iteration that proposes the start point itself (z = 0) with forced acceptance (sigma^2 = 1e300)
    -> (state SSq, accept flags, counter deltas)"""
    lanes = dc.size
    engine.set_model(m, 1)
    q0 = dc.reshape(lanes, 1) if d == 1 else np.stack([dc, a, b], axis=1)
    engine.mcmc_init(q0, data, [0.0] * d, [100.0 * dc.max()] + [1.0] * (d - 1), seed=17, prior_len=3)
    V = np.zeros((lanes, d, d))
    for k in range(d):
        V[:, k, k] = (1e-7 * q0[:, k]) ** 2
    engine.set_state(q=q0, V=V, std2=np.full(lanes, 1e300))
    c0 = engine.counters()
    _, _, ta = engine.mcmc_replay(np.zeros((1, lanes, d)), np.full((1, lanes), 1e-300), np.full((1, lanes), 250.0))
    c1 = engine.counters()
    return np.array(engine.get_state()[1]), np.array(ta[0]).astype(bool), {k: c1[k] - c0[k] for k in c1 if k.startswith(("steps", "early"))}


def _all_tight(cnt, steps, waves=2):
    return (cnt["steps_redone"] == cnt["steps_narrow"] == cnt["steps_full"] == 0 and cnt["steps_tight"] == waves * (steps - steps % 2)
            and cnt["steps_wide"] == waves * (steps % 2))  # an odd last step: the WIDE series whatever the tier


CASES = [(s, h, damping, 1) for s in STEPS for h in (0.025, 0.1) for damping in (True, False)] + \
        [(s, h, True, 3) for s in (35, 530) for h in (0.025, 0.1)] + [(200, 0.025, False, 3)]


@pytest.mark.parametrize("steps,h,damping,d", CASES)
def test_rescaled_step_within_float64_rounding(gpu_engine, cpu_engine, oracle_mod, steps, h, damping, d):
    m, dc, a, b, data, r, want, ssq_ext, o = _reference(cpu_engine, oracle_mod, steps, h, damping, d)
    tag = f"steps {steps} h {h} damping {damping} d {d}"
    big = _largest(r)
    top = big.max(axis=0)
    which = [max(T.GUARDS, key=lambda k: (r[k][:, i] / T.GUARDS[k]).max()) for i in (X.WAVE, C - 1)]
    print(f"{tag}: wave 0 Dc {dc[0]:.0f} .. {dc[X.WAVE - 1]:.0f}, largest increment {top[:X.WAVE].max():.3f} of its threshold; "
          f"wave 1 Dc {dc[X.WAVE:].min():.0f} .. {dc[X.WAVE:].max():.0f}, {top[X.WAVE:].min():.3f} .. {top[X.WAVE:].max():.3f} "
          f"(binding: {which[0]} .. {which[1]})")
    # the lanes are where they were meant to be: wave 1 at its targets, every lane below 0.95 of every threshold
    assert np.allclose(top[X.WAVE:], want, rtol=1e-2) and want.min() >= 0.49 and want.max() > 0.75, (top[X.WAVE:], want)
    assert top.max() < 0.95
    ssq, acc, cnt = _sampler(gpu_engine, m, dc, a, b, data, d)
    print(f"{tag}: counters {cnt}")
    assert acc.all(), f"{tag}: {int((~acc).sum())} chains did not accept"
    # guard equivalence, the lanes that stay: nothing redone, every step of both waves a TIGHT step
    assert _all_tight(cnt, steps), cnt
    g = (np.abs(X._w(ssq) - ssq_ext) / ssq_ext).astype(np.float64)
    fails = []
    for w in range(2):
        sl = slice(X.WAVE * w, X.WAVE * (w + 1))
        R._check(f"{tag} wave {w}", g[sl], o[sl], FACTOR, R.SSQ_FLOOR, R.SSQ_CAP, fails)
    assert not fails, fails


def _clear(r):
    """every decision of the a-priori bound at least 10 % from its edge: the float64 predicate on the GPU decides the same"""
    ok = ((r["D"] < 0.9) & (r["rb"] < 0.9)) | (r["D"] > 1.1) | (r["rb"] > 1.1)
    return bool(ok.all() and (((r["dmin"] < 0.9) & (r["rmin"] < 0.9)) | (r["dmin"] > 1.1) | (r["rmin"] > 1.1)).all())


def _strong_loading(t):
    """a caller's loading of amplitude 1.8 V_ref (V_ref = 1): |V_l - v| passes the 1.2 V_ref that TIGHT's a-priori edge allows for"""
    return 1.0 + 1.8 * np.exp(-t / 20) * np.sin(10 * t)


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("kind", ["rho", "dlt"])
def test_guard_on_the_rescaled_increments(gpu_engine, oracle_mod, kind, damping):
    steps = 200
    h, loading = (0.025, None) if kind == "rho" else (0.1, _strong_loading)
    m, data = _model(oracle_mod, steps, h, damping, loading), _data(oracle_mod, steps, h)
    a, b = _ab(m, 1, C, 0)
    # the lanes that stay: both waves at 0.3 .. 0.9 of the binding threshold
    dc, _ = _place(m, a, b, steps, 1, np.linspace(0.3, 0.9, C))
    r = _scan(m, dc, a, b, steps, 1)
    big = _largest(r)
    binding = max(T.GUARDS, key=lambda k: (r[k] / T.GUARDS[k]).max())
    print(f"{kind} damping {damping}: Dc {dc.min():.0f} .. {dc.max():.0f}, largest increments {big.max(axis=0).min():.3f} .. {big.max():.3f}, binding {binding}")
    assert big.max() < 0.95 and big.max() > 0.85 and binding in (("rho", "c1") if kind == "rho" else ("dlt", "dlt_h"))
    _, acc, cnt = _sampler(gpu_engine, m, dc, a, b, data, 1)
    print(f"{kind} damping {damping} inside: {cnt}")
    assert acc.all() and _all_tight(cnt, steps), cnt
    # the lanes that leave: one at a time in place of lane 7 of wave 0, at 1.07 .. 1.35 of the threshold
    for over in (1.07, 1.15, 1.35):
        dco = dc.copy()
        k = 7
        dck, got = _place(m, a[k:k + 1], b[k:k + 1], steps, 1, np.array([over]))
        dco[k] = dck[0]
        ro = _scan(m, dco, a, b, steps, 1)
        bo = _largest(ro)
        assert got[0] == over and abs(bo[:, k].max() / over - 1.0) < 1e-2, (bo[:, k].max(), got, over)  # (the a-priori edge lies beyond: the lane starts in TIGHT)
        band = (bo > 0.95) & (bo < 1.05)
        first = int(np.argmax(bo[:, k] > 1.05))
        assert not band[:first + 1].any() and (np.delete(bo, k, axis=1) < 0.95).all()
        _, acc_o, cnt_o = _sampler(gpu_engine, m, dco, a, b, data, 1)
        print(f"{kind} damping {damping} lane at {over}: first trip over its threshold {first}, {cnt_o}")
        assert acc_o.all()
        # wave 1 as before; wave 0: TIGHT up to and with that trip, the trip redone, NARROW from there on
        assert cnt_o["steps_redone"] >= T.TRIP and cnt_o["steps_narrow"] > 0 and cnt_o["steps_full"] == 0, cnt_o
        assert cnt_o["steps_tight"] >= (steps - steps % 2) + T.TRIP * (first + 1), cnt_o
        assert cnt_o["steps_tight"] + cnt_o["steps_narrow"] + cnt_o["steps_wide"] == 2 * steps, cnt_o


@pytest.mark.parametrize("steps,h,damping,d", [(s, h, damping, 1) for s in STEPS for h in (0.025, 0.1) for damping in (True, False)] +
                         [(200, 0.025, True, 3), (530, 0.1, True, 3)])
def test_guarded_and_unguarded_trips_bit_for_bit(gpu_engine, oracle_mod, steps, h, damping, d):
    m, data = _model(oracle_mod, steps, h, damping), _data(oracle_mod, steps, h)
    trips = steps // T.TRIP
    a1, b1 = _ab(m, d, X.WAVE, 41)
    a, b = np.tile(a1, 2), np.tile(b1, 2)
    # increments at 0.02 .. 0.1 of their thresholds: far inside the a-priori bound as well
    free, _ = _place(m, a1, b1, steps, d, np.linspace(0.02, 0.1, X.WAVE))
    dc = np.tile(free, 2)
    dc[X.WAVE] = _place(m, a[X.WAVE:X.WAVE + 1], b[X.WAVE:X.WAVE + 1], steps, d, np.array([0.6]))[0][0]
    r = _scan(m, dc, a, b, steps, d)
    assert _clear(r), (r["D"].max(axis=0), r["rb"].max(axis=0))
    need = r["need"]
    assert need[:, X.WAVE].all() and not np.delete(need, X.WAVE, axis=1).any() and _largest(r).max() < 0.7
    ssq, acc, cnt = _sampler(gpu_engine, m, dc, a, b, data, d)
    print(f"steps {steps} h {h} damping {damping} d {d}: Dc {free.min():.0f} .. {free.max():.0f} and {dc[X.WAVE]:.0f}; {cnt}")
    assert acc.all() and _all_tight(cnt, steps), cnt
    assert cnt["steps_unguarded"] == T.TRIP * trips, cnt  # wave 0: every whole trip without the guard; wave 1: none
    assert np.isfinite(ssq).all() and np.array_equal(ssq[1:X.WAVE], ssq[X.WAVE + 1:])
