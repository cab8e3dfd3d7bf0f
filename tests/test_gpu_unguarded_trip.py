"""
GPU tests: the float64 sampler's TIGHT trips with and without the guard (csrc/rsf_device.h: tight_needs_guard, trip_fast_ssq
GUARD = false) — the two paths give the same sum of squares to the bit, and the counter steps_unguarded says which one ran.

One replayed iteration that proposes the start point itself (test_gpu_step_forms._sampler), 128 chains = two waves,
delta_t = 0.025, damping on and off, step counts that walk the trip structure (35: two 16-step trips, a pair, the odd step;
18: one trip and a pair; 530: the resync at step 512 inside a run of trips).  What the sampler should have done is predicted
on the CPU by tests/tight_bound.py from the extended-precision trajectory: every lane here is at least 10 % away from the
bound's edge at every trip, so the prediction is exact.
  A       Dc in [600, 2000]: no lane needs the guard at any trip — every whole trip runs without it
  B       the same chains with lane 0 of each wave at Dc = 300: inside every guard, but beyond the bound at every trip — every
          trip keeps the guard, none is redone, and the 126 common lanes hold A's sums of squares bit for bit
  reject  A with lane 5 at Dc = 300 and a current SSq a quarter of its proposal's (sigma^2 ~ 0): it alone holds wave 0 to the
          guarded trips until its running sum has disqualified it, and no longer
  table   a caller's loading with range [0, 10 V_ref]: the bound works from that range; against the same chains with one lane
          per wave that this range — not the built-in history's — keeps under guard
"""
import numpy as np
import pytest

import rk4_extended as X
import test_gpu_step_forms as F
import tight_bound as T

pytestmark = pytest.mark.gpu

C = F.C
H = 0.025
_REF = {}


def _model(oracle_mod, steps, damping, loading=None):
    n = steps + 1
    m = oracle_mod.ModelSpec(n, 0.0, H * n, 1)
    m.RadiationDamping = damping
    assert m.nout == n and abs(m.delta_t - H) < 1e-15
    if loading is not None:
        m.loading = loading
    return m


def _data(oracle_mod, steps):
    """an observation: the built-in model's extended solve at Dc = 1000 plus |acc| N(0, 1) (the bench's recipe)"""
    if steps not in _REF:
        acc, _ = X.forward_ext(_model(oracle_mod, steps, True), np.array([1000.0]))
        acc = acc[:, 0].astype(np.float64)
        _REF[steps] = acc + np.abs(acc) * np.random.default_rng(steps).standard_normal(acc.size)
    return _REF[steps]


def _lanes(lo, hi, seed):
    return np.random.default_rng(seed).uniform(lo, hi, C)


def _scan(m, dc, steps):
    """tight_bound.scan over the whole trips, with the loading table the engine will be given"""
    vl = None
    if getattr(m, "loading", None) is not None:
        t = float(m.t_start) + np.arange(2 * steps + 1, dtype=np.float64) * (0.5 * float(m.delta_t))
        vl = m.loading(t)
    r = T.scan(m, dc, steps, vl=vl)
    # every decision at least 10 % from the bound's edge: the float64 predicate on the GPU decides the same
    clear = ((r["D"] < 0.9) & (r["rb"] < 0.9)) | (r["D"] > 1.1) | (r["rb"] > 1.1)
    assert clear.all(), (r["D"][~clear], r["rb"][~clear])
    clear = ((r["dmin"] < 0.9) & (r["rmin"] < 0.9)) | (r["dmin"] > 1.1) | (r["rmin"] > 1.1)  # the solve's gate (W.never) likewise
    assert clear.all(), (r["dmin"][~clear], r["rmin"][~clear])
    return r


def _inside_guards(r, lanes):
    return np.maximum.reduce([r[k][:, lanes] / thr for k, thr in T.GUARDS.items()])


def _predict(need, alive=None):
    return sum(T.predicted_unguarded(need[:, w * X.WAVE:(w + 1) * X.WAVE], None if alive is None else alive[:, w * X.WAVE:(w + 1) * X.WAVE])
               for w in range(C // X.WAVE))


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("steps", [35, 18, 530])
def test_both_paths_bit_for_bit(gpu_engine, oracle_mod, steps, damping):
    m, data = _model(oracle_mod, steps, damping), _data(oracle_mod, steps)
    trips = steps // T.TRIP
    every = np.full(C, 1e300)
    # ---- A ----
    dca = _lanes(600.0, 2000.0, 21)
    ra = _scan(m, dca, steps)
    assert not ra["need"].any() and ra["need"].shape == (trips, C)
    ssq_a, acc_a, cnt_a = F._sampler(gpu_engine, m, dca, data, every)
    print(f"steps {steps} damping {damping} A: {cnt_a}; bound margins D {ra['D'].max():.3f} rb {ra['rb'].max():.3f}")
    assert acc_a.all()
    assert cnt_a["steps_unguarded"] == _predict(ra["need"]) == 2 * T.TRIP * trips, cnt_a
    assert cnt_a["steps_tight"] == 2 * (steps - steps % 2) and cnt_a["steps_wide"] == 2 * (steps % 2), cnt_a  # an odd last step: WIDE series
    assert cnt_a["steps_redone"] == cnt_a["steps_narrow"] == cnt_a["steps_full"] == 0, cnt_a
    # ---- B ----
    dcb = dca.copy()
    dcb[::X.WAVE] = 300.0
    rb = _scan(m, dcb, steps)
    held = np.arange(0, C, X.WAVE)
    rel = _inside_guards(rb, held)
    print(f"steps {steps} damping {damping} B: the Dc = 300 lanes reach {rel.max():.3f} of a guard; bound D {rb['D'][:, held].min():.3f} rb {rb['rb'][:, held].min():.3f}")
    assert rel.max() < 0.7                    # inside every guard (|rho| 0.52, |dlt| 0.38 of the thresholds) ...
    assert rb["need"][:, held].all()          # ... and beyond the bound at every trip
    ssq_b, acc_b, cnt_b = F._sampler(gpu_engine, m, dcb, data, every)
    print(f"steps {steps} damping {damping} B: {cnt_b}")
    assert acc_b.all()
    assert cnt_b["steps_unguarded"] == _predict(rb["need"]) == 0, cnt_b
    assert cnt_b["steps_redone"] == cnt_b["steps_narrow"] == cnt_b["steps_full"] == 0 and cnt_b["steps_tight"] == cnt_a["steps_tight"], cnt_b
    common = np.ones(C, dtype=bool)
    common[held] = False
    assert common.sum() == C - 2
    assert np.array_equal(ssq_a[common], ssq_b[common])
    assert np.isfinite(ssq_b).all()
    # ---- reject ----
    k = 5
    dcr = dca.copy()
    dcr[k] = 300.0
    rr = _scan(m, dcr, steps)
    assert rr["need"][:, k].all() and not np.delete(rr["need"], k, axis=1).any()
    ssq_r, acc_r, _ = F._sampler(gpu_engine, m, dcr, data, every)  # the lanes' sums of squares, for the states below
    assert acc_r.all() and np.array_equal(np.delete(ssq_r, k), np.delete(ssq_a, k))
    ssq0 = ssq_r.copy()
    ssq0[k] *= 0.25
    std2 = every.copy()
    std2[k] = 1e-300  # accept iff ssq_new < ssq - 2 sigma^2 log u: the lane's bound is its current SSq
    # the lane's running sum at the trips' starts (extended precision): it stops counting at the end of the first trip that
    # STARTS with the sum beyond the bound (integrate_multi: the compare reads the sum as the previous trip left it)
    acc, _ = X.forward_ext(m, np.array([300.0]))
    part = np.cumsum((acc[:, 0] - X._w(data)) ** 2)[0:T.TRIP * trips:T.TRIP].astype(np.float64)  # after samples 0, 16, 32, ...
    thr = ssq0[k]
    assert (np.abs(part / thr - 1.0) > 1e-6).all()
    alive = np.ones((trips, C), dtype=bool)
    alive[1:, k] = part[:-1] <= thr
    ssq_e, acc_e, cnt_e = F._sampler(gpu_engine, m, dcr, data, std2, ssq0, 0.5)
    print(f"steps {steps} damping {damping} reject: {cnt_e}; lane {k} alive at the start of {int(alive[:, k].sum())} of {trips} trips")
    assert not acc_e[k] and ssq_e[k] == ssq0[k] and cnt_e["early_rejected"] == 1, (acc_e[k], ssq_e[k], ssq0[k], cnt_e)
    assert np.delete(acc_e, k).all() and np.array_equal(np.delete(ssq_e, k), np.delete(ssq_a, k))
    assert cnt_e["steps_unguarded"] == _predict(rr["need"], alive), cnt_e
    if steps == 530:
        assert T.TRIP * trips < cnt_e["steps_unguarded"] < 2 * T.TRIP * trips  # wave 0: guarded while the lane lived, not after
    assert cnt_e["steps_redone"] == cnt_e["steps_narrow"] == cnt_e["steps_full"] == 0, cnt_e


def _ends_table(t):
    """a caller's table whose range [0, 10 V_ref] comes from its two end entries alone — the first is felt by stage 1 of step 0,
    the last by stage 4 of the last step; in between the built-in history, so the lanes' increments are the usual ones and the
    RANGE is what decides the bound (V_ref = 1)"""
    v = 1.0 + np.exp(-t / 20) * np.sin(10 * t)
    v[0], v[-1] = 0.0, 10.0
    return v


@pytest.mark.parametrize("damping", [True, False])
def test_callers_loading_brings_its_own_range(gpu_engine, oracle_mod, damping):
    steps = 530
    m, data = _model(oracle_mod, steps, damping, _ends_table), _data(oracle_mod, steps)
    trips = steps // T.TRIP
    t = np.arange(2 * steps + 1, dtype=np.float64) * (0.5 * float(m.delta_t))
    tab = _ends_table(t)
    assert tab.min() == 0.0 and tab.max() == 10.0
    every = np.full(C, 1e300)
    dcu = _lanes(1350.0, 3000.0, 23)
    ru = _scan(m, dcu, steps)
    ssq_u, acc_u, cnt_u = F._sampler(gpu_engine, m, dcu, data, every)
    print(f"table damping {damping}: {cnt_u}; bound margins D {ru['D'].max():.3f} rb {ru['rb'].max():.3f}")
    assert acc_u.all()
    assert cnt_u["steps_unguarded"] == _predict(ru["need"]) == 2 * T.TRIP * trips, cnt_u
    assert cnt_u["steps_redone"] == cnt_u["steps_narrow"] == cnt_u["steps_full"] == 0, cnt_u
    # the guarded run: lane 0 of each wave at Dc = 1000.  By the table's range |V_l - v| may reach 9 V_ref, |dlt| 1.17 x the bound's
    # limit, at every trip; a range hard-coded to the built-in history's [0, 2 V_ref] would have freed the lane
    dcg = dcu.copy()
    held = np.arange(0, C, X.WAVE)
    dcg[held] = 1000.0
    rg = _scan(m, dcg, steps)
    assert rg["need"][:, held].all() and _inside_guards(rg, held).max() < 0.5
    assert not T.scan(m, dcg, steps, vl=tab, vl_range=(0.0, 2.0))["need"].any()
    ssq_g, acc_g, cnt_g = F._sampler(gpu_engine, m, dcg, data, every)
    print(f"table damping {damping} guarded: {cnt_g}")
    assert acc_g.all() and cnt_g["steps_unguarded"] == _predict(rg["need"]) == 0, cnt_g
    assert cnt_g["steps_redone"] == cnt_g["steps_narrow"] == cnt_g["steps_full"] == 0, cnt_g
    common = np.ones(C, dtype=bool)
    common[held] = False
    assert np.array_equal(ssq_u[common], ssq_g[common])
