"""
GPU tests: the float64 sampler's in-step TIGHT trips without the carried ms and without the resync (csrc/rsf_device.h: rk4_tight
INSTEP, rebuild_ms, Wave::ms_stale) — whoever reads ms after in-step trips forms it from (W, Rh) first.

One replayed iteration that proposes the start point itself (test_gpu_series_scale._sampler: test_gpu_step_forms._sampler for one
parameter or three), 128 chains = two waves, damping on and off, one parameter and three (per-lane a in [0.009, 0.013], b - a in
[-0.003, 0.006]).  Step counts: 35; 530, which crosses the old resync point at step 512 inside a run of trips; 1100, which
crosses two of them.  Lane sets (Dc ranges and placement are test_gpu_series_scale's: _headline_wave, _place):
  tight  h = 0.025, the built-in loading: wave 0 headline-like (Dc log-uniform 300 .. 5000, in-step trips under the guard), wave 1
         with every increment at 0.02 .. 0.1 of its threshold (placed on the first 200 steps, where the loading is largest): far
         enough inside the a-priori bound to run its whole trips without the guard;
  bump   h = 0.1, a caller's loading: the built-in one plus a burst of amplitude 1.0 V_ref around t = 2.4 (step 24; its envelope
         exp(-((t - 2.4) / 0.3)^2) leaves nothing of it in the first 16 steps).  Every lane at 0.3 .. 0.9 of the guard threshold
         that binds for it, lane 7 of wave 0 at 1.15: its guard trips at the burst, after in-step trips have run — the cold trip
         reads a rebuilt ms —, its wave goes on in NARROW (the handover reads it too) and comes back to TIGHT once the burst has
         passed;
  full   h = 0.1, a caller's loading with a surge of 40 V_ref that sets in at t = 2.2 (step 22, after one clean trip) and fades over
         the next three seconds: headline-like lanes from 1 % above TIGHT's a-priori edge, which knows 1.2 V_ref.  The guards of
         TIGHT, NARROW and WIDE trip in turn and, in the series long enough for it (530, 1100), the small-Dc lanes reach the FULL
         tier, which starts from the ms rebuilt at the first handover; the waves then stay in NARROW across step 512, whose
         resync reads it too.
Checks:
  SSq       against the extended-precision RK4 on the engine's own loading table (ms_free.walk_ext), at test_gpu_rk4_extended's
            tolerance: per wave, max and median within FACTOR_SSQ (8) x a plain float64 RK4's on the same lanes (x SSQ_FLOOR where
            that is at rounding level itself), the max under SSQ_CAP (5e-13).  The plain float64 RK4 is the CPU restatement where
            it has the loading (tight) and the literal RK4 in float64 (ms_free.walk_ext, dtype float64) under a caller's loading,
            which the restatement library does not take.
  counters  steps per tier, steps redone, steps without the guard and early rejections equal to PARENT: what the build of the
            parent commit (which carried ms and resynced) gave on the same inputs, recorded from a run of that build on an MI355X.
            No decision may move.
"""
import numpy as np
import pytest

import ms_free as M
import rk4_extended as X
import test_gpu_rk4_extended as R
import test_gpu_series_scale as S

pytestmark = pytest.mark.gpu

C = 2 * X.WAVE
STEPS = [35, 530, 1100]
PLACED = 35  # the burst lies inside the first 35 steps: the lanes are placed on those, once for every step count
FREE = 200   # steps the free wave of the tight set is placed on
CASES = [(which, steps, damping, d) for which in ("tight", "bump", "full") for steps in STEPS for damping in (True, False) for d in (1, 3)]
_REF = {}


def _burst(t):
    return 1.0 + (np.exp(-t / 20) + 1.0 * np.exp(-((t - 2.4) / 0.3) ** 2)) * np.sin(10 * t)


def _surge(t):
    return 1.0 + (np.exp(-t / 20) + 40.0 * 0.5 * (1.0 + np.tanh((t - 2.2) / 0.15)) * np.exp(-((t - 2.2) / 3.0) ** 2)) * np.sin(10 * t)


def _model(oracle_mod, which, steps, damping):
    if which == "tight":
        return S._model(oracle_mod, steps, 0.025, damping)
    return S._model(oracle_mod, steps, 0.1, damping, _burst if which == "bump" else _surge)


def _lanes(oracle_mod, which, damping, d):
    key = ("lanes", which, damping, d)
    if key not in _REF:
        m = _model(oracle_mod, which, PLACED, damping)
        a, b = S._ab(m, d, C, 31)
        if which == "bump":
            dc, _ = S._place(m, a, b, PLACED, d, np.linspace(0.3, 0.9, C))
            dc[7] = S._place(m, a[7:8], b[7:8], PLACED, d, np.array([1.15]))[0][0]
            big = S._largest(S._scan(m, dc, a, b, PLACED, d))  # (trips of 16 steps, lanes)
            assert big[0].max() < 0.95 and big[1, 7] > 1.05 and np.delete(big, 7, axis=1).max() < 0.95, (big[0].max(), big[1, 7])
        elif which == "full":
            dc = np.concatenate([S._headline_wave(m, a[:X.WAVE], 32), S._headline_wave(m, a[X.WAVE:], 33)])
            dc[0] = 1.01 * S._edge(m, a[0])
            big = S._largest(S._scan(m, dc, a, b, PLACED, d))
            assert big[0].max() < 0.95 and big[1, 0] > 16.8, (big[0].max(), big[1, 0])  # one clean trip; then past WIDE's |dlt| < 2^-5
        else:
            mf = _model(oracle_mod, which, FREE, damping)
            w1 = slice(X.WAVE, C)
            dc = np.concatenate([S._headline_wave(m, a[:X.WAVE], 32), S._place(mf, a[w1], b[w1], FREE, d, np.linspace(0.02, 0.1, X.WAVE))[0]])
        _REF[key] = (dc, a, b)
    return _REF[key]


def _reference(gpu_engine, cpu_engine, oracle_mod, which, steps, damping, d):
    """model, lanes, observation, extended SSq and a plain float64 RK4's SSq errors (computed once)"""
    key = (which, steps, damping, d)
    if key not in _REF:
        m, data = _model(oracle_mod, which, steps, damping), S._data(oracle_mod, steps, 0.025 if which == "tight" else 0.1)
        dc, a, b = _lanes(oracle_mod, which, damping, d)
        gpu_engine.set_model(m, 1)
        vl = np.array(gpu_engine.loading())  # the table the kernels read
        assert vl.size == 2 * steps + 1
        ext, _ = M.walk_ext(m, dc, a, b, vl, data, steps)
        if which == "tight":
            kw = {} if d == 1 else {"a": a, "b": b}
            assert cpu_engine.set_model(m, 1) == data.size
            plain, _ = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=False, **kw)
        else:
            plain = M.walk_ext(m, dc, a, b, vl, data, steps, dtype=np.float64)[0]["ssq"]
        o = (np.abs(X._w(plain) - ext["ssq"]) / ext["ssq"]).astype(np.float64)
        _REF[key] = (m, dc, a, b, data, ext["ssq"], o)
    return _REF[key]


def run_case(gpu_engine, cpu_engine, oracle_mod, which, steps, damping, d):
    """-> (SSq errors of the sampler, of the plain float64 RK4, accept flags, counter deltas)"""
    m, dc, a, b, data, ssq_ext, o = _reference(gpu_engine, cpu_engine, oracle_mod, which, steps, damping, d)
    ssq, acc, cnt = S._sampler(gpu_engine, m, dc, a, b, data, d)
    g = (np.abs(X._w(ssq) - ssq_ext) / ssq_ext).astype(np.float64)
    return g, o, acc, {k: int(v) for k, v in cnt.items()}


def case_id(which, steps, damping, d):
    return f"{which}-{steps}-{'damp' if damping else 'nodamp'}-d{d}"


def _cnt(tight, narrow, wide, full, redone, unguarded, early_rejected):
    return {"steps_tight": tight, "steps_narrow": narrow, "steps_wide": wide, "steps_full": full, "steps_redone": redone,
            "steps_unguarded": unguarded, "early_rejected": early_rejected}


# The counters of the parent commit's build on these inputs (see the module's docstring), by case_id:
# wave-steps tight, narrow, wide, full, redone, without the guard; early rejections.
PARENT = {
    "tight-35-damp-d1": _cnt(68, 0, 2, 0, 0, 32, 0),
    "tight-35-damp-d3": _cnt(68, 0, 2, 0, 0, 32, 0),
    "tight-35-nodamp-d1": _cnt(68, 0, 2, 0, 0, 32, 0),
    "tight-35-nodamp-d3": _cnt(68, 0, 2, 0, 0, 32, 0),
    "tight-530-damp-d1": _cnt(1060, 0, 0, 0, 0, 528, 0),
    "tight-530-damp-d3": _cnt(1060, 0, 0, 0, 0, 528, 0),
    "tight-530-nodamp-d1": _cnt(1060, 0, 0, 0, 0, 528, 0),
    "tight-530-nodamp-d3": _cnt(1060, 0, 0, 0, 0, 528, 0),
    "tight-1100-damp-d1": _cnt(2200, 0, 0, 0, 0, 1088, 0),
    "tight-1100-damp-d3": _cnt(2200, 0, 0, 0, 0, 1088, 0),
    "tight-1100-nodamp-d1": _cnt(2200, 0, 0, 0, 0, 1088, 0),
    "tight-1100-nodamp-d3": _cnt(2200, 0, 0, 0, 0, 1088, 0),
    "bump-35-damp-d1": _cnt(66, 2, 2, 0, 16, 0, 0),
    "bump-35-damp-d3": _cnt(66, 2, 2, 0, 16, 0, 0),
    "bump-35-nodamp-d1": _cnt(66, 2, 2, 0, 16, 0, 0),
    "bump-35-nodamp-d3": _cnt(66, 2, 2, 0, 16, 0, 0),
    "bump-530-damp-d1": _cnt(980, 80, 0, 0, 16, 0, 0),
    "bump-530-damp-d3": _cnt(980, 80, 0, 0, 16, 0, 0),
    "bump-530-nodamp-d1": _cnt(980, 80, 0, 0, 16, 0, 0),
    "bump-530-nodamp-d3": _cnt(980, 80, 0, 0, 16, 0, 0),
    "bump-1100-damp-d1": _cnt(2120, 80, 0, 0, 16, 0, 0),
    "bump-1100-damp-d3": _cnt(2120, 80, 0, 0, 16, 0, 0),
    "bump-1100-nodamp-d1": _cnt(2120, 80, 0, 0, 16, 0, 0),
    "bump-1100-nodamp-d3": _cnt(2120, 80, 0, 0, 16, 0, 0),
    "full-35-damp-d1": _cnt(64, 4, 2, 0, 36, 0, 0),
    "full-35-damp-d3": _cnt(64, 4, 2, 0, 36, 0, 0),
    "full-35-nodamp-d1": _cnt(64, 4, 2, 0, 36, 0, 0),
    "full-35-nodamp-d3": _cnt(64, 4, 2, 0, 36, 0, 0),
    "full-530-damp-d1": _cnt(64, 892, 40, 64, 56, 0, 0),
    "full-530-damp-d3": _cnt(64, 892, 40, 64, 56, 0, 0),
    "full-530-nodamp-d1": _cnt(64, 892, 40, 64, 56, 0, 0),
    "full-530-nodamp-d3": _cnt(64, 892, 40, 64, 56, 0, 0),
    "full-1100-damp-d1": _cnt(80, 2016, 40, 64, 56, 0, 0),
    "full-1100-damp-d3": _cnt(88, 2008, 40, 64, 56, 0, 0),
    "full-1100-nodamp-d1": _cnt(80, 2016, 40, 64, 56, 0, 0),
    "full-1100-nodamp-d3": _cnt(88, 2008, 40, 64, 56, 0, 0),
}


@pytest.mark.parametrize("which,steps,damping,d", CASES, ids=[case_id(*c) for c in CASES])
def test_sampler_without_the_carried_ms(gpu_engine, cpu_engine, oracle_mod, which, steps, damping, d):
    g, o, acc, cnt = run_case(gpu_engine, cpu_engine, oracle_mod, which, steps, damping, d)
    tag = case_id(which, steps, damping, d)
    print(f"{tag}: counters {cnt}")
    assert acc.all(), f"{tag}: {int((~acc).sum())} chains did not accept"
    # the path each set is there for
    if which == "tight":
        assert S._all_tight(cnt, steps) and cnt["steps_unguarded"] > 0, cnt  # wave 1's whole trips
    elif which == "bump":
        assert cnt["steps_redone"] > 0 and 0 < cnt["steps_narrow"] < steps // 2 and cnt["steps_full"] == 0, cnt
        assert cnt["steps_tight"] > steps, cnt  # wave 1 all of it, wave 0 before the burst and, in the longer series, after it
    else:
        assert (cnt["steps_full"] > 0 or steps == 35) and cnt["steps_tight"] > 0 and cnt["steps_redone"] > 0, cnt
    fails = []
    for w in range(2):
        sl = slice(X.WAVE * w, X.WAVE * (w + 1))
        R._check(f"{tag} wave {w}", g[sl], o[sl], R.FACTOR_SSQ, R.SSQ_FLOOR, R.SSQ_CAP, fails)
    assert not fails, fails
    assert cnt == PARENT[tag], (cnt, PARENT[tag])
