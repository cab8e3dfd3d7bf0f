"""
GPU tests: the float64 sampler's TIGHT trips with the in-step sum of squares (csrc/rsf_device.h: rk4_tight INSTEP, trip_fast_ssq,
trip_cold_ssq) — every step squares its own residual, the half-step stages take the expm1 series one term shorter, the
full-step stage works on the half increment — against the extended-precision RK4 of tests/rk4_extended.py.

The rule and the numbers are test_gpu_rk4_extended.py's own: per wave, max and median of the sampler's SSq error within
FACTOR_SSQ (8) x the CPU restatement's on the same lanes (x SSQ_FLOOR where that is at rounding level itself), and the max
under SSQ_CAP (5e-13).  128 chains (two waves), damping on and off, step counts that walk the trip structure:
  35  two 16-step trips, one pair, the odd last step (WIDE series)
  18  one trip and one pair
  530 the resync at step 512 inside a run of trips
Lane sets:
  tight   wave 0 well inside TIGHT's a-priori bound (Dc ~ 800 .. 3300), wave 1 within 12 % of its edge: no guard trips
  trip    a model with a = 0.03, b = 0.034 (TIGHT's edge at Dc = 205): two lanes of wave 0 at Dc = 207 and 211 — inside the
          a-priori bound on the mu increment, but their rho passes 2^-20 in the first trips (shown here on the CPU, in
          extended precision: the restatement library keeps no tier counters) — among TIGHT lanes that stay inside it: the two
          drop the trip's sum, restore the state and take the cold trip while the others keep the sums they hold
  reject  one lane whose current SSq is a quarter of its proposal's, with sigma^2 ~ 0: its running sum passes the bound
          mid-series and the lane stops counting, next to lanes that run to the end
The second check holds the sampler's SSq against the forward kernel's stored acceleration (the trajectory path, which
this mode leaves alone), summed on the host in np.longdouble: the same 5e-13.
"""
import numpy as np
import pytest

import rk4_extended as X
import test_gpu_rk4_extended as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
C = 2 * X.WAVE
TRIP = 16  # steps per TIGHT trip of the one-parameter sampler
RHO_GUARD = 2.0 ** -20
_REF = {}


def _model(oracle_mod, steps, damping, which):
    n = steps + 1
    m = oracle_mod.ModelSpec(n, 0.0, 0.1 * n, 1)
    m.RadiationDamping = damping
    if which == "trip":
        m.a, m.b = 0.03, 0.034
    assert m.nout == n
    return m


def _lanes(m, which):
    if which == "tight":
        return np.concatenate([X.place_lanes(m, "tight", seed=3), X.place_lanes(m, "tight_edge", seed=4)])
    if which == "reject":
        return X.place_lanes(m, "tight", waves=2, seed=5)
    edge = X.tier_edges(m, m.a)[0]  # trip: TIGHT lanes around Dc = 1000, far inside this model's bound, and the two at its edge
    dc = np.sort(np.random.default_rng(6).uniform(800.0, 2000.0, (2, X.WAVE)), axis=1).reshape(-1)
    dc[:2] = [1.006 * edge, 1.026 * edge]
    return dc


def _largest_rho(m, dc, steps):
    """max over the stages of each of the first `steps` RK4 steps of |rho| = |dtheta / theta| as the TIGHT step forms it
    (half-step stages h/2 k, full-step stage h k3, the step's end), per trip of TRIP steps: (trips, lanes), extended precision"""
    dc = X._w(dc)
    a, b = X._w(np.full(dc.shape, m.a)), X._w(np.full(dc.shape, m.b))
    V_ref, mu_ref, k1 = X._w(m.V_ref), X._w(m.mu_ref), X._w(m.k1)
    h = X._w(float(m.delta_t))
    hh, h6 = h / 2, h / 6
    mu, th = np.full(dc.shape, X._w(m.mu_t_zero)), dc / V_ref

    def f(t, mu_, th_):
        return X._rhs(t, mu_, th_, dc, a, b, V_ref, mu_ref, k1, bool(m.RadiationDamping))

    out, rho = [], np.zeros(dc.shape, LD)
    for j in range(steps):
        t = X._w(m.t_start) + j * h
        a0, a1, _ = f(t, mu, th)
        b0, b1, _ = f(t + hh, mu + hh * a0, th + hh * a1)
        c0, c1, _ = f(t + hh, mu + hh * b0, th + hh * b1)
        e0, e1, _ = f(t + h, mu + h * c0, th + h * c1)
        s1 = h6 * (a1 + 2 * b1 + 2 * c1 + e1)
        rho = np.maximum.reduce([rho, abs(hh * a1 / th), abs(hh * b1 / th), abs(h * c1 / th), abs(s1 / th)])
        mu, th = mu + h6 * (a0 + 2 * b0 + 2 * c0 + e0), th + s1
        if (j + 1) % TRIP == 0:
            out.append(rho.astype(np.float64))
            rho = np.zeros(dc.shape, LD)
    return np.array(out)


def _reference(cpu_engine, oracle_mod, steps, damping, which):
    """model, lanes, observation, extended SSq, the restatement's SSq errors and the forward trajectory's host-side SSq inputs"""
    key = (steps, damping, which)
    if key not in _REF:
        m = _model(oracle_mod, steps, damping, which)
        dc = _lanes(m, which)
        acc, _ = X.forward_ext(m, np.array([1000.0]))
        acc = acc[:, 0].astype(np.float64)
        data = acc + np.abs(acc) * np.random.default_rng(steps).standard_normal(acc.size)
        _, ssq_ext = X.forward_ext(m, dc, data=data)
        assert cpu_engine.set_model(m, 1) == data.size
        s_cpu, _ = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=False)
        o = (np.abs(X._w(s_cpu) - ssq_ext) / ssq_ext).astype(np.float64)
        _REF[key] = (m, dc, data, ssq_ext, o)
    return _REF[key]


def _sampler(engine, m, dc, data, std2, ssq0=None, u=1e-300):
    """one replayed iteration that proposes the start point itself (z = 0) -> (state SSq, accept flags, counter deltas)"""
    engine.set_model(m, 1)
    q0 = dc.reshape(C, 1)
    engine.mcmc_init(q0, data, [0.0], [100.0 * dc.max()], seed=17, prior_len=3)
    engine.set_state(q=q0, V=((1e-7 * q0) ** 2).reshape(C, 1, 1), std2=std2, ssq=ssq0)
    c0 = engine.counters()
    _, _, ta = engine.mcmc_replay(np.zeros((1, C, 1)), np.full((1, C), u), np.full((1, C), 250.0))
    c1 = engine.counters()
    return np.array(engine.get_state()[1]), np.array(ta[0]).astype(bool), {k: c1[k] - c0[k] for k in c1 if k.startswith(("steps", "early"))}


def _judge(tag, ssq, keep, ssq_ext, o, fails):
    g = (np.abs(X._w(ssq) - ssq_ext) / ssq_ext).astype(np.float64)
    for w in range(2):
        sl = np.arange(X.WAVE * w, X.WAVE * (w + 1))
        sl = sl[keep[sl]]
        R._check(f"{tag} wave {w}", g[sl], o[sl], R.FACTOR_SSQ, R.SSQ_FLOOR, R.SSQ_CAP, fails)


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("steps", [35, 18, 530])
def test_in_step_ssq_within_float64_rounding(gpu_engine, cpu_engine, oracle_mod, steps, damping):
    fails = []
    every = np.ones(C, dtype=bool)
    for which in ("tight", "trip", "reject"):
        m, dc, data, ssq_ext, o = _reference(cpu_engine, oracle_mod, steps, damping, which)
        tag = f"steps {steps} damping {damping} {which}"
        keep, std2, ssq0, u = every, np.full(C, 1e300), None, 1e-300
        if which == "trip":  # on the CPU: the two lanes leave the rho guard in the first trip, the others never do
            rho = _largest_rho(m, dc, steps - steps % TRIP)
            print(f"{tag}: largest |rho| / 2^-20 per trip, lanes 0 1: {rho[:, :2] / RHO_GUARD}, others: {rho[:, 2:].max() / RHO_GUARD:.3f}")
            assert (rho[0, :2] > 1.2 * RHO_GUARD).all() and rho[:, 2:].max() < 0.5 * RHO_GUARD
        if which == "reject":
            k = 5
            keep = every.copy()
            keep[k] = False
            std2 = std2.copy()
            std2[k] = 1e-300  # accept iff ssq_new < ssq - 2 sigma^2 log u: the lane's bound is its current SSq
            ssq0 = ssq_ext.astype(np.float64)
            ssq0[k] *= 0.25
            u = 0.5
        ssq, acc, cnt = _sampler(gpu_engine, m, dc, data, std2, ssq0, u)
        print(f"{tag}: counters {cnt}")
        assert acc[keep].all(), f"{tag}: {int((~acc[keep]).sum())} chains did not accept"
        assert cnt["steps_tight"] > 0
        if which == "trip":
            assert cnt["steps_redone"] > 0, cnt
        else:
            assert cnt["steps_redone"] == cnt["steps_narrow"] == cnt["steps_full"] == 0 and cnt["steps_wide"] <= 2, cnt
        if which == "reject":
            assert not acc[k] and ssq[k] == ssq0[k] and cnt["early_rejected"] == 1, (acc[k], ssq[k], ssq0[k], cnt)
        _judge(tag, ssq, keep, ssq_ext, o, fails)
        # the same sum from the forward kernel's stored acceleration (the trajectory path), formed on the host
        gpu_engine.set_model(m, 1)
        _, traj = gpu_engine.forward(dc, want_acc=True)
        r = X._w(traj) - X._w(data)[:, None]
        host = (r * r).sum(axis=0)
        d = (np.abs(X._w(ssq) - host) / host).astype(np.float64)[keep]
        print(f"{tag}: sampler SSq against the stored trajectory's: max {d.max():.2e} med {np.median(d):.2e}")
        if not d.max() < R.SSQ_CAP:
            fails.append(f"{tag} against the trajectory")
    assert not fails, fails
