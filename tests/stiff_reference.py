"""
Specification of the state-law solve with the STIFFNESS OF THE APPARATUS a constant independent of Dc (a test helper; TEST
INFRASTRUCTURE ONLY) — what include/rsf_stiff.h's rsf_stiff_observe, rsf_stiff_dr_run and rsf_stiff_dr_ssq are checked against.

The reference's spring is tied to the parameter being inferred, k' = 1e-2 * 10 / Dc (RateStateModel.py:324), and so is
tests/law_reference.py's `_rhs`.  Here the stiffness `k` is the caller's: `_rhs` is law_reference's RESTATED with kprime = k and
nothing else changed, and `trajectory` / `forward` are tests/observe_reference.py's recurrence around it, statement for
statement, in the reference's own variables (mu, theta, V), float64 or np.longdouble.  With k = 1e-2 * 10 / Dc on every lane
they are observe_reference's bit for bit.

`trajectory_lane` is the SECOND float64 arrangement, in the device's variables, with the constants formed as
include/rsf_stiff.h states them: kappa = k Dc, ikappa = 1.0 / kappa, kprime = kappa (1 / Dc), beta = (b V_ref) ikappa,
ms_0 = (mu_t_zero Dc) ikappa, every other constant and the step observe_reference.trajectory_lane's.  Where k Dc == 0.1 exactly
it is that function bit for bit.
"""
import numpy as np

import law_reference as R
import observe_reference as O
from observe_reference import ALIASES, OBSERVABLES, _inputs, _ssq, _widen


def _rhs(V_l, mu, th, dc, a, b, V_ref, mu_ref, k1, damping, slip, kprime):
    """law_reference._rhs with the spring's stiffness kprime given: (d mu/dt, d theta/dt, dV/dt)."""
    v = V_ref * np.exp((mu - mu_ref - b * np.log(V_ref * th / dc)) / a)
    om = v * th / dc
    d1 = -om * np.log(om) if slip else 1 - om
    d0 = kprime * V_l - kprime * v
    d2 = v / a * (d0 - b / th * d1)
    if damping:
        d0 = d0 - k1 * d2
        d2 = v / a * (d0 - b / th * d1)
    return d0, d1, d2


def trajectory(m, k, dc, vl=None, law="aging", a=None, b=None, dtype=np.float64):
    """-> {observable: series [nout, C]} in `dtype` with the stiffness k (a scalar, or one value per lane): observe_reference.trajectory's
    loop, statement for statement"""
    slip = R.LAW_ALIASES[law] == "slip"
    w = _widen(dtype)
    dc, a, b, vl = _inputs(m, dc, vl, a, b, w)
    kprime = w(np.broadcast_to(k, dc.shape))
    V_ref, mu_ref, k1 = w(m.V_ref), w(m.mu_ref), w(m.k1)
    damping, S, n = bool(m.RadiationDamping), int(m.substeps), R.nout(m)
    h = w(float(m.delta_t) / S)
    hh, h6, dt = h / 2, h / 6, w(m.delta_t)
    mu = np.full(dc.shape, w(m.mu_t_zero))
    th = dc / V_ref
    V = np.full(dc.shape, V_ref)
    out = {o: np.zeros((n, dc.size), dtype=dtype) for o in OBSERVABLES}
    out["mu"][0], out["theta"][0], out["velocity"][0] = mu, th, V

    def f(V_l, mu_, th_):
        return _rhs(V_l, mu_, th_, dc, a, b, V_ref, mu_ref, k1, damping, slip, kprime)

    j = 0
    with np.errstate(all="ignore"):
        for i in range(1, n):
            vprev = V
            for _ in range(S):
                a0, a1, a2 = f(vl[j], mu, th)
                b0, b1, b2 = f(vl[j + 1], mu + hh * a0, th + hh * a1)
                c0, c1, c2 = f(vl[j + 1], mu + hh * b0, th + hh * b1)
                e0, e1, e2 = f(vl[j + 2], mu + h * c0, th + h * c1)
                mu = mu + h6 * (a0 + 2 * b0 + 2 * c0 + e0)
                th = th + h6 * (a1 + 2 * b1 + 2 * c1 + e1)
                V = V + h6 * (a2 + 2 * b2 + 2 * c2 + e2)
                j += 2
            out["acc"][i] = (V - vprev) / dt
            out["mu"][i], out["theta"][i], out["velocity"][i] = mu, th, V
    return out


def forward(m, k, dc, vl=None, law="aging", observable="acc", a=None, b=None, data=None, dtype=np.float64):
    """-> (series [nout, C], ssq [C] or None) of `observable` in `dtype`; observe_reference.forward's arguments behind (m, k)"""
    series = trajectory(m, k, dc, vl, law, a, b, dtype)[ALIASES[observable]]
    with np.errstate(all="ignore"):
        return series, _ssq(series, data, _widen(dtype))


def trajectory_lane(m, k, dc, vl=None, law="aging", a=None, b=None):
    """-> {observable: series [nout, C]}, float64, in the device's variables with the lane constants of include/rsf_stiff.h; the
    step is observe_reference.trajectory_lane's, every fused multiply-add written as a product and a sum"""
    slip = R.LAW_ALIASES[law] == "slip"
    dc, a, b, vl = _inputs(m, dc, vl, a, b, _widen(np.float64))
    V_ref, mu_ref, k1 = float(m.V_ref), float(m.mu_ref), float(m.k1)
    damp = bool(m.RadiationDamping) and k1 != 0.0
    S, n = int(m.substeps), R.nout(m)
    h = float(m.delta_t) / S
    hh, h6, inv_dt, inv_vref = 0.5 * h, h / 6.0, 1.0 / float(m.delta_t), 1.0 / V_ref
    with np.errstate(all="ignore"):
        kappa = np.broadcast_to(np.float64(k), dc.shape) * dc
        ikappa = 1.0 / kappa
    # rsf::make_lane<DAMP, STIFF = true>
    inv_a, inv_dc = 1.0 / a, 1.0 / dc
    kprime = kappa * inv_dc
    kia = kprime * inv_a
    via = V_ref * inv_a
    vdc = V_ref * inv_dc
    vk = via * kprime
    beta = (b * V_ref) * ikappa
    kvk = k1 * via
    vkw = vk * (1.0 / kvk) if damp else vk
    h6v = h6 * vkw
    boa = b * inv_a
    tc = -mu_ref * inv_a
    h6d = h6 * vdc
    # rsf::initial_state<STIFF = true>
    ms = (float(m.mu_t_zero) * dc) * ikappa
    x = V_ref * ((dc * inv_vref) * inv_dc)
    V = np.full(dc.shape, V_ref)
    tscale = dc * inv_vref
    out = {o: np.zeros((n, dc.size)) for o in OBSERVABLES}
    out["mu"][0], out["theta"][0], out["velocity"][0] = kprime * ms, x * tscale, V

    def rhs(ms_, x_, V_l):  # rsfk::law_rhs
        lx = np.log(x_)
        e = (ms_ * kia + tc) - boa * lx
        wv, rx = np.exp(e), 1.0 / x_
        d1 = -(wv * x_) * (e + lx) if slip else 1.0 - wv * x_
        d0 = V_l - V_ref * wv
        bt = (beta * d1) * rx
        g = d0 - bt
        if damp:
            kw = kvk * wv
            d0 = d0 - kw * g
            g = d0 - bt
            return d0, d1, kw * g
        return d0, d1, wv * g

    j = 0
    with np.errstate(all="ignore"):
        for i in range(1, n):
            vprev = V
            for _ in range(S):  # rsfk::law_step
                p0 = p1 = 0.0
                s0 = s1 = s2 = 0.0
                for c, wgt, V_l in ((0.0, 1.0, vl[j]), (hh, 2.0, vl[j + 1]), (hh, 2.0, vl[j + 1]), (h, 1.0, vl[j + 2])):
                    d0, d1, d2 = rhs(ms + c * p0, x + (c * vdc) * p1, V_l)
                    s0, s1, s2 = s0 + wgt * d0, s1 + wgt * d1, s2 + wgt * d2
                    p0, p1 = d0, d1
                ms = ms + h6 * s0
                x = x + h6d * s1
                V = V + h6v * s2
                j += 2
            out["acc"][i] = (V - vprev) * inv_dt
            out["mu"][i], out["theta"][i], out["velocity"][i] = kprime * ms, x * tscale, V
    return out


def forward_lane(m, k, dc, vl=None, law="aging", observable="acc", a=None, b=None, data=None):
    """forward's results from the second float64 arrangement (trajectory_lane)"""
    series = trajectory_lane(m, k, dc, vl, law, a, b)[ALIASES[observable]]
    with np.errstate(all="ignore"):
        return series, _ssq(series, data, _widen(np.float64))


excursion, range_error = O.excursion, O.range_error
