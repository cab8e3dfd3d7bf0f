"""
The float64 sampler's a-priori bound on a TIGHT trip, restated (a test helper; TEST INFRASTRUCTURE ONLY).

csrc/rsf_device.h, tight_needs_guard: from a trip's start state (W0, Rh0), the lane's constants and the range [vl_lo, vl_hi] of
the loading table, decide whether any increment of the trip's 16 steps could reach TIGHT's guard; where no lane of a wave
needs the guard the trip runs without it.  `needs_guard` is that predicate in float64, operation for operation (without the
fused roundings: every use here keeps the lanes some per cent away from its edge).  `scan` walks the extended-precision RK4
of rk4_extended.py through a series and returns, for every whole trip, the predicate at the trip's start state and the four
maxima the guard would have measured in it, in extended precision:
  rho     |dtheta / theta| of the two half-step stages and of the step's end          guard: 2^-20
  c1      half the full-step stage's |dtheta / theta|                                 guard: 2^-21
  dlt     |log(v_stage / v_step_start)| of the full-step stage and the step's end     guard: 2^-9
  dlt_h   the same of the two half-step stages                                        guard: 2^-10
"""
import numpy as np

import rk4_extended as X

LD = np.longdouble
TRIP = 16  # steps per TIGHT trip of the one-parameter sampler (2 * kTightUnroll)
GUARDS = {"rho": 2.0 ** -20, "c1": 2.0 ** -21, "dlt": 2.0 ** -9, "dlt_h": 2.0 ** -10}
# tight_needs_guard's constants
R, B, DMAX = 2.0 ** -20, 2.0 ** -21, 0.9 * 2.0 ** -9


def damped(m):
    """the kernels' DAMP: with k1 = 0 the host launches the kernels without the damping pass (rsf_hip.hip, damped)"""
    return bool(m.RadiationDamping) and float(m.k1) != 0.0


def builtin_table(m, steps=None):
    """the built-in loading at the RK4 stage times t_start + j h/2 as rsf_set_model tabulates it (float64, substeps = 1)"""
    steps = m.nout - 1 if steps is None else steps
    t = float(m.t_start) + np.arange(2 * steps + 1, dtype=np.float64) * (0.5 * float(m.delta_t))
    return m.V_ref * (1 + np.exp(-t / 20) * np.sin(10 * t))


def never(m, dc, a, b, vl_lo, vl_hi, nu=TRIP):
    """W.never of wave_begin: the lanes the solve does not evaluate the bound for.  -> (never, dmin / Dmax, rmin / (0.9 B))"""
    dc, a, b = (np.asarray(x, dtype=np.float64) for x in (dc, a, b))
    h = float(m.delta_t)
    with np.errstate(all="ignore"):
        kh = (0.1 / dc) * (1.0 / a) * h
        hhd = (0.5 * h) * (m.V_ref / dc)
        dmin = np.abs(kh) * (0.5 * (vl_hi - vl_lo)) + np.abs(b / a) * R
        rmin = np.abs(hhd) * (dmin * (1.02 * nu) + (nu + 1) * R)
        nev = ~((dmin < DMAX) & (rmin < 0.9 * B))
    return nev, dmin / DMAX, rmin / (0.9 * B)


def needs_guard(w, theta, m, dc, a, b, vl_lo, vl_hi, nu=TRIP):
    """tight_needs_guard in float64, with the solve's gate W.never (wave_begin): a lane whose two figures cannot come under their
    limits even at the steady state — |V_l - v| at half the table's range, x = 1 — is never asked and keeps the guard.
    w = v / V_ref and theta at the trip's start (the kernel carries W0 = kvk w with damping, w without, and
    Rh0 = (h/2 Dc) / x = (h/2) / theta); a, b, dc per lane.  -> (needs, D / Dmax, rb / (0.9 B)), the figures being the bound's"""
    w, theta, dc, a, b = (np.asarray(x, dtype=np.float64) for x in (w, theta, dc, a, b))
    h = float(m.delta_t)
    hh = 0.5 * h
    damp = damped(m)
    inv_a, inv_dc = 1.0 / a, 1.0 / dc
    kh = (0.1 * inv_dc) * inv_a * h
    kvk = m.k1 * (m.V_ref * inv_a)
    ikw = 1.0 / kvk if damp else 1.0
    vrw = m.V_ref * ikw
    hhd = hh * (m.V_ref * inv_dc)
    hhdw = hhd * ikw
    boa = b * inv_a
    bh = (b * m.V_ref) * 10.0 / hhd
    W0 = kvk * w if damp else w
    Rh0 = hhd / (m.V_ref * theta * inv_dc)
    gm1 = 1.02 * nu * DMAX
    with np.errstate(all="ignore"):
        p = vrw * W0
        c = Rh0 - W0 * hhdw
        D0 = np.abs(p) * gm1 + np.maximum(np.abs(vl_hi - p), np.abs(vl_lo - p))
        if damp:
            D0 = D0 + ((1.0 + gm1) * np.abs(W0)) * (np.abs(bh) * B + D0)
        D = np.abs(kh) * D0 + np.abs(boa) * R
        rb = (np.abs(Rh0) + np.abs(c)) * (D * (1.02 * nu) + (nu + 1) * R) + np.abs(c)
        ok = (D < DMAX) & (rb < 0.9 * B)  # NaN: not ok
    return ~ok | never(m, dc, a, b, vl_lo, vl_hi, nu)[0], D / DMAX, rb / (0.9 * B)


def _rhs_vl(V_l, mu, th, dc, a, b, V_ref, mu_ref, k1, damping):
    """rk4_extended._rhs with the loading's value supplied instead of the built-in history at t"""
    kprime = LD(1e-2) * 10 / dc
    v = V_ref * np.exp((mu - mu_ref - b * np.log(V_ref * th / dc)) / a)
    d1 = 1 - v * th / dc
    d0 = kprime * V_l - kprime * v
    d2 = v / a * (d0 - b / th * d1)
    if damping:
        d0 = d0 - k1 * d2
        d2 = v / a * (d0 - b / th * d1)
    return d0, d1, d2


def scan(m, dc, steps, a=None, b=None, vl=None, vl_range=None):
    """The first `steps` RK4 steps (substeps = 1) of lanes dc [, a, b] in extended precision.  vl: the loading table at the
    2 steps + 1 stage times (float64), or None for the built-in history evaluated by rk4_extended._rhs; vl_range: the
    (vl_lo, vl_hi) the predicate is given — default: the range of the table over the WHOLE series of m, as the host forms it.
    -> dict of arrays (trips, lanes): need (bool), D, rb (the predicate's two figures over their thresholds), rho, c1, dlt,
    dlt_h (the trip's extended-precision maxima, float64), and w, theta (float64) at the trips' starts; per lane: never, dmin, rmin."""
    dcw = X._w(np.atleast_1d(dc))
    aw = X._w(np.full(dcw.shape, m.a) if a is None else np.broadcast_to(a, dcw.shape))
    bw = X._w(np.full(dcw.shape, m.b) if b is None else np.broadcast_to(b, dcw.shape))
    V_ref, mu_ref, k1 = X._w(m.V_ref), X._w(m.mu_ref), X._w(m.k1)
    damping = bool(m.RadiationDamping)
    h = X._w(float(m.delta_t))
    hh, h6 = h / 2, h / 6
    if vl_range is None:
        tab = builtin_table(m) if vl is None else np.asarray(vl, dtype=np.float64)
        vl_range = (float(tab.min()), float(tab.max()))
    vlw = None if vl is None else X._w(vl)
    mu, th = np.full(dcw.shape, X._w(m.mu_t_zero)), dcw / V_ref

    def f(j, mu_, th_):  # stage time index j (units of h/2)
        if vlw is None:
            return X._rhs(X._w(m.t_start) + j * hh, mu_, th_, dcw, aw, bw, V_ref, mu_ref, k1, damping)
        return _rhs_vl(vlw[j], mu_, th_, dcw, aw, bw, V_ref, mu_ref, k1, damping)

    def dl(dmu, dth):  # log(v' / v) for the increments (dmu, dth) from the step's start point
        return np.abs((dmu - bw * np.log1p(dth / th)) / aw)

    out = {k: [] for k in ("need", "D", "rb", "rho", "c1", "dlt", "dlt_h", "w", "theta")}
    mx = None
    with np.errstate(all="ignore"):
        for s in range(steps - steps % TRIP):
            if s % TRIP == 0:
                v = V_ref * np.exp((mu - mu_ref - bw * np.log(V_ref * th / dcw)) / aw)
                w64, th64 = (v / V_ref).astype(np.float64), th.astype(np.float64)
                need, D, rb = needs_guard(w64, th64, m, dcw.astype(np.float64), aw.astype(np.float64), bw.astype(np.float64), *vl_range)
                for k, x in zip(("need", "D", "rb", "w", "theta"), (need, D, rb, w64, th64)):
                    out[k].append(x)
                mx = {k: np.zeros(dcw.shape, LD) for k in GUARDS}
            a0, a1, _ = f(2 * s, mu, th)
            b0, b1, _ = f(2 * s + 1, mu + hh * a0, th + hh * a1)
            c0, c1, _ = f(2 * s + 1, mu + hh * b0, th + hh * b1)
            e0, e1, _ = f(2 * s + 2, mu + h * c0, th + h * c1)
            s0, s1 = h6 * (a0 + 2 * b0 + 2 * c0 + e0), h6 * (a1 + 2 * b1 + 2 * c1 + e1)
            mx["rho"] = np.maximum.reduce([mx["rho"], abs(hh * a1 / th), abs(hh * b1 / th), abs(s1 / th)])
            mx["c1"] = np.maximum(mx["c1"], abs(hh * c1 / th))
            mx["dlt_h"] = np.maximum.reduce([mx["dlt_h"], dl(hh * a0, hh * a1), dl(hh * b0, hh * b1)])
            mx["dlt"] = np.maximum.reduce([mx["dlt"], dl(h * c0, h * c1), dl(s0, s1)])
            mu, th = mu + s0, th + s1
            if (s + 1) % TRIP == 0:
                for k in GUARDS:
                    out[k].append(mx[k].astype(np.float64))
    out = {k: np.array(x) for k, x in out.items()}
    out["never"], out["dmin"], out["rmin"] = never(m, dcw.astype(np.float64), aw.astype(np.float64), bw.astype(np.float64), *vl_range)
    return out


def predicted_unguarded(need, alive=None):
    """wave-steps the sampler runs without the guard: TRIP for every trip in which no alive lane of the wave needs it.
    need: (trips, 64) of one wave; alive: the same shape (default: every lane alive in every trip)"""
    need = np.asarray(need, dtype=bool)
    alive = np.ones_like(need) if alive is None else np.asarray(alive, dtype=bool)
    return TRIP * int((~(need & alive).any(axis=1)).sum())
