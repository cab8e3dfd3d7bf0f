"""
The in-step TIGHT step of the float64 sampler without the carried ms, restated in NumPy float64 (a test helper; TEST
INFRASTRUCTURE ONLY).

csrc/rsf_device.h, rk4_tight<..., INSTEP> / tight_incr_scaled / make_lane / make_series: the step as the sampler's TIGHT trips
take it, operation for operation, on the tier's scaled state (W, Rh) = (kvk w, hhd / x).  Fused operations are formed in
np.longdouble and rounded once (a 64-bit mantissa does not hold every product exactly: a fused result may differ from the
hardware's in its last bit, in about one operation in two thousand; both forms below go through the same code).  The kernel's
own log / exp / reciprocal (<= 1 ulp .. 4 ulp) are NumPy's here.

`walk` takes a whole series in trips of 16 steps (then pairs), in one of two forms:
  carry=True   the form before the change: ms carried by one fma per step, and (W, Rh) re-evaluated in full from (ms, hhd / Rh)
               at the first trip at or after every 512th step (kResync);
  carry=False  the form after it: (W, Rh) a plain two-variable recurrence, ms not carried, nothing anchored.
A trip index in `cold` is taken by the cold trip instead (trip_cold_ssq: full evaluations from (ms, x)), as a lane does whose guard
tripped: in the second form ms is rebuilt from (W, Rh) in front of it (rebuild_ms) — unless `forget` is set, the mutation the tests
must catch.  `walk_ext` is the same series by the extended-precision RK4 of rk4_extended.py, with the end state.
"""
import numpy as np

import rk4_extended as X

LD = np.longdouble
TRIP = 16
RESYNC = 512
KP = 1e-2 * 10


def fma(a, b, c):
    return (X._w(a) * b + c).astype(np.float64)


class Lane:
    """make_lane and make_series (float64, the kernel's operation order)"""

    def __init__(self, m, dc, a, b):
        dc, a, b = (np.asarray(x, dtype=np.float64) for x in (dc, a, b))
        self.damp = bool(m.RadiationDamping) and float(m.k1) != 0.0
        h = float(m.delta_t)
        self.h, self.hh, self.h6 = h, 0.5 * h, h / 6.0
        self.V_ref = float(m.V_ref)
        cacc = self.h6 * (1.0 / h)
        inv_a = 1.0 / a
        self.inv_dc = 1.0 / dc
        self.kprime = KP * self.inv_dc
        self.kia = self.kprime * inv_a
        self.khh, self.kh, self.kh6 = self.kia * self.hh, self.kia * self.h, self.kia * self.h6
        via = self.V_ref * inv_a
        self.vdc = self.V_ref * self.inv_dc
        vk = via * self.kprime
        self.beta = (b * self.V_ref) * (1.0 / KP)
        self.kvk = float(m.k1) * via
        ikw = 1.0 / self.kvk if self.damp else np.ones_like(dc)
        vkw = vk * ikw
        self.cv = cacc * vkw
        self.boa = b * inv_a
        self.tc = -float(m.mu_ref) * inv_a
        self.hhd, self.hd, self.h6d = self.hh * self.vdc, self.h * self.vdc, self.h6 * self.vdc
        self.vrw, self.hhdw, self.hdw = self.V_ref * ikw, self.hhd * ikw, self.hd * ikw
        self.bh = self.beta * (1.0 / self.hhd)
        self.cv2, self.bh2 = 2.0 * self.cv, -2.0 * self.bh
        # make_series
        khh = self.khh
        ik = 1.0 / khh
        self.B = self.boa * ik
        self.N, self.N6 = -0.5 * self.B, self.B * (-1.0 / 6.0)
        kh, kh6 = khh + khh, khh * (1.0 / 3.0)
        k2, f2, e2 = khh * khh, kh * kh, kh6 * kh6
        self.h1, self.h2 = 0.5 * k2, (k2 * khh) * (1.0 / 6.0)
        self.f1, self.f2, self.f3 = 0.5 * f2, (f2 * kh) * (1.0 / 6.0), (f2 * f2) * (1.0 / 24.0)
        self.e1, self.e2, self.e3 = 0.5 * e2, (e2 * kh6) * (1.0 / 6.0), (e2 * e2) * (1.0 / 24.0)
        # initial_state
        self.ms0 = (float(m.mu_t_zero) * dc) * (1.0 / KP)
        self.x0 = self.V_ref * ((dc * (1.0 / self.V_ref)) * self.inv_dc)


def eval_full(L, ms, x):
    """-> (w, 1/x)"""
    return np.exp(fma(-L.boa, np.log(x), fma(ms, L.kia, L.tc))), 1.0 / x


def enter(L, w, rx):
    """tier_enter: (w, 1/x) -> (W, Rh)"""
    return (w * L.kvk if L.damp else w), rx * L.hhd


def rebuild_ms(L, W, Rh):
    """rebuild_ms of rsf_device.h: ms = (log w - tc + (b/a) log x) / kia with x = hhd / Rh, w = W / kvk"""
    lx = np.log(L.hhd * (1.0 / Rh))
    lw = np.log(W * (1.0 / L.kvk) if L.damp else W)
    return (fma(L.boa, lx, lw) - L.tc) * (1.0 / L.kia)


def rebuild_ms_ext(L, W, Rh):
    """the same formula in extended precision, from the same float64 (W, Rh) and constants"""
    W, Rh = X._w(W), X._w(Rh)
    w = W / X._w(L.kvk) if L.damp else W
    return (np.log(w) - X._w(L.tc) + X._w(L.boa) * np.log(X._w(L.hhd) / Rh)) / X._w(L.kia)


def _rhs(L, w, xr, Rh, vl, brx):
    d1 = fma(-w, xr, Rh)
    d0 = fma(-L.vrw, w, vl)
    g = fma(-brx, d1, d0)
    if L.damp:
        d0 = fma(-w, g, d0)
        g = fma(-w, g, g)
    return d0, d1, g


def _incr(L, stage, r, d, w0):
    """tight_incr_scaled -> (w, q)"""
    if stage == 0:
        pb = fma(r, L.N, L.B)
    elif stage == 1:
        pb = fma(-r, L.B, L.B)
    else:
        pb = fma(r, L.N6, L.B)
    dl = fma(-r, pb, d)
    if stage == 0:
        e = fma(fma(L.h2, dl, L.h1), dl, L.khh)
    elif stage == 1:
        e = fma(fma(fma(L.f3, dl, L.f2), dl, L.f1), dl, L.kh)
    else:
        e = fma(fma(fma(L.e3, dl, L.e2), dl, L.e1), dl, L.kh6)
    w = fma(w0 * dl, e, w0)
    if stage == 1:
        return w, fma(r, L.bh2, L.bh)
    if stage == 2:
        rho = r * (1.0 / 3.0)
        return w, fma(rho, rho, -rho)
    return w, None


def step(L, W, Rh, ms, vl0, vlm, vl1, obs, tsum, carry):
    """rk4_tight<DAMP, TIGHT, INSTEP = true> -> (W, Rh, ms, tsum); tsum None starts the trip's sum"""
    xh, xf = L.hhdw, L.hdw
    a0, a1, a2 = _rhs(L, W, xh, Rh, vl0, L.bh)
    sv = W * a2
    w, _ = _incr(L, 0, a1, a0, W)
    b0, b1, b2 = _rhs(L, w, fma(xh, a1, xh), Rh, vlm, fma(-L.bh, a1, L.bh))
    sm = w * b2
    w, _ = _incr(L, 0, b1, b0, W)
    c0, c1, c2 = _rhs(L, w, fma(xh, b1, xh), Rh, vlm, fma(-L.bh, b1, L.bh))
    sm = fma(w, c2, sm)
    w, brx = _incr(L, 1, c1, c0, W)
    e0, e1, e2 = _rhs(L, w, fma(xf, c1, xh), Rh, vl1, brx)
    sv = fma(w, e2, sv)
    t0 = a0 + 2.0 * b0 + 2.0 * c0 + e0
    t1 = a1 + 2.0 * b1 + 2.0 * c1 + e1
    w, q = _incr(L, 2, t1, t0, W)
    if carry:
        ms = fma(L.h6, t0, ms)
    r = fma(sv, L.cv, fma(sm, L.cv2, -obs))
    tsum = r * r if tsum is None else fma(r, r, tsum)
    return w, fma(Rh, q, Rh), ms, tsum


def _cold_step(L, ms, x, vl0, vlm, vl1):
    """rk4_cold -> (ms, x, the V-derivative sum)"""
    k0 = k1 = s0 = s1 = s2 = np.zeros_like(x)
    for st in range(4):
        c = 0.0 if st == 0 else (L.h if st == 3 else L.hh)
        wgt = 1.0 if st in (0, 3) else 2.0
        vl = vl0 if st == 0 else (vl1 if st == 3 else vlm)
        x1 = fma(c * L.vdc, k1, x)
        w, rx = eval_full(L, fma(c, k0, ms), x1)
        d1 = fma(-w, x1, 1.0)
        d0 = fma(-L.V_ref, w, vl)
        bt = (L.beta * d1) * rx
        g = d0 - bt
        if L.damp:
            kw = L.kvk * w
            d0 = fma(-kw, g, d0)
            g = d0 - bt
            d2 = kw * g
        else:
            d2 = w * g
        s0, s1, s2 = fma(wgt, d0, s0), fma(wgt, d1, s1), fma(wgt, d2, s2)
        k0, k1 = d0, d1
    return fma(L.h6, s0, ms), fma(L.h6d, s1, x), s2


def walk(m, dc, a, b, vl, data, steps, carry, cold=(), forget=False):
    """-> dict(w, Rh at the series' end — the plain w = v / V_ref —, ssq), float64 per lane"""
    L = Lane(m, dc, a, b)
    ms, x = L.ms0, L.x0
    W, Rh = enter(L, *eval_full(L, ms, x))
    ssq = np.full(np.shape(dc), float(data[0]) ** 2)
    nxt, r, trip = RESYNC, 0, 0
    with np.errstate(all="ignore"):
        while r < steps:
            nu = TRIP if r + TRIP <= steps else 2
            assert r + nu <= steps, "an even number of steps: the odd last step (the WIDE series) is not restated"
            if carry and r >= nxt:  # resync_t
                W, Rh = enter(L, *eval_full(L, ms, L.hhd * (1.0 / Rh)))
                nxt = (r & ~(RESYNC - 1)) + RESYNC
            if trip in cold:  # trip_cold_ssq
                if not carry and not forget:
                    ms = rebuild_ms(L, W, Rh)
                x = L.hhd * (1.0 / Rh)
                for j in range(r, r + nu):
                    ms, x, dvs = _cold_step(L, ms, x, vl[2 * j], vl[2 * j + 1], vl[2 * j + 2])
                    res = fma(dvs, L.cv, -data[j + 1])
                    ssq = fma(res, res, ssq)
                W, Rh = enter(L, *eval_full(L, ms, x))
            else:
                tsum = None
                for j in range(r, r + nu):
                    W, Rh, ms, tsum = step(L, W, Rh, ms, vl[2 * j], vl[2 * j + 1], vl[2 * j + 2], data[j + 1], tsum, carry)
                ssq = ssq + tsum
            r += nu
            trip += 1
    return {"w": W * (1.0 / L.kvk) if L.damp else W, "Rh": Rh, "ssq": ssq}


def walk_ext(m, dc, a, b, vl, data, steps, at=(), dtype=LD):
    """the extended-precision RK4 on the tabulated loading -> dict(w, Rh, ssq) in np.longdouble, and the states (mu, theta) after the
    step counts in `at`.  dtype=np.float64: the same literal RK4 in plain float64 — what a float64 solve can be expected to reach"""
    def wd(x):
        return np.asarray(np.asarray(x, dtype=np.float64), dtype=dtype)

    dcw, aw, bw = wd(dc), wd(a), wd(b)
    V_ref, mu_ref, k1 = wd(m.V_ref), wd(m.mu_ref), wd(m.k1)
    damping = bool(m.RadiationDamping)
    h = wd(float(m.delta_t))
    hh, h6 = h / 2, h / 6
    vlw, dw = wd(vl), wd(data)
    kprime = dtype(1e-2) * 10 / dcw

    def f(j, mu_, th_):
        v = V_ref * np.exp((mu_ - mu_ref - bw * np.log(V_ref * th_ / dcw)) / aw)
        d1 = 1 - v * th_ / dcw
        d0 = kprime * vlw[j] - kprime * v
        d2 = v / aw * (d0 - bw / th_ * d1)
        if damping:
            d0 = d0 - k1 * d2
            d2 = v / aw * (d0 - bw / th_ * d1)
        return d0, d1, d2

    mu, th = np.full(dcw.shape, wd(m.mu_t_zero)), dcw / V_ref
    ssq = np.full(dcw.shape, dw[0] * dw[0])
    states = {}
    with np.errstate(all="ignore"):
        for s in range(steps):
            a0, a1, a2 = f(2 * s, mu, th)
            b0, b1, b2 = f(2 * s + 1, mu + hh * a0, th + hh * a1)
            c0, c1, c2 = f(2 * s + 1, mu + hh * b0, th + hh * b1)
            e0, e1, e2 = f(2 * s + 2, mu + h * c0, th + h * c1)
            mu, th = mu + h6 * (a0 + 2 * b0 + 2 * c0 + e0), th + h6 * (a1 + 2 * b1 + 2 * c1 + e1)
            res = h6 * (a2 + 2 * b2 + 2 * c2 + e2) / h - dw[s + 1]
            ssq = ssq + res * res
            if s + 1 in at:
                states[s + 1] = (mu, th)
    w = np.exp((mu - mu_ref - bw * np.log(V_ref * th / dcw)) / aw)
    return {"w": w, "Rh": hh / th, "ssq": ssq}, states


def errors(got, ext):
    """relative error per lane of w, Rh and the sum of squares (float64)"""
    return {k: (np.abs(X._w(got[k]) - ext[k]) / np.abs(ext[k])).astype(np.float64) for k in ("w", "Rh", "ssq")}
