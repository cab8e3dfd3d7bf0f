"""
The in-step TIGHT step with one log1p bracket for its two half-step stages, and the per-lane limit on rho that goes with it,
restated (a test helper; TEST INFRASTRUCTURE ONLY).

csrc/rsf_device.h, rk4_tight<..., INSTEP> / tight_incr_scaled / tight_bracket / tight_pb_limit / make_series: the step of
tests/ms_free.py (imported, not edited: its `step` stays the form before this change) with the bracket pb = B + N rho formed once,
at the first half-step stage's rho_a = a1, and taken by the second with its own r = b1.  `share` names the form:
  "none"  every stage its own bracket — ms_free.step, the parent's form;
  "half"  the two half-step stages share the first one's — the kernel's form;
  "full"  the full-step stage takes it too, B + N a1 in place of B - B c1 — the form first proposed, NOT the kernel's: that stage's
          rho is 2 c1, twice a half-step stage's, so what it leaves out is (b/a) |c1| |2 c1 - a1| ~ (b/a) c1^2, first order in the
          bracket and beyond 2^-44 at the guard's edge (`dropped_term`; tests/test_shared_bracket.py measures it);
  "drop"  no second-order term in the three stage brackets at all (pb = B), for the record.
`lim_pb` is tight_pb_limit in float64, operation for operation; `lim_rho` the lane's limit with it, min(tight_rho_limit's, lim_pb);
`predicate` tests/linear_bracket.py's with that limit; `dropped_term` what the shared bracket leaves out of dlt, from an
extended-precision walk of its own.
"""
import numpy as np

import linear_bracket as LB
import ms_free as M
import rk4_extended as X
import tight_bound as T

fma = M.fma
EPS = 2.0 ** -43  # what the limit holds the dropped term to (2^-44, first meant, binds on lanes the guard's tests keep in TIGHT)
C_PB = float.fromhex("0x1.ff801ff801ff8p-34")  # 2^-33 / (1 + 2^-10), truncated: the kernel's constant


def lim_pb(boa, Rh):
    """tight_pb_limit: ((1 - 2^-30) C) * (1 / |boa Rh|) in float64 (NumPy's reciprocal for the kernel's, <= 1 ulp apart).  A zero,
    infinite or NaN product gives NaN here as there: `lim_rho` keeps the other limit"""
    with np.errstate(all="ignore"):
        den = np.abs(np.asarray(boa, dtype=np.float64) * np.asarray(Rh, dtype=np.float64))
        # fm::rcp(0): inf seed, fm::rcp(inf): 0 seed — either way the Newton step forms inf * 0 and the result is NaN
        r = np.where((den == 0.0) | np.isinf(den), np.nan, 1.0 / den)
        return ((1.0 - 2.0 ** -30) * C_PB) * r


def lim_pb_ext(boa, Rh):
    """the limit as the derivation states it, in extended precision: EPS / ((b/2a) (2^-10 + 2^-20) 2 |Rh|)"""
    LD = X.LD
    with np.errstate(all="ignore"):
        return LD(EPS) / (np.abs(X._w(boa)) / 2 * (LD(2.0 ** -10) + LD(2.0 ** -20)) * 2 * np.abs(X._w(Rh)))


def rh_entry(m, dc, theta=None):
    """Rh = (h/2 Dc) / x = (h/2) / theta of a state (default: the series' start, theta = Dc / V_ref)"""
    dc = np.asarray(dc, dtype=np.float64)
    theta = dc / float(m.V_ref) if theta is None else theta
    return 0.5 * float(m.delta_t) / theta


def lim_rho(m, dc, a, b, Rh):
    """the lane's limit on |rho| as make_series forms it: fmin(tight_rho_limit, tight_pb_limit) — fmin keeps the first where the
    second is NaN"""
    return np.fmin(LB.lim_rho(m, dc, b), lim_pb(np.asarray(b, dtype=np.float64) / np.asarray(a, dtype=np.float64), Rh))


def predicate(r, m, dc, a, b):
    """linear_bracket.predicate with the new limit in tight_needs_guard's bmax — formed from the Rh of every trip's start state, as a
    loop entered there would.  wave_begin's gate W.never keeps tight_rho_limit's figure (the kernel's does)"""
    old = LB.predicate(r, m, dc, b)
    lim = lim_rho(m, dc, a, b, rh_entry(m, dc, r["theta"]))  # (trips, lanes)
    rb = r["rb"] * (LB.R20 / lim)
    with np.errstate(all="ignore"):
        need = ~((r["D"] < 1.0) & (rb < 1.0)) | old["never"]
    return {"need": need, "D": r["D"], "rb": rb, "never": old["never"], "dmin": old["dmin"], "rmin": old["rmin"], "lim": lim}


def step(L, W, Rh, vl0, vlm, vl1, obs, tsum, share="half"):
    """rk4_tight<DAMP, TIGHT, INSTEP = true> with the shared bracket -> (W, Rh, tsum); tsum None starts the trip's sum"""

    def incr(stage, r, pb, d):
        dl = fma(-r, pb, d)
        if stage == 0:
            e = fma(fma(L.h2, dl, L.h1), dl, L.khh)
        elif stage == 1:
            e = fma(fma(fma(L.f3, dl, L.f2), dl, L.f1), dl, L.kh)
        else:
            e = fma(fma(fma(L.e3, dl, L.e2), dl, L.e1), dl, L.kh6)
        return fma(W * dl, e, W)

    xh, xf = L.hhdw, L.hdw
    a0, a1, a2 = M._rhs(L, W, xh, Rh, vl0, L.bh)
    sv = W * a2
    pb = L.B if share == "drop" else fma(a1, L.N, L.B)
    w = incr(0, a1, pb, a0)
    b0, b1, b2 = M._rhs(L, w, fma(xh, a1, xh), Rh, vlm, fma(-L.bh, a1, L.bh))
    sm = w * b2
    w = incr(0, b1, pb if share != "none" else fma(b1, L.N, L.B), b0)
    c0, c1, c2 = M._rhs(L, w, fma(xh, b1, xh), Rh, vlm, fma(-L.bh, b1, L.bh))
    sm = fma(w, c2, sm)
    w = incr(1, c1, pb if share in ("full", "drop") else fma(-c1, L.B, L.B), c0)
    e0, e1, e2 = M._rhs(L, w, fma(xf, c1, xh), Rh, vl1, fma(c1, L.bh2, L.bh))
    sv = fma(w, e2, sv)
    t0 = a0 + 2.0 * b0 + 2.0 * c0 + e0
    t1 = a1 + 2.0 * b1 + 2.0 * c1 + e1
    w = incr(2, t1, fma(t1, L.N6, L.B), t0)
    rho = t1 * (1.0 / 3.0)
    r = fma(sv, L.cv, fma(sm, L.cv2, -obs))
    tsum = r * r if tsum is None else fma(r, r, tsum)
    return w, fma(Rh, fma(rho, rho, -rho), Rh), tsum


def walk(m, dc, a, b, vl, data, steps, share="half"):
    """ms_free.walk(carry=False) with `step` above -> dict(w, Rh, ssq); share="none" is that walk to the bit"""
    L = M.Lane(m, dc, a, b)
    W, Rh = M.enter(L, *M.eval_full(L, L.ms0, L.x0))
    ssq = np.full(np.shape(dc), float(data[0]) ** 2)
    r = 0
    with np.errstate(all="ignore"):
        while r < steps:
            nu = M.TRIP if r + M.TRIP <= steps else 2
            assert r + nu <= steps, "an even number of steps"
            tsum = None
            for j in range(r, r + nu):
                W, Rh, tsum = step(L, W, Rh, vl[2 * j], vl[2 * j + 1], vl[2 * j + 2], data[j + 1], tsum, share)
            ssq = ssq + tsum
            r += nu
    return {"w": W * (1.0 / L.kvk) if L.damp else W, "Rh": Rh, "ssq": ssq}


def dropped_term(m, dc, steps, a=None, b=None, vl=None):
    """What a shared bracket leaves out of a stage's dlt, (b/2a) |rho_s| |rho_s - rho_a|, largest over the first `steps` steps of the
    extended-precision RK4: -> dict of float64 per lane
      half   the second half-step stage, rho_s = b1' (the kernel's form)
      full   the full-step stage had it taken the bracket too, rho_s = 2 c1'
      rho    the largest |rho| of the half-step stages and the step's end, c1 the largest |c1'| (tight_bound.scan's, over the series)
      bound  the derivation's (b/2a) |rho_b| (|Rh| + |rho_a|)(|dlt_a| + |rho_a|), largest over the steps, for comparison
    (d1' = (h/2)(d theta/dt)/theta_0, the kernel's scaled derivative; Rh = (h/2)/theta_0)"""
    dcw = X._w(np.atleast_1d(dc))
    aw = X._w(np.full(dcw.shape, m.a) if a is None else np.broadcast_to(a, dcw.shape))
    bw = X._w(np.full(dcw.shape, m.b) if b is None else np.broadcast_to(b, dcw.shape))
    V_ref, mu_ref, k1 = X._w(m.V_ref), X._w(m.mu_ref), X._w(m.k1)
    damping = bool(m.RadiationDamping)
    h = X._w(float(m.delta_t))
    hh, h6 = h / 2, h / 6
    vlw = None if vl is None else X._w(vl)
    b2a = np.abs(bw / aw) / 2
    mu, th = np.full(dcw.shape, X._w(m.mu_t_zero)), dcw / V_ref

    def f(j, mu_, th_):
        if vlw is None:
            return X._rhs(X._w(m.t_start) + j * hh, mu_, th_, dcw, aw, bw, V_ref, mu_ref, k1, damping)
        return T._rhs_vl(vlw[j], mu_, th_, dcw, aw, bw, V_ref, mu_ref, k1, damping)

    out = {k: np.zeros(dcw.shape, X.LD) for k in ("half", "full", "rho", "c1", "bound")}
    with np.errstate(all="ignore"):
        for s in range(steps):
            a0, a1, _ = f(2 * s, mu, th)
            b0, b1, _ = f(2 * s + 1, mu + hh * a0, th + hh * a1)
            c0, c1, _ = f(2 * s + 1, mu + hh * b0, th + hh * b1)
            e0, e1, _ = f(2 * s + 2, mu + h * c0, th + h * c1)
            ra, rb_, rc = (hh * x / th for x in (a1, b1, c1))
            s1 = h6 * (a1 + 2 * b1 + 2 * c1 + e1)
            dlt_a = np.abs((hh * a0 - bw * np.log1p(ra)) / aw)
            out["half"] = np.maximum(out["half"], b2a * abs(rb_) * abs(rb_ - ra))
            out["full"] = np.maximum(out["full"], b2a * abs(2 * rc) * abs(2 * rc - ra))
            out["rho"] = np.maximum.reduce([out["rho"], abs(ra), abs(rb_), abs(s1 / th)])
            out["c1"] = np.maximum(out["c1"], abs(rc))
            out["bound"] = np.maximum(out["bound"], b2a * abs(rb_) * (hh / th + abs(ra)) * (dlt_a + abs(ra)))
            mu, th = mu + h6 * (a0 + 2 * b0 + 2 * c0 + e0), th + s1
    return {k: v.astype(np.float64) for k, v in out.items()}


# --- the guard's thresholds with the new limit, and lanes placed against them ---------------------------------------------------

def thresholds(m, dc, a, b, Rh=None):
    """tight_bound.GUARDS per lane, with the lane's limit on rho and c1 as make_series forms it from Rh (default: the series' start)"""
    lim = lim_rho(m, dc, a, b, rh_entry(m, dc) if Rh is None else Rh)
    one = np.ones_like(lim)
    return {"rho": lim, "c1": 0.5 * lim, "dlt": T.GUARDS["dlt"] * one, "dlt_h": T.GUARDS["dlt_h"] * one}


def largest(r, m, dc, a, b):
    """(trips, lanes): the trip's largest increment over its own threshold"""
    thr = thresholds(m, dc, a, b)
    return np.maximum.reduce([r[k] / thr[k] for k in T.GUARDS])


def binding(r, m, dc, a, b):
    """per lane: the threshold its largest increment of the series comes closest to; "pb" where that is rho or c1 AND the lane's
    limit is lim_pb, the shared bracket's"""
    thr = thresholds(m, dc, a, b)
    keys = list(T.GUARDS)
    which = np.array(keys)[np.argmax([(r[k] / thr[k]).max(axis=0) for k in keys], axis=0)]
    pb = np.isin(which, ("rho", "c1")) & (thr["rho"] < LB.lim_rho(m, dc, b))
    return np.where(pb, "pb", which)


# --- a model on which the new limit is the one that decides ---------------------------------------------------------------------
# lim_pb falls below tight_rho_limit's where (b/a) |Rh| > 1.22e-4 while |rho| = |Rh (1 - w x)| stays under it: small Dc, b/a raised,
# and a state close to steady.  h = 0.1; b = BOA a (the model's b for one parameter, per lane for three); mu_t_zero raised so that the
# slip rate starts at W0 V_ref, |1 - w x| = 0.003 from the first stage on and for the whole series (theta relaxes over Dc / V_ref,
# thousands of seconds); a caller's loading of amplitude 0.02 V_ref, so that no increment of mu is anywhere near its threshold and
# the a-priori bound (tight_needs_guard) can free the lanes well inside the limit.  There Dc of 560 .. 1700 has lim_pb at 0.23 .. 0.98
# of the parent's limit, and |rho| over lim_pb falls like Dc^-2 through 2.5 .. 0.26.
BOA, W0, H_BIND = 6.0, 1.003, 0.1


def quiet_loading(t):
    return 1.0 + 0.02 * np.exp(-t / 20) * np.sin(10 * t)


def binding_model(model, steps, damping):
    """model: test_gpu_series_scale._model's signature without the oracle module bound, (steps, h, damping, loading) -> ModelSpec"""
    m = model(steps, H_BIND, damping, quiet_loading)
    m.b = BOA * float(m.a)
    return LB.raised(m, W0)
