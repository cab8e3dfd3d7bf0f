"""
The in-step TIGHT step's stage brackets to first order in rho, and the per-lane limit on rho that goes with them, restated (a test
helper; TEST INFRASTRUCTURE ONLY).

csrc/rsf_device.h, tight_incr_scaled / tight_rho_limit: the stages form g = d0 - brx d1' with brx = bh (1 - rho) in place of
bh (1 - rho + rho^2), and the guard holds |rho| to
    lim_rho = min(2^-20, cbrt(2^-47 V_ref / |bh|)),    bh = beta / hhd = 20 b Dc / h,
|c1| to half of it, and the a-priori bound of tight_needs_guard its figure rb (and wave_begin's rmin) to 0.9 lim_rho / 2.  Here:
the limit in float64 (the kernel's is at most 1.3e-5 below it: two Newton steps, rounded down), the thresholds per lane, the
predicate of tests/tight_bound.py with the lane's limit in place of 2^-21, the lanes of the GPU tests (placed on the CPU by
bisection on the extended-precision scan), and the dropped term itself, |bh| rho^2 |d1'| of every stage, from an extended-precision
walk of its own.
"""
import numpy as np

import rk4_extended as X
import test_gpu_series_scale as S
import tight_bound as T

EPS = 2.0 ** -47
R20 = 2.0 ** -20
C = 2 * X.WAVE


def bh(m, dc, b):
    """Lane::bh = beta / hhd = (10 b V_ref) / ((h/2) V_ref / Dc): the factor of the theta term in a stage's bracket"""
    return 20.0 * np.asarray(b, dtype=np.float64) * np.asarray(dc, dtype=np.float64) / float(m.delta_t)


def lim_rho(m, dc, b):
    with np.errstate(all="ignore"):
        return np.minimum(R20, np.cbrt(EPS * float(m.V_ref) / np.abs(bh(m, dc, b))))


def thresholds(m, dc, b):
    """the guard's four thresholds per lane (tight_bound.GUARDS with the lane's limit on rho and c1)"""
    lim = lim_rho(m, dc, b)
    one = np.ones_like(lim)
    return {"rho": lim, "c1": 0.5 * lim, "dlt": T.GUARDS["dlt"] * one, "dlt_h": T.GUARDS["dlt_h"] * one}


def largest(r, m, dc, b):
    """(trips, lanes): the trip's largest increment over its own threshold"""
    thr = thresholds(m, dc, b)
    return np.maximum.reduce([r[k] / thr[k] for k in T.GUARDS])


def binding(r, m, dc, b):
    """per lane: the threshold its largest increment of the series comes closest to"""
    thr = thresholds(m, dc, b)
    keys = list(T.GUARDS)
    return np.array(keys)[np.argmax([(r[k] / thr[k]).max(axis=0) for k in keys], axis=0)]


def predicate(r, m, dc, b):
    """tight_needs_guard and W.never with the lane's limit: tight_bound.scan's figures rb and rmin are over 0.9 * 2^-21, the
    kernel's limit is 0.9 lim_rho / 2.  -> dict need (trips, lanes), D, rb (trips, lanes), never, dmin, rmin (lanes)"""
    scale = R20 / lim_rho(m, dc, b)
    rb, rmin = r["rb"] * scale, r["rmin"] * scale
    with np.errstate(all="ignore"):
        never = ~((r["dmin"] < 1.0) & (rmin < 1.0))
        need = ~((r["D"] < 1.0) & (rb < 1.0)) | never
    return {"need": need, "D": r["D"], "rb": rb, "never": never, "dmin": r["dmin"], "rmin": rmin}


def clear(p):
    """every decision of the predicate at least 10 % from its edge (as test_gpu_series_scale._clear requires)"""
    return S._clear(p)


def raised(m, w0):
    """the model with mu_t_zero raised so that the slip rate starts at w0 V_ref (for a lane with the model's a): theta starts
    at Dc / V_ref, so d theta / dt = 1 - w0 from the first stage on and |rho| ~ (h / 2 Dc) |1 - w0| — of order 1e-7 at Dc ~ 1e4,
    where bh is far beyond 8192 and the increments of mu are nowhere near their thresholds"""
    m.mu_t_zero = float(m.mu_ref) + float(m.a) * float(np.log(w0))
    return m


def place(m, a, b, steps, d, target, span=1.0e5):
    """Dc per lane at which the lane's largest increment of the series is `target` x the threshold that binds for it (the
    per-lane ones): log-bisection from 1.005 x TIGHT's a-priori edge upwards — every figure falls monotonically with Dc (rho over
    its limit like Dc^-2/3 where the new limit binds) — or 0.98 of what the edge allows, if that is less"""
    lo = 1.005 * S._edge(m, a) * np.ones(np.shape(target))

    def top(dc):
        return largest(S._scan(m, dc, a, b, steps, d), m, dc, b).max(axis=0)

    target = np.minimum(target, 0.98 * top(lo))
    hi = span * lo
    for _ in range(13):  # (Dc to 0.14 %, the figure to 0.1 %)
        mid = np.sqrt(lo * hi)
        above = top(mid) > target
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    return np.sqrt(lo * hi), target


def dropped_term(m, dc, steps, a=None, b=None, vl=None):
    """|bh| rho^2 |d1'| of the three stages whose bracket takes rho (d1' = (h/2) (d theta/dt) / theta_0, the kernel's scaled
    derivative; rho = the previous stage's d1', twice it at the full-step stage), largest over the first `steps` steps, from the
    extended-precision RK4.  -> float64 per lane, in the units of g (V_ref per unit)"""
    dcw = X._w(np.atleast_1d(dc))
    aw = X._w(np.full(dcw.shape, m.a) if a is None else np.broadcast_to(a, dcw.shape))
    bw = X._w(np.full(dcw.shape, m.b) if b is None else np.broadcast_to(b, dcw.shape))
    V_ref, mu_ref, k1 = X._w(m.V_ref), X._w(m.mu_ref), X._w(m.k1)
    damping = bool(m.RadiationDamping)
    h = X._w(float(m.delta_t))
    hh, h6 = h / 2, h / 6
    vlw = None if vl is None else X._w(vl)
    bhw = np.abs(20 * bw * dcw / h)
    mu, th = np.full(dcw.shape, X._w(m.mu_t_zero)), dcw / V_ref

    def f(j, mu_, th_):
        if vlw is None:
            return X._rhs(X._w(m.t_start) + j * hh, mu_, th_, dcw, aw, bw, V_ref, mu_ref, k1, damping)
        return T._rhs_vl(vlw[j], mu_, th_, dcw, aw, bw, V_ref, mu_ref, k1, damping)

    worst = np.zeros(dcw.shape, X.LD)
    with np.errstate(all="ignore"):
        for s in range(steps):
            a0, a1, _ = f(2 * s, mu, th)
            b0, b1, _ = f(2 * s + 1, mu + hh * a0, th + hh * a1)
            c0, c1, _ = f(2 * s + 1, mu + hh * b0, th + hh * b1)
            e0, e1, _ = f(2 * s + 2, mu + h * c0, th + h * c1)
            ra, rb_, rc, re = (hh * x / th for x in (a1, b1, c1, e1))  # the stages' d1'
            worst = np.maximum.reduce([worst, bhw * ra * ra * abs(rb_), bhw * rb_ * rb_ * abs(rc), bhw * (2 * rc) ** 2 * abs(re)])
            mu, th = mu + h6 * (a0 + 2 * b0 + 2 * c0 + e0), th + h6 * (a1 + 2 * b1 + 2 * c1 + e1)
    return worst.astype(np.float64)


# --- the lanes of the GPU tests (tests/test_gpu_linear_bracket.py), all found on the CPU ---------------------------------------

STEPS = [35, 200, 530]
W0 = 1.2  # the raised model's starting slip rate over V_ref: |1/x - w| = 0.2
# (steps, h, damping, d, model kind): "builtin" — wave 0 headline-like, wave 1 at 0.5 .. 0.9 of what binds (small Dc: the old
# thresholds); "raised" — both waves where bh > 8192 and the NEW limit binds, wave 0 at 0.1 .. 0.4 of it, wave 1 at 0.5 .. 0.9
ACCURACY = [(s, h, damping, 1, kind) for kind in ("builtin", "raised") for s in STEPS for h in (0.025, 0.1) for damping in (True, False)] + \
           [(35, 0.025, True, 3, "raised"), (530, 0.1, True, 3, "raised"), (200, 0.025, False, 3, "raised"), (530, 0.025, True, 3, "builtin")]


def model(oracle_mod, steps, h, damping, kind):
    m = S._model(oracle_mod, steps, h, damping)
    return raised(m, W0) if kind == "raised" else m


def accuracy_lanes(oracle_mod, steps, h, damping, d, kind):
    """-> (m, dc, a, b, targets of wave 1)"""
    m = model(oracle_mod, steps, h, damping, kind)
    a, b = S._ab(m, d, C, 31)
    dc = np.empty(C)
    want = np.linspace(0.5, 0.9, X.WAVE)
    w = slice(0, X.WAVE)
    if kind == "builtin":
        dc[w] = S._headline_wave(m, a[w], 32)
    else:
        dc[w], _ = place(m, a[w], b[w], steps, d, np.linspace(0.1, 0.4, X.WAVE))
    w = slice(X.WAVE, C)
    dc[w], want = place(m, a[w], b[w], steps, d, want)
    return m, dc, a, b, want


def series_scale_lanes(oracle_mod, steps, h, damping, d):
    """the lanes of test_gpu_series_scale's accuracy cases (its _reference, without the solves)"""
    m = S._model(oracle_mod, steps, h, damping)
    a, b = S._ab(m, d, C, 31)
    dc = np.empty(C)
    dc[:X.WAVE] = S._headline_wave(m, a[:X.WAVE], 32)
    dc[X.WAVE:], _ = S._place(m, a[X.WAVE:], b[X.WAVE:], steps, d, np.linspace(0.5, 0.9, X.WAVE))
    return m, dc, a, b


OVERS = (1.07, 1.15, 1.35)
PATHS = [(s, h, damping, 1) for s in STEPS for h in (0.025, 0.1) for damping in (True, False)] + [(200, 0.025, True, 3), (530, 0.1, True, 3)]
FREE = [(200, 0.025), (530, 0.1)]


def decision_lanes(oracle_mod, h, damping, steps=200, k=7):
    """test_guard_on_the_lanes_limit: raised model, both waves at 0.3 .. 0.9 of the new limit; then lane k of wave 0 at each of OVERS
    x its limit.  -> (m, a, b, dc of the lanes that stay, {over: (dc with lane k moved, the target reached)})"""
    m = model(oracle_mod, steps, h, damping, "raised")
    a, b = S._ab(m, 1, C, 0)
    dc, _ = place(m, a, b, steps, 1, np.linspace(0.3, 0.9, C))
    over = {}
    for o in OVERS:
        dck, got = place(m, a[k:k + 1], b[k:k + 1], steps, 1, np.array([o]))
        dco = dc.copy()
        dco[k] = dck[0]
        over[o] = (dco, got[0])
    return m, a, b, dc, over


def paths_lanes(oracle_mod, steps, h, damping, d):
    """test_paths_with_the_lanes_bound_bit_for_bit: built-in model, wave 0 at 0.02 .. 0.1 of the lane's thresholds, wave 1 the same
    Dc but for its first lane at 0.6 of its threshold"""
    m = S._model(oracle_mod, steps, h, damping)
    a1, b1 = S._ab(m, d, X.WAVE, 41)
    a, b = np.tile(a1, 2), np.tile(b1, 2)
    free, _ = place(m, a1, b1, steps, d, np.linspace(0.02, 0.1, X.WAVE))
    dc = np.tile(free, 2)
    dc[X.WAVE] = place(m, a[X.WAVE:X.WAVE + 1], b[X.WAVE:X.WAVE + 1], steps, d, np.array([0.6]))[0][0]
    return m, dc, a, b


def free_lanes(oracle_mod, steps, h, damping):
    """test_bound_frees_lanes_inside_their_own_limit: raised model, both waves at 0.3 .. 0.75 of the new limit"""
    m = model(oracle_mod, steps, h, damping, "raised")
    a, b = S._ab(m, 1, C, 0)
    dc, _ = place(m, a, b, steps, 1, np.linspace(0.3, 0.75, C))
    return m, dc, a, b


def held_lanes(oracle_mod, steps, h, damping, k=7, over=1.35):
    """test_lanes_bound_keeps_the_guard: raised model, both waves the same 64 lanes at 0.3 .. 0.6 of the new limit — free under the
    lane's Bmax — but for lane k of wave 0 at `over` x its limit: beyond its own Bmax, inside the constant 0.9 * 2^-21"""
    m = model(oracle_mod, steps, h, damping, "raised")
    a1, b1 = S._ab(m, 1, X.WAVE, 0)
    a, b = np.tile(a1, 2), np.tile(b1, 2)
    dc = np.tile(place(m, a1, b1, steps, 1, np.linspace(0.3, 0.6, X.WAVE))[0], 2)
    dc[k] = place(m, a[k:k + 1], b[k:k + 1], steps, 1, np.array([over]))[0][0]
    return m, dc, a, b


def series_scale_decision_lanes(oracle_mod, kind, damping, steps=200, k=7):
    """the lanes of test_gpu_series_scale.test_guard_on_the_rescaled_increments: placed against the CONSTANT thresholds
    -> (m, a, b, [dc of the lanes that stay, and with lane k at 1.07, 1.15, 1.35 of a constant threshold])"""
    h, loading = (0.025, None) if kind == "rho" else (0.1, S._strong_loading)
    m = S._model(oracle_mod, steps, h, damping, loading)
    a, b = S._ab(m, 1, C, 0)
    dc, _ = S._place(m, a, b, steps, 1, np.linspace(0.3, 0.9, C))
    out = [dc]
    for o in OVERS:
        dco = dc.copy()
        dco[k] = S._place(m, a[k:k + 1], b[k:k + 1], steps, 1, np.array([o]))[0][0]
        out.append(dco)
    return m, a, b, out


def series_scale_paths_lanes(oracle_mod, steps, h, damping, d):
    """the lanes of test_gpu_series_scale.test_guarded_and_unguarded_trips_bit_for_bit"""
    m = S._model(oracle_mod, steps, h, damping)
    a1, b1 = S._ab(m, d, X.WAVE, 41)
    a, b = np.tile(a1, 2), np.tile(b1, 2)
    free, _ = S._place(m, a1, b1, steps, d, np.linspace(0.02, 0.1, X.WAVE))
    dc = np.tile(free, 2)
    dc[X.WAVE] = S._place(m, a[X.WAVE:X.WAVE + 1], b[X.WAVE:X.WAVE + 1], steps, d, np.array([0.6]))[0][0]
    return m, dc, a, b
