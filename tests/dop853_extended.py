"""
Extended-precision reference of the DOP853 forward model (a test helper; TEST INFRASTRUCTURE ONLY).

`solve` is RateStateModel.evaluate with the reference's own integrator — Hairer's DOP853 as scipy.integrate.ode('dop853',
rtol=1e-6, atol=1e-10) drives it, one call per output interval (RateStateModel.py:374-389) — computed in np.longdouble (the
x87 80-bit format, 64-bit mantissa) and vectorised over lanes.  It restates the published algorithm as the C restatement
does (oracle/rsf_oracle.c: dp_hinit, dp_call, solve_dop853): safety 0.9, step factors 0.3 .. 6, beta 0, NMAX 500, HMAX = the
interval, the 1.01 `last` test, the uround test, HINIT on the first call and the step size carried between calls.  The
tableau is the float64 table the kernels compile (include/rsf_dop853_tableau.h), parsed and widened exactly, so the same
discrete map is computed and only rounding separates this reference from the kernels.  Output times are the model's float64
grid, x_k = x_(k-1) + delta_t as the oracle accumulates it; inside an interval x advances in the solve's own arithmetic.

`dtype=np.float64` runs the same code in float64: it must then reproduce the C restatement to rounding and take the same
decisions — the check that the two restate the same algorithm.

Every solve keeps a record of each lane's decisions (Record): steps and rejections per interval, whether every interval
after the first was ONE accepted step of the full interval (the precondition of the kernels' steady-state fast path,
csrc/rsf_device_dop853.h), the largest |rho| = |dtheta/theta_0| and |dlt| = |log(v/v_0)| of the stage increments of those
steps against friction_incr's guard (2^-20, 2^-9), and the smallest relative margin of any decision from its threshold:
err against 1 (accept), err against kErrStandard (the fast path continues) and x + 1.01 h - xend (the last step).  The
kernels form err and the carried step size to ~1e-7 in the fast path, so a lane whose margin is below MARGIN may decide
otherwise on the GPU, legitimately: such lanes are "decision-adjacent" and are held only to the parity tolerance.
"""
import ctypes
import ctypes.util
import os
import re

import numpy as np

LD = np.longdouble
if np.finfo(LD).nmant < 63:  # a float64 "longdouble" (aarch64 Linux: binary128, MSVC: binary64) is no reference
    raise RuntimeError(f"np.longdouble has a {np.finfo(LD).nmant}-bit mantissa: the extended-precision reference needs >= 63")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE = 64
RTOL, ATOL = 1e-6, 1e-10
SAFE, FACC1, FACC2, EXPO1, UROUND, NMAX = 0.9, 1.0 / 0.3, 1.0 / 6.0, 1.0 / 8.0, 2.3e-16, 500
ERR_STANDARD = (1.01 * 0.9) ** 8          # rsf_device_dop853.h kErrStandard (the same product, rounded per factor there)
GUARD_RHO, GUARD_DLT = 2.0 ** -20, 2.0 ** -9  # friction_incr's series range (guard_tripped)
MARGIN = 1e-5                             # decision-adjacent below this relative margin


def _tableau():
    """include/rsf_dop853_tableau.h -> float64 arrays C[12], A[11, 11], W[8], B[8], E5[8], E3[8] (hex literals: exact)"""
    with open(os.path.join(ROOT, "include", "rsf_dop853_tableau.h")) as f:
        src = f.read()

    def arr(name):
        body = re.search(r"RSF_DP_" + name + r"(?:\[\d+\])+\s*=\s*\{(.*?)\};", src, re.S).group(1)
        toks = re.findall(r"-?0x[0-9a-fA-F.]+p[-+]?\d+|-?\d+", body)
        return np.array([float.fromhex(t) if "x" in t else int(t) for t in toks])

    A = arr("A").reshape(11, 11)
    return arr("C"), A, arr("W_STAGE").astype(int), arr("B"), arr("E5"), arr("E3")


TAB_C, TAB_A, TAB_W, TAB_B, TAB_E5, TAB_E3 = _tableau()


class Record:
    """per lane (L lanes, n intervals)"""

    def __init__(self, n, L):
        self.steps = np.zeros((n, L), np.int16)    # accepted + rejected steps of interval k (k = 0 unused)
        self.rejects = np.zeros((n, L), np.int16)
        self.one_step = np.zeros((n, L), bool)     # interval k was one accepted step of its full length
        self.rho = np.zeros((n, L), np.float32)    # max |rho|, |dlt| over the stages of interval k's steady-state step
        self.dlt = np.zeros((n, L), np.float32)    # (intervals >= 2; 0 where the interval was not one full step)
        self.margin = np.full(L, np.inf)           # smallest relative margin of any decision
        self.failed_at = np.full(L, -1)            # interval whose call failed (-1: none)

    @property
    def steady(self):
        """every interval after the first one step of the full interval (the fast path's precondition)"""
        return self.one_step[2:].all(axis=0) & (self.failed_at < 0)

    @property
    def adjacent(self):
        return self.margin < MARGIN

    def guard_frac(self, k0=2):
        """max over the steady-state stages of intervals >= k0 of |rho| / 2^-20 and |dlt| / 2^-9"""
        return np.fmax(self.rho[k0:].max(axis=0) / GUARD_RHO, self.dlt[k0:].max(axis=0) / GUARD_DLT).astype(np.float64)


def _libm(name, *extra):
    """the C library's own function, elementwise (float64 mode: NumPy's exp/log/sin/pow may differ from libm's in the last
    bit; IEEE results for every argument, which Python's math module does not give)"""
    f = getattr(ctypes.CDLL(ctypes.util.find_library("m")), name)
    f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double] * (1 + len(extra))
    u = np.frompyfunc(lambda x: f(x, *extra), 1, 1)
    return lambda x: np.asarray(u(x), dtype=np.float64)


_LIBM = {"exp": _libm("exp"), "log": _libm("log"), "sin": _libm("sin"), "pow8": _libm("pow", 1.0 / 8.0)}
_NP = {"exp": np.exp, "log": np.log, "sin": np.sin, "pow8": lambda x: x ** x.dtype.type(EXPO1)}


def solve(m, dc, a=None, b=None, data=None, dtype=LD):
    """-> (acc [nout, L], ssq [L] or None, Record).  `m`: any object with RateStateModel's attributes (a, b, mu_ref, V_ref,
    k1, mu_t_zero, t_start, t_final, num_tsteps, RadiationDamping).  dtype: LD (the reference) or np.float64; in float64 the
    transcendental functions are the C library's (those the C restatement calls), so the two compute the same numbers."""
    T = dtype
    fn = _LIBM if T is np.float64 else _NP

    def w(x):  # float64 -> T exactly
        return np.asarray(np.asarray(x, dtype=np.float64), dtype=T)

    dc = w(np.atleast_1d(dc))
    L = dc.size
    a = w(np.full(L, m.a) if a is None else np.broadcast_to(a, (L,)))
    b = w(np.full(L, m.b) if b is None else np.broadcast_to(b, (L,)))
    V_ref, mu_ref, k1 = T(m.V_ref), T(m.mu_ref), T(m.k1)
    damping = bool(m.RadiationDamping)
    n = int(np.floor((m.t_final - m.t_start) / m.delta_t))       # RateStateModel.py:358
    dt64 = (float(m.t_final) - float(m.t_start)) / int(m.num_tsteps)  # rsf_set_model's delta_t
    grid = np.empty(n)                                           # the float64 output times, accumulated as the oracle does
    x64 = float(m.t_start)
    for k in range(n):
        grid[k] = x64
        x64 = x64 + dt64
    C, A, B, E5, E3 = (w(v) for v in (TAB_C, TAB_A, TAB_B, TAB_E5, TAB_E3))
    kp_all = T(1e-2) * 10 / dc
    one, rtol, atol = T(1), T(RTOL), T(ATOL)

    def f(t, y, ix):  # RateStateModel.py:318-355, literal (friction() of the oracle)
        kp, dci, ai, bi = kp_all[ix], dc[ix], a[ix], b[ix]
        V_l = V_ref * (1 + fn["exp"](-t / 20) * fn["sin"](10 * t))
        v = V_ref * fn["exp"](1 / ai * (y[0] - mu_ref - bi * fn["log"](V_ref * y[1] / dci)))
        d1 = 1 - v * y[1] / dci
        d0 = kp * V_l - kp * v
        d2 = v / ai * (d0 - bi / y[1] * d1)
        if damping:
            d0 = d0 - k1 * d2
            d2 = v / ai * (d0 - bi / y[1] * d1)
        return np.stack([d0, d1, d2])

    def hinit(x, y, f0, hmax, ix):  # dp_hinit (posneg = +1)
        sk = atol + rtol * np.abs(y)
        dnf = ((f0 / sk) ** 2).sum(axis=0)
        dny = ((y / sk) ** 2).sum(axis=0)
        h = np.where((dnf <= T(1e-10)) | (dny <= T(1e-10)), T(1e-6), np.sqrt(dny / dnf) * T(0.01))
        h = np.fmin(h, hmax)
        f1 = f(x + h, y + h * f0, ix)
        der2 = np.sqrt((((f1 - f0) / sk) ** 2).sum(axis=0)) / h
        der12 = np.fmax(np.abs(der2), np.sqrt(dnf))
        h1 = np.where(der12 <= T(1e-15), np.fmax(T(1e-6), np.abs(h) * T(1e-3)), fn["pow8"](T(0.01) / der12))
        return np.fmin(np.fmin(100 * np.abs(h), h1), hmax)

    rec = Record(n, L)
    acc = np.zeros((n, L), dtype=T)
    y = np.stack([np.full(L, T(m.mu_t_zero)), dc / V_ref, np.full(L, V_ref)])
    x = np.full(L, w(m.t_start))
    hc = np.zeros(L, dtype=T)  # WORK(7): the carried step size (0 => HINIT)
    vprev = np.full(L, V_ref)
    dt = T(dt64)
    alive = np.ones(L, bool)
    with np.errstate(all="ignore"):
        for kk in range(1, n):
            xend = w(grid[kk])
            ix = np.flatnonzero(alive)
            if ix.size == 0:
                break
            # one dp_call for every live lane: a masked loop until each lane is done (stiff lanes cost only their own steps)
            xs, ys, h = x[ix], y[:, ix], hc[ix]
            hmax = xend - xs
            k0 = f(xs, ys, ix)
            cold = h == 0
            if cold.any():
                h[cold] = hinit(xs[cold], ys[:, cold], k0[:, cold], hmax[cold], ix[cold])
            last = np.zeros(ix.size, bool)
            reject = np.zeros(ix.size, bool)
            nstep = np.zeros(ix.size, np.int32)
            nrej = np.zeros(ix.size, np.int32)
            ok = np.zeros(ix.size, bool)
            run = np.arange(ix.size)
            while run.size:
                r = run
                xr, yr, hr, kr0 = xs[r], ys[:, r], h[r], k0[:, r]
                bad = (nstep[r] > NMAX) | (T(0.1) * np.abs(hr) <= np.abs(xr) * T(UROUND))
                lt = xr + T(1.01) * hr - xend
                rec.margin[ix[r]] = np.fmin(rec.margin[ix[r]], np.where(bad, np.inf, np.abs(lt / (T(1.01) * hr)).astype(np.float64)))
                go_last = (lt > 0) & ~bad
                hr = np.where(go_last, xend - xr, hr)
                lr = last[r] | go_last
                first_full = go_last & (nstep[r] == 0)
                nstep[r] += 1
                k = [kr0]
                for st in range(1, 12):
                    s = np.zeros_like(yr)
                    for j in range(st):
                        if TAB_A[st - 1, j] != 0.0:  # (the C restatement adds 0 k_j: the same sum for finite k_j)
                            s = s + A[st - 1, j] * k[j]
                    ysx = yr + hr * s
                    k.append(f(xr + hr if st == 11 else xr + C[st] * hr, ysx, ix[r]))
                    if kk >= 2:  # the steady state's stage increments (friction_incr's series arguments)
                        rho = (ysx[1] - yr[1]) / yr[1]
                        dlt = ((ysx[0] - yr[0]) - b[ix[r]] * np.log1p(rho)) / a[ix[r]]
                        sel = ix[r][first_full]
                        rec.rho[kk, sel] = np.fmax(rec.rho[kk, sel], np.abs(rho[first_full]).astype(np.float32))
                        rec.dlt[kk, sel] = np.fmax(rec.dlt[kk, sel], np.abs(dlt[first_full]).astype(np.float32))
                s = np.zeros_like(yr)
                for j in range(8):
                    s = s + B[j] * k[TAB_W[j]]
                k5 = yr + hr * s
                sk = atol + rtol * np.fmax(np.abs(yr), np.abs(k5))
                e3 = np.zeros_like(yr)
                e5 = np.zeros_like(yr)
                for j in range(8):
                    e3 = e3 + E3[j] * k[TAB_W[j]]
                    e5 = e5 + E5[j] * k[TAB_W[j]]
                err2 = ((e3 / sk) * (e3 / sk)).sum(axis=0)
                err = ((e5 / sk) * (e5 / sk)).sum(axis=0)
                deno = err + T(0.01) * err2
                deno = np.where(deno <= 0, one, deno)
                err = np.abs(hr) * err * np.sqrt(1 / (3 * deno))
                fac11 = fn["pow8"](err)
                fac = np.fmax(T(FACC2), np.fmin(T(FACC1), fac11 / T(SAFE)))
                hnew = hr / fac
                acc_ = err <= 1
                e64 = err.astype(np.float64)
                mg = np.abs(e64 - 1)
                # the fast path continues while err < kErrStandard: a decision wherever the step was the full interval
                mg = np.where(first_full, np.fmin(mg, np.abs(e64 / ERR_STANDARD - 1)), mg)
                rec.margin[ix[r]] = np.fmin(rec.margin[ix[r]], np.where(bad, np.inf, mg))
                # accepted: first-same-as-last, x += h
                up = acc_ & ~bad
                if up.any():
                    u = r[up]
                    k0[:, u] = f(xr[up] + hr[up], k5[:, up], ix[u])
                    ys[:, u] = k5[:, up]
                    xs[u] = xr[up] + hr[up]
                done = up & lr
                ok[r[done]] = True
                hc[ix[r[done]]] = hnew[done]
                rec.one_step[kk, ix[r[done]]] = first_full[done]
                cont = up & ~lr
                hn = np.where(np.abs(hnew) > hmax[r], hmax[r], hnew)
                hn = np.where(reject[r], np.fmin(np.abs(hn), np.abs(hr)), hn)
                hn_rej = hr / np.fmin(T(FACC1), fac11 / T(SAFE))
                rj = ~acc_ & ~bad
                nrej[r[rj]] += 1
                h[r] = np.where(rj, hn_rej, np.where(cont, hn, hr))
                reject[r] = np.where(rj, True, np.where(cont, False, reject[r]))
                last[r] = np.where(rj, False, lr)
                # bad: the call fails (returns 0) with its partial state
                run = r[~(bad | done)]
            rec.steps[kk, ix] = nstep
            rec.rejects[kk, ix] = nrej
            x[ix], y[:, ix] = xs, ys
            acc[kk, ix] = (ys[2] - vprev[ix]) / dt
            vprev[ix] = ys[2]
            fl = ix[~ok]
            rec.failed_at[fl] = kk
            alive[fl] = False
    ssq = None
    if data is not None:
        res = acc - w(data)[:, None]
        ssq = (res * res).sum(axis=0)
    return acc, ssq, rec


# ---------------------------------------------------------------------------------------------------------------------
# Lane placement by the reference's own record.  A GPU wave takes the fast path only if EVERY lane takes the standard step
# (__all(takes_standard_step)), so each set is one whole wave of 64 lanes, sorted, whose path follows from its own lanes:
#   fast        steady state over the whole series, increments at 2 .. 30 % of friction_incr's guard
#   fast_edge   steady state, increments at 55 .. 90 % of the guard
#   guard_trip  steady state, increments past the guard (x 2 .. 20): the interval is redone by call_general
#   mixed       fast lanes and two stiff ones: the whole wave runs the general loop with full evaluations
#   stiff       small Dc: rejections, several steps per interval, short predicted steps
#   failed      fast lanes and one lane (a = 1e-9, b = 1e-3) whose second call fails: the wave leaves the steady state for good
SETS = ("fast", "fast_edge", "guard_trip", "mixed", "stiff", "failed")
FRAC = {"fast": (0.02, 0.3), "fast_edge": (0.55, 0.9), "guard_trip": (2.0, 20.0)}
FAIL_LANE, FAIL_A, FAIL_B = 1000.0, 1e-9, 1e-3   # tests/test_gpu_parity.py::test_dop853_failed_calls_leave_zeros' first lane
MIXED_STIFF = (17, 45)                           # positions of the stiff lanes in the mixed wave


def pilot(m):
    """a float64 solve over a log grid of Dc: where each path lies for model m -> (dc grid, Record).  The model is scale-free
    in V_ref (Dc / V_ref is what matters): the grid scales with it."""
    g = float(m.V_ref) * np.exp(np.linspace(np.log(0.05), np.log(1e6), 52))
    return g, solve(m, g, dtype=np.float64)[2]


def place_lanes(m, seed=0, scan=None):
    """-> {set: (dc[64], a[64] or None, b[64] or None)}; a/b are given only where a lane needs its own (the failed set)"""
    g, rec = pilot(m) if scan is None else scan
    rng = np.random.default_rng(seed)
    # a model with mu_t_zero off mu_ref starts with large increments in every lane (they trip the guard there): its sets
    # are placed by the second half of the series, where the lanes have settled
    frac, steady = rec.guard_frac(placement_from(m)), rec.steady
    # the steady region is Dc above the last non-steady grid point; there log(frac) falls monotonically with log(Dc)
    i0 = np.flatnonzero(~steady)
    i0 = i0.max() + 1 if i0.size else 0
    lg, lf = np.log(g), np.log(np.fmax(frac, 1e-300))

    def dc_at(fr):  # where the fraction falls through fr for the last time, going up in Dc (log-log interpolation); at
        i = np.flatnonzero(lf >= np.log(fr)).max()  # most the steady region's bottom (the offset model's increments stay < 20)
        assert i + 1 < g.size, (fr, i)
        if i < i0:
            return g[i0]
        return np.exp(lg[i] + (lg[i + 1] - lg[i]) * (lf[i] - np.log(fr)) / (lf[i] - lf[i + 1]))

    def logu(lo, hi, size=WAVE):
        return np.sort(np.exp(rng.uniform(np.log(lo), np.log(hi), size)))

    out = {}
    for s, (flo, fhi) in FRAC.items():
        lo, hi = dc_at(fhi), dc_at(flo)
        out[s] = (logu(lo, hi), None, None)
    # stiff: grid points with rejections (and no failure); the range below the largest of them, a factor 4 wide
    rj = np.flatnonzero((rec.rejects.sum(axis=0) > 0) & (rec.failed_at < 0))
    hi = g[rj.max()]
    out["stiff"] = (logu(hi / 4, hi), None, None)
    fast = out["fast"][0]
    mixed = logu(fast[0], fast[-1])
    mixed[list(MIXED_STIFF)] = out["stiff"][0][[5, 60]]
    out["mixed"] = (mixed, None, None)
    failed = logu(fast[0], fast[-1])
    a, b = np.full(WAVE, float(m.a)), np.full(WAVE, float(m.b))
    failed[3], a[3], b[3] = FAIL_LANE * float(m.V_ref), FAIL_A, FAIL_B
    out["failed"] = (failed, a, b)
    return out


def placement_from(m):
    """the first interval whose increments place a lane"""
    return 2 if m.mu_t_zero == m.mu_ref else m.nout // 2


def lane_b(a, n_lanes, seed=0):
    """per-lane b for the (a, b) variant: b - a in [0.001, 0.005] (the default 0.003 in the middle: the paths stay put)"""
    return a + np.random.default_rng(seed + 1).uniform(0.001, 0.005, n_lanes)


# The models: (n, attribute overrides, variants, on the CPU test).  "ab" runs the same Dc with per-lane (a, b).
CASES = {
    "n500": (500, {}, ("plain", "ab"), True),
    "n500_nodamp": (500, {"RadiationDamping": False}, ("plain",), True),
    "n500_k1zero": (500, {"k1": 0.0}, ("plain",), False),  # (the reference: the same map as n500_nodamp)
    # every model constant away from its default (test_forward_with_non_default_model_constants)
    "nondefault": (400, {"t_start": 1.5, "t_final": 37.0, "V_ref": 1.7, "mu_ref": 0.55, "mu_t_zero": 0.5505, "k1": 3.0e-7,
                         "a": 0.012, "b": 0.0155}, ("plain", "ab"), True),
    # slip rates in SI units: atol = 1e-10 is no longer negligible against the V component
    "vref_si": (500, {"V_ref": 1.0e-6, "k1": 1.0e-7 / 1.0e-6}, ("plain",), True),
    # mu_t_zero off mu_ref: the first intervals start with large increments
    "n500_mu+5e-4": (500, {"mu_t_zero": 0.6 + 5e-4}, ("plain",), True),
    # more than one LDS chunk at some shapes; resync at (kk & 63) == 63 within each chunk
    "n2000": (2000, {}, ("plain", "ab"), False),
    "n2000_mu-4e-4_nodamp": (2000, {"mu_t_zero": 0.6 - 4e-4, "RadiationDamping": False}, ("plain",), False),
    "n4000": (4000, {}, ("plain",), False),
}


def make_model(ModelSpec, name):
    """the model of CASES[name] on any class with RateStateModel's attributes (ModelSpec(n, t0, t1, substeps)), dop853"""
    n, attrs, _, _ = CASES[name]
    t0, t1 = attrs.get("t_start", 0.0), attrs.get("t_final", 50.0)
    m = ModelSpec(n, t0, t1, 1)
    for k, v in attrs.items():
        setattr(m, k, v)
    m.delta_t = (t1 - t0) / n
    m.integrator = "dop853"
    return m


class Problem:
    """One model's lanes and their extended-precision solve.  Lanes: one wave of 64 per set (SETS order), per variant:
    "plain" the model's (a, b) (the failed set: per-lane arrays, the model's values but for its failing lane), "ab" the same
    Dc with per-lane b (lane_b).  The observation: the extended solve at the middle fast lane plus |acc| N(0, 1) (the
    bench's recipe), rounded to float64."""

    def __init__(self, ModelSpec, name, seed=0):
        self.name, self.sets, self.variants = name, SETS, CASES[name][2]
        self.m = make_model(ModelSpec, name)
        self.place = place_lanes(self.m, seed)
        self.dc = np.concatenate([self.place[s][0] for s in SETS])
        L = self.dc.size
        a0, b0 = float(self.m.a), float(self.m.b)
        self.a = {"plain": np.full(L, a0), "ab": np.full(L, a0)}
        self.b = {"plain": np.full(L, b0), "ab": lane_b(a0, L, seed)}
        fs = self.lanes("failed")
        for v in ("plain", "ab"):
            self.a[v][fs], self.b[v][fs] = self.place["failed"][1], self.place["failed"][2]
        self.plain_ab = {s: self.place[s][1] is not None for s in SETS}  # sets that pass per-lane (a, b) in "plain" too
        acc = solve(self.m, self.dc[WAVE // 2:WAVE // 2 + 1])[0][:, 0].astype(np.float64)
        self.data = acc + np.abs(acc) * np.random.default_rng(seed + 2).standard_normal(acc.size)
        V = len(self.variants)
        acc, ssq, rec = solve(self.m, np.tile(self.dc, V), np.concatenate([self.a[v] for v in self.variants]),
                              np.concatenate([self.b[v] for v in self.variants]), data=self.data)
        self.ext, self.rec = {}, {}
        for i, v in enumerate(self.variants):
            sl = slice(L * i, L * (i + 1))
            self.ext[v] = (acc[:, sl], ssq[sl])
            self.rec[v] = _sub(rec, sl)

    def lanes(self, s):
        i = self.sets.index(s)
        return slice(WAVE * i, WAVE * (i + 1))

    def forward(self, engine, variant, s=None, **kw):
        """engine.forward on every lane (or set s) of the variant: (ssq, acc).  Sets of the plain variant without lanes of
        their own (a, b) go in one launch without per-lane arrays (the kernels' no-(a, b) path), the others in a second."""
        if s is not None:
            sl = self.lanes(s)
            if variant == "plain" and not self.plain_ab[s]:
                return engine.forward(self.dc[sl], data=self.data, want_ssq=True, want_acc=True, **kw)
            return engine.forward(self.dc[sl], a=self.a[variant][sl], b=self.b[variant][sl], data=self.data, want_ssq=True,
                                  want_acc=True, **kw)
        if variant == "ab":
            return engine.forward(self.dc, a=self.a["ab"], b=self.b["ab"], data=self.data, want_ssq=True, want_acc=True, **kw)
        ssq, acc = np.empty(self.dc.size), np.empty((self.data.size, self.dc.size))
        own = np.concatenate([np.full(WAVE, self.plain_ab[s]) for s in SETS])
        s1, a1 = engine.forward(self.dc[~own], data=self.data, want_ssq=True, want_acc=True, **kw)
        s2, a2 = engine.forward(self.dc[own], a=self.a["plain"][own], b=self.b["plain"][own], data=self.data, want_ssq=True,
                                want_acc=True, **kw)
        ssq[~own], acc[:, ~own], ssq[own], acc[:, own] = s1, a1, s2, a2
        return ssq, acc


def _sub(rec, sl):
    r = Record(rec.steps.shape[0], 0)
    for k in ("steps", "rejects", "one_step", "rho", "dlt"):
        setattr(r, k, getattr(rec, k)[:, sl])
    for k in ("margin", "failed_at"):
        setattr(r, k, getattr(rec, k)[sl])
    return r


def rel_errors(acc, ssq, acc_ext, ssq_ext):
    """per-lane trajectory error max_k |acc - acc_ext| / max_k |acc_ext| and the sum of squares' relative error (float64)"""
    acc_ext = np.asarray(acc_ext, dtype=LD)
    w = np.asarray(np.asarray(acc, dtype=np.float64), dtype=LD)
    scale = np.abs(acc_ext).max(axis=0)
    scale = np.where(scale > 0, scale, LD(1))  # (a lane that fails in its first call can have acc = 0 throughout)
    traj = (np.abs(w - acc_ext).max(axis=0) / scale).astype(np.float64)
    s = None
    if ssq is not None:
        s = (np.abs(np.asarray(np.asarray(ssq, np.float64), LD) - ssq_ext) / ssq_ext).astype(np.float64)
    return traj, s
