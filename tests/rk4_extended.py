"""
Extended-precision reference of the fixed-step RK4 forward model (a test helper; TEST INFRASTRUCTURE ONLY).

`forward_ext` is RateStateModel.evaluate's fixed-step RK4 (BASELINE: classical RK4, `substeps` steps per output interval,
acc_k = (V_k - V_{k-1}) / delta_t, acc_0 = 0) computed in np.longdouble — the x87 80-bit format, 64-bit mantissa, eps 1.1e-19 —
vectorised over lanes.  Its own rounding is ~1e-17 relative over a 4000-step solve, so the distance of a float64 solve
from it is that solve's OWN rounding error: the yardstick for the incremental tiers' claim to be exact to rounding inside
their guards (csrc/rsf_device.h), which a float64 restatement (oracle/rsf_oracle.c, same rounding size) cannot judge.

It is written from the model's specification, not from any of the float64 code paths: the literal RHS with the damping
pass (RateStateModel.py:318-355), stage times t_start + j h/2 with h = delta_t / S formed in float64 and then widened,
the sum of squares sum_k (acc_k - data_k)^2 over every sample including k = 0.  Inputs are widened exactly from float64.
Not modelled: how the product rounds its float64 h or its V_l(t) table (1e-16 effects).

`place_lanes` puts whole waves of 64 lanes into one tier of the float64 kernels, by the kernel's own a-priori bound of
the mu increment (rsf_device.h wave_begin): dk = 1.2 V_ref h k'/a with k' = 0.1/Dc, against 2^-9 / 2^-7 / 2^-3.
"""
import numpy as np

LD = np.longdouble
if np.finfo(LD).nmant < 63:  # a float64 "longdouble" (e.g. aarch64 Linux has binary128, MSVC has binary64) is no reference
    raise RuntimeError(f"np.longdouble has a {np.finfo(LD).nmant}-bit mantissa: the extended-precision reference needs >= 63")

WAVE = 64
# the a-priori tier bounds of wave_begin (rsf_device.h): TIGHT below 2^-9, NARROW below 2^-7, FULL from 2^-3
DK_TIGHT, DK_NARROW, DK_FULL = 2.0 ** -9, 2.0 ** -7, 2.0 ** -3


def _w(x):
    """float64 -> longdouble, exactly"""
    return np.asarray(np.asarray(x, dtype=np.float64), dtype=LD)


def _rhs(t, mu, th, dc, a, b, V_ref, mu_ref, k1, damping):
    """RateStateModel.py:318-355, literal: (d mu/dt, d theta/dt, dV/dt)."""
    kprime = LD(1e-2) * 10 / dc
    V_l = V_ref * (1 + np.exp(-t / 20) * np.sin(10 * t))
    v = V_ref * np.exp((mu - mu_ref - b * np.log(V_ref * th / dc)) / a)
    d1 = 1 - v * th / dc
    d0 = kprime * V_l - kprime * v
    d2 = v / a * (d0 - b / th * d1)
    if damping:
        d0 = d0 - k1 * d2
        d2 = v / a * (d0 - b / th * d1)
    return d0, d1, d2


def forward_ext(m, dc, a=None, b=None, data=None):
    """-> (acc [nout, C] longdouble, ssq [C] longdouble or None).  `m` is any object with RateStateModel's attributes
    (a, b, mu_ref, V_ref, k1, mu_t_zero, t_start, delta_t, RadiationDamping, substeps, nout or t_final)."""
    dc = _w(np.atleast_1d(dc))
    a = _w(np.full(dc.shape, m.a) if a is None else np.broadcast_to(a, dc.shape))
    b = _w(np.full(dc.shape, m.b) if b is None else np.broadcast_to(b, dc.shape))
    V_ref, mu_ref, k1 = _w(m.V_ref), _w(m.mu_ref), _w(m.k1)
    damping, S = bool(m.RadiationDamping), int(m.substeps)
    n = int(np.floor((m.t_final - m.t_start) / m.delta_t))  # RateStateModel.py:358
    h = _w(float(m.delta_t) / S)  # the float64 step, widened
    hh, h6 = h / 2, h / 6
    t0, dt = _w(m.t_start), _w(m.delta_t)
    mu = np.full(dc.shape, _w(m.mu_t_zero))
    th = dc / V_ref
    V = np.full(dc.shape, V_ref)
    acc = np.zeros((n, dc.size), dtype=LD)

    def f(t, mu_, th_):
        return _rhs(t, mu_, th_, dc, a, b, V_ref, mu_ref, k1, damping)

    j = 0
    with np.errstate(all="ignore"):
        for k in range(1, n):
            vprev = V
            for _ in range(S):
                ta, tm, te = t0 + j * hh, t0 + (j + 1) * hh, t0 + (j + 2) * hh
                a0, a1, a2 = f(ta, mu, th)
                b0, b1, b2 = f(tm, mu + hh * a0, th + hh * a1)
                c0, c1, c2 = f(tm, mu + hh * b0, th + hh * b1)
                e0, e1, e2 = f(te, mu + h * c0, th + h * c1)
                mu = mu + h6 * (a0 + 2 * b0 + 2 * c0 + e0)
                th = th + h6 * (a1 + 2 * b1 + 2 * c1 + e1)
                V = V + h6 * (a2 + 2 * b2 + 2 * c2 + e2)
                j += 2
            acc[k] = (V - vprev) / dt
    ssq = None
    if data is not None:
        r = acc - _w(data)[:, None]
        ssq = (r * r).sum(axis=0)
    return acc, ssq


def tier_edges(m, a):
    """Dc at which the a-priori bound dk = 1.2 V_ref h (0.1/Dc)/a reaches 2^-9, 2^-7 and 2^-3 (TIGHT above the first)."""
    h = float(m.delta_t) / int(m.substeps)
    c = 1.2 * m.V_ref * h * 0.1 / a
    return c / DK_TIGHT, c / DK_NARROW, c / DK_FULL


SETS = ("tight", "tight_edge", "narrow", "wide", "full")


def place_lanes(m, which, waves=1, a=None, seed=0):
    """Dc of `waves` whole, sorted waves of 64 lanes whose a-priori tier (rsf_device.h wave_begin) is `which`:
      tight       well inside TIGHT's bound (1.4 .. 6 x its edge)
      tight_edge  TIGHT within 12 % of its edge (1.005 .. 1.12 x)
      narrow      dk in [2^-9, 2^-7), wave_begin's NARROW
      wide        dk in [2^-7, 2^-3)
      full        dk >= 2^-3 (stiff: FULL for the whole solve), 0.45 .. 0.95 of the FULL edge — where fixed-step RK4 still
                  gives a finite solve at the shapes tested here (the caller asserts that it does)
    a: the lanes' a (default m.a).  Each wave is sorted, so a wave's tier is decided by its own lanes."""
    a = m.a if a is None else a
    e_t, e_n, e_f = tier_edges(m, a)
    lo, hi = {"tight": (1.4 * e_t, 6.0 * e_t), "tight_edge": (1.005 * e_t, 1.12 * e_t), "narrow": (1.02 * e_n, 0.98 * e_t),
              "wide": (1.02 * e_f, 0.98 * e_n), "full": (0.45 * e_f, 0.95 * e_f)}[which]
    rng = np.random.default_rng(seed)
    # log-uniform over the range: the wide tiers span a factor 4 (NARROW) and 16 (WIDE) in Dc
    dc = np.exp(rng.uniform(np.log(lo), np.log(hi), (waves, WAVE)))
    return np.sort(dc, axis=1).reshape(-1)


def lane_b(a, n_lanes, seed=0):
    """per-lane b for the (a, b) variant: b - a in [-0.003, 0.006]"""
    return a + np.random.default_rng(seed + 1).uniform(-0.003, 0.006, n_lanes)


def rel_errors(acc, ssq, acc_ext, ssq_ext):
    """per-lane trajectory error max_k |acc - acc_ext| / max_k |acc_ext| and the sum of squares' relative error (float64)"""
    acc_ext = np.asarray(acc_ext, dtype=LD)
    traj = (np.abs(_w(acc) - acc_ext).max(axis=0) / np.abs(acc_ext).max(axis=0)).astype(np.float64)
    s = None
    if ssq is not None:
        s = (np.abs(_w(ssq) - ssq_ext) / ssq_ext).astype(np.float64)
    return traj, s


# The models every extended-precision test runs: (name, substeps, attribute overrides, sets).  The mu_t_zero-offset models
# start the TIGHT lanes off their steady state (|1 - v theta/Dc| ~ 4 %): their guards trip from the first trip — a cold redo,
# then the handover to a wider tier, later demotion back (rsf_device.h struct Wave).
TIGHT_SETS = ("tight", "tight_edge")
CASES = {
    "n500_S1": (500, 1, {}, SETS),
    "n500_S1_nodamp": (500, 1, {"RadiationDamping": False}, SETS),
    "n500_S3": (500, 3, {}, SETS),
    "n500_S3_nodamp": (500, 3, {"RadiationDamping": False}, SETS),
    "n2000_S1": (2000, 1, {}, SETS),
    "n2000_S1_nodamp": (2000, 1, {"RadiationDamping": False}, SETS),
    "n4000_S1": (4000, 1, {}, SETS),
    "n500_S1_k1zero": (500, 1, {"k1": 0.0}, SETS),
    # test_forward_with_non_default_model_constants: every attribute away from its default
    "nondefault": (400, 2, {"t_start": 1.5, "t_final": 37.0, "V_ref": 1.7, "mu_ref": 0.55, "mu_t_zero": 0.58, "k1": 3.0e-7,
                            "a": 0.012, "b": 0.0155}, SETS),
    # slip rates in SI units, k1 carrying 1/velocity (test_forward_is_scale_free_in_v_ref)
    "vref_si": (500, 1, {"V_ref": 1.0e-6, "k1": 1.0e-7 / 1.0e-6}, SETS),
    "n500_S1_mu+5e-4": (500, 1, {"mu_t_zero": 0.6 + 5e-4}, TIGHT_SETS),
    "n2000_S2_mu-4e-4": (2000, 2, {"mu_t_zero": 0.6 - 4e-4}, TIGHT_SETS),
    "n4000_S1_mu+5e-4": (4000, 1, {"mu_t_zero": 0.6 + 5e-4}, TIGHT_SETS),
}


def make_model(ModelSpec, name):
    """the model of CASES[name], built on any class with RateStateModel's attributes (ModelSpec(n, t0, t1, substeps))"""
    n, S, attrs, _ = CASES[name]
    t0, t1 = attrs.get("t_start", 0.0), attrs.get("t_final", 50.0)
    m = ModelSpec(n, t0, t1, S)
    for k, v in attrs.items():
        setattr(m, k, v)
    m.delta_t = (t1 - t0) / n
    return m


class Problem:
    """One model's lanes and their extended-precision solve.  Lanes: for each set of CASES[name] one wave of 64, first with
    the model's (a, b) ("plain", the kernels' no-(a, b) path), then the same Dc with per-lane b ("ab": b - a in
    [-0.003, 0.006], a = m.a so that the a-priori tier placement holds).  The observation: the extended solve at the first
    TIGHT lane plus |acc| N(0, 1) (the bench's recipe), rounded to float64."""

    def __init__(self, ModelSpec, name, seed=0):
        self.name, self.sets = name, CASES[name][3]
        self.m = make_model(ModelSpec, name)
        self.dc = np.concatenate([place_lanes(self.m, s, seed=seed + 11 * i) for i, s in enumerate(self.sets)])
        L = self.dc.size
        self.a = np.full(L, float(self.m.a))
        self.b = lane_b(float(self.m.a), L, seed)
        acc, _ = forward_ext(self.m, self.dc[:1])
        acc = acc[:, 0].astype(np.float64)
        self.data = acc + np.abs(acc) * np.random.default_rng(seed + 2).standard_normal(acc.size)
        acc, ssq = forward_ext(self.m, np.concatenate([self.dc, self.dc]), np.concatenate([self.a, self.a]),
                               np.concatenate([np.full(L, float(self.m.b)), self.b]), data=self.data)
        self.ext = {"plain": (acc[:, :L], ssq[:L]), "ab": (acc[:, L:], ssq[L:])}
        fin = np.isfinite(ssq.astype(np.float64)) & np.isfinite(acc.astype(np.float64)).all(axis=0)
        assert fin.all(), f"{name}: extended solve not finite on lanes {np.flatnonzero(~fin)}"

    def kw(self, variant):
        return {} if variant == "plain" else {"a": self.a, "b": self.b}

    def lanes(self, s):
        i = self.sets.index(s)
        return slice(WAVE * i, WAVE * (i + 1))
