"""
Specification of the forward model under a caller-supplied loading history and either state law (a test helper; TEST
INFRASTRUCTURE ONLY) — what include/rsf_law.h's rsf_set_loading and rsf_law_forward are checked against.

Written in the manner of tests/rk4_extended.py and from the model's specification, not from any device code path: the
literal RHS with the damping pass (RateStateModel.py:318-355) in the reference's own variables (mu, theta, V), with the
d(theta)/dt line switched by law,

    ageing   d(theta)/dt = 1 - v theta / Dc
    slip     d(theta)/dt = -(v theta / Dc) log(v theta / Dc)

classical RK4 with `substeps` steps per output interval, V_l read from a TABLE at the stage times t_start + j h / 2
(h = delta_t / substeps, j = 0 .. 2 substeps (nout - 1)), acc_k = (V_k - V_{k-1}) / delta_t with acc_0 = 0, and the sum of
squares over every sample including k = 0.  `dtype` is np.float64 or np.longdouble (x87 80-bit, 64-bit mantissa); the
computation is vectorised over lanes.  The distance of the float64 form from the long-double form is a plain float64 RK4's
own rounding error: the yardstick of tests/test_gpu_law.py.

Also here: the built-in, the velocity-step and the slide-hold-slide histories, and the 1-D quadrature of SSq^-shape over a box
for the log evidence, with the constants of Engine.evidence_finish.
"""
import math

import numpy as np

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise RuntimeError(f"np.longdouble has a {np.finfo(LD).nmant}-bit mantissa: the extended-precision reference needs >= 63")

LAWS = ("aging", "slip")
LAW_ALIASES = {"aging": "aging", "ageing": "aging", "slip": "slip"}
# the lanes of the precision tests: Dc from the stiff end of the stable range to the reference's largest
LANES = (5.0, 6.0, 8.0, 10.0, 15.0, 20.0, 35.0, 50.0, 100.0, 200.0, 1000.0, 5000.0)


class Spec:
    """RateStateModel's attributes with the reference's defaults (RateStateModel.py:5-11, 167-180)"""

    def __init__(self, nsteps=500, t_start=0.0, t_final=50.0, substeps=1):
        self.a, self.b, self.mu_ref, self.V_ref, self.k1 = 0.011, 0.014, 0.6, 1.0, 1.0e-7
        self.t_start, self.t_final, self.num_tsteps = t_start, t_final, nsteps
        self.delta_t = (t_final - t_start) / nsteps
        self.mu_t_zero = 0.6
        self.RadiationDamping = True
        self.substeps = substeps


def nout(m):
    return int(np.floor((m.t_final - m.t_start) / m.delta_t))  # RateStateModel.py:358


def table_size(m):
    return 2 * int(m.substeps) * (nout(m) - 1) + 1


def stage_times(m):
    """t_start + j (h / 2), j = 0 .. 2 S (nout - 1), in float64 as rsf_set_model forms them"""
    hh = 0.5 * (float(m.delta_t) / int(m.substeps))
    return float(m.t_start) + np.arange(table_size(m), dtype=np.float64) * hh


def builtin_history(t, V_ref=1.0):
    """RateStateModel.py:327-329"""
    return V_ref * (1 + np.exp(-t / 20) * np.sin(10 * t))


def step_history(t, V_ref=1.0):
    """a velocity step: V_ref, then 10 V_ref on [10, 30), then V_ref"""
    t = np.asarray(t, dtype=np.float64)
    return V_ref * np.where((t >= 10.0) & (t < 30.0), 10.0, 1.0)


def hold_history(t, V_ref=1.0):
    """slide-hold-slide: V_ref, a hold (V_l = 0) on [10, 30), then V_ref"""
    t = np.asarray(t, dtype=np.float64)
    return V_ref * np.where((t >= 10.0) & (t < 30.0), 0.0, 1.0)


HISTORIES = {"builtin": builtin_history, "step": step_history, "hold": hold_history}


def table(m, history):
    """the float64 table of `history` (a name of HISTORIES or a callable t -> V_l) at the model's stage times"""
    fn = HISTORIES[history] if isinstance(history, str) else history
    return np.ascontiguousarray(fn(stage_times(m), m.V_ref) if isinstance(history, str) else fn(stage_times(m)), dtype=np.float64)


def _rhs(V_l, mu, th, dc, a, b, V_ref, mu_ref, k1, damping, slip):
    """RateStateModel.py:318-355, literal, the d(theta)/dt line by law: (d mu/dt, d theta/dt, dV/dt)."""
    kprime = dc.dtype.type(1e-2) * 10 / dc
    v = V_ref * np.exp((mu - mu_ref - b * np.log(V_ref * th / dc)) / a)
    om = v * th / dc
    d1 = -om * np.log(om) if slip else 1 - om
    d0 = kprime * V_l - kprime * v
    d2 = v / a * (d0 - b / th * d1)
    if damping:
        d0 = d0 - k1 * d2
        d2 = v / a * (d0 - b / th * d1)
    return d0, d1, d2


def forward(m, dc, vl=None, law="aging", a=None, b=None, data=None, dtype=np.float64):
    """-> (acc [nout, C], ssq [C] or None) in `dtype`.  vl: the float64 table of V_l at stage_times(m) (None: the built-in
    history's); inputs are widened exactly from float64."""
    slip = LAW_ALIASES[law] == "slip"
    w = lambda x: np.asarray(np.asarray(x, dtype=np.float64), dtype=dtype)
    dc = w(np.atleast_1d(dc))
    a = w(np.full(dc.shape, m.a) if a is None else np.broadcast_to(a, dc.shape))
    b = w(np.full(dc.shape, m.b) if b is None else np.broadcast_to(b, dc.shape))
    V_ref, mu_ref, k1 = w(m.V_ref), w(m.mu_ref), w(m.k1)
    damping, S, n = bool(m.RadiationDamping), int(m.substeps), nout(m)
    vl = w(table(m, "builtin") if vl is None else vl)
    if vl.shape != (table_size(m),):
        raise ValueError(f"the loading table has {table_size(m)} values, not {vl.shape}")
    h = w(float(m.delta_t) / S)
    hh, h6, dt = h / 2, h / 6, w(m.delta_t)
    mu = np.full(dc.shape, w(m.mu_t_zero))
    th = dc / V_ref
    V = np.full(dc.shape, V_ref)
    acc = np.zeros((n, dc.size), dtype=dtype)

    def f(V_l, mu_, th_):
        return _rhs(V_l, mu_, th_, dc, a, b, V_ref, mu_ref, k1, damping, slip)

    j = 0
    with np.errstate(all="ignore"):
        for k in range(1, n):
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
            acc[k] = (V - vprev) / dt
        ssq = None
        if data is not None:
            r = acc - w(data)[:, None]
            ssq = (r * r).sum(axis=0)
    return acc, ssq


def rel_error(acc, acc_ext):
    """per lane: max_k |acc - acc_ext| / max_k |acc_ext|, in float64"""
    acc_ext = np.asarray(acc_ext, dtype=LD)
    return (np.abs(np.asarray(acc, dtype=LD) - acc_ext).max(axis=0) / np.abs(acc_ext).max(axis=0)).astype(np.float64)


def trapezoid_weights(x):
    x = np.asarray(x, dtype=np.float64)
    w = np.zeros_like(x)
    w[:-1] += 0.5 * np.diff(x)
    w[1:] += 0.5 * np.diff(x)
    return w


def log_evidence_1d(x, w, ssq, shape, lo, hi):
    """log of sum_i w_i SSq_i^-shape, long double and shifted by the largest term, with the constants of
    Engine.evidence_finish: - log(hi - lo) + lgamma(shape) - shape log pi.  Nodes whose SSq is not finite and > 0 carry no
    density.  -> (log_evidence, log_integral) as floats."""
    ssq, w = np.asarray(ssq, dtype=LD), np.asarray(w, dtype=LD)
    ok = np.isfinite(ssq) & (ssq > 0)
    l = np.where(ok, -LD(shape) * np.log(np.where(ok, ssq, LD(1))), -np.inf)
    lmax = l.max()
    logi = lmax + np.log((w * np.exp(l - lmax)).sum())
    return float(logi - np.log(LD(hi) - LD(lo)) + LD(math.lgamma(shape)) - LD(shape) * np.log(np.arccos(LD(-1)))), float(logi)


# ---- the Bayes-factor problem of the tests: step history, nsteps 500, substeps 1, truth Dc = 20, box [5, 200] -------------
BF_TRUTH, BF_BOX, BF_NODES, BF_SEED = 20.0, (5.0, 200.0), 4001, 20261019


def bf_data(m, vl, truth_law):
    """clean series of `truth_law` at Dc = BF_TRUTH plus 0.05 max|clean| N(0, 1), default_rng(BF_SEED)"""
    clean = forward(m, [BF_TRUTH], vl, truth_law)[0][:, 0]
    return clean + 0.05 * np.abs(clean).max() * np.random.default_rng(BF_SEED).standard_normal(clean.size)


def bf_log_evidences(m, vl, data, x=None, w=None):
    """{law: log evidence} of the float64 specification on the nodes x with weights w (default: BF_NODES uniform nodes over
    BF_BOX, trapezoid), and {law: SSq at the nodes}"""
    if x is None:
        x = np.linspace(BF_BOX[0], BF_BOX[1], BF_NODES)
        w = trapezoid_weights(x)
    ssq = {law: forward(m, x, vl, law, data=data)[1] for law in LAWS}
    return {law: log_evidence_1d(x, w, ssq[law], 0.5 * nout(m), *BF_BOX)[0] for law in LAWS}, ssq
