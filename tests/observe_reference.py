"""
Specification of the observables of the state-law solve (a test helper; TEST INFRASTRUCTURE ONLY) — what
include/rsf_observe.h's rsf_law_observe is checked against.

`forward` follows tests/law_reference.py's recurrence: the reference's own variables (mu, theta, V), literal, its `_rhs`
imported from there, classical RK4 with `substeps` steps per output interval and V_l read from the table.  The loop that the
reference throws three of its four series away in (RateStateModel.py:384-388) keeps them here:

    acc       acc_k = (V_k - V_{k-1}) / delta_t,  acc_0 = 0         (law_reference.forward's series, bit for bit)
    velocity  V_k,      V_0 = V_ref
    mu        mu_k,     mu_0 = mu_t_zero
    theta     theta_k,  theta_0 = Dc / V_ref

and the sum of squares runs over every sample including k = 0.  `dtype` is np.float64 or np.longdouble.

`forward_lane` is a SECOND float64 arrangement of the same recurrence, in the device's variables: ms = mu / k',
x = V_ref theta / Dc, the per-lane constants of rsf::make_lane, the update of rsfk::law_step, mu = k' ms and
theta = x (Dc (1 / V_ref)) — plain NumPy, no FMA.  The device differs from it by FMA contraction and by its own log, exp and
reciprocal only; the distance between the two arrangements says how far two correct float64 programs lie apart, which a
yardstick taken from one of them alone does not.

`range_error` measures a series against the long-double one relative to the series' EXCURSION max_k |ext - ext_0|, not its
size: mu sits at 0.6 and moves by 3.5e-3 to 2.4e-2, so relative to max|mu| every error is 1e-15 and a test on it shows nothing.
"""
import numpy as np

import law_reference as R
from law_reference import LD, _rhs

OBSERVABLES = ("acc", "mu", "theta", "velocity")
ALIASES = {"acc": "acc", "mu": "mu", "friction": "mu", "theta": "theta", "state": "theta", "velocity": "velocity", "V": "velocity"}


def _widen(dtype):
    return lambda x: np.asarray(np.asarray(x, dtype=np.float64), dtype=dtype)


def _inputs(m, dc, vl, a, b, w):
    dc = w(np.atleast_1d(dc))
    a = w(np.full(dc.shape, m.a) if a is None else np.broadcast_to(a, dc.shape))
    b = w(np.full(dc.shape, m.b) if b is None else np.broadcast_to(b, dc.shape))
    vl = w(R.table(m, "builtin") if vl is None else vl)
    if vl.shape != (R.table_size(m),):
        raise ValueError(f"the loading table has {R.table_size(m)} values, not {vl.shape}")
    return dc, a, b, vl


def _ssq(series, data, w):
    if data is None:
        return None
    r = series - w(data)[:, None]
    return (r * r).sum(axis=0)


def trajectory(m, dc, vl=None, law="aging", a=None, b=None, dtype=np.float64):
    """-> {observable: series [nout, C]} in `dtype`, all four from one solve: law_reference.forward's loop, statement for statement"""
    slip = R.LAW_ALIASES[law] == "slip"
    w = _widen(dtype)
    dc, a, b, vl = _inputs(m, dc, vl, a, b, w)
    V_ref, mu_ref, k1 = w(m.V_ref), w(m.mu_ref), w(m.k1)
    damping, S, n = bool(m.RadiationDamping), int(m.substeps), R.nout(m)
    h = w(float(m.delta_t) / S)
    hh, h6, dt = h / 2, h / 6, w(m.delta_t)
    mu = np.full(dc.shape, w(m.mu_t_zero))
    th = dc / V_ref
    V = np.full(dc.shape, V_ref)
    out = {k: np.zeros((n, dc.size), dtype=dtype) for k in OBSERVABLES}
    out["mu"][0], out["theta"][0], out["velocity"][0] = mu, th, V

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
            out["acc"][k] = (V - vprev) / dt
            out["mu"][k], out["theta"][k], out["velocity"][k] = mu, th, V
    return out


def forward(m, dc, vl=None, law="aging", observable="acc", a=None, b=None, data=None, dtype=np.float64):
    """-> (series [nout, C], ssq [C] or None) of `observable` in `dtype`.  vl: the float64 table of V_l at R.stage_times(m)
    (None: the built-in history's); data: a series of the same observable; inputs are widened exactly from float64."""
    series = trajectory(m, dc, vl, law, a, b, dtype)[ALIASES[observable]]
    with np.errstate(all="ignore"):
        return series, _ssq(series, data, _widen(dtype))


def trajectory_lane(m, dc, vl=None, law="aging", a=None, b=None):
    """-> {observable: series [nout, C]}, float64, in the device's variables and constants (rsf::make_lane, rsfk::law_rhs,
    rsfk::law_step, rsf::initial_state), every fused multiply-add written as a product and a sum"""
    slip = R.LAW_ALIASES[law] == "slip"
    dc, a, b, vl = _inputs(m, dc, vl, a, b, _widen(np.float64))
    V_ref, mu_ref, k1 = float(m.V_ref), float(m.mu_ref), float(m.k1)
    damp = bool(m.RadiationDamping) and k1 != 0.0  # with k1 = 0 the host launches the kernels without the damping pass
    S, n = int(m.substeps), R.nout(m)
    h = float(m.delta_t) / S
    hh, h6, inv_dt, inv_vref = 0.5 * h, h / 6.0, 1.0 / float(m.delta_t), 1.0 / V_ref
    tenth = 1e-2 * 10
    # rsf::make_lane
    inv_a, inv_dc = 1.0 / a, 1.0 / dc
    kprime = tenth * inv_dc
    kia = kprime * inv_a
    via = V_ref * inv_a
    vdc = V_ref * inv_dc
    vk = via * kprime
    beta = (b * V_ref) * (1.0 / tenth)
    kvk = k1 * via
    vkw = vk * (1.0 / kvk) if damp else vk
    h6v = h6 * vkw
    boa = b * inv_a
    tc = -mu_ref * inv_a
    h6d = h6 * vdc
    # rsf::initial_state
    ms = (float(m.mu_t_zero) * dc) * (1.0 / tenth)
    x = V_ref * ((dc * inv_vref) * inv_dc)
    V = np.full(dc.shape, V_ref)
    tscale = dc * inv_vref
    out = {k: np.zeros((n, dc.size)) for k in OBSERVABLES}
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
        for k in range(1, n):
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
            out["acc"][k] = (V - vprev) * inv_dt
            out["mu"][k], out["theta"][k], out["velocity"][k] = kprime * ms, x * tscale, V
    return out


def forward_lane(m, dc, vl=None, law="aging", observable="acc", a=None, b=None, data=None):
    """forward's results from the second float64 arrangement (trajectory_lane)"""
    series = trajectory_lane(m, dc, vl, law, a, b)[ALIASES[observable]]
    with np.errstate(all="ignore"):
        return series, _ssq(series, data, _widen(np.float64))


def excursion(ext):
    """per lane: max_k |ext - ext_0|"""
    ext = np.asarray(ext, dtype=LD)
    return np.abs(ext - ext[0]).max(axis=0)


def range_error(s, ext):
    """per lane: max_k |s - ext| / max_k |ext - ext_0|, in float64"""
    ext = np.asarray(ext, dtype=LD)
    return (np.abs(np.asarray(s, dtype=LD) - ext).max(axis=0) / excursion(ext)).astype(np.float64)


# ---- the Bayes-factor problem on friction data: law_reference's BF_* constants, noise 5 % of the friction's excursion --------
def bf_data(m, vl, truth_law, observable="mu"):
    """clean series of `truth_law` at Dc = BF_TRUTH plus 0.05 max|clean - clean_0| N(0, 1), default_rng(BF_SEED)"""
    clean = forward(m, [R.BF_TRUTH], vl, truth_law, observable)[0][:, 0]
    return clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(R.BF_SEED).standard_normal(clean.size)


def bf_posteriors(m, vl, data, observable="mu"):
    """{law: (log evidence, posterior mean of Dc, posterior SD of Dc)} of the float64 specification on BF_NODES uniform
    trapezoid nodes over BF_BOX, and {law: SSq at the nodes}"""
    x = np.linspace(R.BF_BOX[0], R.BF_BOX[1], R.BF_NODES)
    w = R.trapezoid_weights(x)
    shape, out, ssq = 0.5 * R.nout(m), {}, {}
    for law in R.LAWS:
        ssq[law] = forward(m, x, vl, law, observable, data=data)[1]
        ok = np.isfinite(ssq[law]) & (ssq[law] > 0)
        l = np.where(ok, -LD(shape) * np.log(np.where(ok, ssq[law], 1.0).astype(LD)), -np.inf)
        p = w * np.exp(l - l.max())
        p = p / p.sum()
        mean = float((p * x).sum())
        out[law] = (R.log_evidence_1d(x, w, ssq[law], shape, *R.BF_BOX)[0], mean, float(np.sqrt((p * (x - mean) ** 2).sum())))
    return out, ssq
