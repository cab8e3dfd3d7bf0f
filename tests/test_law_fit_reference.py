"""
CPU tests of the specification of the Levenberg-Marquardt fit under a state law (tests/law_fit_reference.py; include/rsf_law_fit.h):
  1. the helper in float64 against the helper in long double, on observe_cases.friction_problem("aging")'s data;
  2. sample 0 carries a sensitivity: X_p0 != 0 for p = Dc for the state and the friction, so it is summed like every other sample;
  3. the specification's own fits of the end-to-end problems of tests/test_gpu_law_fit.py: every start CONVERGED at the same
     minimum, the best Dc within one posterior SD of the quadrature's mean (d = 1); every start CONVERGED on the same ssq and the
     same product Dc a (d = 3).  The GPU tests compare against these fits, so the starts are known to be good here.
No GPU.
"""
import numpy as np
import pytest

import fit_reference as F
import law_cases as C
import law_fit_reference as LF
import law_reference as R
import observe_cases as OC
import observe_reference as O

LD = np.longdouble
EPS = 2.0 ** -53


@pytest.mark.parametrize("d", [1, 3])
def test_float64_helper_against_long_double(d):
    """The two precisions differ by the float64 solve's own error e = max |s64 - sLD| of the 1 + d trajectories of a point, and the
    bound on each sum follows from it term by term (the sums themselves are long double in both):
        |r64 - rLD| <= e_0 + u|r|,  |X64 - XLD| <= (e_p + e_0) / (q^(p)_p fd) + 3u|X|     (u = 2^-53: the difference, the product and
                                                                                            the quotient of F.normal, each rounded once)
        |dssq| <= sum 2|r| dr + dr^2,   |dgrad_p| <= sum |X_p| dr + |r| dX_p + dX_p dr,   |djtj_pr| <= sum |X_p| dX_r + |X_r| dX_p + dX_p dX_r
    plus u of the result for the final rounding to float64."""
    p = OC.friction_problem("aging")
    m, vl, data, fd = p["m"], p["vl"], p["data"], LF.FD[d]
    q = np.array([[12.0, 0.0105, 0.0145], [20.0, 0.011, 0.014], [33.0, 0.0118, 0.0131], [90.0, 0.0095, 0.0155]])[:, :d]
    n = len(q)
    got = LF.normal(m, vl, "aging", "mu", q, data, fd)
    want = LF.normal(m, vl, "aging", "mu", q, data, fd, dtype=LD, out=LD)
    pq = F.perturbed(q, fd)
    s64 = LF.solve(m, vl, "aging", "mu")(pq.reshape(-1, d)).reshape(-1, d + 1, n)
    sLD = LF.solve(m, vl, "aging", "mu", LD)(pq.reshape(-1, d)).reshape(-1, d + 1, n)
    e = np.abs(s64.astype(LD) - sLD)                                   # (nout, d + 1, n)
    r = np.abs(sLD[:, 0] - data[:, None].astype(LD))
    den = np.stack([np.abs(pq[k + 1, :, k]).astype(LD) * LD(fd) for k in range(d)])
    X = np.stack([np.abs(sLD[:, k + 1] - sLD[:, 0]) / den[k] for k in range(d)])  # (d, nout, n)
    dr = e[:, 0] + EPS * r
    dX = np.stack([(e[:, k + 1] + e[:, 0]) / den[k] + 3 * EPS * X[k] for k in range(d)])
    b_ssq = (2 * r * dr + dr * dr).sum(axis=0)
    b_g = np.stack([(X[k] * dr + r * dX[k] + dX[k] * dr).sum(axis=0) for k in range(d)], axis=1)
    b_H = np.stack([np.stack([(X[k] * dX[j] + X[j] * dX[k] + dX[k] * dX[j]).sum(axis=0) for j in range(d)], axis=1) for k in range(d)], axis=1)
    worst = {}
    for name, g, w, b in zip(("ssq", "grad", "jtj"), got, want, (b_ssq, b_g, b_H)):
        err = np.abs(g.astype(LD) - w)
        bound = b + EPS * np.abs(w)
        worst[name] = float((err / bound).max())
        assert np.isfinite(g).all() and (err <= bound).all(), (name, err, bound)
    print(f"d {d}: largest solve error {float(e.max()):.2e}; |float64 - long double| over its bound: {worst}")
    # ... and the bound is no blank cheque: relative to the sums themselves it is small
    assert float((b_ssq / want[0]).max()) < 1e-9


@pytest.mark.parametrize("law", R.LAWS)
def test_sample_zero_carries_a_sensitivity(law):
    """theta_0 = Dc / V_ref: X_00 = 1 / (V_ref (1 + fd)) in every arrangement (a difference of Dc fd known to 1e-16 Dc: rtol 1e-9
    at fd 1e-6).  mu_0: mu_t_zero exactly in the specification's variables, but
    the device forms it as k' ms_0 from the lane's own rounded k' = 0.1 (1 / Dc) and ms_0 = (mu_t_zero Dc) 10
    (observe_reference.trajectory_lane), which differs between Dc and Dc (1 + fd) by roundings: X_00 is then a rounding over
    Dc fd, not 0 — and not negligible beside an ulp of the sums, so the fit kernels exchange sample 0 like every other sample
    instead of skipping it as fit_kernel may for the acceleration, whose sample 0 is 0 in every trajectory."""
    m = C.spec()
    vl, fd = R.table(m, "step"), LF.FD[1]
    dc = np.array(R.LANES)
    pq = F.perturbed(dc[:, None], fd)
    both = np.concatenate([pq[0, :, 0], pq[1, :, 0]])
    X0 = {}
    for name, traj in (("spec", O.trajectory(m, both, vl, law)), ("lane", O.trajectory_lane(m, both, vl, law))):
        for obs in O.OBSERVABLES:
            s0 = traj[obs][0]
            X0[name, obs] = (s0[dc.size:] - s0[:dc.size]) / (pq[1, :, 0] * fd)
    for name in ("spec", "lane"):
        assert (X0[name, "acc"] == 0).all() and (X0[name, "velocity"] == 0).all()
        np.testing.assert_allclose(X0[name, "theta"], 1.0 / (m.V_ref * (1 + fd)), rtol=1e-9)  # the perturbed value in the denominator
    assert (X0["spec", "mu"] == 0).all()
    assert (X0["lane", "mu"] != 0).any()
    # the normal equations hold it: jtj minus the sum over k >= 1 is X_00^2
    data = O.forward(m, [20.0], vl, law, "theta")[0][:, 0]
    q = np.array([[15.0]])
    ssq, g, H = LF.normal(m, vl, law, "theta", q, data, fd, out=LD)
    s = LF.solve(m, vl, law, "theta")(F.perturbed(q, fd).reshape(-1, 1))
    X = ((s[:, 1] - s[:, 0]) / (q[0, 0] * (1 + fd) * fd)).astype(LD)
    assert X[0] != 0 and abs(H[0, 0, 0] - (X[1:] * X[1:]).sum() - X[0] * X[0]) <= 4 * EPS * H[0, 0, 0]


@pytest.mark.parametrize("truth", R.LAWS)
def test_the_specification_fits_the_end_to_end_problems(truth):
    p = OC.friction_problem(truth)
    st = LF.fit_d1(truth)
    best = int(np.argmin(st["ssq"]))
    print(f"truth {truth}, d 1: status {st['status'].tolist()} iters {st['iters'].tolist()} Dc {st['q'][:, 0].tolist()} ssq / best - 1 "
          f"{(st['ssq'] / st['ssq'][best] - 1).tolist()}; quadrature mean {p['mean'][truth]!r} sd {p['sd'][truth]!r}")
    assert (st["status"] == F.CONVERGED).all() and (st["iters"] <= 60).all()
    assert (st["ssq"] <= (1 + 1e-9) * st["ssq"][best]).all()
    assert (np.abs(st["q"][:, 0] / st["q"][best, 0] - 1) <= 1e-7).all()
    assert abs(st["q"][best, 0] - p["mean"][truth]) <= p["sd"][truth]
    s3 = LF.fit_d3(truth)
    b3 = int(np.argmin(s3["ssq"]))
    prod = s3["q"][:, 0] * s3["q"][:, 1]
    print(f"truth {truth}, d 3: status {s3['status'].tolist()} iters {s3['iters'].tolist()} q {s3['q'].tolist()} ssq {s3['ssq'].tolist()} Dc a {prod.tolist()}")
    # LF.STARTS3 as first chosen: the specification converges from all four, under both truths
    assert (s3["status"] == F.CONVERGED).all() and (s3["iters"] <= 60).all()
    assert s3["ssq"][b3] < st["ssq"][best]  # three parameters fit better than one
    assert (np.abs(s3["ssq"] / s3["ssq"][b3] - 1) <= 1e-3).all() and (np.abs(prod / prod[b3] - 1) <= 1e-3).all()
