"""
The specification of the observables (tests/observe_reference.py) against the specification of the state-law solve
(tests/law_reference.py) and against itself: the CPU side of tests/test_gpu_observe.py.  No GPU.
"""
import numpy as np
import pytest

import law_cases as C
import law_reference as R
import observe_cases as OC
import observe_reference as O


@pytest.mark.parametrize("law", R.LAWS)
def test_acc_is_law_references_forward_bit_for_bit(law):
    for m, history in ((C.spec(), "step"), (C.spec(60, 3, RadiationDamping=False), "builtin")):
        vl = R.table(m, history)
        dc, a, b = np.array([6.0, 20.0, 700.0]), np.array([0.010, 0.011, 0.012]), np.array([0.013, 0.014, 0.015])
        data = R.forward(m, [20.0], vl, law)[0][:, 0] + 0.01
        for dtype in (np.float64, R.LD):
            want = R.forward(m, dc, vl, law, a=a, b=b, data=data, dtype=dtype)
            got = O.forward(m, dc, vl, law, "acc", a=a, b=b, data=data, dtype=dtype)
            assert got[0].dtype == want[0].dtype and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert O.forward(m, dc, vl, law)[1] is None


@pytest.mark.parametrize("law", R.LAWS)
def test_velocity_is_the_series_acc_differences(law):
    m = C.spec()
    for arrangement, dt in ((O.forward, None), (O.forward_lane, 1.0 / m.delta_t)):
        v = arrangement(m, R.LANES, R.table(m, "step"), law, "velocity")[0]
        acc = arrangement(m, R.LANES, R.table(m, "step"), law, "acc")[0]
        diff = (v[1:] - v[:-1]) / m.delta_t if dt is None else (v[1:] - v[:-1]) * dt
        assert np.array_equal(diff, acc[1:]) and (acc[0] == 0.0).all() and (v[0] == m.V_ref).all()


def test_initial_samples_and_aliases():
    m = C.spec(50)
    dc = np.array([5.0, 300.0])
    t = O.trajectory(m, dc)
    assert (t["mu"][0] == m.mu_t_zero).all() and np.array_equal(t["theta"][0], dc / m.V_ref)
    tl = O.trajectory_lane(m, dc)
    assert np.allclose(tl["mu"][0], m.mu_t_zero, rtol=4e-16, atol=0.0) and np.allclose(tl["theta"][0], dc / m.V_ref, rtol=4e-16, atol=0.0)
    for alias, name in (("friction", "mu"), ("state", "theta"), ("V", "velocity")):
        assert np.array_equal(O.forward(m, dc, observable=alias)[0], t[name])
    data = t["mu"][:, 0] + 1e-4
    ssq = O.forward(m, dc, observable="mu", data=data)[1]
    assert ssq.shape == (2,) and abs(ssq[0] - R.nout(m) * 1e-8) < 1e-12  # every sample counts, k = 0 included


@pytest.mark.parametrize("history", ["step", "hold"])
@pytest.mark.parametrize("law", R.LAWS)
def test_both_arrangements_are_finite_and_close(history, law):
    """Both float64 arrangements are finite on R.LANES, and their distance from long double, relative to the excursion, is
    rounding error: below law_cases.CAP (the largest figure when this was written: 8.8e-12, theta under the hold history)."""
    s = OC.precision_set(history, law)
    for k in O.OBSERVABLES:
        assert np.isfinite(s["spec"][k]).all() and np.isfinite(s["lane"][k]).all() and np.isfinite(s["ext"][k].astype(np.float64)).all()
        ratio = s["err_lane"][k] / s["err_spec"][k]
        print(f"{history} {law} {k}: specification {s['err_spec'][k].max():.2e}, device arrangement {s['err_lane'][k].max():.2e} "
              f"(x {s['err_lane'][k].max() / s['err_spec'][k].max():.2f}; per lane {ratio.min():.2f} .. {ratio.max():.2f}); excursion "
              f"{float(O.excursion(s['ext'][k]).min()):.2e} .. {float(O.excursion(s['ext'][k]).max()):.2e}")
        assert s["yardstick"][k] < C.CAP
    # the error relative to the series' size would show nothing for the friction: it is the excursion that is small
    assert R.rel_error(s["spec"]["mu"], s["ext"]["mu"]).max() < 1e-14 < s["err_spec"]["mu"].max()


@pytest.mark.parametrize("truth, sign", [("slip", +1), ("aging", -1)])
def test_friction_data_name_the_true_law(truth, sign):
    """law_reference's BF_* problem on friction data, noise 0.05 max|mu - mu_0|: the log Bayes factor has the sign of its truth
    and lies beyond 100 (+664.7 and -672.5 when this was written; acceleration data give +14 .. +36)."""
    p = OC.friction_problem(truth)
    bf = p["log_bayes_factor"]
    other = "aging" if truth == "slip" else "slip"
    print(f"truth {truth}: log Bayes factor {bf:+.1f}; Dc under the true law {p['mean'][truth]:.3f} +- {p['sd'][truth]:.3f}, under the wrong law "
          f"{p['mean'][other]:.3f}; on acceleration data: log Bayes factor {C.bayes_factor_problem(truth)['log_bayes_factor']:+.1f}, SD {OC.acc_sd(truth):.3f}")
    assert np.sign(bf) == sign and abs(bf) > 100.0
    assert p["sd"][truth] < 0.5 * OC.acc_sd(truth)
    assert abs(p["mean"][truth] - R.BF_TRUTH) < 4.0 * p["sd"][truth] < abs(p["mean"][other] - R.BF_TRUTH)
