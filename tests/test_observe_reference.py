"""
The specification of the observables (tests/observe_reference.py) against the specification of the state-law solve
(tests/law_reference.py) and against itself: the CPU side of tests/test_gpu_observe.py.  No GPU.
"""
import numpy as np
import pytest

import law_cases as C
import law_matrix_cases as M
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


# ---- the configuration matrix (tests/law_matrix_cases.py): the CPU side of tests/test_gpu_law_matrix.py ----------------------------
@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("name", M.NAMES)
def test_matrix_arrangements_are_finite_and_close(name, law, history):
    """Every matrix entry: both float64 arrangements and the long-double series are finite, and both arrangements' distance from
    long double is rounding error, below law_cases.CAP (the largest when this was written: 2.4e-11, theta of chunks_ab under the
    hold history).  The yardstick the GPU test uses is never below the default model's."""
    s = M.solve(name, history, law)
    floor = dict(OC.precision_set(history, law)["yardstick"], acc=C.precision_set(history, law)["yardstick"])
    for k in O.OBSERVABLES:
        assert np.isfinite(s["spec"][k]).all() and np.isfinite(s["lane"][k]).all() and np.isfinite(s["ext"][k].astype(np.float64)).all(), k
        assert s["spec"][k].shape == s["lane"][k].shape == s["ext"][k].shape == (R.nout(s["m"]), len(R.LANES))
        print(f"{name} {history} {law} {k}: specification {s['err_spec'][k].max():.2e}, device arrangement {s['err_lane'][k].max():.2e}, yardstick "
              f"{s['yardstick'][k]:.2e} (the default model's {floor[k]:.2e}); excursion {float(O.excursion(s['ext'][k]).min()):.2e} .. "
              f"{float(O.excursion(s['ext'][k]).max()):.2e}")
        assert (O.excursion(s["ext"][k]) > 0).all(), k
        assert O.range_error(s["spec"][k], s["ext"][k]).max() < C.CAP and O.range_error(s["lane"][k], s["ext"][k]).max() < C.CAP, k
        assert s["err_spec"][k].max() < C.CAP and s["err_lane"][k].max() < C.CAP, k
        assert s["yardstick"][k] == max(s["own"][k], floor[k]) and s["own"][k] > 0.0, k


def test_matrix_is_the_issues():
    """the entries' attributes, so that an edit of the matrix that makes a row the default model again does not pass unseen"""
    a, b = M.lane_ab()
    assert a.shape == b.shape == (len(R.LANES),) and (0.009 <= a).all() and (a < 0.013).all() and (0.012 <= b).all() and (b < 0.016).all()
    want = {"ab": (500, 1, True), "undamped_ab": (500, 1, True), "k1zero": (500, 1, False), "sub2": (500, 2, False), "chunks_ab": (900, 4, True),
            "nondefault": (400, 1, False), "nondefault_sub3_ab": (400, 3, True), "si": (500, 1, False)}
    assert sorted(want) == sorted(M.NAMES)
    for name, (nsteps, substeps, ab) in want.items():
        m, dc, ca, cb = M.config(name)
        assert (m.num_tsteps, m.substeps, ca is not None, cb is not None) == (nsteps, substeps, ab, ab), name
        assert np.array_equal(dc, np.asarray(R.LANES) * (1e-6 if name == "si" else 1.0)), name
        chunks = R.table_size(m) + R.nout(m) > 56 * 1024 // 8  # the table and the observation against the kernels' 56 KiB of LDS
        assert chunks == (name == "chunks_ab"), name
    assert not M.config("undamped_ab")[0].RadiationDamping and M.config("k1zero")[0].k1 == 0.0 and M.config("k1zero")[0].RadiationDamping
    for name in ("nondefault", "nondefault_sub3_ab"):
        m = M.config(name)[0]
        assert (m.t_start, m.t_final, m.V_ref, m.mu_ref, m.mu_t_zero, m.k1, m.a, m.b) == (1.5, 37.0, 1.7, 0.55, 0.58, 3e-7, 0.012, 0.0155)
    m = M.config("si")[0]
    assert m.V_ref == 1e-6 and m.k1 * m.V_ref == C.spec().k1


@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("law", R.LAWS)
def test_k1_zero_is_no_damping_bit_for_bit(law, history):
    """With the damping on, k1 = 0 makes the damping pass an identity: O.trajectory's series are RadiationDamping = False's, bit
    for bit — the model's (a, b) and per-lane ones."""
    for name, other in (("k1zero", dict(RadiationDamping=False)), ("ab", dict(k1=0.0))):
        s = M.solve(name, history, law)
        m = C.spec(**other)
        if name == "ab":  # ab is damped with k1 = 1e-7: compare its k1 = 0 twin with undamped_ab
            got, want = O.trajectory(m, s["dc"], s["vl"], law, s["a"], s["b"]), M.solve("undamped_ab", history, law)["spec"]
        else:
            got, want = s["spec"], O.trajectory(m, s["dc"], s["vl"], law, s["a"], s["b"])
        for k in O.OBSERVABLES:
            assert np.array_equal(got[k], want[k]), (name, k)
    # ... and the damping is not idle otherwise
    assert not np.array_equal(M.solve("ab", history, law)["spec"]["velocity"], M.solve("undamped_ab", history, law)["spec"]["velocity"])


@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("law", R.LAWS)
def test_other_units_are_the_same_problem(law, history):
    """`si` (V_ref = 1e-6, Dc and 1 / k1 scaled along) is the default problem in other units: theta and mu are the V_ref = 1
    series' to 1e-12 of every sample, velocity and acc 1e-6 times it to 1e-12 of the lane's largest (both cross or approach zero,
    where a sample's own size measures nothing).  Measured when this was written: 2.1e-15 mu, 1.4e-14 theta, 1.9e-13 velocity,
    9.1e-13 acc.  With a power of two for V_ref the scaling is exact in every operation of both arrangements, and the series are
    the same bits: what tests/test_gpu_law_matrix.py asks of the device."""
    one = OC.precision_set(history, law)
    for name, f in (("si", 1.0e-6), ("pow2", M.POW2)):
        s = M.solve(name, history, law)
        assert np.array_equal(s["vl"], one["vl"] * f)
        for arrangement in ("spec", "lane"):
            for k in O.OBSERVABLES:
                got, want = s[arrangement][k], one[arrangement][k] * (f if k in ("acc", "velocity") else 1.0)
                if name == "pow2":
                    assert np.array_equal(got, want), (arrangement, k)
                    continue
                d = np.abs(got - want)
                d = (d / np.abs(want)).max() if k in ("mu", "theta") else (d.max(axis=0) / np.abs(want).max(axis=0)).max()
                print(f"si {history} {law} {arrangement} {k}: {d:.2e}")
                assert d < 1e-12, (arrangement, k)


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
