"""
The specification of the state-law solve with a stiffness independent of Dc (tests/stiff_reference.py) against the coupled
specification it restates (tests/observe_reference.py) and against long double.  No GPU.
  1. With k = 1e-2 * 10 / Dc the restated recurrence is observe_reference's bit for bit, in both float64 arrangements.
  2. At k = 4e-3 the two float64 arrangements agree with long double on every lane of law_reference.LANES.
  3. At k = 1e-3 the step history's slip-law solve is non-finite on exactly the lanes Dc = 5, 6, 8.
  4. The target test's data set: the coupled model cannot reach the constant-k model's sum of squares.
"""
import numpy as np
import pytest

import law_cases as C
import law_matrix_cases as M
import law_reference as R
import observe_reference as O
import stiff_cases as SC
import stiff_reference as S


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("law", R.LAWS)
def test_coupling_identity(law, history):
    """Every lane at Dc = 64 with per-lane (a, b) and k = 1e-2 * 10 / 64: k Dc is 0.1 exactly, and both arrangements are the
    coupled specification's bit for bit — damped and with k1 = 0."""
    dc, a, b = SC.coupled_lanes()
    assert SC.K64 * SC.DC64 == 1e-2 * 10 and 1.0 / (SC.K64 * SC.DC64) == 1.0 / (1e-2 * 10)
    for m in (C.spec(), C.spec(k1=0.0)):
        vl = R.table(m, history)
        want, got = O.trajectory(m, dc, vl, law, a, b), S.trajectory(m, SC.K64, dc, vl, law, a, b)
        want_lane, got_lane = O.trajectory_lane(m, dc, vl, law, a, b), S.trajectory_lane(m, SC.K64, dc, vl, law, a, b)
        for obs in O.OBSERVABLES:
            assert np.isfinite(want[obs]).all() and np.abs(want[obs] - want[obs][0]).max() > 0, obs
            assert np.array_equal(_bits(got[obs]), _bits(want[obs])), obs
            assert np.array_equal(_bits(got_lane[obs]), _bits(want_lane[obs])), obs
    # ... and another stiffness gives another series
    other = S.trajectory(C.spec(), 2.0 * SC.K64, dc, R.table(C.spec(), history), law, a, b)
    assert not np.array_equal(other["mu"], want["mu"])


@pytest.mark.parametrize("history", M.HISTORIES)
@pytest.mark.parametrize("law", R.LAWS)
@pytest.mark.parametrize("name", SC.ENTRIES)
def test_arrangements_against_long_double(name, law, history):
    """k = 4e-3: all twelve lanes are finite and both float64 arrangements lie within law_cases.CAP of long double, measured as
    law_matrix_cases.error measures (the errors were 1e-14 to 1.5e-12 when this was written)."""
    s = SC.solve(name, history, law)
    assert s["finite"].all()
    for obs in O.OBSERVABLES:
        for arrangement in ("spec", "lane"):
            assert np.isfinite(s[arrangement][obs]).all(), (obs, arrangement)
        print(f"{name} {history} {law} {obs}: specification {s['err_spec'][obs].max():.2e}, device arrangement {s['err_lane'][obs].max():.2e}, "
              f"yardstick {s['yardstick'][obs]:.2e}")
        assert s["own"][obs] < C.CAP, obs
        assert s["yardstick"][obs] >= s["own"][obs]


def test_low_stiffness_is_non_finite_on_the_stiff_lanes():
    """k = 1e-3 on the default model under the step history and the slip law: the fixed-step solve leaves the finite numbers on exactly the lanes
    Dc = 5, 6, 8, in float64 (both arrangements) and in long double alike."""
    s = SC.solve("default", "step", "slip", SC.K_LOW)
    bad = np.isin(s["dc"], SC.LOW_LANES)
    for series in (s["spec"], s["lane"], s["ext"]):
        finite = np.isfinite(np.asarray(series["mu"], dtype=np.float64)).all(axis=0)
        assert np.array_equal(finite, ~bad), finite
    assert np.array_equal(s["finite"], ~bad)


@pytest.mark.parametrize("history, floor", [("step", 3.0), ("hold", 3.0)])
def test_the_coupled_model_cannot_fit_constant_stiffness_data(history, floor):
    """Friction data from Dc = 20 at k = 2e-3 (k Dc = 0.04): over BF_BOX the constant-k model's SSq is smallest near 20; the
    coupled model's best SSq is several times larger and lies elsewhere (5.0 x at 24.75 under the step history, 4.6 x at 43.25
    under the hold when this was written)."""
    p = SC.why_problem(history)
    i, j = int(np.argmin(p["ssq_stiff"])), int(np.argmin(p["ssq_coupled"]))
    ratio = p["ssq_coupled"][j] / p["ssq_stiff"][i]
    print(f"{history}: constant-k argmin Dc {p['x'][i]:.2f}, min SSq {p['ssq_stiff'][i]:.3e}; coupled argmin Dc {p['x'][j]:.2f}, min SSq "
          f"{p['ssq_coupled'][j]:.3e} ({ratio:.1f} x)")
    assert abs(p["x"][i] - R.BF_TRUTH) <= 1.0
    assert abs(p["x"][j] - R.BF_TRUTH) > 4.0
    assert ratio >= floor
