"""
The specification of the loading history and the state law (tests/law_reference.py) against itself and against the
extended-precision RK4 of tests/rk4_extended.py.  No GPU, no library.
"""
import numpy as np
import pytest

import law_cases as C
import law_reference as R
import rk4_extended as X


def test_ageing_law_with_the_builtin_table_is_the_extended_rk4():
    """rk4_extended.forward_ext evaluates V_l(t) in long double at long-double times; this specification reads the float64
    table.  Long double against long double the two differ by the table's rounding alone (1.1e-16 relative on V_l, which
    enters the series with a sensitivity of order one: 1e-13 leaves a factor of twenty over the 5e-15 measured); the float64
    form is then as far from forward_ext as from its own long-double form, a plain float64 RK4's rounding, below the
    project's Tier-1 bound."""
    m = C.spec()
    ext, _ = X.forward_ext(m, R.LANES)
    ld, _ = R.forward(m, R.LANES, None, "aging", dtype=R.LD)
    f64, _ = R.forward(m, R.LANES, None, "ageing")
    e_ld, e_64 = R.rel_error(ld, ext).max(), R.rel_error(f64, ext).max()
    print(f"long double vs forward_ext {e_ld:.2e}, float64 vs forward_ext {e_64:.2e}")
    assert e_ld < 1e-13
    assert e_64 < C.CAP


@pytest.mark.parametrize("law", R.LAWS)
def test_fourth_order_in_substeps(law):
    """Under the built-in (smooth) history the global error of classical RK4 is c h^4 (1 + O(h)): halving h divides it by 16,
    an observed order of 4 — accepted within 0.3, which allows for the O(h) term at the coarsest pair (h = 0.1 and 0.05)."""
    dc = [20.0, 100.0, 1000.0]
    acc = {S: R.forward(C.spec(substeps=S), dc, None, law, dtype=R.LD)[0] for S in (1, 2, 4, 8, 32)}
    err = [(np.abs(acc[S] - acc[32]).max(axis=0) / np.abs(acc[32]).max(axis=0)).astype(np.float64) for S in (1, 2, 4, 8)]
    orders = np.array([np.log2(err[i] / err[i + 1]) for i in range(3)])
    print(law, "observed orders", orders, "error at substeps 1", err[0])
    assert np.all(np.abs(orders - 4.0) < 0.3)


@pytest.mark.parametrize("history", sorted(R.HISTORIES))
@pytest.mark.parametrize("law", R.LAWS)
def test_float64_against_long_double(history, law):
    """The float64 specification's own rounding error on the precision lanes: the yardstick of tests/test_gpu_law.py, recorded
    here (1e-14 to 7e-13 when this was written) and held below the project's Tier-1 bound."""
    s = C.precision_set(history, law)
    print(f"{history} {law}: per-lane error {s['err'].min():.2e} .. {s['yardstick']:.2e}")
    assert np.isfinite(s["acc"]).all()
    assert s["yardstick"] < C.CAP


def test_the_laws_agree_under_the_builtin_history_and_separate_under_a_step():
    """Under the built-in loading the slider stays in the linear neighbourhood of steady state, where the laws coincide; a
    velocity step takes it out.  (Relative to max|acc|: 2e-5 at Dc = 100 against ~10 % at Dc = 20 when this was written.)"""
    m = C.spec()
    d = {h: [R.forward(m, [20.0, 100.0, 1325.0], R.table(m, h), law)[0] for law in R.LAWS] for h in ("builtin", "step")}
    rel = {h: np.abs(a - s).max(axis=0) / np.abs(a).max(axis=0) for h, (a, s) in d.items()}
    print("builtin", rel["builtin"], "step", rel["step"])
    assert rel["builtin"].max() < 1e-3
    assert rel["step"][0] > 0.03


@pytest.mark.parametrize("truth, sign", [("slip", +1), ("aging", -1)])
def test_bayes_factor_names_the_true_law(truth, sign):
    """step history, truth Dc = 20, noise 5 % of max|clean|, box [5, 200], 4001 trapezoid nodes: every node finite under both
    laws, and the log Bayes factor (slip - ageing) beyond 5 on the truth's side (+13.9 and -34.0 when this was written)."""
    p = C.bayes_factor_problem(truth)
    print(truth, "log BF", p["log_bayes_factor"], p["log_evidence"])
    assert all(np.isfinite(s).all() and (s > 0).all() for s in p["ssq"].values())
    assert sign * p["log_bayes_factor"] > 5.0


def test_a_lane_below_the_stability_box_goes_non_finite():
    """Dc = 0.5 under the step history: fixed-step RK4 blows up under both laws (what the GPU's non-finite test relies on)"""
    m = C.spec()
    for law in R.LAWS:
        acc, ssq = R.forward(m, [0.5], R.table(m, "step"), law, data=np.zeros(R.nout(m)))
        assert not np.isfinite(ssq[0])
