"""
CPU tests of the extended-precision RK4 reference (tests/rk4_extended.py) and of the float64 CPU restatement against it.

The reference is pinned to the reference project's own trajectories (fourth-order convergence to the golden dop853
vectors), and the restatement's distance from it — the rounding error of a plain float64 RK4 — is measured on the lane
sets and models the GPU tests use (tests/test_gpu_rk4_extended.py), where it is the yardstick the kernels are held to.
"""
import numpy as np
import pytest

import rk4_extended as X

# The C restatement's own error against the extended reference, over every case and set of rk4_extended.CASES (both (a, b)
# variants): measured max 6.3e-13 (trajectory, n4000_S1 tight) and 1.6e-13 (sum of squares, n2000_S1 narrow); the caps leave
# 2.4x and 3x.  A series term or guard of the float64 kernels that costs more than that shows up against these numbers
# in the GPU tests, not against the 1e-9 of the restatement parity tests.
ORACLE_TRAJ_CAP, ORACLE_SSQ_CAP = 1.5e-12, 5e-13


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).nmant >= 63
    assert np.longdouble(1) + np.longdouble(2.0 ** -62) != np.longdouble(1)


def test_reference_converges_to_reference_dop853_at_fourth_order(oracle_mod, golden):
    """Same ladder as test_rk4_converges_to_reference_at_fourth_order, on the extended-precision reference: it IS the RK4
    scheme of the model (a wrong stage time, weight or RHS term would not converge to the reference's trajectory)."""
    g = golden.npz("forward")
    table = {500: {1: 3.6e-4, 2: 2.2e-5, 4: 1.4e-6, 8: 8.4e-8}, 2000: {1: 1.4e-6, 2: 8.5e-8}}
    dcs = (100.0, 1000.0, 5000.0)
    for n, ladder in table.items():
        ref = np.stack([g[f"n{n}_dc{dc:g}"] for dc in dcs], axis=1)
        prev = None
        for S, bound in ladder.items():
            acc, _ = X.forward_ext(oracle_mod.ModelSpec(n, substeps=S), dcs)
            err = (np.abs(acc.astype(np.float64) - ref).max(axis=0) / np.abs(ref).max(axis=0)).max()
            assert err <= 2 * bound, (n, S, err)
            if prev is not None and err > 5e-9:
                assert 12 <= prev / err <= 20, (n, S, prev / err)
            prev = err


def test_reference_other_golden_cases(oracle_mod, golden):
    """No damping and (a, b) away from the defaults: the reference's golden dop853 trajectories at S = 8."""
    g, meta = golden.npz("forward"), golden.json("forward")
    for case in meta["cases"]:
        if case["nsteps"] != 500 or case["dc"] < 100:
            continue
        m = oracle_mod.ModelSpec(500, substeps=8)
        m.RadiationDamping = case["damping"]
        acc, _ = X.forward_ext(m, [case["dc"]], case["a"], case["b"])
        ref = g[case["tag"]]
        assert np.abs(acc[:, 0].astype(np.float64) - ref).max() < 5e-7 * np.abs(ref).max(), case["tag"]


def test_reference_honours_model_attributes(oracle_mod, golden):
    """forward_nondefault.*: the reference project run with V_ref, mu_ref, mu_t_zero, k1, t_start all away from their
    defaults; the extended RK4 with 8 substeps converges to it like the default cases."""
    g, meta = golden.npz("forward_nondefault"), golden.json("forward_nondefault")
    for case in meta["cases"]:
        m = oracle_mod.ModelSpec(meta["number_time_steps"], meta["start_time"], meta["end_time"], 8)
        for k, v in meta["attrs"].items():
            setattr(m, k, v)
        m.RadiationDamping = case["damping"]
        acc, _ = X.forward_ext(m, [case["dc"]])
        ref = g[case["tag"]]
        assert acc.shape[0] == len(ref)
        assert np.abs(acc[:, 0].astype(np.float64) - ref).max() < 5e-7 * np.abs(ref).max(), case["tag"]


def test_lane_placement_follows_the_kernel_bound(oracle_mod):
    m = X.make_model(oracle_mod.ModelSpec, "n500_S1")
    h = m.delta_t / m.substeps
    for s, (lo, hi) in {"tight": (0, 2 ** -9), "tight_edge": (2 ** -9 / 1.12, 2 ** -9), "narrow": (2 ** -9, 2 ** -7),
                        "wide": (2 ** -7, 2 ** -3), "full": (2 ** -3, np.inf)}.items():
        dc = X.place_lanes(m, s, waves=2)
        assert dc.size == 2 * X.WAVE and (np.diff(dc.reshape(2, X.WAVE), axis=1) >= 0).all()
        dk = 1.2 * m.V_ref * h * (0.1 / dc) / m.a
        assert ((dk >= lo) & (dk < hi)).all(), s


@pytest.mark.parametrize("name", list(X.CASES))
def test_c_restatement_is_within_float64_rounding_of_the_reference(cpu_engine, oracle_mod, name):
    """The float64 CPU restatement (oracle/rsf_oracle.c) against the extended reference, set by set: a plain float64 RK4
    stays within ~1e-12 of the exact scheme — the size the GPU tests compare the kernels' error with."""
    p = X.Problem(oracle_mod.ModelSpec, name)
    assert cpu_engine.set_model(p.m, p.m.substeps) == p.data.size
    worst = []
    for variant in ("plain", "ab"):
        ssq, acc = cpu_engine.forward(p.dc, data=p.data, want_ssq=True, want_acc=True, **p.kw(variant))
        traj, serr = X.rel_errors(acc, ssq, *p.ext[variant])
        for s in p.sets:
            sl = p.lanes(s)
            worst.append((traj[sl].max(), serr[sl].max(), variant, s))
            print(f"{name:18s} {variant:5s} {s:10s} traj max {traj[sl].max():.1e} med {np.median(traj[sl]):.1e}   "
                  f"ssq max {serr[sl].max():.1e} med {np.median(serr[sl]):.1e}")
    t, s, variant, which = max(worst)
    assert t < ORACLE_TRAJ_CAP, (variant, which, t)
    t, s, variant, which = max(worst, key=lambda w: w[1])
    assert s < ORACLE_SSQ_CAP, (variant, which, s)
