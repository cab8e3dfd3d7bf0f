"""
GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs.  Tier-1 tolerance (BASELINE.json north_star): float64 agreement to rtol 1e-9 on the
trajectory, the sum of squares and the log-likelihood -0.5*SSq/sigma^2.
"""
import os

import numpy as np
import pytest

from chain_parity import RTOL, Rerun, assert_chains_match
from conftest import ROOT, synthetic_data

pytestmark = pytest.mark.gpu


def _models(oracle_mod, n, substeps=1, damping=True, t1=50.0):
    m = oracle_mod.ModelSpec(n, 0.0, t1, substeps)
    m.RadiationDamping = damping
    return m


def _traj_err(a, b):
    scale = np.abs(b).max(axis=0)
    return (np.abs(a - b).max(axis=0) / scale).max()


def test_backend_and_devices(gpu_engine):
    assert gpu_engine.lib.rsf_backend() == b"hip-gfx950"
    assert gpu_engine.lib.rsf_device_count() >= 1


def test_philox_known_answers_on_device(gpu_engine):
    # Random123 kat_vectors, philox4x32-10
    e = gpu_engine
    assert e.philox([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert e.philox([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert e.philox([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_device_variates_match_oracle(gpu_engine, cpu_engine):
    for chain, it in ((0, 0), (5, 17), (2 ** 33 + 7, 123456), (65535, 999)):
        zg, ug, gg = gpu_engine.draws(2025, chain, it, 3, 250.005)
        zc, uc, gc = cpu_engine.draws(2025, chain, it, 3, 250.005)
        np.testing.assert_allclose(zg, zc, rtol=1e-12, atol=1e-14)
        assert ug == uc
        np.testing.assert_allclose(gg, gc, rtol=1e-12)


@pytest.mark.parametrize("n,substeps,damping", [(500, 1, True), (500, 1, False), (500, 3, True), (2000, 1, True), (4000, 2, True), (37, 1, True)])
def test_forward_trajectory_and_ssq(gpu_engine, cpu_engine, oracle_mod, n, substeps, damping):
    m = _models(oracle_mod, n, substeps, damping)
    rng = np.random.default_rng(n + substeps)
    C = 203
    dc = rng.uniform(50.0, 9000.0, C)
    dc[:4] = [100.0, 1000.0, 5000.0, 9999.0]
    a = rng.uniform(0.008, 0.016, C)
    b = a + rng.uniform(-0.004, 0.008, C)
    for e in (gpu_engine, cpu_engine):
        assert e.set_model(m, substeps) == m.nout
    data = synthetic_data(cpu_engine)
    for kw in (dict(), dict(a=a, b=b)):
        sg, ag = gpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True, **kw)
        sc, ac = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True, **kw)
        assert _traj_err(ag, ac) < RTOL
        np.testing.assert_allclose(sg, sc, rtol=RTOL)
        # SSq-only and trajectory-only launches are separate kernel instantiations
        s2, _ = gpu_engine.forward(dc, data=data, want_ssq=True, want_acc=False, **kw)
        _, a2 = gpu_engine.forward(dc, want_acc=True, **kw)
        np.testing.assert_array_equal(s2, sg)
        np.testing.assert_array_equal(a2, ag)


@pytest.mark.parametrize("precision,integrator,rtol", [("float64", "rk4", RTOL), ("float64", "dop853", RTOL), ("float32", "rk4", None)])
def test_forward_with_non_default_model_constants(gpu_engine, cpu_engine, oracle_mod, precision, integrator, rtol):
    """Every model attribute of RateStateModel is user-settable (RateStateModel.py:167-184); nothing in the kernels may
    assume the defaults (V_ref = 1, mu_t_zero = mu_ref, t_start = 0 ...).  fp32 is checked against the fp64 GPU solve."""
    m = _models(oracle_mod, 400, 2 if integrator == "rk4" else 1, True, t1=37.0)
    m.t_start, m.delta_t = 1.5, (37.0 - 1.5) / 400
    m.V_ref, m.mu_ref, m.mu_t_zero, m.k1, m.a, m.b = 1.7, 0.55, 0.58, 3.0e-7, 0.012, 0.0155
    m.integrator = integrator
    rng = np.random.default_rng(5)
    C = 130
    dc = rng.uniform(300.0, 6000.0, C)
    a = rng.uniform(0.009, 0.015, C)
    b = a + rng.uniform(-0.003, 0.006, C)
    for e in (gpu_engine, cpu_engine):
        assert e.set_model(m, m.substeps) == m.nout
    data = synthetic_data(cpu_engine)
    for kw in (dict(), dict(a=a, b=b)):
        sc, ac = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True, **kw)
        if precision == "float64":
            sg, ag = gpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True, **kw)
            assert _traj_err(ag, ac) < rtol
            np.testing.assert_allclose(sg, sc, rtol=rtol)
        else:
            m.precision = "float32"
            gpu_engine.set_model(m, m.substeps)
            sg, ag = gpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True, **kw)
            m.precision = "float64"
            assert _traj_err(ag, ac) < 2e-3  # float32 solve: DESIGN "float32 solve" tolerance band
            np.testing.assert_allclose(sg, sc, rtol=5e-3)
    # and the sampler on top of it (initial covariance + a few iterations) for the float64 modes
    if precision == "float64":
        q0 = np.full((C, 1), 1500.0)
        tg, tc, rerun = _run_pair(gpu_engine, cpu_engine, 12, C, q0, data, [0.0], [1e4], seed=9, prior_len=3)
        assert_chains_match(tg, tc, rerun)


@pytest.mark.parametrize("integrator", ["rk4", "dop853"])
def test_forward_is_scale_free_in_v_ref(gpu_engine, cpu_engine, oracle_mod, integrator):
    """Slip rates in SI units: V_ref = 1e-6 with Dc scaled along (theta_0 = Dc/V_ref unchanged) is the same problem in
    other units; no absolute threshold in the kernels (tier heuristics, guards) may notice.  (DOP853's atol = 1e-10 is
    the reference's own absolute tolerance and applies to both sides alike.)"""
    m = _models(oracle_mod, 500)
    m.V_ref, m.integrator = 1.0e-6, integrator
    m.k1 = m.k1 / m.V_ref  # the damping coefficient carries units of 1/velocity: k1 v/a is what must stay the same
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
    dc = np.array([3.0e-4, 1.0e-3, 2.5e-3, 6.0e-3])
    data = synthetic_data(cpu_engine, dc_true=1.0e-3)
    sg, ag = gpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True)
    sc, ac = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True)
    assert np.isfinite(ac).all() and np.abs(ac).max() < 1e-4
    assert _traj_err(ag, ac) < RTOL
    np.testing.assert_allclose(sg, sc, rtol=RTOL)
    if integrator == "rk4":  # and it IS the V_ref = 1 problem in other units: acc scales with V_ref
        m1 = _models(oracle_mod, 500)
        gpu_engine.set_model(m1, 1)
        _, a1 = gpu_engine.forward(dc * 1.0e6)
        np.testing.assert_allclose(ag, a1 * 1.0e-6, rtol=1e-9, atol=1e-20)


@pytest.mark.parametrize("n,substeps,damping,mu_offset", [(500, 1, True, 0.0), (500, 1, False, 0.0), (500, 3, True, 0.0), (2000, 1, True, 0.0),
                                                           (500, 1, True, 5e-4), (2000, 2, True, -4e-4), (4000, 1, True, 5e-4)])
def test_forward_tight_tier_and_its_handover(gpu_engine, cpu_engine, oracle_mod, n, substeps, damping, mu_offset):
    """The sampler's steady state is the TIGHT tier (rsf_device.h rk4_tight: theta derivatives scaled by (h/2Dc)/x, x not
    carried), chosen per WAVE — the random Dc spreads of the other forward tests put a small-Dc lane into every wave and so
    only ever run the wider tiers.  Here the waves are homogeneous: every lane inside the tier's a-priori bound
    (start_tier: 1.2 V_ref h k'/a < 2^-9), four waves well inside and four just inside.  With the reference's constants the
    guards of such a wave never trip (that is what the bound is for); mu_offset != 0 starts the lanes off their steady state
    (mu_t_zero is a user-settable attribute, RateStateModel.py:167-184), |1 - v theta/Dc| ~ 4 % puts rho over its guard from the
    first trip: every chunk starts TIGHT, trips, is redone cold — x rebuilt from the carried (h/2Dc)/x — and hands its rest
    to the NARROW tier.  Same oracle, same 1e-9."""
    m = _models(oracle_mod, n, substeps, damping)
    m.mu_t_zero = m.mu_ref + mu_offset
    for e in (gpu_engine, cpu_engine):
        assert e.set_model(m, substeps) == m.nout
    h = 50.0 / (n - 1) / substeps
    a0 = 0.011
    edge = 1.2 * m.V_ref * h * 0.1 / a0 * 512.0  # Dc at which the a-priori bound sits for a = 0.011
    rng = np.random.default_rng(n + 7 * substeps)
    inside = np.sort(rng.uniform(1.4 * edge, 6.0 * edge, 256))
    at_edge = np.sort(rng.uniform(1.005 * edge, 1.12 * edge, 256))
    dc = np.concatenate([inside, at_edge])
    a = np.full(dc.shape, a0)
    b = a + rng.uniform(0.0, 0.006, dc.shape)
    data = synthetic_data(cpu_engine)
    for kw in (dict(), dict(a=a, b=b)):
        sg, ag = gpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True, **kw)
        sc, ac = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True, **kw)
        assert np.isfinite(sc).all()
        for lanes in (slice(0, 256), slice(256, 512)):
            assert _traj_err(ag[:, lanes], ac[:, lanes]) < RTOL
            np.testing.assert_allclose(sg[lanes], sc[lanes], rtol=RTOL)
        s2, _ = gpu_engine.forward(dc, data=data, want_ssq=True, want_acc=False, **kw)
        np.testing.assert_array_equal(s2, sg)


def test_forward_random_shapes(gpu_engine, cpu_engine, oracle_mod):
    """Seeded sweep over series lengths and substeps (loop trips of 8, remainders in pairs, odd last step, samples
    completing at any position of a trip, chunk boundaries) with lanes spread over all three tiers."""
    rng = np.random.default_rng(2026)
    for _ in range(24):
        n = int(rng.integers(2, 260))
        S = int(rng.choice([1, 1, 2, 3, 5, 8]))
        damping = bool(rng.integers(0, 2))
        m = _models(oracle_mod, n, S, damping, t1=0.1 * n)
        for e in (gpu_engine, cpu_engine):
            assert e.set_model(m, S) == m.nout
        C = int(rng.integers(1, 140))
        dc = np.exp(rng.uniform(np.log(30.0), np.log(9000.0), C))  # small Dc: NARROW / WIDE tiers and cold steps
        data = rng.normal(0.0, 3e-3, m.nout)
        sg, ag = gpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True)
        sc, ac = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True)
        fin = np.isfinite(sc)
        assert (np.isfinite(sg) == fin).all(), (n, S)
        if fin.any():
            assert _traj_err(ag[:, fin], ac[:, fin]) < RTOL, (n, S, damping, C)
            np.testing.assert_allclose(sg[fin], sc[fin], rtol=RTOL, err_msg=str((n, S, damping, C)))


def test_sampler_random_shapes(gpu_engine, cpu_engine, oracle_mod):
    """The same sweep through the sampler kernel (16 steps per loop trip in the one-parameter kernel)."""
    rng = np.random.default_rng(2027)
    for _ in range(10):
        n = int(rng.integers(20, 400))
        S = int(rng.choice([1, 1, 2, 3, 8]))
        m = _models(oracle_mod, n, S, True, t1=0.1 * n)
        for e in (gpu_engine, cpu_engine):
            e.set_model(m, S)
        data = synthetic_data(cpu_engine)
        C = int(rng.integers(3, 200))
        q0 = np.full((C, 1), float(rng.uniform(300.0, 3000.0)))
        tg, tc, rerun = _run_pair(gpu_engine, cpu_engine, 5, C, q0, data, [0.0], [1e4], seed=int(rng.integers(1, 1000)), prior_len=3)
        assert_chains_match(tg, tc, rerun)


def test_forward_edge_sizes(gpu_engine, cpu_engine, oracle_mod):
    m = _models(oracle_mod, 500)
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
    for C in (1, 63, 64, 65, 256, 257):
        dc = np.linspace(300.0, 3000.0, C)
        _, ag = gpu_engine.forward(dc)
        _, ac = cpu_engine.forward(dc)
        assert ag.shape == (500, C)
        assert _traj_err(ag, ac) < RTOL
    # stiff corner: fixed-step RK4 blows up for tiny Dc; both sides must agree it is non-finite
    data = synthetic_data(cpu_engine)
    sg, _ = gpu_engine.forward([0.05, 0.2, 1000.0], data=data, want_ssq=True, want_acc=False)
    sc, _ = cpu_engine.forward([0.05, 0.2, 1000.0], data=data, want_ssq=True, want_acc=False)
    assert (np.isfinite(sg) == np.isfinite(sc)).all() and not np.isfinite(sg[0])


def test_non_default_attributes_against_the_reference(gpu_engine, oracle_mod, golden):
    """The reference's own trajectories with every model attribute off its default (tests/golden/forward_nondefault.*):
    DOP853 mode on the GPU reproduces them; the RK4 path converges to them (S = 8)."""
    g, meta = golden.npz("forward_nondefault"), golden.json("forward_nondefault")
    for damping in (True, False):
        cases = [c for c in meta["cases"] if c["damping"] == damping]
        dc = np.array([c["dc"] for c in cases])
        ref = np.stack([g[c["tag"]] for c in cases], axis=1)
        for integrator, S, tol in (("dop853", 1, 1e-9), ("rk4", 8, 2e-7)):
            m = oracle_mod.ModelSpec(meta["number_time_steps"], meta["start_time"], meta["end_time"], S)
            for k, v in meta["attrs"].items():
                setattr(m, k, v)
            m.RadiationDamping, m.integrator = damping, integrator
            assert gpu_engine.set_model(m, S) == ref.shape[0]
            _, acc = gpu_engine.forward(dc)
            assert _traj_err(acc, ref) < tol, (integrator, damping, _traj_err(acc, ref))


@pytest.mark.parametrize("integrator", ["rk4", "dop853"])
def test_forward_smallest_series(gpu_engine, cpu_engine, oracle_mod, integrator):
    """nout = 2, 3, 4, 5: only the odd last step / one pair / pair + odd step / two pairs of the hot loop run."""
    for n in (2, 3, 4, 5):
        m = _models(oracle_mod, n, 1, True, t1=0.1 * n)
        m.integrator = integrator
        for e in (gpu_engine, cpu_engine):
            assert e.set_model(m, 1) == n
        dc = np.array([400.0, 1000.0, 2500.0])
        data = np.linspace(0.001, 0.002, n)
        sg, ag = gpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True)
        sc, ac = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True)
        np.testing.assert_allclose(ag, ac, rtol=RTOL, atol=1e-18)
        np.testing.assert_allclose(sg, sc, rtol=RTOL)


def test_forward_against_reference_golden(gpu_engine, oracle_mod, golden):
    """Tier 2: the GPU trajectory converges to the reference's dop853 output at 16x per halving."""
    g = golden.npz("forward")
    table = {500: {1: 3.6e-4, 2: 2.2e-5, 4: 1.4e-6, 8: 8.4e-8}, 2000: {1: 1.4e-6, 2: 8.5e-8, 4: 5.3e-9}}
    for n, ladder in table.items():
        ref = np.stack([g[f"n{n}_dc{dc:g}"] for dc in (100.0, 1000.0, 5000.0)], axis=1)
        prev = None
        for S, bound in ladder.items():
            gpu_engine.set_model(_models(oracle_mod, n, S), S)
            _, acc = gpu_engine.forward([100.0, 1000.0, 5000.0])
            err = _traj_err(acc, ref)
            assert err <= 2 * bound, (n, S, err)
            if prev is not None and err > 5e-9:
                assert 12 <= prev / err <= 20, (n, S, prev / err)
            prev = err


@pytest.mark.parametrize("prior_len", [3, 2])
def test_initial_covariance(gpu_engine, cpu_engine, oracle_mod, prior_len):
    m = _models(oracle_mod, 500)
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
    data = synthetic_data(cpu_engine)
    q0 = np.linspace(400.0, 2500.0, 70).reshape(-1, 1)
    for e in (gpu_engine, cpu_engine):
        e.mcmc_init(q0, data, [0.0], [1e4], seed=1, prior_len=prior_len)
    qg, sg, dg, Vg = gpu_engine.get_state()
    qc, sc, dc_, Vc = cpu_engine.get_state()
    np.testing.assert_array_equal(qg, qc)
    np.testing.assert_allclose(sg, sc, rtol=RTOL)
    np.testing.assert_allclose(dg, dc_, rtol=RTOL)
    # Vstart divides by a forward difference with relative step 1e-6 (MCMC.py:251): rounding noise of
    # ~1e-16 in acc is amplified by ~1e6..1e7, so agreement is limited to ~1e-7
    np.testing.assert_allclose(Vg, Vc, rtol=2e-6)


def _run_pair(gpu, cpu, n_iters, C, q0, data, lo, hi, **kw):
    for e in (gpu, cpu):
        e.mcmc_init(q0, data, lo, hi, **kw)
    state0 = cpu.get_state()
    gpu.set_state(*state0)  # identical start (see test_initial_covariance for why)
    q0 = np.asarray(q0, dtype=np.float64)
    rerun = Rerun(type(cpu), cpu, q0.reshape(q0.shape[0], -1), data, lo, hi, state0, kw)
    return gpu.mcmc_run(n_iters), cpu.mcmc_run(n_iters), rerun


@pytest.mark.parametrize("d", [1, 3])
def test_initial_covariance_from_stiff_and_ordinary_start_points(gpu_engine, cpu_engine, oracle_mod, d):
    """The init kernels — one lane per trajectory, the chain's 1 + d lanes meeting at every output sample by lane shuffles —
    from start points that span every integration tier: Dc down to 6, where the incremental tiers' guards trip and the lane
    redoes the trip with full evaluations (a path no test reached before round 4; the lockstep kernel it replaced restored
    the wrong state representation there), up to 6000.  Initial SSq and sigma^2_0 against the checker to 1e-9; the proposal
    covariance on its own scale (d = 1: the forward-difference noise of MCMC.py:251 allows 2e-6 there; stiff start points
    amplify it further and are held to 1e-3)."""
    m = _models(oracle_mod, 500)
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
    data = synthetic_data(cpu_engine)
    C = 777  # not a multiple of the 64 / 128 chains a workgroup's lane groups hold
    rng = np.random.default_rng(9)
    q0 = np.column_stack([np.exp(rng.uniform(np.log(6.0), np.log(6000.0), C)), rng.uniform(0.009, 0.014, C), rng.uniform(0.012, 0.018, C)])[:, :d]
    lo, hi = [0.0, 0.005, 0.005][:d], [1e4, 0.02, 0.03][:d]
    for e in (gpu_engine, cpu_engine):
        e.mcmc_init(q0, data, lo, hi, seed=1, prior_len=3, fd_rel_step=1e-6 if d == 1 else 1e-4)
    sg, sc = [np.asarray(x) for x in gpu_engine.get_state()], [np.asarray(x) for x in cpu_engine.get_state()]
    assert np.isfinite(sg[1]).all() and np.isfinite(sg[3]).all()
    np.testing.assert_allclose(sg[1], sc[1], rtol=RTOL)
    np.testing.assert_allclose(sg[2], sc[2], rtol=RTOL)
    sd = np.sqrt(np.diagonal(sc[3], axis1=1, axis2=2))
    err = np.abs(sg[3] - sc[3]) / (sd[:, :, None] * sd[:, None, :])
    ordinary = q0[:, 0] > 150.0
    assert err[ordinary].max() < (2e-6 if d == 1 else 1e-4), err[ordinary].max()
    assert err.max() < 1e-3, err.max()
    assert (q0[:, 0] < 20.0).sum() > 50  # the stiff start points are really there


@pytest.mark.parametrize("n,C,adapt", [(500, 300, "none"), (500, 130, "reference_dict"), (500, 130, "am"), (2000, 70, "none")])
def test_mcmc_run_matches_oracle(gpu_engine, cpu_engine, oracle_mod, n, C, adapt):
    m = _models(oracle_mod, n)
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
    data = synthetic_data(cpu_engine)
    q0 = np.full((C, 1), 1000.0)
    tg, tc, rerun = _run_pair(gpu_engine, cpu_engine, 40, C, q0, data, [0.0], [1e4], seed=2025, chain_offset=12345,
                       prior_len=3 if adapt == "none" else 2, adapt_mode=adapt, adapt_interval=10)
    assert_chains_match(tg, tc, rerun)
    sg, sc = gpu_engine.stats(), cpu_engine.stats()
    assert sg["iters_done"] == sc["iters_done"] == 40
    assert abs(sg["accepted"] - sc["accepted"]) <= 0.01 * C * 40
    # log-likelihood -0.5*SSq/sigma^2 at the end state
    _, ssg, s2g, Vg = gpu_engine.get_state()
    _, ssc, s2c, Vc = cpu_engine.get_state()
    same = (tg[2] == tc[2]).all(axis=0)
    np.testing.assert_allclose((-0.5 * ssg / s2g)[same], (-0.5 * ssc / s2c)[same], rtol=RTOL)
    np.testing.assert_allclose(Vg[same], Vc[same], rtol=1e-8)


def test_mcmc_continuation_equals_single_launch(gpu_engine, oracle_mod):
    """Counter-based RNG + persistent state: 3 launches of 7 iterations == 1 launch of 21."""
    m = _models(oracle_mod, 500)
    gpu_engine.set_model(m, 1)
    data = synthetic_data(gpu_engine)
    q0 = np.full((100, 1), 900.0)
    gpu_engine.mcmc_init(q0, data, [0.0], [1e4], seed=3, prior_len=2, adapt_mode="reference_dict", adapt_interval=5)
    one = gpu_engine.mcmc_run(21)
    gpu_engine.mcmc_init(q0, data, [0.0], [1e4], seed=3, prior_len=2, adapt_mode="reference_dict", adapt_interval=5)
    parts = [gpu_engine.mcmc_run(7) for _ in range(3)]
    for k in range(3):
        np.testing.assert_array_equal(np.concatenate([p[k] for p in parts]), one[k])


@pytest.mark.parametrize("d", [1, 3])
def test_host_caller_drain_pipeline_equals_single_launch(pkg, oracle_mod, monkeypatch, d):
    """RSF_MEM_HOST runs longer than the drain budget are cut into launches whose trace rows are copied out on a
    second stream while the next launch computes; the rows must be those of the one-launch run, also when only some
    of the trace arrays are requested."""
    m = _models(oracle_mod, 500)
    C = 200
    q0 = np.tile(np.array([900.0, 0.011, 0.014][:d]), (C, 1))
    lo, hi = [0.0, 0.005, 0.005][:d], [1e4, 0.02, 0.03][:d]
    V0 = np.tile(np.diag(np.array([20.0 ** 2, 1e-4 ** 2, 1e-4 ** 2][:d])), (C, 1, 1))
    adapt = dict(prior_len=2, adapt_mode="reference_dict", adapt_interval=5) if d == 1 else dict(adapt_mode="am", adapt_interval=5)

    def run(want):
        with pkg.Engine(mem="host") as e:
            e.set_model(m, 1)
            data = synthetic_data(e)
            e.mcmc_init(q0, data, lo, hi, seed=5, **adapt)
            e.set_state(V=V0)
            out = e.mcmc_run(23, traces=want)
            return out, e.get_state(), e.stats()

    one, st1, s1 = run(True)
    assert 0 < s1["accepted"] < 23 * C  # the chains move: a row written to the wrong place would show
    monkeypatch.setenv("RSF_DRAIN_BYTES", str(C * (8 * d + 9) * 3 + 5))  # 3 iterations per launch, last launch ragged
    cut, st2, s2 = run(True)
    for k in range(3):
        np.testing.assert_array_equal(cut[k], one[k])
    for a, b in zip(st1, st2):
        np.testing.assert_array_equal(a, b)
    assert s1 == s2 and s2["iters_done"] == 23
    only_q, _, _ = run(("q",))
    np.testing.assert_array_equal(only_q[0], one[0])
    assert only_q[1] is None and only_q[2] is None


def test_out_of_bounds_proposals_skip_the_solve(gpu_engine, cpu_engine, oracle_mod):
    m = _models(oracle_mod, 500)
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
    data = synthetic_data(cpu_engine)
    C = 128
    tg, tc, rerun = _run_pair(gpu_engine, cpu_engine, 30, C, np.full((C, 1), 1000.0), data, [980.0], [1020.0], seed=11, prior_len=3)
    assert_chains_match(tg, tc, rerun)
    sg, sc = gpu_engine.stats(), cpu_engine.stats()
    assert sg["evaluated"] == sc["evaluated"] < C * 30  # some proposals left the box: no forward solve for them
    assert (tg[0] > 980.0).all() and (tg[0] < 1020.0).all()


def test_out_of_bounds_with_chunked_tables(gpu_engine, cpu_engine, oracle_mod):
    """nsteps 4000 x 2 substeps does not fit the LDS budget, so the tables are staged chunk by chunk behind workgroup
    barriers: waves whose lanes are all out of bounds must still take part in the staging (no divergent barrier), and
    chains that are in bounds only sometimes must match the oracle."""
    m = _models(oracle_mod, 4000, 2)
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 2)
    data = synthetic_data(cpu_engine)
    C = 300  # 5 waves, the last one ragged; most proposals leave the box
    tg, tc, rerun = _run_pair(gpu_engine, cpu_engine, 6, C, np.full((C, 1), 1000.0), data, [995.0], [1005.0], seed=3, prior_len=3)
    assert_chains_match(tg, tc, rerun)
    sg, sc = gpu_engine.stats(), cpu_engine.stats()
    assert sg["evaluated"] == sc["evaluated"] < C * 6 // 2


def _dp(oracle_mod, n, damping=True):
    m = _models(oracle_mod, n, 1, damping)
    m.integrator = "dop853"
    return m


def test_dop853_mode_matches_oracle_and_reference(gpu_engine, cpu_engine, oracle_mod, golden):
    """RSF_FLAG_DOP853: the reference's own adaptive scheme on the GPU — against the CPU restatement (Tier 1) and
    directly against the reference's golden trajectories, SSq grid and initial covariance (no RK4 ladder needed)."""
    g, meta = golden.npz("forward"), golden.json("forward")
    for case in meta["cases"]:
        m = _dp(oracle_mod, case["nsteps"], case["damping"])
        m.a, m.b = case["a"], case["b"]
        gpu_engine.set_model(m, 1)
        _, acc = gpu_engine.forward([case["dc"]])
        ref = g[case["tag"]]
        tol = 1e-9 if case["dc"] >= 10 else 1e-6  # Dc = 1 is stiff: 9 000 RHS calls, step decisions near the tolerance
        assert np.abs(acc[:, 0] - ref).max() <= tol * np.abs(ref).max(), case["tag"]
    m = _dp(oracle_mod, 500)
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
    rng = np.random.default_rng(21)
    C = 150
    dc = rng.uniform(80.0, 9000.0, C)
    a = rng.uniform(0.008, 0.016, C)
    b = a + rng.uniform(-0.004, 0.008, C)
    data = synthetic_data(cpu_engine)
    sg, ag = gpu_engine.forward(dc, a=a, b=b, data=data, want_ssq=True)
    sc, ac = cpu_engine.forward(dc, a=a, b=b, data=data, want_ssq=True)
    assert _traj_err(ag, ac) < RTOL
    np.testing.assert_allclose(sg, sc, rtol=RTOL)
    gs = golden.npz("ssq")
    ssq, _ = gpu_engine.forward(gs["qgrid"], data=gs["data"], want_ssq=True, want_acc=False)
    np.testing.assert_allclose(ssq, gs["ssq"], rtol=1e-9)  # == MCMC.SSqcalc of the reference
    for name, c in golden.json("init")["cases"].items():
        gpu_engine.mcmc_init([[c["qstart"]]], gs["data"], [0.0], [1e4], prior_len=c["prior_len"])
        _, _, std2, V = gpu_engine.get_state()
        np.testing.assert_allclose(std2[0], c["std2_0"], rtol=1e-9, err_msg=name)
        np.testing.assert_allclose(V[0, 0, 0], c["vstart"], rtol=1e-5, err_msg=name)


def test_dop853_failed_calls_leave_zeros(gpu_engine, cpu_engine, oracle_mod):
    """A dop853 call that fails (step size underflow on a NaN, > 500 steps) ends the reference's loop — `while r.successful()`,
    RateStateModel.py:361-381 — and the rest of its arrays keep their zeros.  Lanes that fail in their second call share
    waves with healthy ones: the wave then leaves the steady-state loop for good (solve() in rsf_device_dop853.h) and every
    later interval of its healthy lanes goes through the general loop — same results, to the mode's 1e-9."""
    m = _dp(oracle_mod, 300)
    for e in (gpu_engine, cpu_engine):
        assert e.set_model(m, 1) == m.nout
    bad = [(1000.0, 1e-9, 1e-3), (1e-4, 1e-9, 1e-3), (1e-6, 1e-4, 0.5), (1e-12, 0.011, 5.0)]
    rng = np.random.default_rng(8)
    C = 160  # two full waves and a ragged one
    dc, a, b = rng.uniform(400.0, 3000.0, C), np.full(C, 0.011), np.full(C, 0.014)
    where = [3, 64 + 17, 64 + 40, 128 + 5]  # wave 0: one failing lane, wave 1: two, wave 2 (ragged): one
    for i, (d_, a_, b_) in zip(where, bad):
        dc[i], a[i], b[i] = d_, a_, b_
    data = synthetic_data(cpu_engine)
    sg, ag = gpu_engine.forward(dc, a=a, b=b, data=data, want_ssq=True, want_acc=True)
    sc, ac = cpu_engine.forward(dc, a=a, b=b, data=data, want_ssq=True, want_acc=True)
    ok = np.ones(C, bool)
    ok[where] = False
    assert _traj_err(ag[:, ok], ac[:, ok]) < RTOL
    np.testing.assert_allclose(sg[ok], sc[ok], rtol=RTOL)
    for i in where:
        assert np.count_nonzero(ac[2:, i]) == 0, "the fixture lanes are meant to fail in their second call"
        np.testing.assert_array_equal(ag[2:, i], 0.0)
        # the one sample such a lane completes: a = 1e-9 amplifies the rounding of its exponent's argument a millionfold
        np.testing.assert_allclose(ag[:2, i], ac[:2, i], rtol=1e-5, atol=1e-300)
        np.testing.assert_allclose(sg[i], sc[i], rtol=1e-5)


@pytest.mark.parametrize("tag", ["list", "dict", "dict3", "tightbox"])
def test_dop853_mode_replays_the_reference_chain(gpu_engine, golden, oracle_mod, tag):
    """Same variates + same integrator: the GPU kernel walks the reference's chain, every iteration."""
    g, meta = golden.npz("replay_" + tag), golden.json("replay_" + tag)
    is_list = isinstance(meta["prior"], list)
    lo, hi = (meta["prior"][1], meta["prior"][2]) if is_list else (meta["prior"]["1"], meta["prior"]["2"])
    gpu_engine.set_model(_dp(oracle_mod, meta["nsteps"]), 1)
    gpu_engine.mcmc_init([[meta["qstart"]]], g["data"], [lo], [hi], prior_len=len(meta["prior"]),
                         adapt_mode="none" if is_list else "reference_dict", adapt_interval=meta["adapt_interval"])
    _, ssq, std2, V = gpu_engine.get_state()
    np.testing.assert_allclose([ssq[0], std2[0]], [meta["ssq0"], meta["std2_0"]], rtol=1e-9)
    gpu_engine.set_state(V=[[[meta["vstart"]]]])
    n = len(g["z"])
    u = np.where(np.isnan(g["u"]), 1.0, g["u"])
    tq, ts, ta = gpu_engine.mcmc_replay(g["z"].reshape(n, 1, 1), u.reshape(n, 1), g["g"].reshape(n, 1))
    np.testing.assert_allclose(tq[:, 0, 0], np.append(g["q_cur"][1:], g["qparams_kept"][0, -1]), rtol=1e-10)
    np.testing.assert_allclose(ts[:, 0], g["std2_after"], rtol=1e-8)
    assert gpu_engine.stats()["evaluated"] == int(g["inb"].sum())


def test_edge_cases_and_call_order(pkg, cpu_engine, oracle_mod):
    m = _models(oracle_mod, 500)
    cpu_engine.set_model(m, 1)
    data = synthetic_data(cpu_engine)
    for block in (64, 128, 192, 256):  # every legal workgroup size gives the same numbers
        with pkg.Engine(mem="host", block_threads=block) as e:
            e.set_model(m, 1)
            dc = np.linspace(200.0, 4000.0, 321)
            s, a = e.forward(dc, data=data, want_ssq=True)
            if block == 64:
                ref = (s, a)
            np.testing.assert_array_equal(s, ref[0])
            np.testing.assert_array_equal(a, ref[1])
    ref = None
    for block in (64, 256):  # ... including the fused sampler kernel
        with pkg.Engine(mem="host", block_threads=block) as e:
            e.set_model(m, 1)
            e.mcmc_init(np.full((200, 1), 1000.0), data, [0.0], [1e4], seed=3, prior_len=3)
            out = e.mcmc_run(8)
            ref = ref or out
            for k in range(3):
                np.testing.assert_array_equal(out[k], ref[k])
    # ... the three-parameter kernel (Cholesky factors in LDS behind the table chunk) and the float32 sampler, whose lanes
    # carry two chains each (slot layout, LDS factor slots and grid all depend on the workgroup size)
    q3 = np.column_stack([np.linspace(600.0, 2400.0, 333), np.full(333, 0.011), np.full(333, 0.014)])
    V3 = np.tile(np.diag([25.0 ** 2, 1e-4 ** 2, 1e-4 ** 2]), (333, 1, 1))
    for precision, d in (("float64", 3), ("float32", 1), ("float32", 3)):
        m2 = _models(oracle_mod, 500)
        m2.precision = precision
        ref = None
        for block in (64, 128, 256):
            with pkg.Engine(mem="host", block_threads=block) as e:
                e.set_model(m2, 1)
                e.mcmc_init(q3[:, :d], data, [0.0, 0.005, 0.005][:d], [1e4, 0.02, 0.03][:d], seed=4, prior_len=3 if d == 1 else 0,
                            adapt_mode="am", adapt_interval=4)
                if d == 3:
                    e.set_state(V=V3)
                out = e.mcmc_run(9)
                ref = ref or out
                for k in range(3):
                    np.testing.assert_array_equal(out[k], ref[k], err_msg=f"{precision} d={d} block={block}")
    with pytest.raises(pkg._abi.RsfError):
        pkg.Engine(mem="host", block_threads=96)
    with pkg.Engine(mem="host") as e:
        with pytest.raises(pkg._abi.RsfError):  # model not set
            e.forward([1000.0])
        e.set_model(m, 1)
        ssq, acc = e.forward(np.empty(0))  # empty batch
        assert acc.shape == (500, 0)
        with pytest.raises(pkg._abi.RsfError):  # chains not initialised
            e.mcmc_run(1)
        # one chain, huge global chain id (64-bit Philox counter), zero iterations, then a few
        e.mcmc_init([[1000.0]], data, [0.0], [1e4], seed=7, chain_offset=2 ** 33 + 7, prior_len=3)
        cpu_engine.mcmc_init([[1000.0]], data, [0.0], [1e4], seed=7, chain_offset=2 ** 33 + 7, prior_len=3)
        e.set_state(*cpu_engine.get_state())
        assert e.mcmc_run(0)[0].shape == (0, 1, 1) and e.stats()["iters_done"] == 0
        tg, tc = e.mcmc_run(12), cpu_engine.mcmc_run(12)
        np.testing.assert_array_equal(tg[2], tc[2])
        np.testing.assert_allclose(tg[0], tc[0], rtol=RTOL)
        # a new model with another series length invalidates the chains (the observation no longer fits)
        e.set_model(_models(oracle_mod, 400), 1)
        with pytest.raises(pkg._abi.RsfError):
            e.mcmc_run(1)


def test_replay_three_parameters(gpu_engine, cpu_engine, oracle_mod):
    """Caller-supplied variates with d = 3 (z has three columns, lower-Cholesky proposal)."""
    m = _models(oracle_mod, 500)
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
    data = synthetic_data(cpu_engine)
    C, n = 64, 15
    rng = np.random.default_rng(12)
    z, u, g = rng.standard_normal((n, C, 3)), rng.uniform(size=(n, C)), rng.gamma(250.005, size=(n, C))
    q0 = np.tile([1000.0, 0.011, 0.014], (C, 1))
    A = rng.standard_normal((3, 3)) * [[20.0], [1e-4], [1e-4]]
    V0 = np.tile(A @ A.T + np.diag([1.0, 1e-10, 1e-10]), (C, 1, 1))  # a full (correlated) covariance
    for e in (gpu_engine, cpu_engine):
        e.mcmc_init(q0, data, [0.0, 0.005, 0.005], [1e4, 0.02, 0.03], seed=1)
    q, ssq, std2, _ = cpu_engine.get_state()
    for e in (gpu_engine, cpu_engine):
        e.set_state(q, ssq, std2, V0)
    tg, tc = gpu_engine.mcmc_replay(z, u, g), cpu_engine.mcmc_replay(z, u, g)
    rerun = Rerun(type(cpu_engine), cpu_engine, q0, data, [0.0, 0.005, 0.005], [1e4, 0.02, 0.03], (q, ssq, std2, V0), dict(seed=1),
                   variates=(z, u, g))
    same = assert_chains_match(tg, tc, rerun)
    assert 0.05 < tg[2].mean() < 0.98 and same.any()


@pytest.mark.parametrize("d", [1, 3])
def test_one_proposal_replay_graph_equals_plain_replay(pkg, oracle_mod, d):
    """A one-iteration rsf_mcmc_replay from host memory runs as a hipGraph (pinned blocks + kernel node with updated
    arguments); six such calls must give the rows and the final state of one six-iteration call (plain path), also
    across a change of the chain count (graph rebuilt) and with trace arrays left out."""
    m = _models(oracle_mod, 500)
    rng = np.random.default_rng(21)
    n = 6
    for C in (70, 33):
        z, u, g = rng.standard_normal((n, C, d)), rng.uniform(size=(n, C)), rng.gamma(250.005, size=(n, C))
        q0 = np.tile(np.array([1000.0, 0.011, 0.014][:d]), (C, 1))
        lo, hi = [0.0, 0.005, 0.005][:d], [1e4, 0.02, 0.03][:d]
        V0 = np.tile(np.diag(np.array([25.0 ** 2, 1e-4 ** 2, 1e-4 ** 2][:d])), (C, 1, 1))
        with pkg.Engine(mem="host") as e:
            e.set_model(m, 1)
            data = synthetic_data(e)

            def start():
                e.mcmc_init(q0, data, lo, hi, seed=1, adapt_mode="am", adapt_interval=4)
                e.set_state(V=V0)

            start()
            plain = e.mcmc_replay(z, u, g)
            st_plain = e.get_state()
            start()
            rows = [e.mcmc_replay(z[k:k + 1], u[k:k + 1], g[k:k + 1], traces=True if k % 2 else ("q", "accept")) for k in range(n)]
            st_graph = e.get_state()
            assert e.stats()["iters_done"] == n
        assert 0 < plain[2].sum() < plain[2].size  # some accepted, some rejected
        for k in range(n):
            np.testing.assert_array_equal(rows[k][0][0], plain[0][k])
            np.testing.assert_array_equal(rows[k][2][0], plain[2][k])
            if k % 2:
                np.testing.assert_array_equal(rows[k][1][0], plain[1][k])
            else:
                assert rows[k][1] is None
        for a, b in zip(st_plain, st_graph):
            np.testing.assert_array_equal(a, b)


def test_host_and_device_memory_spaces_agree(pkg, oracle_mod):
    """RSF_MEM_HOST stages the caller's arrays, RSF_MEM_DEVICE uses them in place: same kernels, same results —
    forward solve, initial state, a sampler run and the pooled moments."""
    import torch

    m = _models(oracle_mod, 500)
    C = 333
    dc = np.linspace(500.0, 3000.0, C)
    with pkg.Engine(mem="host") as eh, pkg.Engine(mem="device") as ed:
        for e in (eh, ed):
            e.set_model(m, 1)
        data = synthetic_data(eh)
        sh, ah = eh.forward(dc, data=data, want_ssq=True, want_acc=True)
        sd, ad = ed.forward(torch.from_numpy(dc).cuda(), data=torch.from_numpy(data).cuda(), want_ssq=True, want_acc=True)
        np.testing.assert_array_equal(sh, sd.cpu().numpy())
        np.testing.assert_array_equal(ah, ad.cpu().numpy())
        q0 = np.full((C, 1), 1000.0)
        eh.mcmc_init(q0, data, [0.0], [1e4], seed=8, prior_len=3)
        ed.mcmc_init(torch.from_numpy(q0).cuda(), torch.from_numpy(data).cuda(), [0.0], [1e4], seed=8, prior_len=3)
        for a, b in zip(eh.get_state(), ed.get_state()):
            np.testing.assert_array_equal(a, b.cpu().numpy())
        th, td = eh.mcmc_run(9), ed.mcmc_run(9)
        ed.sync()
        for a, b in zip(th, td):
            np.testing.assert_array_equal(a, b.cpu().numpy())
        assert eh.stats() == ed.stats()
        assert eh.pool_summary(th[0]) == ed.pool_summary(td[0])


def test_two_ctxs_from_two_threads(pkg, oracle_mod):
    """rsf_abi.h: a ctx is single-owner, distinct ctxs are independent — two host threads, each with its own ctx
    (host-memory mode, so every call stages and synchronises), must reproduce their sequential results."""
    import threading

    m = _models(oracle_mod, 500)
    with pkg.Engine(mem="host") as e:
        e.set_model(m, 1)
        data = synthetic_data(e)

    def job(seed, C, out):
        with pkg.Engine(mem="host") as e:
            e.set_model(m, 1)
            e.mcmc_init(np.full((C, 1), 1000.0), data, [0.0], [1e4], seed=seed, prior_len=3)
            out[seed] = [e.mcmc_run(7) for _ in range(3)]

    seq, par = {}, {}
    job(1, 500, seq)
    job(2, 300, seq)
    ts = [threading.Thread(target=job, args=(1, 500, par)), threading.Thread(target=job, args=(2, 300, par))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for seed in (1, 2):
        for a, b in zip(seq[seed], par[seed]):
            for k in range(3):
                np.testing.assert_array_equal(a[k], b[k])


def test_pool_summary_and_kde(pkg, cpu_engine):
    """Device reductions over pooled samples vs the oracle and scipy.stats.gaussian_kde (host and device buffers)."""
    import torch
    from scipy.stats import gaussian_kde

    rng = np.random.default_rng(4)
    n = 200_003
    trace = np.stack([rng.normal(1000.0, 40.0, n), rng.normal(0.011, 1e-3, n), rng.gamma(3.0, 2.0, n)], axis=1).reshape(-1, 1, 3)
    grid = np.linspace(800.0, 1200.0, 1000)
    with pkg.Engine(mem="host") as eh, pkg.Engine(mem="device") as ed:
        for p in range(3):
            x = trace[..., p].ravel()
            ref = cpu_engine.pool_summary(trace, param=p)
            for e, arr in ((eh, trace), (ed, torch.as_tensor(trace).cuda())):
                s = e.pool_summary(arr, param=p)
                np.testing.assert_allclose([s[k] for k in ("n", "mean", "var", "min", "max")],
                                           [ref[k] for k in ("n", "mean", "var", "min", "max")], rtol=1e-11)
        dens_h = eh.pool_kde(trace, grid, param=0)
        dens_d = ed.pool_kde(torch.as_tensor(trace).cuda(), torch.as_tensor(grid).cuda(), param=0).cpu().numpy()
        np.testing.assert_array_equal(dens_h, dens_d)  # fixed-order reduction: reproducible
        sub = trace[:5000]
        np.testing.assert_allclose(eh.pool_kde(sub, grid, param=0), gaussian_kde(sub[..., 0].ravel()).pdf(grid), rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(eh.pool_kde(sub, grid, param=0), cpu_engine.pool_kde(sub, grid, param=0), rtol=1e-10, atol=1e-300)
        assert abs(np.trapezoid(dens_h, grid) - 1.0) < 1e-3


def test_pool_histogram(pkg, cpu_engine):
    """Device fixed-bin histogram (LDS-privatised counting, integer atomics) vs the oracle: identical counts, host and device
    buffers, every parameter of a trace block, many and few bins, edge values and NaN."""
    import torch

    rng = np.random.default_rng(6)
    n = 1_000_003
    trace = np.stack([rng.normal(1000.0, 40.0, n), rng.normal(0.011, 1e-3, n), rng.gamma(3.0, 2.0, n)], axis=1).reshape(-1, 1, 3)
    trace[3, 0, 0], trace[4, 0, 0], trace[5, 0, 0], trace[6, 0, 0] = 900.0, 1100.0, np.nan, np.nextafter(1100.0, 0.0)
    with pkg.Engine(mem="host") as eh, pkg.Engine(mem="device") as ed:
        dev = torch.as_tensor(trace).cuda()
        for p, (nbins, lo, hi) in enumerate(((40, 900.0, 1100.0), (1, 0.008, 0.014), (4096, 0.0, 30.0))):
            ref = cpu_engine.pool_histogram(trace, nbins, lo, hi, param=p)
            np.testing.assert_array_equal(eh.pool_histogram(trace, nbins, lo, hi, param=p), ref)
            np.testing.assert_array_equal(ed.pool_histogram(dev, nbins, lo, hi, param=p).cpu().numpy(), ref)
            assert ref.sum() == n
        with pytest.raises(pkg.RsfError):
            eh.pool_histogram(trace, 5000, 0.0, 1.0)
        # samples exactly on the bin edges and one ulp either side: numpy.histogram itself is the reference here
        for nbins, lo, hi in ((10, 0.0, 1.0), (100, 0.005, 0.02), (7, 0.008, 0.014), (1000, 900.0, 1100.0), (3, -1.0, 2.0)):
            edges = np.linspace(lo, hi, nbins + 1)
            x = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [0.3, 0.7, lo + 0.3 * (hi - lo)]])
            ref, _ = np.histogram(x, nbins, (lo, hi))
            got = eh.pool_histogram(x, nbins, lo, hi)
            np.testing.assert_array_equal(got[1:-1], ref, err_msg=f"{(nbins, lo, hi)}")
            np.testing.assert_array_equal(got, cpu_engine.pool_histogram(x, nbins, lo, hi))


def test_observation_groups(gpu_engine, cpu_engine, oracle_mod):
    """One observation series per chain group: GPU vs oracle, and the group blocks are used."""
    m = _models(oracle_mod, 500)
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
    G, per = 3, 256
    data = np.stack([synthetic_data(cpu_engine, dc_true=dc, seed=20 + g) for g, dc in enumerate((300.0, 1000.0, 4000.0))])
    q0 = np.full((G * per, 1), 900.0)
    tg, tc, rerun = _run_pair(gpu_engine, cpu_engine, 25, G * per, q0, data, [0.0], [1e4], seed=8, prior_len=3)
    assert_chains_match(tg, tc, rerun)
    means = [tg[0][10:, g * per:(g + 1) * per, 0].mean() for g in range(G)]
    assert means[0] < means[1] < means[2]  # each group is pulled towards its own true Dc
    with pytest.raises(Exception):
        gpu_engine.mcmc_init(q0[:300], data, [0.0], [1e4])  # 100 chains per group: not a multiple of the workgroup


def test_three_parameter_chains(gpu_engine, cpu_engine, oracle_mod):
    """Extension (BASELINE config 5): joint (Dc, a, b).  The init kernel's proposal covariance — prior-regularised, since
    sigma^2 (X^T X)^-1 alone is astronomically wide along the (Dc, a) ridge (rsf_kernels_core.h::initial_covariance) — agrees with
    the checker's to 1e-4 at a forward-difference step of 1e-4 (condition number ~4e3 times the ~1e-8 the step leaves of the
    trajectories' rounding), from three different start points; then chains from a common explicit state, which must really
    move."""
    m = _models(oracle_mod, 500)
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
    data = synthetic_data(cpu_engine)
    C = 96
    q0 = np.tile([1000.0, 0.011, 0.014], (C, 1))
    q0[1::3] = [1500.0, 0.008, 0.02]
    q0[2::3] = [400.0, 0.016, 0.009]
    lo, hi = [0.0, 0.005, 0.005], [1e4, 0.02, 0.03]
    V0 = np.tile(np.diag([20.0 ** 2, 1e-4 ** 2, 1e-4 ** 2]), (C, 1, 1))
    for e in (gpu_engine, cpu_engine):
        e.mcmc_init(q0, data, lo, hi, seed=5, adapt_mode="am", adapt_interval=10, fd_rel_step=1e-4)
    sg, sc = gpu_engine.get_state(), cpu_engine.get_state()
    np.testing.assert_allclose(sg[1], sc[1], rtol=RTOL)
    np.testing.assert_allclose(sg[2], sc[2], rtol=RTOL)
    sd = np.sqrt(np.diagonal(sc[3], axis1=1, axis2=2))
    # the initial proposal covariance itself, every entry on the scale sqrt(V_pp V_rr) (the correlations with b are ~1e-5: zero)
    assert (np.abs(sg[3] - sc[3]) <= 1e-4 * sd[:, :, None] * sd[:, None, :]).all(), np.abs((sg[3] - sc[3]) / (sd[:, :, None] * sd[:, None, :])).max()
    assert ((sg[3][:, 0, 1] / (sd[:, 0] * sd[:, 1])) < -0.98).all()  # it follows the ridge Dc * a = const
    q, ssq, std2, _ = cpu_engine.get_state()
    for e in (gpu_engine, cpu_engine):
        e.set_state(q, ssq, std2, V0)
    tg, tc = gpu_engine.mcmc_run(40), cpu_engine.mcmc_run(40)
    rerun = Rerun(type(cpu_engine), cpu_engine, q0, data, lo, hi, (q, ssq, std2, V0), dict(seed=5, adapt_mode="am", adapt_interval=10))
    same = assert_chains_match(tg, tc, rerun)
    assert tg[0].shape == (40, C, 3)
    acc_rate = tg[2].mean()
    assert 0.1 < acc_rate < 0.95, acc_rate
    assert tg[0][-1].std(axis=0).min() > 0
    np.testing.assert_allclose(gpu_engine.get_state()[3][same], cpu_engine.get_state()[3][same], rtol=1e-6)


def test_float32_solve_tolerance(pkg, oracle_mod):
    """BASELINE config 5 ("float32 vs float64 tolerance sweep"): the float32 ODE solve against the float64 one."""
    rng = np.random.default_rng(8)
    for n, tol_ssq, tol_traj in ((500, 1e-3, 2e-3), (4000, 1e-3, 2e-3)):
        m64, m32 = _models(oracle_mod, n), _models(oracle_mod, n)
        m32.precision = "float32"
        C = 500
        dc = rng.uniform(100.0, 9000.0, C)
        a = rng.uniform(0.008, 0.016, C)
        b = a + rng.uniform(0.0, 0.008, C)
        with pkg.Engine(mem="host") as e64, pkg.Engine(mem="host") as e32:
            e64.set_model(m64, 1)
            e32.set_model(m32, 1)
            data = synthetic_data(e64)
            s64, a64 = e64.forward(dc, a=a, b=b, data=data, want_ssq=True, want_acc=True)
            s32, a32 = e32.forward(dc, a=a, b=b, data=data, want_ssq=True, want_acc=True)
            assert not np.array_equal(a32, a64)                       # it really is a different arithmetic
            assert _traj_err(a32, a64) < tol_traj
            np.testing.assert_allclose(s32, s64, rtol=tol_ssq)
            if n == 500:                                              # sampler on top of the float32 solve
                q0 = np.full((256, 1), 1000.0)
                out = {}
                for name, e in (("f64", e64), ("f32", e32)):
                    e.mcmc_init(q0, data, [0.0], [1e4], seed=3, prior_len=3)
                    tq, _, ta = e.mcmc_run(60, traces=("q", "accept"))
                    out[name] = (tq[30:].mean(), tq[30:].std(), ta.mean())
                assert abs(out["f32"][0] - out["f64"][0]) < 0.25 * out["f64"][1]
                assert abs(out["f32"][2] - out["f64"][2]) < 0.05


@pytest.mark.parametrize("n,substeps,damping", [(500, 1, True), (4000, 1, True), (500, 2, False)])
def test_float32_solve_against_the_float32_restatement(pkg, oracle_lib, oracle_mod, n, substeps, damping):
    """The float32 kernel against an INDEPENDENT float32 checker: oracle/rsf_oracle.c restates the same float32 formulation in
    plain C `float` with libm's exp2f / log2f (RSF_FLAG_FP32_SOLVE), so the two differ only by the last-place behaviour of
    v_exp_f32 / v_log_f32 / v_rcp_f32 — amplified along the trajectory like any float32 rounding.  This pins every constant
    and term of the kernel two orders below the 1e-3 band of the float32-vs-float64 sweep (a mis-scaled constant that
    hid inside that band cannot hide here).  Measured on MI355X (round 3): SSq max 3.1e-8, median 3e-9, trajectories max
    3.6e-7 — asserted with a factor ~15."""
    rng = np.random.default_rng(80 + n)
    m32 = _models(oracle_mod, n, substeps, damping)
    m32.precision = "float32"
    C = 600
    dc = rng.uniform(100.0, 9000.0, C)
    a = rng.uniform(0.008, 0.016, C)
    b = a + rng.uniform(0.0, 0.008, C)
    with pkg.Engine(mem="host") as g32, pkg.Engine(lib=oracle_lib) as c32, pkg.Engine(lib=oracle_lib) as c64:
        for e in (g32, c32):
            e.set_model(m32, substeps)
        m32.precision = "float64"
        c64.set_model(m32, substeps)
        data = synthetic_data(c64)
        sg, ag = g32.forward(dc, a=a, b=b, data=data, want_ssq=True, want_acc=True)
        sc, ac = c32.forward(dc, a=a, b=b, data=data, want_ssq=True, want_acc=True)
        s64, a64 = c64.forward(dc, a=a, b=b, data=data, want_ssq=True, want_acc=True)
    e_ssq, e_traj = np.abs(sg / sc - 1), np.abs(ag - ac).max(axis=0) / np.abs(ac).max(axis=0)
    band = np.abs(sc / s64 - 1)
    print(f"float32 GPU vs float32 restatement, nsteps {n} S {substeps}: SSq max {e_ssq.max():.2e} median {np.median(e_ssq):.2e}; "
          f"trajectory max {e_traj.max():.2e}; restatement vs float64: SSq max {band.max():.2e}")
    assert np.isfinite(sg).all() and np.isfinite(sc).all()
    assert not np.array_equal(ac, a64)            # the restatement really is a different arithmetic from the float64 one
    assert band.max() < 1e-3                      # ... inside the sweep's band
    assert e_ssq.max() < 5e-7 and np.median(e_ssq) < 5e-8
    assert e_traj.max() < 5e-6


@pytest.mark.parametrize("d,C,groups", [(1, 1000, 1), (3, 777, 1), (1, 2048, 2)])
def test_float32_sampler_two_chains_per_lane(pkg, oracle_lib, oracle_mod, d, C, groups):
    """The float32 sampler carries TWO chains per lane (mcmc_f32x2_kernel: every instruction of its solve is a packed pair).
    (a) Exactness of the packed form: after a run, the SSq the sampler holds for each chain's current point is BIT-identical
    to what the one-chain float32 forward kernel computes for that point (same arithmetic, IEEE per half), chain counts that
    leave the second slot partly / wholly empty, d = 1 and 3, one and two observation groups.  (b) The chains against the
    float32 restatement run as a sampler on the CPU with the same Philox stream: accept decisions may differ only where
    the two SSq — equal to ~3e-8 — straddle a decision, so at least 99.5 % of the chains must be identical in every decision,
    and those agree in q to 1e-9 and in sigma^2 to 1e-6."""
    rng = np.random.default_rng(100 + C)
    m = _models(oracle_mod, 500)
    m.precision = "float32"
    q0 = np.column_stack([rng.uniform(500.0, 2500.0, C), rng.uniform(0.010, 0.012, C), rng.uniform(0.013, 0.015, C)])[:, :d]
    lo, hi = [0.0, 0.005, 0.005][:d], [1.0e4, 0.02, 0.03][:d]
    V0 = np.tile(np.diag(np.array([25.0 ** 2, 1e-4 ** 2, 1e-4 ** 2][:d])), (C, 1, 1))
    n_iters = 12
    with pkg.Engine(mem="host") as g, pkg.Engine(lib=oracle_lib) as c:
        for e in (g, c):
            e.set_model(m, 1)
        m64 = _models(oracle_mod, 500)
        with pkg.Engine(lib=oracle_lib) as c64:
            c64.set_model(m64, 1)
            base = synthetic_data(c64)
        data = base if groups == 1 else np.stack([base, base * 1.1])
        for e in (g, c):
            # (d = 3 without adaptation: a covariance estimated from a 4-sample window in three dimensions is near-singular and
            #  amplifies rounding differences of the host arithmetic into different proposals — not what this test is about)
            e.mcmc_init(q0, data, lo, hi, seed=5, prior_len=3 if d == 1 else 0, adapt_mode="am" if d == 1 else "none", adapt_interval=4)
        state0 = list(c.get_state())
        state0[3] = V0
        for e in (g, c):
            e.set_state(*state0)
        tg, tc = g.mcmc_run(n_iters), c.mcmc_run(n_iters)
        # (a) the state's SSq is the float32 forward solve at the state's point, bit for bit
        q, ssq, _, _ = g.get_state()
        per = C // groups
        for grp in range(groups):
            sl = slice(grp * per, (grp + 1) * per)
            f, _ = g.forward(q[sl, 0], a=q[sl, 1] if d == 3 else None, b=q[sl, 2] if d == 3 else None,
                             data=data if groups == 1 else data[grp], want_ssq=True, want_acc=False)
            moved = tg[2][:, sl].any(axis=0)  # chains that accepted at least once hold an SSq computed by the packed solve
            assert moved.sum() > per // 2
            np.testing.assert_array_equal(ssq[sl][moved], f[moved])
    # (b) against the float32 restatement's chains
    same = (tg[2] == tc[2]).all(axis=0)
    print(f"float32 sampler vs float32 restatement: {int((~same).sum())} of {C} chains differ in a decision")
    assert same.mean() >= 0.995
    np.testing.assert_allclose(tg[0][:, same], tc[0][:, same], rtol=1e-9)
    np.testing.assert_allclose(tg[1][:, same], tc[1][:, same], rtol=1e-6)


@pytest.mark.parametrize("damping", [True, False])
def test_float32_step_forms_mixed_in_one_wave(pkg, oracle_lib, oracle_mod, damping):
    """The float32 solve's two step forms (csrc/rsf_device_f32.h): a chain integrates incrementally — no transcendental
    function; in the sampler as scheduled assembly over a private register file (rsf_f32_trip.inc) — until one of its own
    steps leaves the guard, and by full evaluations from that step on.  Chains of every kind side by side: Dc from 8 (full
    evaluations from the first step) over 60 and 130 (switching somewhere along the series, as the loading's amplitude has
    it) to 3000, in a 7-cycle over the chain index, so that every wave holds all kinds and the two chains of a lane differ
    (replayed trips, waves running both forms).
    (a) one-chain forward kernel (compiled C++) against the restatement: where the chain stays incremental the two execute
        the same IEEE operations — trajectories and SSq BIT-identical; elsewhere the hardware transcendentals' last place
        shows (5e-7 / 5e-6 as in test_float32_solve_against_the_float32_restatement for Dc >= 100; the stiff kinds below, where
        no earlier test went, amplify it: 5e-5 / 5e-4, measured 3e-6 on SSq);
    (b) the sampler (assembly trip, two chains per lane): the SSq it holds for a chain's point is bit-identical to the
        one-chain forward kernel's at that point, for every kind of chain;
    (c) the sampler's chains against the restatement run as a sampler: same decisions in >= 99 % of the chains."""
    n, C = 500, 1792
    m = _models(oracle_mod, n, 1, damping)   # (both variants of the generated trip: with and without the radiation damping pass)
    m.precision = "float32"
    kinds = np.array([8.0, 1200.0, 60.0, 3000.0, 130.0, 500.0, 25.0])
    rng = np.random.default_rng(21)
    dc0 = kinds[np.arange(C) % 7] * rng.uniform(0.9, 1.1, C)
    with pkg.Engine(mem="host") as g, pkg.Engine(lib=oracle_lib) as c, pkg.Engine(lib=oracle_lib) as c64:
        for e in (g, c):
            e.set_model(m, 1)
        c64.set_model(_models(oracle_mod, n, 1, damping), 1)
        data = synthetic_data(c64)
        # (a)
        sg, ag = g.forward(dc0, data=data, want_ssq=True, want_acc=True)
        sc, ac = c.forward(dc0, data=data, want_ssq=True, want_acc=True)
        sg, ag, sc, ac = np.asarray(sg), np.asarray(ag), np.asarray(sc), np.asarray(ac)
        calm = dc0 > 400.0                        # a-priori incremental throughout at this step size (|dlt| < 2^-7 needs Dc a > 1.3)
        exact = (ag == ac).all(axis=0) & (sg == sc)
        print(f"float32 forward, GPU vs restatement: {int(exact.sum())} of {C} chains bit-identical ({int(exact[calm].sum())} of {int(calm.sum())} with Dc > 400)")
        assert exact[calm].all()
        assert not exact[dc0 < 30.0].all()        # the full-evaluation form really runs: its last place differs somewhere
        fin = np.isfinite(sc)
        assert (np.isfinite(sg) == fin).all() and fin.sum() > 0.8 * C
        e_ssq, e_traj = np.abs(sg / sc - 1), np.abs(ag - ac).max(axis=0) / np.abs(ac).max(axis=0)
        stiff = dc0 < 100.0  # full evaluations from early on, and a stiff problem: the transcendentals' last place is amplified
        print("  per kind (Dc: SSq, trajectory): " + "; ".join(
            f"{kd:g}: {e_ssq[fin & (np.abs(dc0 / kd - 1) < 0.11)].max():.1e}, {e_traj[fin & (np.abs(dc0 / kd - 1) < 0.11)].max():.1e}" for kd in kinds))
        assert e_ssq[fin & ~stiff].max() < 5e-7 and e_traj[fin & ~stiff].max() < 5e-6
        assert e_ssq[fin & stiff].max() < 5e-5 and e_traj[fin & stiff].max() < 5e-4
        # (b), (c)
        q0 = dc0[:, None]
        for e in (g, c):
            e.mcmc_init(q0, data, [0.0], [1.0e4], seed=5, prior_len=3, adapt_mode="none")
        state0 = list(c.get_state())
        state0[3] = ((0.02 * dc0) ** 2)[:, None, None]
        for e in (g, c):
            e.set_state(*state0)
        tg, tc = g.mcmc_run(10), c.mcmc_run(10)
        q, ssq, _, _ = g.get_state()
        f, _ = g.forward(q[:, 0], data=data, want_ssq=True, want_acc=False)
        moved = tg[2].any(axis=0)
        for kd in kinds:
            sel = moved & (np.abs(dc0 / kd - 1) < 0.11)
            assert sel.sum() > 20, (kd, int(sel.sum()))
            np.testing.assert_array_equal(ssq[sel], f[sel])
    same = (tg[2] == tc[2]).all(axis=0)
    print(f"float32 sampler, mixed forms, vs restatement: {int((~same).sum())} of {C} chains differ in a decision")
    assert same.mean() >= 0.99
    np.testing.assert_allclose(tg[0][:, same], tc[0][:, same], rtol=1e-9)


@pytest.mark.parametrize("d,substeps", [(1, 1), (3, 1), (1, 2)])
def test_float32_replay_of_given_variates(pkg, oracle_lib, oracle_mod, d, substeps):
    """The float32 sampler fed its variates by the caller (rsf_mcmc_replay: the REPLAY instantiation of mcmc_f32x2_kernel, which
    the public sub-methods run on) — the same assembly trip, the chain logic on replayed normals, uniforms and gamma variates:
    against the restatement replaying the same variates every decision is the same and the samples agree to 1e-9, chain counts
    that leave a lane's second slot empty, one iteration at a time as well as in one call.  With two RK4 steps per output
    interval no step belongs to a trip: the two-chain form goes step by step throughout (step_any, compiled code)."""
    m = _models(oracle_mod, 500, substeps)
    m.precision = "float32"
    rng = np.random.default_rng(33 + d)
    C, n = 333, 9
    z, u, g = rng.standard_normal((n, C, d)), rng.uniform(size=(n, C)), rng.gamma(250.005, size=(n, C))
    q0 = np.column_stack([rng.uniform(600.0, 2000.0, C), rng.uniform(0.010, 0.012, C), rng.uniform(0.013, 0.015, C)])[:, :d]
    lo, hi = [0.0, 0.005, 0.005][:d], [1.0e4, 0.02, 0.03][:d]
    V0 = np.tile(np.diag(np.array([25.0 ** 2, 1e-4 ** 2, 1e-4 ** 2][:d])), (C, 1, 1))
    with pkg.Engine(mem="host") as gpu, pkg.Engine(lib=oracle_lib) as cpu, pkg.Engine(lib=oracle_lib) as c64:
        c64.set_model(_models(oracle_mod, 500, substeps), substeps)
        data = synthetic_data(c64)
        for e in (gpu, cpu):
            e.set_model(m, substeps)
            e.mcmc_init(q0, data, lo, hi, seed=1, prior_len=3 if d == 1 else 0, adapt_mode="none")
        st = list(cpu.get_state())
        st[3] = V0
        for e in (gpu, cpu):
            e.set_state(*st)
        tg, tc = gpu.mcmc_replay(z, u, g), cpu.mcmc_replay(z, u, g)
        np.testing.assert_array_equal(tg[2], tc[2])
        np.testing.assert_allclose(tg[0], tc[0], rtol=1e-9)
        np.testing.assert_allclose(tg[1], tc[1], rtol=1e-6)
        assert 0.05 < tg[2].mean() < 0.98
        gpu.set_state(*st)           # the same again, one iteration per call (the hipGraph path of a one-proposal replay)
        rows = [gpu.mcmc_replay(z[k:k + 1], u[k:k + 1], g[k:k + 1]) for k in range(n)]
        np.testing.assert_array_equal(np.concatenate([r[0] for r in rows]), tg[0])
        np.testing.assert_array_equal(np.concatenate([r[2] for r in rows]), tg[2])


def test_float32_sampler_is_exact_at_config5_shape(pkg, oracle_mod):
    """The packed two-chains-per-lane solve at BASELINE configs[4]'s own per-GPU shape (131 072 chains, nsteps 4000, joint
    (Dc, a, b): two LDS chunks per solve): after three proposals every chain's SSq is bit-identical to the one-chain float32
    forward kernel at the chain's current point — 131 072 of 131 072."""
    import torch

    C, n = 131072, 4000
    m = _models(oracle_mod, n)
    m.precision = "float32"
    rng = np.random.default_rng(9)
    q0 = np.column_stack([rng.uniform(500.0, 2500.0, C), rng.uniform(0.010, 0.012, C), rng.uniform(0.013, 0.015, C)])
    with pkg.Engine(mem="device") as e, pkg.Engine(mem="host") as h:
        h.set_model(_models(oracle_mod, n), 1)
        data = synthetic_data(h)
        e.set_model(m, 1)
        e.mcmc_init(q0, data, [0.0, 0.005, 0.005], [1.0e4, 0.02, 0.03], seed=11, adapt_mode="none")
        e.set_state(V=torch.diag(torch.tensor([20.0 ** 2, 1e-4 ** 2, 1e-4 ** 2], dtype=torch.float64, device="cuda")).repeat(C, 1, 1))
        _, _, ta = e.mcmc_run(3, traces=("accept",))
        q, ssq, _, _ = e.get_state()
        f, _ = e.forward(q[:, 0].contiguous(), a=q[:, 1].contiguous(), b=q[:, 2].contiguous(), data=data, want_ssq=True, want_acc=False)
        e.sync()
        assert float(ta.double().mean()) > 0.3 and bool(torch.isfinite(ssq).all())
        assert bool(torch.equal(ssq, f)), int((ssq != f).sum())


def test_float32_tolerance_at_config5_shape():
    """BASELINE configs[4] per-GPU shard (131 072 chains, nsteps 4000, joint (Dc, a, b)) in BOTH precisions, same seeds —
    tools/fp32_sweep_cfg5.py with a shorter sampler run.  Bands (profiles/r04/fp32_sweep_cfg5.json holds the 400-iteration
    numbers): relative |SSq32 - SSq64| <= 1e-4 on every lane (median <= 1e-6); posterior mean / std of each parameter move by less than
    0.02 / 0.02 float64 posterior standard deviations; acceptance rates within 0.01."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fp32_sweep_cfg5

    out = fp32_sweep_cfg5.sweep(iters=60)
    assert out["shape"] == {"chains": 131072, "nsteps": 4000, "n_params": 3, "iters": 60}
    assert out["ssq"]["nonfinite_f64"] == out["ssq"]["nonfinite_f32"] == 0 and out["ssq"]["lanes"] == 131072
    # (round 4, incremental float32 step: measured 2.6e-5 / 1.0e-7 — profiles/r04/fp32_sweep_cfg5.json; until then 1.2e-4 / 1.7e-6)
    assert out["ssq"]["rel_max"] < 1e-4 and out["ssq"]["rel_median"] < 1e-6, out["ssq"]
    post = out["posterior"]
    assert max(post["drift_in_units_of_f64_posterior_std"]["mean"]) < 0.02, post
    assert max(post["drift_in_units_of_f64_posterior_std"]["std"]) < 0.02, post
    assert post["accept_diff"] < 0.01 and 0.05 < post["float64"]["accept"] < 0.95
    assert post["float64"]["nonfinite"] == 0 and post["float32"]["nonfinite"] == 0


def test_replay_of_reference_variates(gpu_engine, golden, oracle_mod):
    """The reference's own recorded chain (tests/golden/replay_*.npz): feeding the GPU kernel the variates the
    reference consumed reproduces its accept decisions and samples up to the RK4-vs-dop853 difference."""
    for tag, S in (("list", 8), ("dict", 8), ("dict3", 8), ("tightbox", 8)):
        g, meta = golden.npz("replay_" + tag), golden.json("replay_" + tag)
        m = _models(oracle_mod, meta["nsteps"], S)
        gpu_engine.set_model(m, S)
        lo, hi = (meta["prior"][1], meta["prior"][2]) if isinstance(meta["prior"], list) else (meta["prior"]["1"], meta["prior"]["2"])
        gpu_engine.mcmc_init([[meta["qstart"]]], g["data"], [lo], [hi], prior_len=len(meta["prior"]),
                             adapt_mode="reference_dict" if meta["prior_is_dict"] else "none", adapt_interval=meta["adapt_interval"])
        q, ssq, std2, V = gpu_engine.get_state()
        np.testing.assert_allclose(std2[0], meta["std2_0"], rtol=1e-6)
        np.testing.assert_allclose(ssq[0], meta["ssq0"], rtol=1e-6)
        np.testing.assert_allclose(V[0, 0, 0], meta["vstart"], rtol=1e-4)
        gpu_engine.set_state(V=[[[meta["vstart"]]]], std2=[meta["std2_0"]], ssq=[meta["ssq0"]])
        n = len(g["z"])
        u = np.where(np.isnan(g["u"]), 1.0, g["u"])
        tq, ts, ta = gpu_engine.mcmc_replay(g["z"].reshape(n, 1, 1), u.reshape(n, 1), g["g"].reshape(n, 1))
        nb = meta["nburn"]
        np.testing.assert_allclose(tq[nb - 1:, 0, 0], g["qparams_kept"][0], rtol=1e-6)
        np.testing.assert_allclose(ts[nb - 1:, 0], g["std2_kept"], rtol=1e-5)


@pytest.mark.parametrize("C,n,d,iters,variant", [(65536, 500, 1, 5, "rk4"), (262144, 2000, 1, 2, "rk4"), (131072, 4000, 3, 1, "rk4"),
                                                 (65536, 500, 1, 3, "rk4_substeps2"), (65536, 500, 1, 2, "dop853")])
def test_full_size_configs_against_the_oracle(pkg, oracle_lib, oracle_mod, C, n, d, iters, variant):
    """Tier 1 AT the BASELINE shapes (configs[1], configs[2], one GPU's share of configs[4]): every chain of the full
    grid, HIP sampler vs the CPU oracle on the same Philox stream — accept flags, samples and sigma^2 of all C chains
    (rtol 1e-9; a fork only where proven a near-tie), plus SSq / log-likelihood of the end state.  The oracle needs
    about 1-25 s of the host's cores for each (OpenMP over chains).  Variants at the configs[1] shape: two RK4 steps per output
    interval, and the reference's own DOP853 scheme (the register-bounded sampler kernel with its spills, at scale)."""
    S = 2 if variant == "rk4_substeps2" else 1
    m = _models(oracle_mod, n, S)
    if variant == "dop853":
        m.integrator = "dop853"
    rng = np.random.default_rng(C + n)
    start = np.array([1000.0, 0.011, 0.014][:d])
    q0 = np.tile(start, (C, 1))
    q0[:, 0] = rng.uniform(400.0, 2500.0, C)   # chains spread over the posterior's neighbourhood and its far tails
    lo, hi = [0.0, 0.005, 0.005][:d], [1e4, 0.02, 0.03][:d]
    kw = dict(seed=2025, chain_offset=3 * C, prior_len=3 if d == 1 else 0)
    with pkg.Engine(mem="host") as gpu, pkg.Engine(lib=oracle_lib) as cpu:
        assert gpu.lib.rsf_backend() == b"hip-gfx950" and cpu.lib.rsf_backend() != b"hip-gfx950"
        for e in (gpu, cpu):
            e.set_model(m, S)
        data = synthetic_data(cpu)
        for e in (gpu, cpu):
            e.mcmc_init(q0, data, lo, hi, **kw)
        sg, sc = gpu.get_state(), cpu.get_state()
        np.testing.assert_allclose(sg[1], sc[1], rtol=RTOL)        # initial SSq of every chain (init kernel)
        np.testing.assert_allclose(sg[2], sc[2], rtol=RTOL)        # sigma^2_0
        state0 = list(sc)  # the checker's whole start state, its (prior-regularised, d = 3) proposal covariance included
        for e in (gpu, cpu):
            e.set_state(*state0)
        rerun = Rerun(type(cpu), cpu, q0, data, lo, hi, state0, kw)
        tg, tc = gpu.mcmc_run(iters), cpu.mcmc_run(iters)
        same = assert_chains_match(tg, tc, rerun)
        stg, stc = gpu.stats(), cpu.stats()
        # (d = 3 proposes from the init kernel's prior-wide covariance: part of the proposals leave the box on both sides alike)
        assert stg["evaluated"] == stc["evaluated"] and (d == 3 or stg["evaluated"] == iters * C) and stg["nonfinite"] <= stc["nonfinite"]
        assert abs(stg["accepted"] - stc["accepted"]) <= (~same).sum() * iters
        eg, ec = gpu.get_state(), cpu.get_state()
        np.testing.assert_allclose(eg[1][same], ec[1][same], rtol=RTOL)                                   # SSq
        np.testing.assert_allclose((-0.5 * eg[1] / eg[2])[same], (-0.5 * ec[1] / ec[2])[same], rtol=RTOL)  # log-likelihood
        assert 0.05 < tg[2].mean() < 0.98 and same.mean() > 0.999


@pytest.mark.parametrize("C,n,d,iters", [(65536, 500, 1, 5), (262144, 2000, 1, 2), (131072, 4000, 3, 1)])
def test_device_memory_path_and_full_size_properties(pkg, oracle_mod, C, n, d, iters):
    """BASELINE sizes (configs[1], configs[2], one GPU's share of configs[4]) with device-resident buffers,
    checked through size-independent properties: determinism, and shard invariance — splitting the chains
    into two ctxs by global chain id gives the identical pool (what makes the multi-GPU pool independent of
    the GPU count)."""
    import torch

    m = _models(oracle_mod, n)
    with pkg.Engine(mem="host") as e:
        e.set_model(m, 1)
        data = synthetic_data(e)
    start = [1000.0, 0.011, 0.014][:d]
    q0 = torch.tensor(start, dtype=torch.float64, device="cuda").repeat(C, 1)
    lo, hi = [0.0, 0.005, 0.005][:d], [1e4, 0.02, 0.03][:d]
    V0 = torch.diag(torch.tensor([20.0 ** 2, 1e-4 ** 2, 1e-4 ** 2][:d], dtype=torch.float64, device="cuda"))

    def run(off, cnt):
        with pkg.Engine(mem="device") as e:
            e.set_model(m, 1)
            e.mcmc_init(q0[off:off + cnt], data, lo, hi, seed=2025, chain_offset=off, prior_len=3 if d == 1 else 0)
            if d == 3:  # a small explicit proposal: this test wants every proposal inside the box (the init kernel's own,
                e.set_state(V=V0.repeat(cnt, 1, 1))  # prior-wide in two directions, is tested in test_three_parameter_chains)
            tq, ts, ta = e.mcmc_run(iters)
            e.sync()
            return tq.cpu().numpy(), ts.cpu().numpy(), ta.cpu().numpy(), e.stats()

    full = run(0, C)
    again = run(0, C)
    for k in range(3):
        np.testing.assert_array_equal(full[k], again[k])
    lo_half, hi_half = run(0, C // 2), run(C // 2, C // 2)
    for k in range(3):
        np.testing.assert_array_equal(np.concatenate([lo_half[k], hi_half[k]], axis=1), full[k])
    assert full[3]["evaluated"] == iters * C and full[3]["nonfinite"] == 0
    acc_rate = full[3]["accepted"] / (iters * C)
    assert 0.3 < acc_rate < 0.95
    assert np.isfinite(full[0]).all() and (full[1] > 0).all()
    assert full[0].shape == (iters, C, d)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_pool_collectives_through_rccl_one_rank(pkg, mem):
    """The C-ABI pool collectives with a REAL RCCL communicator (one rank — all a one-GPU box allows): the library
    binds RCCL at run time, creates the communicator on the ctx device and runs ncclAllGather / ncclAllReduce on the
    ctx stream.  Also the copy path (world = 1 without an id)."""
    import torch

    x = np.arange(5000.0).reshape(10, 500)
    for with_id in (True, False):
        with pkg.Engine(mem=mem) as e:
            uid = e.comm_unique_id() if with_id else None
            if with_id:
                assert len(uid) == 128 and any(uid)
            e.comm_init(1, 0, uid)
            xin = torch.from_numpy(x).cuda() if mem == "device" else x
            out = e.pool_allgather(xin)
            y = e.pool_allreduce_sum(torch.from_numpy(x).cuda() if mem == "device" else x.copy())
            e.sync()
            out = out.cpu().numpy() if mem == "device" else out
            y = y.cpu().numpy() if mem == "device" else y
            assert out.shape == (1, 10, 500)
            np.testing.assert_array_equal(out[0], x)
            np.testing.assert_array_equal(y, x)
            e.comm_destroy()
            with pytest.raises(pkg.RsfError, match="comm_init"):
                e.pool_allgather(xin)


# ---------------------------------------------------------------------------------------------
# round 4: the sampler as an operator over a caller-evaluated likelihood; launch counters; early rejection
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["list", "dict", "dict3", "tightbox"])
def test_likelihood_operator_replays_reference_exactly(gpu_engine, golden, tag):
    """SURVEY §8(c) G4/G5 on the HIP kernels: the reference's recorded variates AND sums of squares through
    rsf_mcmc_init_state / rsf_mcmc_propose / rsf_mcmc_replay_ssq — the device's accept rule, sigma^2 update, box test and
    adaptation quirks with NO integrator in the loop — reproduce the reference's chain to 1e-14 (sigma^2: 1e-13), in one call
    and one iteration per call.  (CPU twin on the checker: tests/test_oracle_golden.py.)"""
    import likelihood_operator as lo

    g, meta = golden.npz("replay_" + tag), golden.json("replay_" + tag)
    lo.replay_in_one_call(gpu_engine, g, meta)
    lo.replay_step_by_step(gpu_engine, g, meta)
    import bayesian_markov_chain_monte_carlo_amd as pkg

    with pytest.raises(pkg._abi.RsfError):  # no observation behind such chains: the solving entry points refuse them
        gpu_engine.mcmc_run(1)


def test_likelihood_operator_three_parameters_and_many_chains(gpu_engine, cpu_engine):
    """The same operator for d = 3 and a few thousand chains with adaptation on, GPU against the checker, from random states
    and random supplied sums of squares: proposals bit-comparable (1e-15), chains equal.  (Windows of 12 samples at ~75 %
    acceptance: a three-parameter window with fewer than four distinct points has a singular covariance, and whether its
    Cholesky factorisation "exists" is then decided by the last bit — legitimately differently on the two sides.)"""
    rng = np.random.default_rng(5)
    C, d, n = 3000, 3, 25
    q = np.column_stack([rng.uniform(700, 1300, C), rng.uniform(0.008, 0.015, C), rng.uniform(0.01, 0.02, C)])  # inside the box
    A = rng.standard_normal((C, d, d)) * np.array([20.0, 1e-4, 1e-4])[None, :, None]
    V = A @ A.transpose(0, 2, 1) + np.diag([1.0, 1e-10, 1e-10])[None]
    ssq, std2 = rng.uniform(1e-3, 2e-3, C), rng.uniform(1e-6, 2e-6, C)
    # gamma variates of shape 25: sigma^2 = 0.5 (n0 sigma^2 + SSq) / g stays ~3e-5, the log ratios of the supplied sums O(1), and
    # the chains keep moving — with the usual shape (~250) a chain that once accepted a low sum rejects everything after it
    z, u, g = rng.standard_normal((n, C, d)), rng.uniform(size=(n, C)), rng.gamma(25.0, size=(n, C))
    sn = ssq[None, :] * rng.uniform(0.97, 1.01, (n, C))
    res = []
    for e in (gpu_engine, cpu_engine):
        e.mcmc_init_state(q, ssq, std2, V, [600.0, 0.005, 0.005], [1400.0, 0.02, 0.03], adapt_mode="am", adapt_interval=12)
        qn, inb = e.mcmc_propose(z[0])
        tq, ts, ta = e.mcmc_replay_ssq(z, u, g, sn)
        res.append((np.asarray(qn), np.asarray(inb), np.asarray(tq), np.asarray(ts), np.asarray(ta), e.counters(), [np.asarray(x) for x in e.get_state()]))
    (qn_g, inb_g, tq_g, ts_g, ta_g, c_g, st_g), (qn_c, inb_c, tq_c, ts_c, ta_c, c_c, st_c) = res
    np.testing.assert_allclose(qn_g, qn_c, rtol=1e-15)
    assert np.array_equal(inb_g, inb_c) and 0 < inb_g.sum() < C
    # chains whose two adaptation windows each hold at least five accepted moves: the covariance of fewer than four distinct
    # points in three dimensions is singular, and which side of zero its last Cholesky pivot falls is then rounding's call
    ok = (ta_c[:12].sum(axis=0) >= 5) & (ta_c[12:24].sum(axis=0) >= 5)
    assert ok.mean() > 0.97, ok.mean()
    assert np.array_equal(ta_g[:, ok], ta_c[:, ok]) and 0.4 < ta_g.mean() < 0.95
    np.testing.assert_allclose(tq_g[:, ok], tq_c[:, ok], rtol=1e-9)
    np.testing.assert_allclose(ts_g[:, ok], ts_c[:, ok], rtol=1e-12)
    # the first window's chains are identical on both sides whatever comes later
    assert np.array_equal(ta_g[:12], ta_c[:12])
    np.testing.assert_allclose(tq_g[:12], tq_c[:12], rtol=1e-12)
    assert c_g["evaluated"] + c_g["out_of_bounds"] == n * C and c_g["wave_solves"] == 0 and c_g["steps_tight"] == 0
    if ok.all():
        for k in ("accepted", "evaluated", "out_of_bounds", "nonfinite"):
            assert c_g[k] == c_c[k], k
    for a, b in zip(st_g, st_c):
        np.testing.assert_allclose(a[ok], b[ok], rtol=1e-6)


def test_dict_prior_adaptation_is_numpys_covariance_to_the_bit_that_matters(pkg, gpu_engine):
    """rsf::np_cov_1d on the device against NumPy itself (CPU twin on the checker: tests/test_oracle_golden.py)."""
    import likelihood_operator as lo

    lo.adapt_matches_numpy_on_degenerate_windows(pkg, gpu_engine, trials=300)


def test_duck_typed_model_reproduces_the_reference_chain(pkg, golden):
    """MCMC(model=<any object with .Dc and .evaluate()>).sample() — the reference's model contract (MCMC.py:65-66, 127,
    381-384) — with the chain steps on the GPU and the model evaluated on the host where the reference evaluates it: the chain
    the REFERENCE's own sampler produced on tests/duck_model.DecayModel under the same seed (list prior, dict prior with its
    adaptation quirk, a tight box with out-of-bounds proposals), and as many model calls."""
    import likelihood_operator as lo

    for case in golden.json("duck_model")["cases"]:
        qp, std2, vstart, calls, g = lo.duck_model_chain(pkg, golden, case)
        tag = case["tag"]
        assert qp.shape == g[f"{tag}_qparams"].shape and calls == case["model_calls"]
        np.testing.assert_allclose(vstart, g[f"{tag}_vstart"], rtol=1e-12)
        np.testing.assert_allclose(qp, g[f"{tag}_qparams"], rtol=1e-13, err_msg=tag)
        np.testing.assert_allclose(std2, g[f"{tag}_std2"], rtol=1e-12, err_msg=tag)


def _wide_proposal_problem(engine, oracle_mod, C, dc_true=100.0, n=500, seed=11):
    engine.set_model(oracle_mod.ModelSpec(n), 1)
    _, acc = engine.forward([dc_true])
    acc = np.asarray(acc)[:, 0]
    return acc + np.abs(acc) * np.random.default_rng(seed).standard_normal(acc.shape[0])


def test_wide_proposals_against_the_oracle_with_counters(gpu_engine, cpu_engine, oracle_mod):
    """The reference's own main.py situation (main.py:50-56: qstart 1000 against a true Dc of 100, list prior, no adaptation): a
    proposal as wide as Vstart throws four in ten outside the box and spreads the rest over every integration tier down to
    stiff small-Dc lanes.  Every chain against the oracle (zero unproven forks), and the counters: the chain-level ones equal
    the oracle's, the wave-level ones are consistent — early rejection happened, every tier was visited, stiff lanes were
    integrated in the full-evaluation tier instead of fast-then-cold on every trip."""
    C, iters = 2048, 12
    data = _wide_proposal_problem(gpu_engine, oracle_mod, C)
    cpu_engine.set_model(oracle_mod.ModelSpec(500), 1)
    q0 = np.random.default_rng(3).uniform(60.0, 1500.0, (C, 1))
    kw = dict(seed=77, prior_len=3)
    for e in (gpu_engine, cpu_engine):
        e.mcmc_init(q0, data, [0.0], [1e4], **kw)
    state0 = [np.array(x) for x in cpu_engine.get_state()]
    state0[3] = np.full_like(state0[3], 600.0 ** 2)  # the width main.py's Vstart has at qstart 1000 (sqrt(Vstart) ~ 647)
    for e in (gpu_engine, cpu_engine):
        e.set_state(*state0)
    rerun = Rerun(type(cpu_engine), cpu_engine, q0, data, [0.0], [1e4], state0, kw)
    tg, tc = gpu_engine.mcmc_run(iters), cpu_engine.mcmc_run(iters)
    assert_chains_match(tg, tc, rerun)
    cg, cc = gpu_engine.counters(), cpu_engine.counters()
    for k in ("accepted", "evaluated", "out_of_bounds"):
        assert cg[k] == cc[k], (k, cg[k], cc[k])
    assert cg["evaluated"] + cg["out_of_bounds"] == C * iters and cg["out_of_bounds"] > 0.25 * C * iters
    assert cg["nonfinite"] <= cc["nonfinite"]  # a lane rejected early never reaches the point where its series blows up
    assert cg["early_rejected"] > 0.3 * cg["evaluated"] and cc["early_rejected"] == 0
    # lanes run ahead over their out-of-bounds proposals (kProposalTries), so a wave needs FEWER solves than iterations
    assert 0.5 * (C // 64) * iters < cg["wave_solves"] + cg["wave_skips"] < (C // 64) * iters
    steps = cg["steps_tight"] + cg["steps_narrow"] + cg["steps_wide"] + cg["steps_full"]
    assert steps <= cg["wave_solves"] * 499 and cg["steps_full"] > 0 and cg["steps_wide"] > 0
    assert 0.0 < cg["lane_utilisation"] <= 1.0
    # stiff lanes are integrated in the FULL tier: the incremental trips thrown away stay a small share of the work
    assert cg["steps_redone"] < 0.15 * steps, cg
    print("wide-proposal counters:", cg)


def test_early_rejection_changes_nothing_observable(pkg, oracle_mod, golden):
    """The same chains on the round-3 build of this library (rsf_build_id() 96c179e837e4be05: no early rejection, tier decided
    by a wave's worst lane for the whole solve) and on this one: every accept flag and every sample bit-identical — the RNG is
    keyed by the chain id and a rejected proposal leaves nothing behind — and sigma^2 equal to rounding (it sees the accepted
    proposals' sums of squares, whose last bits depend on the tier that integrated them).  Headline-like all-TIGHT chains
    and the wide-proposal mix.  The round-3 run is stored in tests/golden/round3_chains.npz (tools/capture_round3_chains.py,
    from the start state this library gave): its accept flags, the SHA-256 of its sample trace, and its sigma^2 trace for
    a fixed sample of the chains."""
    import hashlib

    g = golden.npz("round3_chains")
    for case, wide in (("tight", False), ("wide", True)):
        C, iters, n = 8192, 30, 500
        with pkg.Engine(mem="host") as e:
            data = _wide_proposal_problem(e, oracle_mod, C, dc_true=100.0 if wide else 1000.0)
            q0 = np.random.default_rng(3).uniform(60.0, 1500.0, (C, 1)) if wide else np.full((C, 1), 1000.0)
            e.mcmc_init(q0, data, [0.0], [1e4], seed=4242, prior_len=3)
            # the round-3 run's start state (the init kernels are not under test here)
            e.set_state(*(g[f"{case}_start_{k}"] for k in ("q", "ssq", "std2", "V")))
            tq_n, ts_n, ta_n = (np.asarray(x) for x in e.mcmc_run(iters))
        ta_o = np.unpackbits(g[f"{case}_accept_bits"], axis=1, count=C).astype(ta_n.dtype)
        # The round-3 build ACCEPTED a proposal whose sum of squares was NaN (fmin(NaN, 0) = 0 > log u: see accept_test in
        # rsf_kernel_common.h) — a stiff Dc < 0.35 proposal under fixed-step RK4 — and such a chain then accepts everything.  Those
        # chains are that build's bug, not a difference to explain: they show as a non-finite sigma^2 there, are few, are
        # finite here, and are left out of the comparison.
        bugged = np.unpackbits(g[f"{case}_nonfinite_bits"], count=C).astype(bool)
        assert np.isfinite(ts_n).all() and np.isfinite(tq_n).all()
        assert bugged.sum() <= (0.01 * C if wide else 0), f"{bugged.sum()} chains of the old build went non-finite (wide={wide})"
        ok = ~bugged
        assert np.array_equal(ta_n[:, ok], ta_o[:, ok]), f"accept flags differ (wide={wide}): {(ta_n[:, ok] != ta_o[:, ok]).sum()} of {ta_n[:, ok].size}"
        digest = hashlib.sha256(np.ascontiguousarray(tq_n[:, ok], dtype=np.float64).tobytes()).digest()
        assert digest == g[f"{case}_q_sha256"].tobytes(), f"samples differ (wide={wide})"
        cols = np.sort(np.random.default_rng(0).choice(C, g[f"{case}_std2_sample"].shape[1], replace=False))
        keep = ok[cols]
        np.testing.assert_allclose(ts_n[:, cols[keep]], g[f"{case}_std2_sample"][:, keep], rtol=1e-11)
        print(f"old vs new build (wide={wide}): {ok.sum()} chains bit-identical in q and accept; {bugged.sum()} chains of the old build NaN-accepted")


def test_nonfinite_sum_of_squares_is_rejected(gpu_engine, cpu_engine, oracle_mod):
    """MCMC.py:327-331: np.clip keeps a NaN and NaN > log u is False — a proposal whose series blew up is rejected, however
    small the uniform.  Dc = 0.13 under fixed-step RK4 at nsteps 500 is such a proposal (NaN/Inf for Dc <= 0.35).
    Until round 4 the kernel clamped with fmin(., 0), which turns NaN into 0 > log u: accepted.  Replayed variates aim
    every chain at Dc = 0.13 with a uniform that would accept any finite sum; GPU and oracle must both stay where they were."""
    m = _models(oracle_mod, 500)
    C = 192
    q0 = np.linspace(40.0, 90.0, C).reshape(C, 1)
    res = []
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
        if not res:
            data = synthetic_data(cpu_engine if e is cpu_engine else gpu_engine, dc_true=60.0)
        e.mcmc_init(q0, data, [0.0], [1e4], seed=1, prior_len=3)
        V = np.full((C, 1, 1), 25.0)
        e.set_state(V=V)
        z = ((0.13 - q0) / 5.0).reshape(1, C, 1)      # q + sqrt(V) z = 0.13
        u = np.full((1, C), 1e-300)                   # log u = -690: any finite ratio passes
        g = np.full((1, C), 250.0)
        tq, ts, ta = e.mcmc_replay(z, u, g)
        res.append((np.asarray(tq), np.asarray(ta), e.counters(), np.asarray(e.get_state()[1])))
    for tq, ta, cnt, ssq in res:
        assert not ta.any() and np.array_equal(tq[0, :, 0], q0[:, 0]) and np.isfinite(ssq).all()
        assert cnt["evaluated"] == C and cnt["accepted"] == 0
    assert res[1][2]["nonfinite"] == C  # the oracle integrates every series to its (non-finite) end
