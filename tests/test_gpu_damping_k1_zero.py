"""
Radiation damping switched on with k1 = 0.  The float64 RK4 kernels carry W = kvk w (kvk = k1 V_ref / a) in place of
w = v / V_ref inside their incremental tiers, which is undefined at k1 = 0; the host then launches the instantiation
without the damping pass, an exact identity at k1 = 0.  Checked against the CPU oracle, which runs the pass as written,
and against the GPU run with damping switched off.
"""
import numpy as np
import pytest

from chain_parity import RTOL, Rerun, assert_chains_match
from conftest import synthetic_data

pytestmark = pytest.mark.gpu


def _model(oracle_mod, n, substeps, damping):
    m = oracle_mod.ModelSpec(n, 0.0, 50.0, substeps)
    m.RadiationDamping = damping
    m.k1 = 0.0
    return m


def _traj_err(a, b):
    scale = np.abs(b).max(axis=0)
    return (np.abs(a - b).max(axis=0) / scale).max()


@pytest.mark.parametrize("n,substeps", [(500, 1), (500, 3)])
def test_forward_with_damping_on_and_k1_zero(gpu_engine, cpu_engine, oracle_mod, n, substeps):
    rng = np.random.default_rng(11 + substeps)
    C = 203
    dc = rng.uniform(50.0, 9000.0, C)
    dc[:4] = [6.0, 100.0, 1000.0, 9999.0]  # Dc = 6: the wide and full-evaluation tiers as well
    a = rng.uniform(0.008, 0.016, C)
    b = a + rng.uniform(-0.004, 0.008, C)
    m = _model(oracle_mod, n, substeps, True)
    for e in (gpu_engine, cpu_engine):
        assert e.set_model(m, substeps) == m.nout
    data = synthetic_data(cpu_engine)
    for kw in (dict(), dict(a=a, b=b)):
        sg, ag = gpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True, **kw)
        sc, ac = cpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True, **kw)
        assert np.isfinite(ag).all() and np.isfinite(sg).all()
        assert _traj_err(ag, ac) < RTOL
        np.testing.assert_allclose(sg, sc, rtol=RTOL)
        # the same kernel as with damping off: the same bits
        gpu_engine.set_model(_model(oracle_mod, n, substeps, False), substeps)
        s0, a0 = gpu_engine.forward(dc, data=data, want_ssq=True, want_acc=True, **kw)
        gpu_engine.set_model(m, substeps)
        np.testing.assert_array_equal(sg, s0)
        np.testing.assert_array_equal(ag, a0)


@pytest.mark.parametrize("d", [1, 3])
def test_sampler_with_damping_on_and_k1_zero(gpu_engine, cpu_engine, oracle_mod, d):
    m = _model(oracle_mod, 500, 1, True)
    for e in (gpu_engine, cpu_engine):
        e.set_model(m, 1)
    data = synthetic_data(cpu_engine)
    C = 300
    rng = np.random.default_rng(3)
    q0 = np.column_stack([rng.uniform(600.0, 2000.0, C), rng.uniform(0.010, 0.013, C), rng.uniform(0.013, 0.016, C)])[:, :d]
    lo, hi = [0.0, 0.005, 0.005][:d], [1e4, 0.02, 0.03][:d]
    kw = dict(seed=2025, prior_len=3 if d == 1 else 0)
    for e in (gpu_engine, cpu_engine):
        e.mcmc_init(q0, data, lo, hi, **kw)
    # the init kernel against the checker, then both chains from the checker's start state
    np.testing.assert_allclose(gpu_engine.get_state()[1], cpu_engine.get_state()[1], rtol=RTOL)
    state0 = cpu_engine.get_state()
    gpu_engine.set_state(*state0)
    rerun = Rerun(type(cpu_engine), cpu_engine, q0, data, lo, hi, state0, kw)
    assert_chains_match(gpu_engine.mcmc_run(15), cpu_engine.mcmc_run(15), rerun)
