"""
GPU tests: every sampler kernel against its exact target, computed by quadrature (tests/posterior_reference.py).

Test in stationarity: each chain's start (q, sigma^2) is drawn from the target pi, the kernel runs, and the chains' states
must still be distributed as pi — at iteration 0 (which validates the draws) and at two later checkpoints, each its own
mcmc_run call so that the launch continuation is part of what is tested.  Chains are independent, so every standard error
is exact: no burn-in, no autocorrelation estimate.  A kernel that is subtly wrong drifts towards its own wrong target.

Every leg uses n0 = 0, where one iteration is an exact Metropolis-within-Gibbs step for
pi(q) ~ 1_box(q) SSq(q)^(-shape); the target of each kernel is integrated over the SSq of the checker's restatement of its
own solve (float64, float32 or DOP853).  Production legs take the kernel's own ssq0 from get_state() and draw
sigma^2 ~ InvGamma(shape, ssq0 / 2) with NumPy.  Seeds are fixed; thresholds (posterior_reference.Z_MAX, KS_MAX) come from
the false-alarm probability alone (~1e-5 per check).
"""
import numpy as np
import pytest

import posterior_reference as R
from conftest import synthetic_data

pytestmark = pytest.mark.gpu

BOX1 = (0.0, 1.0e4)
LO3, HI3 = [0.0, 0.005, 0.005], [1.0e4, 0.02, 0.03]
_REFS = {}


def _model(pkg, nsteps=500, damping=True, precision="float64", integrator="rk4"):
    m = pkg.RateStateModel(number_time_steps=nsteps)
    m.RadiationDamping, m.precision, m.integrator = damping, precision, integrator
    return m


def _data(pkg, cpu_engine, nsteps):
    cpu_engine.set_model(_model(pkg, nsteps), 1)
    return synthetic_data(cpu_engine)


def _reference(pkg, cpu_engine, d, lo, hi, **model_kw):
    """the target of the kernel that integrates with model_kw, over the checker's SSq (cached for the module)"""
    key = (d, tuple(np.ravel(lo)), tuple(np.ravel(hi)), tuple(sorted(model_kw.items())))
    if key not in _REFS:
        nsteps = model_kw.get("nsteps", 500)
        data = _data(pkg, cpu_engine, nsteps)
        cpu_engine.set_model(_model(pkg, **model_kw), 1)
        fn = R.checker_ssq(cpu_engine, data)
        ref = R.Posterior1(fn, lo, hi, 0.5 * data.size) if d == 1 else R.Posterior3(fn, lo, hi, 0.5 * data.size)
        assert ref.outside < 1e-9, ref.outside
        _REFS[key] = (ref, data)
    return _REFS[key]


def _production_leg(tag, pkg, gpu_engine, cpu_engine, d, C, checkpoints, seed, lo=None, hi=None, vscale=1.0, halves=False, **model_kw):
    lo = (BOX1[0] if d == 1 else LO3) if lo is None else lo
    hi = (BOX1[1] if d == 1 else HI3) if hi is None else hi
    ref, data = _reference(pkg, cpu_engine, d, lo, hi, **model_kw)
    rng = np.random.default_rng(seed)
    q0 = ref.draw(rng, C)
    gpu_engine.set_model(_model(pkg, **model_kw), 1)
    gpu_engine.mcmc_init(q0, data, lo, hi, seed=seed, n0=0.0, prior_len=3)
    _, ssq0, _, V = (np.asarray(x) for x in gpu_engine.get_state())
    # one proposal covariance for every chain — the init kernel's at chain 0's start.  Each chain's own V would be a function of
    # its start point: a state-dependent proposal, under which a pool started in pi does not stay in pi (each chain's kernel
    # keeps pi, their mixture weighted by the start does not; at d = 3, where V follows the (Dc, a) ridge, a drifts by 18 SE)
    V = np.ascontiguousarray(np.broadcast_to(vscale * V[:1], V.shape))
    gpu_engine.set_state(std2=R.draw_std2(rng, ssq0, ref.shape), V=V)
    fails, zmax, kmax, done = [], 0.0, 0.0, 0
    for it in (0,) + tuple(checkpoints):
        if it > done:
            gpu_engine.mcmc_run(it - done, traces=False)
            done = it
        q, _, std2, _ = (np.asarray(x) for x in gpu_engine.get_state())
        parts = [(f"{tag} it {it}", q, std2)]
        if halves:  # a float32 lane's two chains, 2k and 2k + 1
            parts += [(f"{tag} it {it} chains {h}::2", q[h::2], std2[h::2]) for h in (0, 1)]
        for t, qq, ss in parts:
            z, k = R.check(t, ref, qq, ss, fails)
            zmax, kmax = max(zmax, z), max(kmax, k)
    st = gpu_engine.stats()
    print(f"{tag}: largest |z| {zmax:.2f}, largest sqrt(C) D {kmax:.2f}; stats {st}")
    return fails, st


@pytest.mark.parametrize("damping", [True, False])
def test_float64_rk4_sampler_keeps_its_target(pkg, gpu_engine, cpu_engine, damping):
    """mcmc_kernel<1, *, false, RK4_F64>, the production path: Philox normals, uniforms and gammas at full power."""
    fails, _ = _production_leg(f"d1 f64 damp={damping}", pkg, gpu_engine, cpu_engine, 1, 262144, (100, 200), 101 + damping,
                               damping=damping)
    assert not fails, fails


def test_float64_rk4_sampler_chunked_tables(pkg, gpu_engine, cpu_engine):
    """nsteps 2000 (configs[2]): tables staged chunk by chunk, longer solves."""
    fails, _ = _production_leg("d1 f64 n2000", pkg, gpu_engine, cpu_engine, 1, 65536, (100, 200), 103, nsteps=2000)
    assert not fails, fails


def test_float64_rk4_sampler_truncating_box(pkg, gpu_engine, cpu_engine):
    """A box ending at the mode + 0.5 SD and a proposal 3x the initial one: a large share of proposals out of bounds, the
    run-ahead over them (kProposalTries) and early rejection at full load."""
    full, _ = _reference(pkg, cpu_engine, 1, *BOX1)
    mg = full.marg["Dc"]
    hi = float(mg.quantiles((0.5,))[0] + 0.5 * mg.sd)
    fails, st = _production_leg("d1 f64 box", pkg, gpu_engine, cpu_engine, 1, 262144, (100, 200), 104, hi=hi, vscale=9.0)
    assert not fails, fails
    assert st["evaluated"] < 0.8 * 262144 * 200  # the box does truncate the proposals


def test_float32_sampler_keeps_its_target(pkg, gpu_engine, cpu_engine):
    """mcmc_f32x2_kernel<1, *, false>: the float32 restatement's target; a lane's two chains also checked apart."""
    fails, _ = _production_leg("d1 f32", pkg, gpu_engine, cpu_engine, 1, 262144, (100, 200), 105, halves=True, precision="float32")
    assert not fails, fails


def test_dop853_sampler_keeps_its_target(pkg, gpu_engine, cpu_engine):
    """mcmc_kernel<1, *, false, DOP853>: the restatement's DOP853 target."""
    fails, _ = _production_leg("d1 dop853", pkg, gpu_engine, cpu_engine, 1, 65536, (50, 100), 106, integrator="dop853")
    assert not fails, fails


@pytest.mark.parametrize("precision", ["float64", "float32"])
def test_three_parameter_sampler_keeps_its_target(pkg, gpu_engine, cpu_engine, precision):
    """mcmc_kernel<3, *, false, RK4_F64> / mcmc_f32x2_kernel<3, *, false> with the init kernel's fixed proposal: Cholesky
    proposal, the box on every parameter, the non-finite region — against something other than their own restatement."""
    fails, _ = _production_leg(f"d3 {precision}", pkg, gpu_engine, cpu_engine, 3, 65536, (1000, 2000), 107 + (precision == "float32"),
                               halves=precision == "float32", precision=precision)
    assert not fails, fails


# ---- the chain logic alone: caller-supplied SSq from the closed forms -------------------------------------------------------

@pytest.mark.parametrize("d", [1, 3])
def test_injected_ssq_chain_logic_keeps_the_closed_form_target(gpu_engine, d):
    """mcmc_kernel<D, false, true, RK4_F64, INJECT>: the chain logic alone (no integrator) on SSq = S0 + (q-q0)^T K (q-q0),
    in a box that truncates."""
    ref, fn, c = R.closed_reference(d)
    fails = []
    R.run_injected(gpu_engine, ref, fn, c, 262144, (15, 30), 200 + d, f"injected d{d}", fails)
    assert not fails, fails


def test_adaptive_three_parameter_product_recipe(pkg, cpu_engine):
    """MCMC.sample_batched's defaults for d = 3 (adapt_mode 'am', fd_rel_step 1e-4, burn = half) from (1600, 0.008, 0.022),
    n0 = 0: the pooled post-burn means of Dc, a, b and Dc a against the quadrature, SE from the spread of per-chain means."""
    ref, data = _reference(pkg, cpu_engine, 3, LO3, HI3)
    model = _model(pkg)
    mc = pkg.MCMC(model, data, 1000.0, [["Uniform", lo, hi] for lo, hi in zip(LO3, HI3)], [1600.0, 0.008, 0.022],
                  nsamples=6000, verbose=False)
    mc.n0 = 0.0
    pool = mc.sample_batched(16384, seed=2026, iters_per_launch=1000)
    x = np.asarray(pool.samples)
    vals = {"Dc": x[..., 0], "a": x[..., 1], "b": x[..., 2], "Dc*a": x[..., 0] * x[..., 1]}
    fails, worst = [], 0.0
    for name, v in vals.items():
        cm = v.mean(axis=0)
        se = cm.std(ddof=1) / np.sqrt(cm.size)
        z = (cm.mean() - ref.marg[name].mean) / se
        print(f"am {name}: pooled mean {cm.mean():.6g} quadrature {ref.marg[name].mean:.6g} se {se:.3g} z {z:+.2f}")
        worst = max(worst, abs(z))
        if abs(z) >= R.Z_MAX:
            fails.append(f"am {name}: z {z:+.2f}")
    print(f"am: largest |z| {worst:.2f}")
    assert not fails, fails
