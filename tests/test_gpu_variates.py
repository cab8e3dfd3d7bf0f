"""
The device's variates against their long-double specification (tests/variates_reference.py): the probe kernel draw by draw, the
production kernels that call rsf::gamma_draw with whole waves whose lanes leave the attempt loop at different trips, and the
sampler's own Gibbs update of sigma^2 in mcmc_kernel and mcmc_f32x2_kernel.

The bounds (eps = 2^-52), from what tests/test_gpu_math.py establishes on the device — fm::log within 4 ulp, sin / cos(2 pi u) within
3e-16 absolute (< 2 eps), fm::rcp within 2 ulp, sqrt correctly rounded:
    z = r (cos, sin)(2 pi u2), r = sqrt(-2 ln u1): the logarithm's 4 ulp reach r halved, r's own roundings and the product add less
        than two more — under 4 eps |z| in all — and the angle's absolute error enters times r:  |z - z_ref| <= eps (4 |z| + 2 r).
    g = d (1 + c x)^3: d = shape - 1 / 3 (two roundings), the sum 1 + c x (one, three times over in the cube), the cube and d v
        (three) stay under 4 eps; the error of x, and of c with it, is amplified by d ln v / dx = 3 c / (1 + c x):
        |g - g_ref| / g_ref <= eps (4 + 3 c (4 |x| + 2 r) / (1 + c x)), x and r of the accepted attempt.
    u: equal as numbers.
    sigma^2 = b rcp(g) or b / g with b = SSq / 2: g's bound + 3 eps (the reciprocal's 2 ulp and the product).  With n0 > 0,
        b = (n0 sigma^2 + SSq) / 2 takes two more roundings of half an ulp: g's bound + 4 eps.
No draw of the input set is a tie (tests/test_variates_reference.py: every decision is further than 1e-9 from its edge), so the
device has to make the reference's number of attempts: a draw from another attempt is off by O(1) and fails every bound here.
"""
import numpy as np
import pytest
from scipy import stats

import variates_reference as vr
from test_variates_reference import ITER, KS_LIMIT, N, SEED, SHAPES

pytestmark = pytest.mark.gpu

N_WAVES = 200_037  # a partial last wave and a partial last workgroup
EPS = vr.EPS
_cache = {}


def reference(shape, seed=SEED, offset=0, iteration=ITER, n=N_WAVES):
    key = (shape, seed, offset, iteration, n)
    if key not in _cache:
        ref = vr.gamma(seed, np.uint64(offset) + np.arange(n, dtype=np.uint64), iteration, shape)
        for v in ref.values():
            v.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def std2_ratio(std2, b, ref, shape, extra):
    """|sigma^2 g_ref / b - 1| over (g's bound + extra eps), per draw"""
    err = np.abs(np.asarray(std2, dtype=vr.LD) * ref["g"] / np.asarray(b, dtype=vr.LD) - 1)
    return (err / (vr.g_bound(shape, ref["x"], ref["r"]) + extra * EPS)).astype(np.float64)


@pytest.mark.parametrize("shape", SHAPES)
def test_probe_kernel_draw_by_draw(gpu_engine, shape):
    """Engine.draws on the draws of the input set (seed 77, iteration 3, chains 0 .. 199 999) that went through the rejection path —
    those with two or more attempts (at most 300, the most attempts first), those that met 1 + c x <= 0 (at most 300) — and 200
    one-attempt draws, with d = 3 (and d = 1, 2 on the first 30 of them); then chain ids 2^33 + 7 and 2^63 - 1, the largest the ABI's
    int64 holds, and iterations 0 and 2^32 - 1, 60 draws each."""
    ref = {k: v[:N] for k, v in reference(shape).items()}
    idx = vr.selection(ref)
    multi, vle0 = int((ref["attempts"][idx] >= 2).sum()), int(ref["vle0"][idx].sum())
    assert multi >= (1 if shape == 2000.5 else 20) and (shape != 1.0 or vle0 >= 100)
    sets = [(idx, ITER)]
    for base, it in ((2 ** 33 + 7, 0), (2 ** 63 - 60, 2 ** 32 - 1), (2 ** 33 + 7, 2 ** 32 - 1), (2 ** 63 - 60, 0)):
        sets.append((base + np.arange(60, dtype=np.uint64), it))
    worst = dict(z=0.0, g=0.0)
    calls = 0
    for chains, it in sets:
        chains = np.asarray(chains, dtype=np.uint64)
        want = vr.draws(SEED, chains, it, 3, shape)
        zb, gb = vr.z_bound(want["z"], want["r"]), vr.g_bound(shape, want["gamma"]["x"], want["gamma"]["r"])
        for k, chain in enumerate(chains):
            for d in (3, 1, 2) if k < 30 else (3,):
                z, u, g = gpu_engine.draws(SEED, int(chain), int(it), d, shape)
                calls += 1
                assert u == want["u"][k], (int(chain), it)
                worst["z"] = max(worst["z"], float((np.abs(np.asarray(z, dtype=vr.LD) - want["z"][k, :d]) / zb[k, :d]).max()))
                rg = float(abs(vr.LD(g) / want["gamma"]["g"][k] - 1) / gb[k])
                worst["g"] = max(worst["g"], rg)
                assert rg <= 1.0, f"chain {int(chain)} iteration {it}: g = {g!r}, reference {want['gamma']['g'][k]!r} after {int(want['gamma']['attempts'][k])} attempts"
    print(f"probe kernel, shape {shape}: {calls} launches, {multi} draws with two or more attempts (up to {int(ref['attempts'][idx].max())}), {vle0} that met "
          f"1 + c x <= 0; largest ratio to the bound: z {worst['z']:.3f}, g {worst['g']:.3f}")
    assert worst["z"] <= 1.0 and worst["g"] <= 1.0


@pytest.mark.parametrize("shape,offset,iteration", [(s, 0, ITER) for s in SHAPES] + [(1.0, 2 ** 33, 12345)])
def test_smc_std2_whole_waves_with_divergent_exits(gpu_engine, shape, offset, iteration):
    """rsf_smc_std2 with l = 0: SSq = 1 and sigma^2_j = 0.5 / G_j, for 200 037 particles: every wave holds lanes that leave the attempt
    loop at different trips (shape 1: one lane in twenty makes a second attempt).  Every sigma^2 inside g's bound + 3 eps, and the
    device's own 0.5 / sigma^2 gamma distributed."""
    ref = reference(shape, SEED, offset, iteration)
    std2 = np.asarray(gpu_engine.smc_std2(np.zeros(N_WAVES), shape, seed=SEED, offset=offset, iteration=iteration))
    ratio = std2_ratio(std2, 0.5, ref, shape, 3)
    ks = vr.ks_sqrt_n(0.5 / std2, stats.gamma(shape).cdf)
    k = int(np.argmax(ratio))
    print(f"smc_std2, shape {shape}, offset {offset}, iteration {iteration}: {int((ref['attempts'] >= 2).sum())} of {N_WAVES} draws with two or more attempts; "
          f"largest ratio to the bound {ratio.max():.3f} (particle {k}, {int(ref['attempts'][k])} attempts); sqrt(n) D of 0.5 / sigma^2 = {ks:.3f}")
    assert ratio.max() <= 1.0
    assert ks < KS_LIMIT


def test_smc_batch_std2_three_populations(gpu_engine):
    """rsf_smc_batch_std2: three populations of 1 037 with their own seed, offset and iteration in one launch, shape 1."""
    seeds, offsets, iters, n = [SEED, 5, 2 ** 40 + 3], [0, 2 ** 33, 12345], [ITER, 0, 2 ** 31 + 1], 1037
    std2 = np.asarray(gpu_engine.smc_batch_std2(np.zeros((3, n)), 1.0, seeds, offsets, iters))
    worst, multi = 0.0, 0
    for p in range(3):
        ref = reference(1.0, seeds[p], offsets[p], iters[p], n)
        worst = max(worst, float(std2_ratio(std2[p], 0.5, ref, 1.0, 3).max()))
        multi += int((ref["attempts"] >= 2).sum())
    print(f"smc_batch_std2: 3 x {n} draws, {multi} with two or more attempts, largest ratio to the bound {worst:.3f}")
    assert multi >= 50 and worst <= 1.0


@pytest.mark.parametrize("precision,d", [("float64", 1), ("float64", 3), ("float32", 1)])
def test_sampler_gibbs_update(gpu_engine, oracle_mod, precision, d):
    """gibbs_std2 inside mcmc_kernel and mcmc_f32x2_kernel.  The series is the shortest rsf_set_model accepts with nout >= 3 (nsteps 3:
    shape 0.5 nout = 1.5, where 2.7 % of the draws make a second attempt), 4 096 + 37 chains (one observation group: the float32
    sampler's whole-workgroup rule binds only with several, so its last workgroup holds 37 chains in its first slot and none in
    its second), adapt_mode none.  Six launches of one iteration with n0 = 0: sigma^2 = 0.5 SSq / g_ref(iteration) with the SSq of
    get_state(), inside g's bound + 3 eps.  Then two launches with n0 = 0.01 (shape 1.505):
    sigma^2_t = 0.5 (n0 sigma^2_(t-1) + SSq_t) / g_ref, inside g's bound + 4 eps."""
    C, offset, nsteps = 4096 + 37, 2 ** 33 - 2000, 3
    m = oracle_mod.ModelSpec(nsteps, 0.0, 0.1 * nsteps, 1)
    m.precision = precision
    assert gpu_engine.set_model(m, 1) == 3
    data = np.linspace(0.001, 0.002, 3)
    rng = np.random.default_rng(31)
    q0 = np.column_stack([rng.uniform(600.0, 2400.0, C), rng.uniform(0.010, 0.012, C), rng.uniform(0.013, 0.015, C)])[:, :d]
    lo, hi = [0.0, 0.005, 0.005][:d], [1e4, 0.02, 0.03][:d]
    V0 = np.tile(np.diag(np.array([25.0 ** 2, 1e-4 ** 2, 1e-4 ** 2][:d])), (C, 1, 1))
    chains = np.uint64(offset) + np.arange(C, dtype=np.uint64)
    legs = [(0.0, 6, 3), (0.01, 2, 4)]
    # on the CPU beforehand: the legs go through the rejection path
    refs = {(n0, it): vr.gamma(SEED, chains, it, 0.5 * (n0 + 3)) for n0, iters, _ in legs for it in range(iters)}
    multi = sum(int((r["attempts"] >= 2).sum()) for r in refs.values())
    assert multi >= 50
    worst, accepted = 0.0, 0
    for n0, iters, extra in legs:
        # prior_len 2: the initial sigma^2 is SSq / (nout - prior_len), finite for nout = 3 whatever d
        gpu_engine.mcmc_init(q0, data, lo, hi, seed=SEED, chain_offset=offset, n0=n0, prior_len=2, adapt_mode="none")
        gpu_engine.set_state(V=V0)
        prev = np.asarray(gpu_engine.get_state()[2]).copy()
        for it in range(iters):
            _, _, ta = gpu_engine.mcmc_run(1)
            accepted += int(np.asarray(ta).sum())
            _, ssq, std2, _ = (np.asarray(x) for x in gpu_engine.get_state())
            assert np.isfinite(ssq).all() and (ssq > 0).all()
            b = 0.5 * (vr.LD(n0) * prev.astype(vr.LD) + ssq.astype(vr.LD))
            ratio = std2_ratio(std2, b, refs[(n0, it)], 0.5 * (n0 + 3), extra)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, f"n0 {n0} iteration {it}: chain {int(np.argmax(ratio))} at {ratio.max():.3f} of its bound"
            prev = std2.copy()
    print(f"sampler {precision} d = {d}: {C} chains, 8 launches, {multi} draws with two or more attempts, {accepted} accepted proposals; "
          f"largest ratio of sigma^2 to its bound {worst:.3f}")
    assert accepted > C  # the chains move: SSq_t is not the initial one throughout
