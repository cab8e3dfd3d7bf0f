"""
The long-double specification of the sampler's variates (tests/variates_reference.py), without a GPU: its distribution, the
coverage of the rejection path that the GPU tests rely on, its own precision against 50-digit arithmetic, and the CPU checker
held to it with the bounds of tests/test_gpu_variates.py.
"""
import mpmath
import numpy as np
import pytest
from scipy import stats

import smc_reference as sr
import variates_reference as vr

SEED, ITER, N = 77, 3, 200_000
SHAPES = (1.0, 1.5, 12.0, 250.005, 2000.5)
KS_LIMIT = 1.95  # the 0.1 % point of the Kolmogorov distribution
# measured with this reference (seed 77, iteration 3, chains 0 .. 199 999): draws with 1, 2, ... attempts
ATTEMPTS = {1.0: (190302, 9249, 426, 22, 1), 1.5: (194580, 5268, 144, 7, 1), 12.0: (199555, 445), 250.005: (199975, 25), 2000.5: (199998, 2)}

_cache = {}


def reference(shape):
    """gamma() of the fixed input set, computed once per shape and never changed"""
    if shape not in _cache:
        ref = vr.gamma(SEED, np.arange(N, dtype=np.uint64), ITER, shape)
        for v in ref.values():
            v.setflags(write=False)
        _cache[shape] = ref
    return _cache[shape]


def normals_reference():
    if "z" not in _cache:
        ref = vr.draws(SEED, np.arange(N, dtype=np.uint64), ITER, 3)
        for v in ref.values():
            v.setflags(write=False)
        _cache["z"] = ref
    return _cache["z"]


@pytest.mark.parametrize("shape", SHAPES)
def test_gamma_reference_is_gamma_distributed(shape):
    ks = vr.ks_sqrt_n(reference(shape)["g"], stats.gamma(shape).cdf)
    print(f"shape {shape}: sqrt(n) D = {ks:.3f} (n = {N})")
    assert ks < KS_LIMIT


def test_normal_reference_is_normally_distributed():
    z = normals_reference()["z"]
    ks = [vr.ks_sqrt_n(z[:, p], stats.norm.cdf) for p in range(3)]
    print("sqrt(n) D of z0, z1 (slot 0), z2 (slot 1):", ", ".join(f"{k:.3f}" for k in ks))
    assert max(ks) < KS_LIMIT
    u = normals_reference()["u"]
    ku = vr.ks_sqrt_n(u, stats.uniform.cdf)
    print(f"sqrt(n) D of u: {ku:.3f}")
    assert ku < KS_LIMIT and u.min() > 0.0 and u.max() <= 1.0


@pytest.mark.parametrize("shape", SHAPES)
def test_input_set_covers_the_rejection_path(shape):
    """What tests/test_gpu_variates.py relies on.  These are facts of (seed 77, iteration 3, chains 0 .. 199 999): another input
    set has to establish its own."""
    ref = reference(shape)
    counts = tuple(int(c) for c in np.bincount(ref["attempts"])[1:])
    multi, vle0, edge = int((ref["attempts"] >= 2).sum()), int(ref["vle0"].sum()), float(ref["edge"].min())
    print(f"shape {shape}: attempts {counts}, {multi} draws with two or more, {vle0} met 1 + c x <= 0, smallest edge distance {edge:.2e}")
    assert counts == ATTEMPTS[shape]
    assert multi >= (1 if shape == 2000.5 else 20)
    if shape == 1.0:
        assert vle0 >= 100
    assert edge > 1e-9  # no tie: a float64 implementation with a 4-ulp log decides every attempt as the reference does


def _mp_normal_pair(w):
    u1 = mpmath.mpf(int(sr.u53(w[0:1], w[1:2])[0] * 2.0 ** 53)) / 2 ** 53
    u2 = mpmath.mpf(int(sr.u53(w[2:3], w[3:4])[0] * 2.0 ** 53)) / 2 ** 53
    r = mpmath.sqrt(-2 * mpmath.log(u1))
    return r * mpmath.cos(2 * mpmath.pi * u2), r * mpmath.sin(2 * mpmath.pi * u2), r


def _mp_gamma(seed, chain, iteration, shape):
    """Marsaglia & Tsang at the working precision of mpmath, one draw → (g, attempts, x, r)"""
    d = mpmath.mpf(shape) - mpmath.mpf(1) / 3
    c = 1 / mpmath.sqrt(9 * d)
    for j in range(vr.MAX_ATTEMPTS):
        x, _, r = _mp_normal_pair(sr.words(seed, [chain], iteration, vr.SLOT_GAMMA + 2 * j)[0])
        t = 1 + c * x
        if t <= 0:
            continue
        v = t ** 3
        w = sr.words(seed, [chain], iteration, vr.SLOT_GAMMA + 2 * j + 1)[0]
        u = mpmath.mpf(int(sr.u53(w[0:1], w[1:2])[0] * 2.0 ** 53)) / 2 ** 53
        if mpmath.log(u) < x * x / 2 + d * (1 - v + mpmath.log(v)):
            return d * v, j + 1, x, r
    return d, vr.MAX_ATTEMPTS, x, r


def _mp(x):
    """a long double as an mpf, exactly"""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - vr.LD(hi)))


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_precision_against_50_digits(shape):
    """The long-double reference against the same algorithm at 50 digits, on 200 chains per shape plus, at shape 1, every draw with
    three or more attempts: z within 2^-60 (1 + |z|); g within 2^-58 relative, or g_bound with 2^-60 in the place of eps (the
    conditioning of v = (1 + c x)^3 in x, which the accepted x's own 2^-60 enters with) where that is larger; the same number of
    attempts.  This pins the reference far below a float64 ulp."""
    ref = reference(shape)
    idx = np.arange(200)
    if shape == 1.0:
        idx = np.union1d(idx, np.flatnonzero(ref["attempts"] >= 3))
    zref = normals_reference()
    worst_z = worst_g = 0.0
    with mpmath.workdps(50):
        for i in idx:
            g, attempts, x, r = _mp_gamma(SEED, int(i), ITER, shape)
            assert attempts == ref["attempts"][i]
            tol = max(2.0 ** -58, float(vr.g_bound(shape, ref["x"][i], ref["r"][i], eps=2.0 ** -60)))
            worst_g = max(worst_g, float(abs(_mp(ref["g"][i]) - g) / g) / tol)
            assert abs(_mp(ref["x"][i]) - x) <= 2.0 ** -60 * (1 + abs(x))
        for i in idx[:200]:
            z0, z1, _ = _mp_normal_pair(sr.words(SEED, [int(i)], ITER, sr.SLOT_Z01)[0])
            z2, _, _ = _mp_normal_pair(sr.words(SEED, [int(i)], ITER, sr.SLOT_Z2)[0])
            for p, z in enumerate((z0, z1, z2)):
                worst_z = max(worst_z, float(abs(_mp(zref["z"][i, p]) - z) / (2.0 ** -60 * (1 + abs(z)))))
    print(f"shape {shape}: {idx.size} draws, largest ratio to the bound: g {worst_g:.3f}, z {worst_z:.3f}")
    assert worst_g <= 1.0 and worst_z <= 1.0


def test_cpu_checker_normals_and_uniform(cpu_engine):
    """The checker's z and u on chains 0 .. 4999 of the input set (d = 3), chain ids past 2^32 and the ends of the iteration range:
    u equal as numbers, z inside z_bound."""
    worst, count = 0.0, 0
    for chains, it in ((np.arange(5000), ITER), (2 ** 33 + 7 + np.arange(50), 0), (2 ** 63 - 1 - np.arange(50), 2 ** 32 - 1)):
        ref = vr.draws(SEED, chains, it, 3)
        bound = vr.z_bound(ref["z"], ref["r"])
        for k, chain in enumerate(chains):
            z, u, _ = cpu_engine.draws(SEED, int(chain), int(it), 3, 12.0)
            assert u == ref["u"][k]
            worst = max(worst, float((np.abs(np.asarray(z, dtype=vr.LD) - ref["z"][k]) / bound[k]).max()))
            count += 1
    print(f"checker z: {count} draws of 3, largest ratio to eps (4 |z| + 2 r): {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_checker_gamma(cpu_engine, shape):
    """The checker's gamma variate on a subset of the input set that holds EVERY draw with two or more attempts, every draw that met
    1 + c x <= 0 and 2000 one-attempt draws, inside g_bound."""
    ref = reference(shape)
    idx = vr.selection(ref, n_multi=N, n_vle0=N, n_single=2000)
    assert np.isin(np.flatnonzero(ref["attempts"] >= 2), idx).all() and np.isin(np.flatnonzero(ref["vle0"]), idx).all()
    got = np.array([cpu_engine.draws(SEED, int(i), ITER, 1, shape)[2] for i in idx])
    ratio = np.abs(got.astype(vr.LD) / ref["g"][idx] - 1) / vr.g_bound(shape, ref["x"][idx], ref["r"][idx])
    print(f"checker g, shape {shape}: {idx.size} draws ({int((ref['attempts'][idx] >= 2).sum())} with two or more attempts), "
          f"largest ratio to the bound {float(ratio.max()):.3f} (draw {int(idx[np.argmax(ratio)])}, {int(ref['attempts'][idx][np.argmax(ratio)])} attempts)")
    assert float(ratio.max()) <= 1.0
