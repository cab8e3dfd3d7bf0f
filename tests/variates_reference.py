"""
Specification of the sampler's variates in NumPy long double (TEST INFRASTRUCTURE ONLY, no GPU): the normals, the accept uniform
and the gamma variate that rsf_mcmc_draws reports for a (seed, chain, iteration) — csrc/rsf_device.h: normal_pair, u53, gamma_draw —
written from the algorithms' definitions on the Philox words of tests/smc_reference.py, vectorised over chains.

    u53(a, b)    (((a << 32 | b) >> 11) + 1) 2^-53 in (0, 1]: a float64, exact.
    normals      Box-Muller on the four words of a slot: r = sqrt(-2 ln u53(w0, w1)), (z0, z1) = r (cos, sin)(2 pi u53(w2, w3)).  The
                 angle is reduced exactly, as tests/test_gpu_math.py::test_sincos2pi does: k = rint(4 u), u - k / 4 is exact in float64,
                 the sine and cosine of 2 pi (u - k / 4) in [-pi / 4, pi / 4] are rotated by the quadrant k mod 4.
    gamma        Marsaglia & Tsang (2000), shape >= 1: d = shape - 1 / 3, c = 1 / sqrt(9 d).  Attempt j = 0, 1, ... takes x = z0 of slot
                 8 + 2 j; 1 + c x <= 0: next attempt; v = (1 + c x)^3, u = u53(w0, w1) of slot 9 + 2 j; accepted when
                 ln u < x^2 / 2 + d (1 - v + ln v) (the log test alone, no squeeze): g = d v.  At most 64 attempts, then g = d.
    draws        z: z0, z1 of slot 0 and z0 of slot 1 (the first d of them); u: u53(w0, w1) of slot 2; g.

The bounds a float64 implementation is held to (tests/test_gpu_variates.py derives them; eps = 2^-52):
    z_bound      |z - z_ref| <= eps (4 |z| + 2 r)
    g_bound      |g - g_ref| / g_ref <= eps (4 + 3 c (4 |x| + 2 r) / (1 + c x)), x and r of the accepted attempt
"""
import numpy as np

import smc_reference as sr

LD = np.longdouble
EPS = 2.0 ** -52
SLOT_GAMMA = 8
MAX_ATTEMPTS = 64
# pi to long double: the float64 nearest pi plus what it leaves out
PI_LD = LD(np.pi) + LD(1.2246467991473532e-16)


def normal_pair(words):
    """words (n, 4) uint32 → (z0, z1, r), long double"""
    u1, u2 = sr.u53(words[:, 0], words[:, 1]), sr.u53(words[:, 2], words[:, 3])
    r = np.sqrt(LD(-2) * np.log(u1.astype(LD)))
    k = np.rint(4.0 * u2)
    th = (u2 - 0.25 * k).astype(LD) * (LD(2) * PI_LD)  # u2 - k / 4: exact
    s0, c0 = np.sin(th), np.cos(th)
    quad = k.astype(np.int64) & 3
    s = np.where(quad == 0, s0, np.where(quad == 1, c0, np.where(quad == 2, -s0, -c0)))
    c = np.where(quad == 0, c0, np.where(quad == 1, -s0, np.where(quad == 2, -c0, s0)))
    return r * c, r * s, r


def gamma_constants(shape):
    d = LD(shape) - LD(1) / LD(3)
    return d, LD(1) / np.sqrt(LD(9) * d)


def gamma(seed, chains, iteration, shape):
    """→ dict(g, x, r: long double (n,); attempts: int (n,); vle0: bool (n,), an attempt with 1 + c x <= 0 was met; edge: float64
    (n,), the smallest distance of any examined decision from its edge — |1 + c x| / c (in units of x) for the sign of v and, where
    v > 0, |ln u - x^2 / 2 - d (1 - v + ln v)| for the log test)"""
    chains = np.atleast_1d(np.asarray(chains, dtype=np.uint64))
    n = chains.size
    d, c = gamma_constants(shape)
    g, xa, ra = np.full(n, d, dtype=LD), np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    attempts, vle0, edge = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.full(n, np.inf)
    todo = np.arange(n)
    for j in range(MAX_ATTEMPTS):
        if todo.size == 0:
            break
        x, _, r = normal_pair(sr.words(seed, chains[todo], iteration, SLOT_GAMMA + 2 * j))
        attempts[todo] += 1
        t = LD(1) + c * x
        edge[todo] = np.minimum(edge[todo], (np.abs(t) / c).astype(np.float64))
        pos = t > 0
        vle0[todo[~pos]] = True
        w = sr.words(seed, chains[todo], iteration, SLOT_GAMMA + 2 * j + 1)
        u = sr.u53(w[:, 0], w[:, 1]).astype(LD)
        v = np.where(pos, t, LD(1)) ** 3
        margin = np.log(u) - (LD(0.5) * x * x + d * (LD(1) - v + np.log(v)))
        edge[todo[pos]] = np.minimum(edge[todo[pos]], np.abs(margin[pos]).astype(np.float64))
        ok = pos & (margin < 0)
        g[todo[ok]], xa[todo[ok]], ra[todo[ok]] = (d * v)[ok], x[ok], r[ok]
        todo = todo[~ok]
    assert todo.size == 0, f"{todo.size} draws made {MAX_ATTEMPTS} attempts"
    return dict(g=g, x=xa, r=ra, attempts=attempts, vle0=vle0, edge=edge)


def draws(seed, chains, iteration, n_params, shape=None):
    """rsf_mcmc_draws' contract → dict(z (n, n_params), r (n, n_params): the Box-Muller radius behind each z, u (n,) float64, and —
    with a shape — gamma()'s dict under 'gamma')"""
    chains = np.atleast_1d(np.asarray(chains, dtype=np.uint64))
    z0, z1, r01 = normal_pair(sr.words(seed, chains, iteration, sr.SLOT_Z01))
    z, r = [z0, z1], [r01, r01]
    if n_params > 2:
        z2, _, r2 = normal_pair(sr.words(seed, chains, iteration, sr.SLOT_Z2))
        z.append(z2)
        r.append(r2)
    w = sr.words(seed, chains, iteration, sr.SLOT_U)
    out = dict(z=np.stack(z[:n_params], axis=1), r=np.stack(r[:n_params], axis=1), u=sr.u53(w[:, 0], w[:, 1]))
    if shape is not None:
        out["gamma"] = gamma(seed, chains, iteration, shape)
    return out


def z_bound(z, r, eps=EPS):
    return eps * (4 * np.abs(np.asarray(z, dtype=LD)) + 2 * np.asarray(r, dtype=LD))


def g_bound(shape, x, r, eps=EPS):
    """relative"""
    _, c = gamma_constants(shape)
    x, r = np.asarray(x, dtype=LD), np.asarray(r, dtype=LD)
    return eps * (4 + 3 * c * (4 * np.abs(x) + 2 * r) / (1 + c * x))


def selection(ref, n_multi=300, n_vle0=300, n_single=200):
    """indices of a gamma() result that a per-call comparison visits: the draws with two or more attempts (at most n_multi, those
    with the most attempts first), the draws that met 1 + c x <= 0 (at most n_vle0) and the first n_single one-attempt draws"""
    a = ref["attempts"]
    multi = np.flatnonzero(a >= 2)
    multi = multi[np.argsort(-a[multi], kind="stable")][:n_multi]
    vle = np.flatnonzero(ref["vle0"])
    vle = vle[np.argsort(-a[vle], kind="stable")][:n_vle0]
    single = np.flatnonzero(a == 1)[:n_single]
    return np.unique(np.concatenate([multi, vle, single]))


def ks_sqrt_n(x, cdf):
    """sqrt(n) D_n of the sample x against the continuous distribution function cdf"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    f = cdf(x)
    return float(np.sqrt(n) * max((np.arange(1, n + 1) / n - f).max(), (f - np.arange(n) / n).max()))
