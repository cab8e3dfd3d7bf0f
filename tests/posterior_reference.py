"""
The sampler's exact target, computed by quadrature (a test helper; TEST INFRASTRUCTURE ONLY, no GPU).

With n0 = 0 one sampler iteration — a symmetric Metropolis step on q given sigma^2 inside a strict box, then the Gibbs draw
sigma^2 = 0.5 SSq / G, G ~ Gamma(shape), shape = 0.5 nout (csrc/rsf_kernels_sampler.h: metropolis, gibbs_std2) — is an exact
Metropolis-within-Gibbs chain for

    pi(q, sigma^2) ~ 1_box(q) sigma^(-2 shape - 2) exp(-SSq(q) / 2 sigma^2)
    pi(q)          ~ 1_box(q) SSq(q)^(-shape)           (a NaN / inf SSq has density 0: accept_test rejects it)
    sigma^2 | q    ~ InvGamma(shape, SSq(q) / 2)

whatever SSq is, so the target of each sampler kernel is an integral over the SSq that kernel's own solve computes — which the
checker library reproduces (bit for bit in float32, to ~1e-12 in float64, and in DOP853).  `Posterior1` (d = 1) and
`Posterior3` (d = 3, (Dc, a, b)) tabulate it; `check` holds a pool of independent chain states to it.

d = 1: a coarse scan over the whole box (linear and log-spaced) finds the mass and bounds what lies outside the fine window,
then a fine grid of `n_fine` (odd) points over +-12 SD of it, clipped to the box: composite Simpson for the moments,
cumulative Simpson for the CDF.  Draws invert the CDF, linearly interpolated.

d = 3: coordinates (p = Dc a, a, b) — the initial proposal's Dc-a correlation is -0.994, a grid in Dc would not resolve the
ridge.  (a, b): Gauss-Legendre nodes over the whole box (the posterior fills it).  p: one window for every (a, b) node, +-12
conditional SD of the widest node found by the coarse scan; SSq is solved on `n_pc` points of it and its logarithm
cubic-spline interpolated onto `n_fine` points (Simpson).  The density in these coordinates is pi(p/a, a, b) / a.  The
marginal CDFs of a and b integrate the Legendre series through the node densities.  Draws take a from its marginal, b from
its conditional at the nearest a node, p from its conditional at the nearest (a, b) node (the target is nearly a product in
these coordinates).

sigma^2's marginal is the mixture of InvGamma(shape, SSq/2) over pi(q): its moments are exact sums, its CDF is evaluated on a
grid from the atoms binned by SSq (bins of 1e-4 relative width against the InvGamma's own 1/sqrt(shape)).
"""
import numpy as np
from scipy import integrate, interpolate, special

WINDOW_SD = 12.0
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
# thresholds of check(): each has a false-alarm probability of ~1e-5 under a correct kernel
Z_MAX = 4.5   # two-sided normal: 6.8e-6
KS_MAX = 2.4  # Kolmogorov: P(sqrt(C) D > 2.4) = 2 sum (-1)^(k-1) exp(-2 k^2 2.4^2) = 2.0e-5


def log_target(ssq, shape):
    """log pi(q) up to a constant from the sums of squares: -shape log SSq, -inf where SSq is not finite and positive."""
    ssq = np.asarray(ssq, dtype=np.float64)
    ok = np.isfinite(ssq) & (ssq > 0)
    return np.where(ok, -shape * np.log(np.where(ok, ssq, 1.0)), -np.inf)


def _simpson_weights(x):
    n = x.size
    assert n % 2 == 1 and n >= 3, "composite Simpson needs an odd number of points"
    h = (x[-1] - x[0]) / (n - 1)
    w = np.full(n, 2.0)
    w[1::2] = 4.0
    w[0] = w[-1] = 1.0
    return w * h / 3.0


def _moments(x, w):
    """weights w (sum 1) at atoms x -> (mean, var, kurtosis)"""
    m = np.dot(w, x)
    c = x - m
    v = np.dot(w, c * c)
    return m, v, np.dot(w, c ** 4) / v ** 2


class Marginal:
    """One scalar quantity of the target: moments, a CDF on a grid (linearly interpolated), quantiles."""

    def __init__(self, mean, var, kurt, xs, F):
        self.mean, self.var, self.kurt = float(mean), float(var), float(kurt)
        self.sd = np.sqrt(self.var)
        F = np.maximum.accumulate(np.clip(F, 0.0, None))
        self.xs, self.F = xs, F / F[-1]

    def cdf(self, x):
        return np.interp(x, self.xs, self.F, left=0.0, right=1.0)

    def quantiles(self, probs=PROBS):
        return np.interp(probs, self.F, self.xs)

    def density(self, x):
        """the CDF's slope (for a quantile's standard error)"""
        h = 1e-3 * self.sd
        return (self.cdf(x + h) - self.cdf(x - h)) / (2 * h)


def sigma2_marginal(ssq, w, shape, n_grid=2001):
    """sigma^2 ~ mixture over atoms (ssq, w) of InvGamma(shape, ssq / 2) -> Marginal (exact raw moments up to the 4th)."""
    ssq, w = np.ravel(ssq), np.ravel(w)
    keep = w > 0
    ssq, w = ssq[keep], w[keep] / w[keep].sum()
    beta = 0.5 * ssq
    raw = [np.dot(w, beta ** k) / np.prod([shape - j for j in range(1, k + 1)]) for k in (1, 2, 3, 4)]
    m = raw[0]
    v = raw[1] - m * m
    k4 = raw[3] - 4 * m * raw[2] + 6 * m * m * raw[1] - 3 * m ** 4
    sd = np.sqrt(v)
    # atoms binned by SSq (relative width ~1e-4; the InvGamma's own relative spread is 1/sqrt(shape))
    lo, hi = ssq.min(), ssq.max()
    nb = int(min(ssq.size, max(1, np.ceil(np.log(hi / lo) / 1e-4))))
    if nb < ssq.size:
        idx = np.minimum(((np.log(ssq / lo) / max(np.log(hi / lo), 1e-300)) * nb).astype(np.int64), nb - 1)
        wb = np.bincount(idx, w, nb)
        bb = np.bincount(idx, w * beta, nb)
        nz = wb > 0
        beta, w = bb[nz] / wb[nz], wb[nz]
    xs = np.linspace(max(m - WINDOW_SD * sd, 1e-300), m + WINDOW_SD * sd, n_grid)
    F = np.empty(n_grid)
    for s in range(0, n_grid, 256):
        F[s:s + 256] = special.gammaincc(shape, beta[None, :] / xs[s:s + 256, None]) @ w
    return Marginal(m, v, k4 / v ** 2, xs, F)


def draw_std2(rng, ssq, shape):
    """sigma^2 ~ InvGamma(shape, ssq / 2) for each chain's SSq (the Gibbs conditional)."""
    return 0.5 * np.asarray(ssq) / rng.standard_gamma(shape, np.shape(ssq))


def _strict(lo, hi, x):
    return (x > lo) & (x < hi)


class Posterior1:
    """d = 1: ssq_fn(x (n,)) -> SSq (n,) for parameter values inside the box (lo, hi)."""

    def __init__(self, ssq_fn, lo, hi, shape, n_fine=4001, n_coarse=4001):
        self.lo, self.hi, self.shape, self.d = float(lo), float(hi), float(shape), 1
        xc = np.linspace(lo, hi, n_coarse)
        if lo >= 0:
            xc = np.union1d(xc, np.geomspace(max(lo, 1e-6 * hi), hi, n_coarse))
        xc = xc[_strict(lo, hi, xc)]
        lc = log_target(ssq_fn(xc), shape)
        assert np.isfinite(lc).any(), "the target has no mass inside the box"
        pc = np.exp(lc - lc.max())
        Z = integrate.trapezoid(pc, xc)
        mc = integrate.trapezoid(xc * pc, xc) / Z
        sc = np.sqrt(integrate.trapezoid((xc - mc) ** 2 * pc, xc) / Z)
        self.wlo, self.whi = max(lo, mc - WINDOW_SD * sc), min(hi, mc + WINDOW_SD * sc)
        x = np.linspace(self.wlo, self.whi, n_fine)
        self.x, self.ssq = x, ssq_fn(x)
        lp = log_target(self.ssq, shape)
        assert np.isfinite(lp).all(), "a non-finite SSq inside the fine window"
        self.lmax = lp.max()
        f = np.exp(lp - self.lmax)
        w = _simpson_weights(x) * f
        self.Z = w.sum()
        self.w = w / self.Z
        self.pdf = f / self.Z
        F = integrate.cumulative_simpson(self.pdf, x=x, initial=0.0)
        m, v, k = _moments(x, self.w)
        self.marg = {"Dc": Marginal(m, v, k, x, F)}
        self.marg["sigma2"] = sigma2_marginal(self.ssq, self.w, shape)
        # mass outside the fine window, bounded from the coarse scan (in units of the window's own normalisation)
        out = ~((xc >= self.wlo) & (xc <= self.whi))
        self.outside = integrate.trapezoid(np.where(out, pc, 0.0), xc) / Z if out.any() else 0.0
        self.names = ("Dc", "sigma2")

    def draw(self, rng, C):
        F = self.marg["Dc"].F
        return np.interp(rng.uniform(size=C), F, self.x).reshape(C, 1)


class Posterior3:
    """d = 3, q = (Dc, a, b): ssq_fn(Dc, a, b) (arrays of one shape) -> SSq, box lo, hi (3,)."""

    def __init__(self, ssq_fn, lo, hi, shape, n_ab=32, n_pc=97, n_fine=2001, n_coarse=801):
        self.lo, self.hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        self.shape, self.d = float(shape), 3
        lo, hi = self.lo, self.hi
        t, gw = np.polynomial.legendre.leggauss(n_ab)
        self.a = lo[1] + (hi[1] - lo[1]) * (t + 1) / 2
        self.b = lo[2] + (hi[2] - lo[2]) * (t + 1) / 2
        self.wa, self.wb = gw * (hi[1] - lo[1]) / 2, gw * (hi[2] - lo[2]) / 2
        # coarse scan in p at 3 x 3 (a, b) nodes spread over the box: the window, and what lies outside it
        sel = np.array([0, n_ab // 2, n_ab - 1])
        pmax = hi[0] * hi[1]
        pc = np.union1d(np.linspace(lo[0] * lo[1], pmax, n_coarse), np.geomspace(max(lo[0] * lo[1], 1e-6 * pmax), pmax, n_coarse))
        A, B, P = np.meshgrid(self.a[sel], self.b[sel], pc, indexing="ij")
        Dc = P / A
        lc = np.where(_strict(lo[0], hi[0], Dc), log_target(ssq_fn(Dc, A, B), shape), -np.inf) - np.log(A)
        ref = lc.max()
        fc = np.exp(lc - ref)
        Zc = integrate.trapezoid(fc, pc, axis=2)
        mc = integrate.trapezoid(P * fc, pc, axis=2) / Zc
        sc = np.sqrt(integrate.trapezoid((P - mc[..., None]) ** 2 * fc, pc, axis=2) / Zc)
        self.plo = max(float((mc - WINDOW_SD * sc).min()), lo[0] * lo[1])
        self.phi = min(float((mc + WINDOW_SD * sc).max()), hi[0] * hi[1])
        out = (pc < self.plo) | (pc > self.phi)
        self.outside = float((integrate.trapezoid(np.where(out, fc, 0.0), pc, axis=2) / Zc).max())
        # SSq on n_pc points of the window for every (a, b) node; log SSq spline-interpolated onto the fine grid
        pk = np.linspace(self.plo, self.phi, n_pc)
        A, B, P = np.meshgrid(self.a, self.b, pk, indexing="ij")
        sk = ssq_fn(np.clip(P / A, lo[0], hi[0]), A, B)
        assert np.isfinite(sk).all() and (sk > 0).all(), "a non-finite SSq inside the fine window"
        self.p = np.linspace(self.plo, self.phi, n_fine)
        ssq = np.exp(interpolate.CubicSpline(pk, np.log(sk), axis=2)(self.p))
        inbox = _strict(lo[0], hi[0], self.p[None, None, :] / self.a[:, None, None])  # Dc = p / a inside its box
        lp = np.where(inbox, log_target(ssq, shape), -np.inf) - np.log(self.a)[:, None, None]
        f = np.exp(lp - lp.max())
        W = self.wa[:, None, None] * self.wb[None, :, None] * _simpson_weights(self.p)[None, None, :] * f
        self.W = W / W.sum()
        self.ssq = ssq
        self.node_mass = self.W.sum(axis=2)  # (n_ab, n_ab)
        cond = integrate.cumulative_simpson(f, x=self.p, axis=2, initial=0.0)
        self.cond_F = np.maximum.accumulate(cond / cond[..., -1:], axis=2)
        self._marginals()
        self.names = ("Dc", "a", "b", "Dc*a", "sigma2")

    def _legendre_cdf(self, f, k, n_grid=4001):
        """density values f (..., n_ab) at the Gauss-Legendre nodes of parameter k -> (grid, CDF (..., n_grid)) from the
        interpolating Legendre series, integrated (the density is smooth inside the box: spectral accuracy)"""
        t = np.polynomial.legendre.leggauss(self.a.size)[0]
        tg = np.linspace(-1.0, 1.0, n_grid)
        c = np.polynomial.legendre.legfit(t, np.moveaxis(np.atleast_2d(f), -1, 0), self.a.size - 1)
        F = np.polynomial.legendre.legval(tg, np.polynomial.legendre.legint(c, lbnd=-1.0))
        F = np.maximum.accumulate(np.clip(np.atleast_2d(F), 0.0, None), axis=-1)
        return self.lo[k] + (self.hi[k] - self.lo[k]) * (tg + 1) / 2, F / F[..., -1:]

    def _marginals(self):
        W, p = self.W, self.p
        mg = {}
        # a and b: moments from the nodes, CDFs from the Legendre series through the node densities
        for name, nodes, gw, axis, k in (("a", self.a, self.wa, (1, 2), 1), ("b", self.b, self.wb, (0, 2), 2)):
            wm = W.sum(axis=axis)
            m, v, ku = _moments(nodes, wm)
            xs, F = self._legendre_cdf(wm / gw, k)
            mg[name] = Marginal(m, v, ku, xs, F[0])
        # draws: a from its marginal, b from its conditional at the nearest a node, p from its conditional at the nearest node
        self.b_grid, self.b_cond_F = self._legendre_cdf(W.sum(axis=2) / self.wb[None, :], 2)
        # p = Dc a: Simpson in p of the (a, b)-marginalised density
        wp = W.sum(axis=(0, 1))
        fp = wp / _simpson_weights(p)
        m, v, ku = _moments(p, wp)
        mg["Dc*a"] = Marginal(m, v, ku, p, integrate.cumulative_simpson(fp, x=p, initial=0.0))
        # Dc = p / a and log Dc: moments from the atoms (a node, p); the CDF P(Dc < x) = sum over a nodes of the node's mass times
        # P(p < x a | a), Gauss-Legendre in a of a smooth function
        wap = W.sum(axis=1)
        dc = (p[None, :] / self.a[:, None]).ravel()
        m, v, ku = _moments(dc, wap.ravel())
        ma = wap.sum(axis=1)
        Fp = integrate.cumulative_simpson(wap / _simpson_weights(p)[None, :], x=p, axis=1, initial=0.0)
        Fp /= Fp[:, -1:]
        xs = np.linspace(max(dc.min(), m - WINDOW_SD * np.sqrt(v)), min(dc.max(), m + WINDOW_SD * np.sqrt(v)), 4001)
        F = sum(ma[i] * np.interp(xs * self.a[i], p, Fp[i], left=0.0, right=1.0) for i in range(self.a.size))
        mg["Dc"] = Marginal(m, v, ku, xs, F)
        pos = wap.ravel() > 0
        m, v, ku = _moments(np.log(dc[pos]), wap.ravel()[pos])
        mg["log Dc"] = Marginal(m, v, ku, np.array([m - 1.0, m + 1.0]), np.array([0.0, 1.0]))  # moments only
        mg["sigma2"] = sigma2_marginal(self.ssq, W, self.shape)
        self.marg = mg

    def draw(self, rng, C):
        a = np.interp(rng.uniform(size=C), self.marg["a"].F, self.marg["a"].xs)
        ia = np.abs(a[:, None] - self.a[None, :]).argmin(axis=1)
        u, b = rng.uniform(size=C), np.empty(C)
        for i in np.unique(ia):
            s = ia == i
            b[s] = np.interp(u[s], self.b_cond_F[i], self.b_grid)
        ib = np.abs(b[:, None] - self.b[None, :]).argmin(axis=1)
        u, p = rng.uniform(size=C), np.empty(C)
        cell = ia * self.b.size + ib
        for c in np.unique(cell):
            s = cell == c
            p[s] = np.interp(u[s], self.cond_F[c // self.b.size, c % self.b.size], self.p)
        return np.stack([p / a, a, b], axis=1)


def quantities(q, std2):
    """chain states (C, d), sigma^2 (C,) -> {name: values}"""
    q = np.asarray(q).reshape(len(std2), -1)
    out = {"Dc": q[:, 0], "sigma2": np.asarray(std2)}
    if q.shape[1] == 3:
        out.update({"a": q[:, 1], "b": q[:, 2], "Dc*a": q[:, 0] * q[:, 1]})
    return out


def ks_distance(x, cdf):
    x = np.sort(x)
    n = x.size
    F = cdf(x)
    return max((np.arange(1, n + 1) / n - F).max(), (F - np.arange(n) / n).max())


def check(tag, ref, q, std2, fails, names=None):
    """Hold C independent chain states to the target: per quantity the mean (|z| < Z_MAX, SE = SD / sqrt(C)), the variance
    (|z| < Z_MAX, SE = v sqrt((kurtosis - 1) / C)) and the KS distance from the marginal CDF (sqrt(C) D < KS_MAX).  Failures are
    appended to `fails`; -> (largest |z|, largest sqrt(C) D)."""
    vals = quantities(q, std2)
    zmax = kmax = 0.0
    for name in names or ref.names:
        x, mg = vals[name], ref.marg[name]
        C = x.size
        if not np.isfinite(x).all():
            fails.append(f"{tag} {name}: {int((~np.isfinite(x)).sum())} non-finite states")
            continue
        zm = (x.mean() - mg.mean) / (mg.sd / np.sqrt(C))
        zv = (x.var() - mg.var) / (mg.var * np.sqrt((mg.kurt - 1.0) / C))
        ks = np.sqrt(C) * ks_distance(x, mg.cdf)
        print(f"{tag} {name}: C {C} mean z {zm:+.2f} var z {zv:+.2f} sqrt(C) D {ks:.2f}")
        zmax, kmax = max(zmax, abs(zm), abs(zv)), max(kmax, ks)
        if not (abs(zm) < Z_MAX and abs(zv) < Z_MAX and ks < KS_MAX):
            fails.append(f"{tag} {name}: mean z {zm:+.2f} var z {zv:+.2f} sqrt(C) D {ks:.2f}")
    return zmax, kmax


def se_table(ref, C):
    """Monte-Carlo standard errors the checks use at C chains, per quantity: mean, variance and each quantile of PROBS."""
    out = {}
    for name, mg in ref.marg.items():
        qs = mg.quantiles() if mg.xs.size > 2 else None
        out[name] = dict(mean=mg.sd / np.sqrt(C), var=mg.var * np.sqrt(max(mg.kurt - 1.0, 1e-12) / C),
                         q=None if qs is None else np.sqrt(np.array(PROBS) * (1 - np.array(PROBS)) / C) / mg.density(qs))
    return out


def grid_shift_in_se(r1, r2, C):
    """Largest change of a reported moment or quantile between two quadratures, in r1's Monte-Carlo SE at C chains."""
    se, worst = se_table(r1, C), {}
    for name, mg in r1.marg.items():
        m2 = r2.marg[name]
        s = [abs(mg.mean - m2.mean) / se[name]["mean"], abs(mg.var - m2.var) / se[name]["var"]]
        if se[name]["q"] is not None:
            s += list(np.abs(mg.quantiles() - m2.quantiles()) / se[name]["q"])
        worst[name] = max(s)
    return worst


# ---- the closed forms, and the chain logic alone on them -------------------------------------------------------------------

CLOSED = {
    1: dict(S0=1.0, q0=[1.0], K=[[4.0]], lo=[0.0], hi=[1.3], shape=12.0),
    3: dict(S0=1.0, q0=[1.0, 2.0, 3.0], K=[[4.0, 1.0, 0.5], [1.0, 3.0, -0.8], [0.5, -0.8, 2.0]], lo=[0.0, 1.4, 2.5],
            hi=[10.0, 2.6, 3.1], shape=12.0),
}


def closed_reference(d):
    c = CLOSED[d]
    fn = quadratic_ssq(c["S0"], c["q0"], c["K"])
    ref = (Posterior1 if d == 1 else Posterior3)(fn, c["lo"][0] if d == 1 else c["lo"], c["hi"][0] if d == 1 else c["hi"], c["shape"])
    return ref, fn, c


def run_injected(engine, ref, fn, c, C, checkpoints, seed, tag, fails):
    """chains from the reference, advanced by mcmc_replay_ssq one iteration at a time with NumPy variates"""
    d, shape = len(c["q0"]), c["shape"]
    rng = np.random.default_rng(seed)
    q = ref.draw(rng, C)
    ssq = fn(*q.T)
    std2 = draw_std2(rng, ssq, shape)
    V = np.tile(np.linalg.inv(np.asarray(c["K"])) * c["S0"] / (2 * shape - d), (C, 1, 1))  # about the posterior's covariance
    engine.mcmc_init_state(q, ssq, std2, V, c["lo"], c["hi"], n0=0.0, prior_len=3)
    zmax, kmax = check(f"{tag} it 0", ref, q, std2, fails)
    for it in range(1, max(checkpoints) + 1):
        z = rng.standard_normal((1, C, d))
        qn, inb = engine.mcmc_propose(z[0])
        qn, inb = np.asarray(qn), np.asarray(inb).astype(bool)
        sn = np.where(inb, fn(*np.where(inb[:, None], qn, np.asarray(c["q0"])[None, :]).T), 0.0)
        engine.mcmc_replay_ssq(z, rng.uniform(size=(1, C)), rng.standard_gamma(shape, (1, C)), sn[None], traces=False)
        if it in checkpoints:
            q, _, std2, _ = (np.asarray(x) for x in engine.get_state())
            z_, k_ = check(f"{tag} it {it}", ref, q, std2, fails)
            zmax, kmax = max(zmax, z_), max(kmax, k_)
    print(f"{tag}: largest |z| {zmax:.2f}, largest sqrt(C) D {kmax:.2f}")


# ---- SSq functions -------------------------------------------------------------------------------------------------------

def checker_ssq(engine, data, chunk=1 << 16):
    """SSq from the checker library's forward solve (the model set on `engine` decides float64 / float32 / DOP853)."""

    def fn(dc, a=None, b=None):
        dc = np.asarray(dc, dtype=np.float64)
        shape = dc.shape
        dc = dc.ravel()
        a = None if a is None else np.broadcast_to(a, shape).ravel()
        b = None if b is None else np.broadcast_to(b, shape).ravel()
        out = np.empty(dc.size)
        for s in range(0, dc.size, chunk):
            sl = slice(s, s + chunk)
            kw = {} if a is None else dict(a=np.ascontiguousarray(a[sl]), b=np.ascontiguousarray(b[sl]))
            out[sl], _ = engine.forward(np.ascontiguousarray(dc[sl]), data=data, want_ssq=True, want_acc=False, **kw)
        return out.reshape(shape)

    return fn


def quadratic_ssq(S0, q0, K):
    """SSq = S0 + (q - q0)^T K (q - q0): the closed forms (Student-t marginal, nu = 2 shape - d)."""
    q0, K = np.atleast_1d(np.asarray(q0, np.float64)), np.atleast_2d(np.asarray(K, np.float64))

    def fn(*q):
        r = [np.asarray(x, np.float64) - c for x, c in zip(q, q0)]
        s = np.full(np.broadcast(*r).shape, float(S0))
        for i in range(len(r)):
            for j in range(len(r)):
                s = s + K[i, j] * r[i] * r[j]
        return s

    return fn
