"""
What tests/test_kstiff_reference.py (CPU) and tests/test_gpu_kstiff.py share (a test helper): the problems of the sampler with
the stiffness among the parameters (tests/kstiff_reference.py), each solved ONCE per process.

    wrong_k(history)     the "why" table: on stiff_cases.why_problem's friction data (Dc = 20, k = 2e-3) the best Dc over BF_BOX with
                         k fixed 20 % low and 20 % high
    problem2(history)    d = 2, (Dc, k) on why_problem(history)'s data: the least-squares point, its Laplace SDs, the box
    yardstick2(...)      the quadrature of problem2 with a caller's SSq (the CPU specification's, or the parent's kernel's)
    problem4(law)        d = 4, (Dc, a, b, k) on friction data of why_problem's recipe under `law` and the step history: the
                         least-squares point, its Laplace covariance, BOX4, and the importance-sampling yardstick by the specification
    closed4()            the chain logic's closed-form target: dr_cases' quadratic SSq widened to four parameters, with its
                         exact marginals by tensor Gauss-Legendre quadrature and exact draws by rejection
"""
import functools

import numpy as np

import kstiff_reference as KR
import law_cases as C
import law_reference as R
import posterior_reference as P
import stiff_cases as SC
import stiff_reference as S

OBS = "mu"
K_BOX = (5e-4, 8e-3)  # the stiffness's prior box in every sampler test: K_WHY = 2e-3 lies inside
BOX2 = (np.array([R.BF_BOX[0], K_BOX[0]]), np.array([R.BF_BOX[1], K_BOX[1]]))
BOX4 = (np.array([5.0, 0.005, 0.008, K_BOX[0]]), np.array([200.0, 0.02, 0.025, K_BOX[1]]))
# the importance draws: a seed has to meet the yardstick's own conditions, which the tests assert (every draw inside the box, ESS, the
# largest weight); about one seed in ten puts a t5 draw tens of SDs out, beyond the box (11 does)
IS_N, IS_SEED = 16384, 0
WRONG = (0.8, 1.2)  # the calibration errors of the "why" table


def truth(m, d):
    return np.array([R.BF_TRUTH, SC.K_WHY]) if d == 2 else np.array([R.BF_TRUTH, m.a, m.b, SC.K_WHY])


@functools.lru_cache(maxsize=None)
def wrong_k(history):
    """-> {factor: (best Dc, best SSq / the true-k best SSq)} for k fixed at factor * K_WHY, factor in WRONG, on why_problem's nodes"""
    p = SC.why_problem(history)
    floor = p["ssq_stiff"].min()
    out = {}
    for f in WRONG:
        ssq = S.forward(p["m"], f * SC.K_WHY, p["x"], p["vl"], "aging", OBS, data=p["data"])[1]
        out[f] = (float(p["x"][np.argmin(ssq)]), float(ssq.min() / floor))
    return out


@functools.lru_cache(maxsize=None)
def problem2(history):
    """-> dict(m, vl, data, shape, q: the least-squares (Dc, k), sd, cond, ssq, lo, hi)"""
    p = SC.why_problem(history)
    q, J, ssq = KR.fit(p["m"], p["vl"], "aging", OBS, truth(p["m"], 2), p["data"])
    _, sd, cond = KR.laplace(J, ssq, p["data"].size)
    return dict(m=p["m"], vl=p["vl"], data=p["data"], shape=0.5 * p["data"].size, q=q, sd=sd, cond=cond, ssq=ssq, lo=BOX2[0], hi=BOX2[1])


def yardstick2(history, fn=None, n=(129, 65)):
    """problem2's posterior by quadrature with the SSq of fn (default: the CPU specification's)"""
    p = problem2(history)
    fn = KR.ssq_fn(p["m"], p["vl"], "aging", OBS, p["data"]) if fn is None else fn
    return KR.quadrature2(fn, p["q"], p["sd"], p["shape"], n=n)


@functools.lru_cache(maxsize=None)
def data4(law):
    """friction data of why_problem's recipe under `law` and the step history"""
    m = C.spec()
    vl = R.table(m, "step")
    clean = S.forward(m, SC.K_WHY, [R.BF_TRUTH], vl, law, OBS)[0][:, 0]
    return m, vl, clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(SC.WHY_SEED).standard_normal(clean.size)


@functools.lru_cache(maxsize=None)
def problem4(law):
    """-> dict(m, vl, data, shape, q: the least-squares (Dc, a, b, k), cov, sd, cond, lo, hi, truth_sd, truth_cond: the Laplace SDs
    and the condition number AT THE TRUTH, yard: importance4's result by the CPU specification)"""
    m, vl, data = data4(law)
    t = truth(m, 4)
    Jt, _, st = KR.normal(m, vl, law, OBS, t, data)
    _, truth_sd, truth_cond = KR.laplace(Jt, st, data.size)
    q, J, ssq = KR.fit(m, vl, law, OBS, t, data)
    cov, sd, cond = KR.laplace(J, ssq, data.size)
    yard = KR.importance4(KR.ssq_fn(m, vl, law, OBS, data), q, cov, 0.5 * data.size, BOX4[0], BOX4[1], n=IS_N, seed=IS_SEED)
    return dict(m=m, vl=vl, data=data, shape=0.5 * data.size, q=q, cov=cov, sd=sd, cond=cond, ssq=ssq, lo=BOX4[0], hi=BOX4[1], truth_sd=truth_sd,
                truth_cond=truth_cond, yard=yard)


# ---- the closed form at d = 4 -----------------------------------------------------------------------------------------------------
# posterior_reference.CLOSED[3] (dr_cases' closed form) with a fourth parameter, the "stiffness": coupled to the other three, its
# box in k > 0 and cutting the density 0.7 SD above its centre.  SSq = S0 + (q - q0)^T K (q - q0): pi ~ SSq^-shape is a multivariate
# t with nu = 2 shape - 4 = 20 and scale matrix S0 K^-1 / nu, cut by the box.
CLOSED4 = dict(S0=1.0, q0=[1.0, 2.0, 3.0, 0.5], K=[[4.0, 1.0, 0.5, 0.3], [1.0, 3.0, -0.8, -0.4], [0.5, -0.8, 2.0, 0.2], [0.3, -0.4, 0.2, 2.5]],
               lo=[0.0, 1.4, 2.5, 0.1], hi=[10.0, 2.6, 3.1, 0.6], shape=12.0)
NAMES4 = ("Dc", "a", "b", "k", "sigma2")
C_TARGET, CHECKPOINTS, SEED4 = 262144, (4, 8), 31  # dr_cases' own
LEG4 = (1.0, 0.2)  # (scale of the factor, gamma): dr_cases.LEGS' d = 3 leg


class Closed4:
    """The box-cut multivariate t of CLOSED4 on a tensor Gauss-Legendre grid of n = (n0, n1, n2, n3) nodes; the first axis covers
    [lo0, top] only, and what lies above `top` is bounded in `outside`.  marg: posterior_reference.Marginal per name of NAMES4."""

    def __init__(self, n=(48, 24, 24, 24), top=3.0):
        c = CLOSED4
        self.c, self.fn = c, P.quadratic_ssq(c["S0"], c["q0"], c["K"])
        lo, hi = np.array(c["lo"]), np.array(c["hi"])
        hi_q = hi.copy()
        hi_q[0] = top
        nodes, wts = [], []
        for p in range(4):
            t, gw = np.polynomial.legendre.leggauss(n[p])
            nodes.append(lo[p] + (hi_q[p] - lo[p]) * (t + 1) / 2)
            wts.append(gw * (hi_q[p] - lo[p]) / 2)
        G = np.meshgrid(*nodes, indexing="ij")
        ssq = self.fn(*G)
        f = ssq ** -c["shape"]
        W = f * wts[0][:, None, None, None] * wts[1][None, :, None, None] * wts[2][None, None, :, None] * wts[3][None, None, None, :]
        Z = W.sum()
        # above `top`: SSq >= S0 + lam_min (top - q0_0)^2 on a volume of (hi0 - top) x the other widths
        lam = np.linalg.eigvalsh(np.array(c["K"])).min()
        self.outside = float((c["S0"] + lam * (top - c["q0"][0]) ** 2) ** -c["shape"] * (hi[0] - top) * np.prod(hi[1:] - lo[1:]) / Z)
        W = W / Z
        self.marg = {}
        for p, name in enumerate(NAMES4[:4]):
            wm = W.sum(axis=tuple(a for a in range(4) if a != p))
            mean, var, kurt = P._moments(nodes[p], wm)
            xs, F = self._legendre_cdf(wm / wts[p], lo[p], hi_q[p], n[p])
            self.marg[name] = P.Marginal(mean, var, kurt, xs, F)
        self.marg["sigma2"] = P.sigma2_marginal(ssq, W, c["shape"])

    @staticmethod
    def _legendre_cdf(f, lo, hi, n, n_grid=4001):
        """posterior_reference.Posterior3._legendre_cdf: the CDF of the Legendre series through the node densities"""
        t = np.polynomial.legendre.leggauss(n)[0]
        tg = np.linspace(-1.0, 1.0, n_grid)
        coef = np.polynomial.legendre.legfit(t, f, n - 1)
        F = np.polynomial.legendre.legval(tg, np.polynomial.legendre.legint(coef, lbnd=-1.0))
        return lo + (hi - lo) * (tg + 1) / 2, np.maximum.accumulate(np.clip(F, 0.0, None))

    def draw(self, rng, n):
        """n exact draws: the multivariate t, kept where it falls inside the box"""
        c = self.c
        nu = 2 * c["shape"] - 4
        Lc = np.linalg.cholesky(c["S0"] * np.linalg.inv(np.array(c["K"])) / nu)
        lo, hi, out, have = np.array(c["lo"]), np.array(c["hi"]), [], 0
        while have < n:
            z = rng.standard_normal((2 * n, 4)) / np.sqrt(rng.chisquare(nu, 2 * n) / nu)[:, None]
            q = np.array(c["q0"]) + z @ Lc.T
            q = q[((q > lo) & (q < hi)).all(axis=1)]
            out.append(q)
            have += len(q)
        return np.ascontiguousarray(np.concatenate(out)[:n])


@functools.lru_cache(maxsize=None)
def closed4():
    return Closed4()


def closed4_factor(scale):
    """dr_cases.closed_factor at d = 4"""
    c = CLOSED4
    return scale * np.linalg.cholesky(np.linalg.inv(np.array(c["K"])) * c["S0"] / (2 * c["shape"] - 4))


def check4(tag, ref, q, std2, fails):
    """posterior_reference.check's rule and bounds on the four parameters and sigma^2: per quantity the mean and the variance
    (|z| < Z_MAX) and the KS distance from the marginal CDF (sqrt(C) D < KS_MAX) -> (largest |z|, largest sqrt(C) D)"""
    vals = dict(zip(NAMES4, list(np.asarray(q).T) + [np.asarray(std2)]))
    zmax = kmax = 0.0
    for name in NAMES4:
        x, mg = vals[name], ref.marg[name]
        n = x.size
        if not np.isfinite(x).all():
            fails.append(f"{tag} {name}: {int((~np.isfinite(x)).sum())} non-finite states")
            continue
        zm = (x.mean() - mg.mean) / (mg.sd / np.sqrt(n))
        zv = (x.var() - mg.var) / (mg.var * np.sqrt((mg.kurt - 1.0) / n))
        ks = np.sqrt(n) * P.ks_distance(x, mg.cdf)
        print(f"{tag} {name}: C {n} mean z {zm:+.2f} var z {zv:+.2f} sqrt(C) D {ks:.2f}")
        zmax, kmax = max(zmax, abs(zm), abs(zv)), max(kmax, ks)
        if not (abs(zm) < P.Z_MAX and abs(zv) < P.Z_MAX and ks < P.KS_MAX):
            fails.append(f"{tag} {name}: mean z {zm:+.2f} var z {zv:+.2f} sqrt(C) D {ks:.2f}")
    return zmax, kmax
