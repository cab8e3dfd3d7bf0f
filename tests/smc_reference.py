"""
Specification of include/rsf_smc.h in NumPy (TEST INFRASTRUCTURE ONLY, no GPU): tempered sequential Monte Carlo over the box prior.
Every function that sums takes `dtype`: np.longdouble is the specification, np.float64 the restatement whose distance from it
sizes the GPU tolerances (tests/smc_cases.py).  Particles and l are float64 arrays in either case, as the library stores them.

The target with n0 = 0 is pi(q) ~ 1_box(q) SSq(q)^-shape (tests/posterior_reference.py); the particles move through
pi_beta ~ 1_box SSq^(-shape beta), beta from 0 to 1, and carry l = -shape log SSq (-inf where SSq is not finite and positive).

Variates.  Philox4x32-10 with the sampler's keying (csrc/rsf_device.h): counter (particle lo, particle hi, iteration, slot), key =
(seed lo, seed hi); u53(a, b) = (((a << 32 | b) >> 11) + 1) 2^-53 in (0, 1].  Engine.philox reports the words of any counter and
Engine.draws the sampler's normals, uniform and gamma variate of a (seed, particle, iteration): every rule below is one of theirs.
    start      particle = offset + j, iteration 0.  Slot 2 (the accept uniform's): u_0 = u53(w0, w1) — the u of Engine.draws —
               and u_1 = u53(w2, w3); slot 3: u_2 = u53(w0, w1).  q_p = lo_p + u_p (hi_p - lo_p), rounded once; a value on an edge
               moves one ulp into the box.
    move       step k of stage s (`steps` per stage): iteration s steps + k + 1; the normals of slots 0 and 1 (Box-Muller: z0, z1
               = sqrt(-2 log u53(w0, w1)) (cos, sin)(2 pi u53(w2, w3))) and the uniform of slot 2: Engine.draws' z and u.
    resampling one uniform per stage: u53(w0, w1) of the counter (2^32 - 1, 2^32 - 1, stage, 4), the particle no run can hold.
    sigma^2    Engine.draws' gamma variate of iteration `stages steps + 1` (specified in tests/variates_reference.py).

One stage at the temperature beta (steps 2 to 4 of the algorithm):
    lmax = the largest finite l, w_j(delta) = exp(delta (l_j - lmax)), 0 for l_j = -inf.
    delta: the largest step <= 1 - beta with ESS(delta) = (sum w)^2 / sum w^2 >= rho n_finite, by ROUNDS rounds of 16-section: the
        bracket (a, b] starts at (0, 1 - beta]; a round evaluates the SECTIONS candidates a + (b - a) k / 16, k = 1..16 (float64), in
        one read of l, takes k* = the number of leading candidates that pass, and continues in (cand_k*, cand_k*+1]; k* = 16 in the
        first round: delta = 1 - beta, and beta becomes exactly 1.  After the last round delta = a, or b if a is still 0 (progress
        is guaranteed).  n_finite is n from the second stage on, where no particle has l = -inf; the first stage's threshold
        counts the particles that have a target value at all.
    log I += log(sum w / n) + delta lmax; before the first stage log I = log vol(box).
    Systematic resampling: cum = the inclusive prefix sum of w in index order, t_j = ((j + u) cum_{n-1}) / n, ancestor a_j = the
        first i with cum_i > t_j (t_j >= cum_{n-1}: the first i with cum_i >= cum_{n-1}); q and l are gathered through a.
    Move: Sigma = np.cov of the resampled particles (ddof 1), L = chol((2.38^2 / d) Sigma + diag((1e-6 (hi - lo))^2)), `steps`
        Metropolis steps on pi_(beta + delta): q' = q + L z; outside the strict box: rejected; accepted when
        log u < (beta + delta)(l' - l), a non-finite l' rejected (csrc/rsf_kernel_common.h: accept_test).
"""
import math

import numpy as np

LD = np.longdouble
SECTIONS = 16
ROUNDS = 6
SLOT_Z01, SLOT_Z2, SLOT_U, SLOT_U2, SLOT_RESAMPLE = 0, 1, 2, 3, 4
RESAMPLE_PARTICLE = 2 ** 64 - 1
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr (n, 4) and key (2,) of 32-bit words → (n, 4) uint32 (Salmon et al. 2011, Random123's constants)"""
    c = [np.asarray(ctr)[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(int(key[0])), np.uint64(int(key[1]))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=1).astype(np.uint32)


def words(seed, particles, iteration, slot):
    p = np.atleast_1d(np.asarray(particles, dtype=np.uint64))
    ctr = np.stack([p & M32, p >> np.uint64(32), np.full(p.size, int(iteration), np.uint64), np.full(p.size, int(slot), np.uint64)], axis=1)
    return philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))


def u53(hi, lo):
    k = ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> np.uint64(11)
    return (k + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def start_uniforms(seed, particles, d):
    w = words(seed, particles, 0, SLOT_U)
    u = [u53(w[:, 0], w[:, 1]), u53(w[:, 2], w[:, 3])]
    if d > 2:
        w = words(seed, particles, 0, SLOT_U2)
        u.append(u53(w[:, 0], w[:, 1]))
    return np.stack(u[:d], axis=1)


def normals(seed, particles, iteration, d):
    out = []
    for slot in (SLOT_Z01, SLOT_Z2)[:1 if d <= 2 else 2]:
        w = words(seed, particles, iteration, slot)
        r = np.sqrt(-2.0 * np.log(u53(w[:, 0], w[:, 1])))
        a = 2.0 * np.pi * u53(w[:, 2], w[:, 3])
        out += [r * np.cos(a), r * np.sin(a)]
    return np.stack(out[:d], axis=1)


def accept_uniforms(seed, particles, iteration):
    w = words(seed, particles, iteration, SLOT_U)
    return u53(w[:, 0], w[:, 1])


def stage_uniform(seed, stage):
    w = words(seed, [RESAMPLE_PARTICLE], stage, SLOT_RESAMPLE)
    return float(u53(w[:, 0], w[:, 1])[0])


def inbox(q, lo, hi):
    q = np.asarray(q).reshape(-1, np.size(lo))
    return np.all((q > np.asarray(lo)) & (q < np.asarray(hi)), axis=1)


def log_target(ssq, shape, dtype=LD):
    ssq = np.asarray(ssq, dtype=np.float64).reshape(-1)
    ok = np.isfinite(ssq) & (ssq > 0)
    return np.where(ok, (-dtype(shape) * np.log(np.where(ok, ssq, 1).astype(dtype))).astype(np.float64), -np.inf)


def init(seed, offset, n, lo, hi, dtype=LD):
    """the start → q (n, d) float64, strictly inside the box"""
    lo64, hi64 = np.atleast_1d(np.asarray(lo, np.float64)), np.atleast_1d(np.asarray(hi, np.float64))
    u = start_uniforms(seed, offset + np.arange(n, dtype=np.uint64), lo64.size)
    q = (lo64.astype(dtype) + u.astype(dtype) * (hi64 - lo64).astype(dtype)).astype(np.float64)
    q = np.where(q < hi64, q, np.nextafter(hi64, lo64))
    return np.where(q > lo64, q, np.nextafter(lo64, hi64))


def weight_sums(l, deltas, lmax=None, dtype=LD):
    """→ (lmax, n_finite, n_neginf, sums (m, 2) of dtype): sum w and sum w^2 per candidate"""
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    if np.isnan(l).any() or np.isposinf(l).any():
        raise ValueError("l must be finite or -inf")
    fin = np.isfinite(l)
    if not fin.any():
        raise ValueError("every particle has l = -inf")
    lmax = float(l[fin].max()) if lmax is None else float(lmax)
    a = l[fin].astype(dtype) - dtype(lmax)
    sums = np.empty((len(deltas), 2), dtype=dtype)
    for k, dl in enumerate(deltas):
        w = np.exp(dtype(dl) * a)
        sums[k] = w.sum(), (w * w).sum()
    return lmax, int(fin.sum()), int(np.isneginf(l).sum()), sums


def section(target, sums):
    """how many leading candidates keep (sum w)^2 >= target sum w^2"""
    k = 0
    while k < len(sums) and sums[k][0] * sums[k][0] >= target * sums[k][1]:
        k += 1
    return k


def choose_delta(beta, rho, sums_fn):
    """the 16-section search.  sums_fn(deltas) → (lmax, n_finite, n_neginf, sums) → (delta, lmax, sum w at delta, ESS, beta_next)"""
    a, b = 0.0, 1.0 - beta
    last = None
    for rnd in range(ROUNDS):
        cand = [a + (b - a) * k / SECTIONS for k in range(1, SECTIONS + 1)]
        lmax, nfin, _, sums = sums_fn(cand)
        k = section(rho * nfin, sums)
        if k:
            last = (cand[k - 1], sums[k - 1])
        if k == SECTIONS:
            if rnd == 0:
                return b, lmax, sums[-1][0], float(sums[-1][0] ** 2 / sums[-1][1]), 1.0
            break  # cannot happen for a monotone ESS: b failed in the round before
        if k < SECTIONS:
            fail = (cand[k], sums[k])
        a, b = (cand[k - 1] if k else a), cand[k]
    delta, s = last if last is not None else fail
    return delta, lmax, s[0], float(s[0] ** 2 / s[1]), beta + delta


def resample(l, delta, lmax, u, dtype=LD):
    """→ (cum (n,) of dtype, ancestors (n,) int64)"""
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    n = l.size
    fin = np.isfinite(l)
    w = np.where(fin, np.exp(dtype(delta) * (np.where(fin, l, 0).astype(dtype) - dtype(lmax))), dtype(0))
    cum = np.cumsum(w, dtype=dtype)
    W = cum[-1]
    t = ((np.arange(n).astype(dtype) + dtype(u)) * W) / dtype(n)
    anc = np.searchsorted(cum, t, side="right")
    past = ~(t < W)
    if past.any():
        anc[past] = np.searchsorted(cum, W, side="left")
    return cum, anc.astype(np.int64)


def proposal_factor(q, lo, hi):
    q = np.asarray(q, dtype=np.float64).reshape(len(q), -1)
    d = q.shape[1]
    lo, hi = np.atleast_1d(np.asarray(lo, np.float64)), np.atleast_1d(np.asarray(hi, np.float64))
    cov = np.atleast_2d(np.cov(q.T)) if q.shape[0] > 1 else np.zeros((d, d))
    return np.linalg.cholesky((2.38 ** 2 / d) * cov + np.diag((1e-6 * (hi - lo)) ** 2))


def propose(q, L, z, dtype=LD):
    q, z, L = np.asarray(q, dtype=dtype), np.asarray(z, dtype=dtype), np.asarray(L, dtype=dtype)
    qn = np.empty_like(q)
    for p in range(q.shape[1]):
        s = q[:, p].copy()
        for r in range(p + 1):
            s = s + L[p, r] * z[:, r]
        qn[:, p] = s
    return qn.astype(np.float64)


def move_step(q, l, ssq_fn, lo, hi, L, beta, shape, seed, offset, iteration, dtype=LD):
    """one Metropolis step on pi_beta, in place → accepted (n,) bool.  ssq_fn(q (m, d)) → (m,), called inside the box only."""
    n, d = q.shape
    ids = offset + np.arange(n, dtype=np.uint64)
    qn = propose(q, L, normals(seed, ids, iteration, d), dtype)
    inb = inbox(qn, lo, hi)
    ln = np.full(n, -np.inf)
    if inb.any():
        ln[inb] = log_target(ssq_fn(qn[inb]), shape, dtype)
    with np.errstate(invalid="ignore"):
        ratio = np.where(inb, dtype(beta) * (ln.astype(dtype) - l.astype(dtype)), -np.inf)
    logalpha = np.where(ratio > 0, 0, ratio)
    acc = inb & (logalpha > np.log(accept_uniforms(seed, ids, iteration)))
    q[acc], l[acc] = qn[acc], ln[acc]
    return acc


def run(ssq_fn, lo, hi, n, shape, seed=0, offset=0, rho=0.5, steps=3, max_stages=200, dtype=LD, history=False):
    """the whole sampler → dict(q (n, d), l (n,), log_integral, stages [dict(beta, delta, ess, accept_rate, log_integral)]); with
    history also per stage lmax, u, cum, ancestors and the particles and l after every step."""
    lo64, hi64 = np.atleast_1d(np.asarray(lo, np.float64)), np.atleast_1d(np.asarray(hi, np.float64))
    d = lo64.size
    q = init(seed, offset, n, lo64, hi64, dtype)
    l = log_target(ssq_fn(q), shape, dtype)
    logi = dtype(np.sum(np.log((hi64 - lo64).astype(dtype))))
    beta, stages, hist = 0.0, [], []
    while beta < 1.0:
        if len(stages) >= max_stages:
            raise RuntimeError(f"beta = {beta} after {max_stages} stages")
        s = len(stages)
        delta, lmax, sw, ess, beta = choose_delta(beta, rho, lambda cand: weight_sums(l, cand, None, dtype))
        logi = logi + np.log(dtype(sw) / dtype(n)) + dtype(delta) * dtype(lmax)
        u = stage_uniform(seed, s)
        cum, anc = resample(l, delta, lmax, u, dtype)
        q, l = q[anc].copy(), l[anc].copy()
        L = proposal_factor(q, lo64, hi64)
        acc, after = 0, []
        for k in range(steps):
            acc += int(move_step(q, l, ssq_fn, lo64, hi64, L, beta, shape, seed, offset, s * steps + k + 1, dtype).sum())
            if history:
                after.append((q.copy(), l.copy()))
        stages.append(dict(beta=beta, delta=delta, ess=ess, accept_rate=acc / (n * steps), log_integral=float(logi)))
        if history:
            hist.append(dict(lmax=lmax, u=u, cum=cum, ancestors=anc, chol=L, after=after))
    out = dict(q=q, l=l, log_integral=float(logi), stages=stages)
    if history:
        out["history"] = hist
    return out


def log_evidence(log_integral, shape, lo, hi):
    """rsf_evidence_finish's constant: log I - log vol + lgamma(shape) - shape log pi"""
    return float(log_integral - np.sum(np.log(np.asarray(hi, np.float64) - np.asarray(lo, np.float64))) + math.lgamma(shape) - shape * math.log(math.pi))
