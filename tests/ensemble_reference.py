"""
Specification of include/rsf_ensemble.h in NumPy (TEST INFRASTRUCTURE ONLY, no GPU): the affine-invariant stretch move (Goodman &
Weare 2010) in island ensembles, on a supplied ssq_fn(points (m, d)) → SSq (m,).

Islands.  B walkers per half, 2B per island; island k holds the rows k 2B .. (k + 1) 2B - 1 of q (n, d), its first B rows are half
0, the next B half 1.  Walker j draws from the Philox particle offset + j (tests/smc_reference.py: words, u53).

Half-step h of iteration t >= 1, for every walker j of half h of every island:
    draws       the accept slot's (slot 2) four words w0..w3 of (seed, offset + j, t): U_a = u53(w0, w1), U_s = u53(w2, w3); the
                first word w0' of slot 3: partner index r = (w0' B) >> 32 (a 64-bit product), in 0 .. B - 1.  The probability of
                an index differs from 1 / B by at most 2^-32.
    partner     y = walker r of the OTHER half of the same island, in its state at the start of the half-step.
    coordinates bit p of logmask: phi_p(q) = log q_p (needs lo_p >= 0), else q_p; u = phi(x), v = phi(y).
    stretch     s = (a - 1) U_s + 1 (a product, then a sum), z = (s s) / a; u'_p = fma(z, u_p - v_p, v_p), ONE rounding;
                q'_p = exp(u'_p) under a mask bit, else u'_p.  Outside the strict box: rejected, outbox grows.
                J = (d - 1) log z, then + (u'_p - u_p) for the masked p in index order.
    decide      l' = -shape log SSq(q') (-inf where SSq is not finite and > 0); log alpha = J + (l' - l); accepted iff l' is finite
                and min(log alpha, 0) > log U_a.  Accepted: (q, l) <- (q', l'), accepted grows.
    stuck       a walker not strictly inside the box, or with a non-finite l, makes no proposal: stuck grows.  It may still be drawn
                as a partner.

`exact=True` forms the fused multiply-add exactly (math.fma, or rational arithmetic before Python 3.13): with logmask 0 the
proposal is then the library's bit for bit.  `exact=False` rounds the product to long double first — the difference is far below
anything a statistical test sees, and it is vectorised.
"""
import math
from fractions import Fraction

import numpy as np

import smc_reference as smc

SLOT_PARTNER = smc.SLOT_U2


def draws(seed, particles, iteration, B):
    """→ (U_s, U_a, r) of the particles in one iteration"""
    w = smc.words(seed, particles, iteration, smc.SLOT_U)
    ua, us = smc.u53(w[:, 0], w[:, 1]), smc.u53(w[:, 2], w[:, 3])
    w3 = smc.words(seed, particles, iteration, SLOT_PARTNER)
    r = ((w3[:, 0].astype(np.uint64) * np.uint64(B)) >> np.uint64(32)).astype(np.int64)
    return us, ua, r


def stretch(us, a):
    s = (a - 1.0) * us + 1.0
    return (s * s) / a


def _fma_exact(x, y, z):
    if hasattr(math, "fma"):
        return math.fma(x, y, z)
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
        return x * y + z
    return float(Fraction(x) * Fraction(y) + Fraction(z))  # a Fraction rounds to the nearest float64


def fma(x, y, z, exact):
    x, y, z = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(z, np.float64))
    if exact:
        return np.array([_fma_exact(float(a), float(b), float(c)) for a, b, c in zip(x.ravel(), y.ravel(), z.ravel())], dtype=np.float64).reshape(x.shape)
    return (x.astype(np.longdouble) * y.astype(np.longdouble) + z.astype(np.longdouble)).astype(np.float64)


def movers(n, B, half):
    """→ (rows of the walkers of half `half`, first row of the other half of each one's island)"""
    t = np.arange(n // 2)
    base = (t // B) * (2 * B)
    return base + half * B + t % B, base + (1 - half) * B


def healthy(q, l, lo, hi):
    return smc.inbox(q, lo, hi) & np.isfinite(l)


def propose(q, l, lo, hi, B, a, logmask, seed, offset, iteration, half, exact=True):
    """The proposals of one half-step → dict(rows, partner (rows of q), stuck, inbox, q_new (m, d), J, log_ua), m = n / 2 movers"""
    q = np.asarray(q, np.float64)
    n, d = q.shape
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    rows, other = movers(n, B, half)
    us, ua, r = draws(seed, (offset + rows).astype(np.uint64), iteration, B)
    partner = other + r
    ok = healthy(q[rows], np.asarray(l)[rows], lo, hi)
    x, y = q[rows], q[partner]
    z = stretch(us, a)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        J = (d - 1) * np.log(z)
        qn = np.empty_like(x)
        for p in range(d):
            m = (logmask >> p) & 1
            u, v = (np.log(x[:, p]), np.log(y[:, p])) if m else (x[:, p], y[:, p])
            un = fma(z, u - v, v, exact)
            qn[:, p] = np.exp(un) if m else un
            if m:
                J = J + (un - u)
    inb = ok & smc.inbox(qn, lo, hi)
    qn[~ok] = x[~ok]
    return dict(rows=rows, partner=partner, stuck=~ok, inbox=inb, q_new=qn, J=np.where(ok, J, 0.0), log_ua=np.log(ua), z=z)


def decide(pr, l, ssq_new, shape):
    """pr: propose's; ssq_new (m,) at pr['q_new'] (read where inbox) → (accepted (m,), l' (m,), log alpha (m,))"""
    lx = np.asarray(l)[pr["rows"]]
    ln = np.where(pr["inbox"], smc.log_target(np.where(pr["inbox"], ssq_new, 1.0), shape, np.float64), -np.inf)
    with np.errstate(invalid="ignore"):
        la = pr["J"] + (ln - lx)
        acc = pr["inbox"] & np.isfinite(ln) & (np.where(la > 0.0, 0.0, la) > pr["log_ua"])
    return acc, ln, la


def new_counters(n):
    return dict(accepted=np.zeros(n, np.int32), outbox=np.zeros(n, np.int32), stuck=np.zeros(n, np.int32))


def half_step(q, l, ssq_fn, lo, hi, B, a, logmask, shape, seed, offset, iteration, half, counters, exact=True):
    """One half-step IN PLACE in q (n, d), l (n,) and the counters → propose's dict with accepted, l_new and log_alpha added"""
    pr = propose(q, l, lo, hi, B, a, logmask, seed, offset, iteration, half, exact)
    ssq = np.ones(pr["rows"].size)
    if pr["inbox"].any():
        ssq[pr["inbox"]] = np.asarray(ssq_fn(pr["q_new"][pr["inbox"]]), np.float64).reshape(-1)
    acc, ln, la = decide(pr, l, ssq, shape)
    rows = pr["rows"]
    q[rows[acc]] = pr["q_new"][acc]
    l[rows[acc]] = ln[acc]
    counters["accepted"][rows[acc]] += 1
    counters["outbox"][rows[~pr["inbox"] & ~pr["stuck"]]] += 1
    counters["stuck"][rows[pr["stuck"]]] += 1
    pr.update(accepted=acc, l_new=ln, log_alpha=la, ssq_new=ssq)
    return pr


def start_l(q, ssq_fn, shape):
    return smc.log_target(np.asarray(ssq_fn(np.asarray(q, np.float64)), np.float64).reshape(-1), shape, np.float64)


def run(ssq_fn, q0, lo, hi, B, n_iter, shape, a=2.0, logmask=0, seed=0, offset=0, iter0=1, exact=False, checkpoints=()):
    """n_iter iterations from q0 (n, d) → dict(q, l, accepted, outbox, stuck, at={iteration: (q, l) copies})"""
    q = np.array(q0, dtype=np.float64).reshape(len(q0), -1)
    l = start_l(q, ssq_fn, shape)
    cnt, at = new_counters(q.shape[0]), {}
    for it in range(iter0, iter0 + n_iter):
        for half in (0, 1):
            half_step(q, l, ssq_fn, lo, hi, B, a, logmask, shape, seed, offset, it, half, cnt, exact)
        if it in checkpoints:
            at[it] = (q.copy(), l.copy())
    return dict(q=q, l=l, at=at, **cnt)


# ---- the island-level statistic ---------------------------------------------------------------------------------------------------
def island_z(x, island, mean, var):
    """x (n,) a quantity of the walkers, islands of `island` consecutive walkers, the target's mean and variance → (z of the first
    moment, z of the second central moment about the target's mean): (mean of the island means - reference) / (SD of the island
    means / sqrt(islands)).  Islands are independent replicates, so this holds whatever the dependence inside an island."""
    x = np.asarray(x, np.float64).reshape(-1, island)
    k = x.shape[0]
    m1, m2 = x.mean(axis=1), ((x - mean) ** 2).mean(axis=1)
    return ((m1.mean() - mean) / (m1.std(ddof=1) / math.sqrt(k)), (m2.mean() - var) / (m2.std(ddof=1) / math.sqrt(k)))


def island_check(tag, ref, vals, island, fails, z_max):
    """vals {name: (n,)} (posterior_reference.quantities) held to ref.marg by island_z → the largest |z|; failures appended"""
    worst = 0.0
    for name in ref.names:
        mg = ref.marg[name]
        z1, z2 = island_z(vals[name], island, mg.mean, mg.var)
        print(f"{tag} {name}: islands {vals[name].size // island} x {island}: first moment z {z1:+.2f}, second moment z {z2:+.2f}")
        worst = max(worst, abs(z1), abs(z2))
        if not (abs(z1) < z_max and abs(z2) < z_max):
            fails.append(f"{tag} {name}: island z {z1:+.2f} / {z2:+.2f}")
    return worst
