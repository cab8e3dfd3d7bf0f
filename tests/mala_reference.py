"""
The specification of the Gauss-Newton manifold MALA sampler (include/rsf_mala.h), in NumPy (a test helper; TEST INFRASTRUCTURE
ONLY, no GPU).  The simplified manifold MALA of Girolami & Calderhead (2011) with the Gauss-Newton metric; its target is
pi(q) ~ 1_box(q) SSq(q)^-shape (tests/posterior_reference.py).

Chain state: q[d], ssq, g[d] = X^T r, H[d][d] = X^T X (tests/fit_reference.normal's).  Constants eps > 0, lam >= 0, shape > 0.
Draws per chain and iteration: z (d normals) and u in (0, 1].

Propose:
    1. A = H + lam diag(H) = L L^T, fit_reference.trial's factor in its operation order.  A pivot that is not positive and
       finite, or an ssq that is not finite and > 0: no proposal, the chain is STUCK for this iteration.
    2. delta = -A^-1 g (the two triangular solves of fit_reference.trial); L^T w = z.
    3. s = eps sqrt(ssq / (2 shape)).
    4. q'_p = (q_p + (0.5 eps^2) delta_p) + s w_p; inside iff lo_p < q'_p < hi_p for every p.  ld = sum_p log L_pp.
Decide, with (ssq', g', H') at q':
    1. rejected if ssq' is not finite and > 0 or A' = H' + lam diag(H') does not factor.
    2. delta' = -A'^-1 g', e = q - (q' + (0.5 eps^2) delta'), v = L'^T e, ld' = sum_p log L'_pp.
    3. log alpha = -(shape + d / 2) (log ssq' - log ssq) + (ld' - ld) + 1/2 sum z^2 - (shape / (ssq' eps^2)) sum v^2.
    4. accepted iff log u < log alpha (a NaN compares false); the margin is log alpha - log u.
    5. accepted: (q, ssq, g, H) <- (q', ssq', g', H').

Everything is float64 and vectorised over the chains with the coordinates' loops written out, so that every operation is the IEEE
one csrc/rsf_kernels_mala.h takes, in its order (NumPy fuses nothing).
"""
import numpy as np


def factor(H, lam):
    """A = H + lam diag(H) = L L^T for every chain -> (ok (n,) bool, L (n, d, d), ld (n,)); rows that are not ok hold rubbish"""
    H = np.asarray(H, dtype=np.float64)
    n, d = H.shape[0], H.shape[1]
    L = np.zeros((n, d, d))
    ok = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for p in range(d):
            for r in range(p + 1):
                s = H[:, p, r].copy()
                if r == p:
                    s = s + lam * s
                for k in range(r):
                    s = s - L[:, p, k] * L[:, r, k]
                if r == p:
                    ok &= (s > 0.0) & (s < np.inf)
                    L[:, p, p] = np.sqrt(s)
                else:
                    L[:, p, r] = s / L[:, r, r]
        ld = np.log(L[:, 0, 0])
        for p in range(1, d):
            ld = ld + np.log(L[:, p, p])
    return ok, L, np.where(ok, ld, 0.0)


def step(L, g):
    """delta = -(L L^T)^-1 g"""
    n, d = g.shape
    y = np.zeros((n, d))
    with np.errstate(all="ignore"):
        for p in range(d):
            s = -g[:, p]
            for k in range(p):
                s = s - L[:, p, k] * y[:, k]
            y[:, p] = s / L[:, p, p]
        for p in range(d - 1, -1, -1):
            s = y[:, p].copy()
            for k in range(p + 1, d):
                s = s - L[:, k, p] * y[:, k]
            y[:, p] = s / L[:, p, p]
    return y


def propose(q, ssq, g, H, z, lo, hi, eps, lam, shape):
    """-> (q' (n, d): a chain without a proposal inside the box has its q, inbox (n,) bool, stuck (n,) bool, ld (n,))"""
    q, ssq, g, z = (np.asarray(x, dtype=np.float64) for x in (q, ssq, g, z))
    n, d = q.shape
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(d), np.asarray(hi, dtype=np.float64).reshape(d)
    ok, L, ld = factor(H, lam)
    with np.errstate(all="ignore"):
        ok = ok & (ssq > 0.0) & (ssq < np.inf)
        y = step(L, g)
        w = np.zeros((n, d))
        for p in range(d - 1, -1, -1):
            s = z[:, p].copy()
            for k in range(p + 1, d):
                s = s - L[:, k, p] * w[:, k]
            w[:, p] = s / L[:, p, p]
        s = eps * np.sqrt(ssq / (2.0 * shape))
        h = 0.5 * (eps * eps)
        qn = np.stack([(q[:, p] + h * y[:, p]) + s * w[:, p] for p in range(d)], axis=1)
        inbox = ok & ((qn > lo) & (qn < hi)).all(axis=1)
    return np.where(inbox[:, None], qn, q), inbox, ~ok, ld


def decide(q, ssq, ld, z, u, qn, inbox, ssq_n, g_n, H_n, eps, lam, shape):
    """-> (accepted (n,) bool, log alpha (n,), margin (n,) = log alpha - log u); chains whose inbox is False are rejected, their
    log alpha and margin are NaN"""
    q, ssq, z, qn, ssq_n, g_n = (np.asarray(x, dtype=np.float64) for x in (q, ssq, z, qn, ssq_n, g_n))
    n, d = q.shape
    ok, L, ld_n = factor(H_n, lam)
    with np.errstate(all="ignore"):
        ok = ok & np.asarray(inbox, dtype=bool) & (ssq_n > 0.0) & (ssq_n < np.inf)
        y = step(L, g_n)
        eps2 = eps * eps
        h = 0.5 * eps2
        e = np.stack([q[:, p] - (qn[:, p] + h * y[:, p]) for p in range(d)], axis=1)
        zz, vv = np.zeros(n), np.zeros(n)
        for p in range(d):
            zz = zz + z[:, p] * z[:, p]
        for p in range(d):
            v = L[:, p, p] * e[:, p]
            for k in range(p + 1, d):
                v = v + L[:, k, p] * e[:, k]
            vv = vv + v * v
        la = ((-(shape + 0.5 * d) * (np.log(ssq_n) - np.log(ssq)) + (ld_n - ld)) + 0.5 * zz) - (shape / (ssq_n * eps2)) * vv
        la = np.where(ok, la, np.nan)
        log_u = np.log(np.asarray(u, dtype=np.float64))
        acc = ok & (log_u < la)
    return acc, la, la - log_u


def new_state(q, ssq, g, H):
    n = len(q)
    return {"q": np.array(q, dtype=np.float64).reshape(n, -1), "ssq": np.array(ssq, dtype=np.float64), "g": np.array(g, dtype=np.float64),
            "H": np.array(H, dtype=np.float64), "accepted": np.zeros(n, dtype=np.int32), "outbox": np.zeros(n, dtype=np.int32),
            "stuck": np.zeros(n, dtype=np.int32)}


def iterate(normal_fn, st, z, u, lo, hi, eps, lam, shape):
    """One iteration of every chain, in place.  normal_fn(points (n, d)) -> (ssq, g, H); a chain without a proposal inside the
    box is evaluated at its own point and the result ignored.  -> dict(qn, inbox, stuck, accepted, log_alpha, margin, ssq_n, g_n, H_n)"""
    qn, inbox, stuck, ld = propose(st["q"], st["ssq"], st["g"], st["H"], z, lo, hi, eps, lam, shape)
    ssq_n, g_n, H_n = (np.asarray(x, dtype=np.float64) for x in normal_fn(qn))
    acc, la, margin = decide(st["q"], st["ssq"], ld, z, u, qn, inbox, ssq_n, g_n, H_n, eps, lam, shape)
    st["q"][acc], st["ssq"][acc], st["g"][acc], st["H"][acc] = qn[acc], ssq_n[acc], g_n[acc], H_n[acc]
    st["accepted"] += acc
    st["outbox"] += ~inbox & ~stuck
    st["stuck"] += stuck
    return {"qn": qn, "inbox": inbox, "stuck": stuck, "accepted": acc, "log_alpha": la, "margin": margin, "ssq_n": ssq_n, "g_n": g_n, "H_n": H_n}


def run(normal_fn, q0, lo, hi, n_iter, eps, lam, shape, rng, checkpoints=(), on_checkpoint=None):
    """n_iter iterations from q0 with NumPy variates -> state; on_checkpoint(it, state) is called after the iterations listed"""
    q0 = np.asarray(q0, dtype=np.float64).reshape(len(q0), -1)
    st = new_state(q0, *normal_fn(q0))
    n, d = q0.shape
    for it in range(1, int(n_iter) + 1):
        iterate(normal_fn, st, rng.standard_normal((n, d)), 1.0 - rng.uniform(size=n), lo, hi, eps, lam, shape)
        if it in checkpoints and on_checkpoint is not None:
            on_checkpoint(it, st)
    return st
