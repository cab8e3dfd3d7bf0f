"""
Extended-precision reference of compute_initial_covariance and the initial SSq (a test helper; TEST INFRASTRUCTURE ONLY).

`initial_state_ext` is rsf_mcmc_init's float64 part (MCMC.py:244-266, 468; oracle/rsf_oracle.c rsf_mcmc_init) computed in
np.longdouble from the solves of an extended-precision reference — rk4_extended.forward_ext or dop853_extended.solve — so that
its distance from a float64 init is that init's own rounding, amplified by the forward difference:
  ssq0     sum_k (acc_k(q) - data_k)^2 over every sample, the chain's own observation series
  std2_0   ssq0 / (N - (prior_len or d))
  X        X_pk = (acc_k(q^(p)) - acc_k(q)) / (q^(p)_p fd), q^(p) = q with parameter p times (1 + fd), formed in float64 as the
           kernel and the restatement form it, then widened exactly (the perturbed value in the denominator, MCMC.py:264)
  V        d = 1: std2_0 / X^T X (MCMC.py:265-266); d = 3: W M^-1 W with M = W X^T X W / std2_0 + 12 I, W = diag(hi - lo)
           (csrc/rsf_kernels_core.h initial_covariance)
np.linalg rejects longdouble: the 3x3 inverse is written out by cofactors (inverse3).
"""
import numpy as np

LD = np.longdouble


def _w(x):
    """float64 -> longdouble, exactly"""
    return np.asarray(np.asarray(x, dtype=np.float64), dtype=LD)


def inverse3(M):
    """inverse of (..., 3, 3) matrices by cofactors (adjugate / determinant), in M's dtype"""
    M = np.asarray(M)
    a, b, c = M[..., 0, 0], M[..., 0, 1], M[..., 0, 2]
    d, e, f = M[..., 1, 0], M[..., 1, 1], M[..., 1, 2]
    g, h, i = M[..., 2, 0], M[..., 2, 1], M[..., 2, 2]
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    det = a * c00 + b * c01 + c * c02
    adj = np.stack([np.stack([c00, c * h - b * i, b * f - c * e], axis=-1),
                    np.stack([c01, a * i - c * g, c * d - a * f], axis=-1),
                    np.stack([c02, b * g - a * h, a * e - b * d], axis=-1)], axis=-2)
    return adj / det[..., None, None]


def perturbed_points(m, q0, fd):
    """-> pq (d + 1, C, 3) float64: row 0 the start points (Dc, a, b) (d = 1: the model's a, b), row p + 1 parameter p times
    (1 + fd), rounded to float64 as the kernel rounds it"""
    q0 = np.asarray(q0, dtype=np.float64)
    C, d = q0.shape
    pq = np.empty((d + 1, C, 3))
    pq[:, :, 0] = q0[:, 0]
    pq[:, :, 1] = q0[:, 1] if d == 3 else float(m.a)
    pq[:, :, 2] = q0[:, 2] if d == 3 else float(m.b)
    for p in range(d):
        pq[p + 1, :, p] = pq[p + 1, :, p] * (1 + fd)
    return pq


def initial_state_ext(solve, m, q0, data, fd, prior_len, lo, hi, acc0=None):
    """-> (ssq0 [C], std2_0 [C], V [C, d, d]) in longdouble for the start points q0 (C, d), d = 1 (Dc) or 3 (Dc, a, b).
    solve(m, dc, a, b) -> (acc [N, L], ...): an extended-precision forward solve.  data: one series (N,), or one per chain group
    (G, N), the chains split evenly over the groups in order.  acc0: the solve at q0 itself (N, C), if the caller has it."""
    q0 = np.asarray(q0, dtype=np.float64)
    C, d = q0.shape
    data = np.atleast_2d(np.asarray(data, dtype=np.float64))
    G, N = data.shape
    assert C % G == 0, (C, G)
    pq = perturbed_points(m, q0, fd)
    rows = range(d + 1) if acc0 is None else range(1, d + 1)
    pts = pq[list(rows)].reshape(-1, 3)
    acc = np.asarray(solve(m, pts[:, 0], pts[:, 1], pts[:, 2])[0], dtype=LD).reshape(N, len(rows), C)
    if acc0 is None:
        acc0, accp = acc[:, 0], acc[:, 1:]
    else:
        acc0, accp = np.asarray(acc0, dtype=LD), acc
    assert acc0.shape == (N, C), acc0.shape
    r = acc0 - _w(data)[np.arange(C) // (C // G)].T
    ssq0 = (r * r).sum(axis=0)
    X = np.empty((d, N, C), dtype=LD)
    for p in range(d):
        X[p] = (accp[:, p] - acc0) / (_w(pq[p + 1, :, p]) * _w(fd))
    xtx = np.einsum("pkc,rkc->cpr", X, X)
    std2 = ssq0 / LD(N - (prior_len or d))
    if d == 1:
        V = (std2 / xtx[:, 0, 0]).reshape(C, 1, 1)
    else:
        w = _w(np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64))
        M = w[None, :, None] * xtx * w[None, None, :] / std2[:, None, None] + LD(12) * np.eye(3, dtype=LD)
        V = w[None, :, None] * inverse3(M) * w[None, None, :]
    return ssq0, std2, V


def v_errors(V, V_ext):
    """per-chain error of a proposal covariance: d = 1 relative; d = 3 max over entries of |V - V_ext| / sqrt(V_pp V_rr)
    of the reference (test_three_parameter_chains' normalisation) -> float64 (C,)"""
    V_ext = np.asarray(V_ext, dtype=LD)
    dV = np.abs(_w(V).reshape(V_ext.shape) - V_ext)
    sd = np.sqrt(np.diagonal(V_ext, axis1=1, axis2=2))
    return (dV / (sd[:, :, None] * sd[:, None, :])).max(axis=(1, 2)).astype(np.float64)


def rel(g, ref):
    """per-chain relative error of a float64 result against a longdouble reference"""
    return (np.abs(_w(g) - ref) / np.abs(ref)).astype(np.float64)
