"""
NumPy restatement of the convergence diagnostics of include/rsf_diag.h, in np.longdouble: the specification that
tests/test_diagnostics_reference.py and tests/test_gpu_diagnostics.py hold the library to.

A trace is the iteration-major block x[n][C][d] that rsf_mcmc_run writes; chain c of parameter p is x[:, c, p].  Per parameter,
with N = floor(n/2):

Split chains.  Each chain becomes two: its first N and its last N draws (the middle draw is dropped when n is odd), M' = 2C
chains of length N.  Split chain m has mean xbar_m and variance s2_m (ddof 1); W = mean_m s2_m, B/N = var_m(xbar_m) (ddof 1),
var_plus = (N-1)/N W + B/N, split_rhat = sqrt(var_plus / W).

Multi-chain ESS (the non-rank-normalised "mean" ESS of Stan and ArviZ, on the split chains).  acov_m(t) = 1/N
sum_{i<N-t} (y_i - xbar_m)(y_{i+t} - xbar_m), A(t) = mean_m acov_m(t), rho(t) = 1 - (W - A(t)) / var_plus, rho(0) = 1.  Then,
as ArviZ's `_ess` does it (`finish` below, step by step):
  1. even = 1, odd = rho(1); t = 1.
  2. Geyer's initial positive sequence: while t < N - 3 and even + odd > 0: even = rho(t+1), odd = rho(t+2); the pair is kept
     (rho_t[t+1], rho_t[t+2] = even, odd) when even + odd >= 0; t += 2.
  3. max_t = t - 2; if even > 0 the last even term is kept: rho_t[max_t + 1] = even.
  4. Geyer's initial monotone sequence: for t = 1, 3, ... while t <= max_t - 2: if rho_t[t+1] + rho_t[t+2] > rho_t[t-1] +
     rho_t[t], both become (rho_t[t-1] + rho_t[t]) / 2.
  5. tau = -1 + 2 sum_{t <= max_t} rho_t[t] + rho_t[max_t + 1], tau = max(tau, 1/log10(M'N)), ess = M'N / tau,
     mcse_mean = sqrt(var_plus / ess).
  With only the lags [0, n_lags) known, step 2 also stops before it would need lag n_lags (t < n_lags - 2); when that, and
  not N or a non-positive pair, ended it, `lags_complete` is False and the statistics are those of the sequence so cut.

Nested R-hat (Margossian et al. 2024; unsplit chains).  K superchains of S chains, superchain k holding chains [kS, (k+1)S):
chain means xbar_mk, superchain means xbar_k, overall mean xbar.  B_nu = 1/(K-1) sum_k (xbar_k - xbar)^2, Btilde_k = 1/(S-1)
sum_m (xbar_mk - xbar_k)^2 (0 when S = 1), Wtilde_k = mean_m of the chains' variances (ddof 1), W_nu = mean_k (Btilde_k +
Wtilde_k), nested_rhat = sqrt(1 + B_nu / W_nu).  NaN without superchains, with K = 1, or with W_nu = 0.

Degenerate cases.  W = 0 (every split chain constant): split_rhat, ess, tau and mcse_mean are NaN.  A non-finite draw makes
every statistic of its parameter NaN (K and lags_complete excepted).

Additive partials about a centre c[p] (default: the first draw of chain 0), per parameter HEAD + L values:
  [M', sum(xbar_m - c), sum(xbar_m - c)^2, sum s2_m, K, sum_k(xbar_k - c), sum_k(xbar_k - c)^2, sum_k Btilde_k, sum_k Wtilde_k,
   A_sum(lag_begin .. lag_end - 1)],  A_sum(t) = sum_m acov_m(t).
They add across disjoint sets of chains; everything above is a function of them (`finish`).  mean = c + sum(xbar_m - c)/M'.

Rank normalisation, folded R-hat and tail ESS are not part of this.
"""
import numpy as np

LD = np.longdouble
HEAD = 9
OUT = ("mean", "var_plus", "W", "B_over_N", "split_rhat", "nested_rhat", "K", "ess", "tau", "mcse_mean", "lags_complete")


def _trace(trace):
    x = np.asarray(trace)
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3 or x.shape[0] < 4:
        raise ValueError("a trace is (n >= 4, C[, d])")
    return x.astype(LD)


def default_center(trace):
    return np.asarray(_trace(trace)[0, 0], dtype=np.float64)


class Trace:
    """The split chains of a trace, centred on their own means, in long double; lag sums on demand."""

    def __init__(self, trace, superchain_size=None, center=None):
        x = _trace(trace)
        self.n, self.C, self.d = x.shape
        self.N = self.n // 2
        self.S = int(superchain_size or 0)
        self.center = np.asarray(x[0, 0] if center is None else np.broadcast_to(np.asarray(center, dtype=np.float64), (self.d,)), dtype=LD)
        halves = np.concatenate([x[: self.N], x[self.n - self.N:]], axis=1)  # (N, 2C, d)
        self.xbar = halves.mean(axis=0)
        self.s2 = halves.var(axis=0, ddof=1)
        self.y = halves - self.xbar
        c = self.center
        head = np.zeros((self.d, HEAD), dtype=LD)
        head[:, 0] = 2 * self.C
        head[:, 1] = (self.xbar - c).sum(axis=0)
        head[:, 2] = ((self.xbar - c) ** 2).sum(axis=0)
        head[:, 3] = self.s2.sum(axis=0)
        if self.S:
            if self.C % self.S:
                raise ValueError("superchain_size must divide the number of chains")
            K = self.C // self.S
            cm = x.mean(axis=0).reshape(K, self.S, self.d)
            cv = x.var(axis=0, ddof=1).reshape(K, self.S, self.d)
            xk = cm.mean(axis=1)
            bt = cm.var(axis=1, ddof=1) if self.S > 1 else np.zeros_like(xk)
            head[:, 4] = K
            head[:, 5] = (xk - c).sum(axis=0)
            head[:, 6] = ((xk - c) ** 2).sum(axis=0)
            head[:, 7] = bt.sum(axis=0)
            head[:, 8] = cv.mean(axis=1).sum(axis=0)
        self.head = head

    def lag_sums(self, lag_begin, lag_end):
        """A_sum(t) = sum_m acov_m(t) for t in [lag_begin, lag_end) → (d, L)."""
        N = self.N
        out = np.empty((self.d, lag_end - lag_begin), dtype=LD)
        for j, t in enumerate(range(lag_begin, lag_end)):
            out[:, j] = (self.y[: N - t] * self.y[t:]).sum(axis=(0, 1)) / N
        return out

    def partials(self, lag_begin=0, lag_end=None):
        lag_end = self.N if lag_end is None else lag_end
        return np.concatenate([self.head, self.lag_sums(lag_begin, lag_end)], axis=1)


def partials(trace, superchain_size=None, center=None, lag_begin=0, lag_end=None):
    """The additive partials (d, HEAD + L), long double."""
    return Trace(trace, superchain_size, center).partials(lag_begin, lag_end)


def finish(n, partials, center, superchain_size=None, n_lags=None):
    """The statistics of summed partials whose lags are [0, n_lags) → one dict per parameter (long double values)."""
    part = np.asarray(partials, dtype=LD)
    part = part.reshape(-1, part.shape[-1])
    n_lags = part.shape[1] - HEAD if n_lags is None else n_lags
    N = n // 2
    if not 2 <= n_lags <= N or part.shape[1] != HEAD + n_lags:
        raise ValueError("need 2 <= n_lags <= N lags, all present")
    center = np.broadcast_to(np.asarray(center, dtype=LD), (part.shape[0],))
    S = int(superchain_size or 0)
    res = []
    nan = LD("nan")
    for p, q in enumerate(part):
        r = dict.fromkeys(OUT, nan)
        r["K"], r["lags_complete"], r["n_lags"] = int(q[4]), True, n_lags
        res.append(r)
        if not (np.all(np.isfinite(q)) and np.isfinite(center[p])):
            continue
        Mp, Nd = q[0], LD(N)
        W = q[3] / Mp
        BN = (q[2] - q[1] * q[1] / Mp) / (Mp - 1)
        var_plus = (Nd - 1) / Nd * W + BN
        r.update(mean=center[p] + q[1] / Mp, var_plus=var_plus, W=W, B_over_N=BN)
        K = q[4]
        if S > 0 and K > 1:
            B_nu = (q[6] - q[5] * q[5] / K) / (K - 1)
            W_nu = (q[7] + q[8]) / K
            if W_nu > 0:
                r["nested_rhat"] = np.sqrt(1 + B_nu / W_nu)
        if not W > 0:
            continue
        r["split_rhat"] = np.sqrt(var_plus / W)
        rho = 1 - (W - q[HEAD:] / Mp) / var_plus
        rho_t = np.zeros(n_lags, dtype=LD)
        even, odd = LD(1), rho[1]
        rho_t[0], rho_t[1] = even, odd
        t = 1
        lim = min(N - 3, n_lags - 2)
        while t < lim and even + odd > 0:  # Geyer's initial positive sequence
            even, odd = rho[t + 1], rho[t + 2]
            if even + odd >= 0:
                rho_t[t + 1], rho_t[t + 2] = even, odd
            t += 2
        r["lags_complete"] = not (even + odd > 0 and t < N - 3)
        max_t = t - 2
        if even > 0:
            rho_t[max_t + 1] = even
        t = 1
        while t <= max_t - 2:  # Geyer's initial monotone sequence
            if rho_t[t + 1] + rho_t[t + 2] > rho_t[t - 1] + rho_t[t]:
                rho_t[t + 1] = (rho_t[t - 1] + rho_t[t]) / 2
                rho_t[t + 2] = rho_t[t + 1]
            t += 2
        MN = Mp * Nd
        tau = -1 + 2 * rho_t[: max_t + 1].sum() + rho_t[max_t + 1]
        tau = max(tau, 1 / np.log10(MN))
        r.update(tau=tau, ess=MN / tau, mcse_mean=np.sqrt(var_plus / (MN / tau)))
    return res


def diagnostics(trace, superchain_size=None, center=None, n_lags=None, lag_block=64):
    """The statistics of a trace: lags computed `lag_block` at a time until Geyer's truncation (or exactly [0, n_lags))."""
    tr = Trace(trace, superchain_size, center)
    if n_lags is not None:
        return finish(tr.n, tr.partials(0, n_lags), tr.center, superchain_size)
    lags = np.zeros((tr.d, 0), dtype=LD)
    while True:
        end = min(tr.N, lags.shape[1] + lag_block)
        lags = np.concatenate([lags, tr.lag_sums(lags.shape[1], end)], axis=1)
        res = finish(tr.n, np.concatenate([tr.head, lags], axis=1), tr.center, superchain_size)
        if end >= tr.N or all(r["lags_complete"] for r in res):
            return res


def unsplit_rhat(trace):
    """The split-R-hat formula applied to the whole chains (no splitting) → (d,) long double."""
    x = _trace(trace)
    n = x.shape[0]
    W = x.var(axis=0, ddof=1).mean(axis=0)
    B = x.mean(axis=0).var(axis=0, ddof=1)
    return np.sqrt(((n - 1) / LD(n) * W + B) / W)
